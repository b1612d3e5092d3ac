#!/usr/bin/env python
"""Train any of the HIP-backed agents the way the reference's examples/mlp/train_*_agent.py do, on the
synthetic SafetyCarCircle-shaped vector env (this image has no safety-gymnasium / bullet-safety-gym; with them
installed pass real vector envs exposing reset(ids) / step(act, ids) -> (obs, rew, terminated, truncated, info["cost"])).

    python examples/train_agent.py --algo ppol --epoch 3
    python examples/train_agent.py --algo sacl --epoch 2 --device-actor
    python examples/train_agent.py --algo sacl --epoch 2 --prefill /tmp/dataset/dataset.npz     (examples/collect_dataset.py --out /tmp/dataset)
    python examples/train_agent.py --algo ppol --epoch 3 --task device-point-circle    (envs on the GPU: whole collects in one looping kernel)
    python examples/train_agent.py --algo cpo --epoch 3 --task device-linear
    python examples/train_agent.py --algo sacl --epoch 2 --task device-point-circle    (ddpgl and cvpo likewise: nothing per step on the host)
"""
import argparse
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fsrl_amd.agent import CPOAgent, CVPOAgent, DDPGLagAgent, FOCOPSAgent, PPOLagAgent, SACLagAgent, TRPOLagAgent  # noqa: E402
from fsrl_amd.env import SyntheticSafetyVectorEnv  # noqa: E402
from fsrl_amd.utils import BaseLogger  # noqa: E402

AGENTS = {"ppol": PPOLagAgent, "cpo": CPOAgent, "trpol": TRPOLagAgent, "focops": FOCOPSAgent, "sacl": SACLagAgent,
          "ddpgl": DDPGLagAgent, "cvpo": CVPOAgent}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--algo", choices=sorted(AGENTS), default="ppol")
    ap.add_argument("--epoch", type=int, default=3)
    ap.add_argument("--envs", type=int, default=20)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--hidden-sizes", default="", help="hidden_sizes as a tuple, e.g. 64x48x32 or 512x512 (the reference's agents take any tuple); "
                                                       "two layers of at most 256 units run on the fused kernels, anything else on the layered ones")
    ap.add_argument("--cost-limit", type=float, default=10.0)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--seed", type=int, default=10)
    ap.add_argument("--device-actor", action="store_true", help="collector actions from fsrl_actor_sample (library RNG)")
    ap.add_argument("--batch-size", type=int, default=256, help="minibatch size of PPO-Lag / FOCOPS and the off-policy agents")
    ap.add_argument("--tr-batch-size", type=int, default=99999,
                    help="CPO / TRPO-Lag: Batch.split size inside learn (the reference's default 99999 = the whole buffer)")
    ap.add_argument("--task", choices=["synthetic", "point-circle", "device-point-circle", "device-linear"], default="synthetic",
                    help="synthetic: the vectorised stand-in dynamics; point-circle: per-instance gym-style envs built from factories; "
                         "device-point-circle / device-linear: the same two envs as device functions (every agent; at most 64 envs; any "
                         "--hidden-sizes: two layers of at most 256 units collect through fsrl_collect_device, every other shape through "
                         "fsrl_collect_device_layered), collected by DeviceCollector")
    ap.add_argument("--workers", type=int, default=0, help="> 0: the training envs step in that many worker processes (ShmemVectorEnv)")
    # options of the on-policy agents (the reference's constructor arguments of the same names)
    ap.add_argument("--unbounded", action=argparse.BooleanOptionalAction, default=None,
                    help="actor mean without max_action * tanh; --no-unbounded: with it (sacl, cvpo and the on-policy agents; "
                         "absent: the agent's own default -- sacl unbounded, every other agent bounded)")
    ap.add_argument("--reward-normalization", action="store_true", help="critics learn returns / running std")
    ap.add_argument("--value-clip", action="store_true", help="PPO-Lag clipped value loss (needs --reward-normalization)")
    ap.add_argument("--recompute-advantage", action="store_true", help="PPO-Lag / FOCOPS: GAE from the current critics before every pass")
    ap.add_argument("--prefill", default=None, metavar="PATH",
                    help="sacl / ddpgl / cvpo: start from a replay store filled with the episodes of this dataset (the .npz that "
                         "examples/collect_dataset.py or TrajectoryBuffer.save writes) instead of an empty one")
    ap.add_argument("--per-alpha", type=float, default=None, help="sacl / ddpgl: prioritised replay with this priority exponent")
    ap.add_argument("--per-beta", type=float, default=0.4, help="... and this importance-weight exponent (with --per-alpha)")
    a = ap.parse_args()
    if a.per_alpha is not None and a.algo not in ("sacl", "ddpgl"):
        ap.error(f"--per-alpha: prioritised replay is built for sacl and ddpgl, not {a.algo}")
    if a.prefill is not None and a.algo not in ("sacl", "ddpgl", "cvpo"):
        ap.error(f"--prefill fills a replay store: --algo must be sacl, ddpgl or cvpo, not {a.algo}")
    device_task = a.task.startswith("device-")
    if device_task and (a.envs > 64 or a.workers > 0):
        ap.error("a device env holds at most 64 envs and needs no worker processes")
    if a.task in ("point-circle", "device-point-circle"):
        # the reference's own construction (train_ppol_agent.py:120-123): one factory per env, in process or in worker processes
        from fsrl_amd.env import DummyVectorEnv, PointCircleEnv, ShmemVectorEnv
        fns = [lambda: PointCircleEnv(max_episode_steps=100) for _ in range(a.envs)]
        env = ShmemVectorEnv(fns, workers=a.workers, seed=a.seed) if a.workers > 0 else DummyVectorEnv(fns, seed=a.seed)
        test_env = DummyVectorEnv(fns[:2], seed=a.seed + 1000)
    elif a.workers > 0:
        from fsrl_amd.env import ShmemVectorEnv
        env = ShmemVectorEnv(env_num=a.envs, workers=a.workers, obs_dim=8, act_dim=2, episode_len=300, seed=a.seed)
    else:
        env = SyntheticSafetyVectorEnv(env_num=a.envs, obs_dim=8, act_dim=2, episode_len=300, seed=a.seed)
    if a.task not in ("point-circle", "device-point-circle"):
        test_env = SyntheticSafetyVectorEnv(env_num=2, obs_dim=8, act_dim=2, episode_len=300, seed=a.seed + 1)
    logger = BaseLogger(tempfile.mkdtemp(prefix="fsrl_amd_"), name=a.algo)
    kw = dict(cost_limit=a.cost_limit, device=a.device, seed=a.seed, hidden_sizes=(tuple(int(x) for x in a.hidden_sizes.split("x")) if a.hidden_sizes else (a.hidden, a.hidden)),
              training_num=a.envs)
    if a.algo in ("ppol", "cpo", "trpol", "focops"):
        kw.update(unbounded=bool(a.unbounded), reward_normalization=a.reward_normalization)
    if a.algo in ("sacl", "cvpo") and a.unbounded is not None:
        kw.update(unbounded=a.unbounded)
    if a.algo == "ppol":
        kw.update(value_clip=a.value_clip)
    if a.algo in ("ppol", "focops"):
        kw.update(recompute_advantage=a.recompute_advantage)
    agent = AGENTS[a.algo](env, logger, **kw)
    if device_task:
        # the host envs above gave the agent its spaces; the training envs and the test envs live on the agent's GPU: learn() and
        # evaluate() run whole evaluations there too, storing nothing (fsrl_evaluate_device; layered --hidden-sizes step the device
        # test envs from the host instead)
        from fsrl_amd.env import DeviceLinear, DevicePointCircle
        if a.task == "device-point-circle":
            env = DevicePointCircle(agent.policy, a.envs, max_episode_steps=100, seed=a.seed)
            test_env = DevicePointCircle(agent.policy, 2, max_episode_steps=100, seed=a.seed + 1000)
        else:
            env, test_env = DeviceLinear(agent.policy, like=env, seed=a.seed), DeviceLinear(agent.policy, like=test_env, seed=a.seed + 1)
    if a.algo in ("sacl", "ddpgl", "cvpo"):
        out = agent.learn(env, test_env, epoch=a.epoch, episode_per_collect=a.envs, step_per_epoch=6000, update_per_step=0.2,
                          batch_size=a.batch_size, testing_num=2, device_actor=a.device_actor, verbose=True, save_ckpt=False,
                          prefill=a.prefill,
                          **({} if a.per_alpha is None else {"prioritized_replay": dict(alpha=a.per_alpha, beta=a.per_beta)}))
    else:
        out = agent.learn(env, test_env, epoch=a.epoch, episode_per_collect=a.envs, step_per_epoch=6000, repeat_per_collect=4,
                          batch_size=a.batch_size if a.algo in ("ppol", "focops") else a.tr_batch_size, testing_num=2, device_actor=a.device_actor,
                          verbose=True, save_ckpt=False)
    print("final:", {k: round(float(v), 4) for k, v in out[1].items() if isinstance(v, (int, float))})
    rew, length, cost = agent.evaluate(test_env, eval_episodes=2)
    print(f"eval: reward {rew:.2f} length {length:.1f} cost {cost:.2f}")


if __name__ == "__main__":
    main()
