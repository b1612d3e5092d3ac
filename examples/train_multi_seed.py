#!/usr/bin/env python
"""Train several seeds of one agent on ONE MI355X from one process: a thread and a HIP context per seed.

Separate processes sharing a GPU time-slice (2 processes reach 70 updates/s together where one reaches
111); contexts of one process overlap instead -- an agent's dependent kernel chain leaves latency gaps that another agent's
kernels fill (3 agents: ~190 updates/s together).  ctypes releases the GIL inside the library calls, so the update phases of
the seeds overlap; the Python collector loops take turns.

    python examples/train_multi_seed.py --algo ppol --seeds 3 --epoch 2
    python examples/train_multi_seed.py --algo ppol --seeds 4 --epoch 2 --grouped     # PPO-Lag, FOCOPS, SAC-Lag, DDPG-Lag and CVPO
    python examples/train_multi_seed.py --algo focops --seeds 4 --epoch 2 --grouped
    python examples/train_multi_seed.py --algo sacl --seeds 4 --epoch 2 --grouped
    python examples/train_multi_seed.py --algo cvpo --seeds 4 --epoch 2 --grouped

--grouped: ONE thread; the seeds collect in lock step (fsrl_amd.data.GroupCollector -> fsrl_group_collect_step: one actor
request per vector step for all seeds, served by one resident kernel) and their updates run in lock step through the grouped
launches (fsrl_amd.policy.PolicyGroup -> fsrl_group_ppo_update: every launch of the minibatch step carries all seeds):
~2x the aggregate updates/s of the thread-per-seed mode at 4 seeds (tools/bench_group.py); collection: tools/bench_group_collect.py.
Per seed the run is the one of collecting the seeds one after the other, bit for bit.  --grouped --algo focops: the same loop
with FOCOPS seeds (each seed's nu step, then one grouped FOCOPS update; tools/bench_group_focops.py).
--grouped --algo sacl: ONE thread; the seeds collect in lock step (GroupCollector over an fsrl_amd.engine.EngineCollectGroup ->
fsrl_collect_group_step: one request per vector step to one resident kernel running every seed's actor network), each seed steps
its PID multiplier, then ONE grouped update (fsrl_amd.policy.SACPolicyGroup -> fsrl_sac_group_update) runs round(update_per_step * n/st)
updates per seed, every launch carrying all seeds (tools/bench_group_sac.py).
--grouped --algo cvpo: the same loop with CVPO seeds (each seed's pre_update_fn resets its M-step multipliers, ONE grouped update
through fsrl_amd.policy.CVPOPolicyGroup -> fsrl_cvpo_group_update, each seed's post_update_fn copies actor -> actor_old;
tools/bench_group_cvpo.py).
--grouped --algo ddpgl: the same loop with DDPG-Lag seeds (ONE grouped update through fsrl_amd.policy.DDPGPolicyGroup ->
fsrl_sac_group_update over deterministic-actor contexts; tools/bench_group_sac.py --algo ddpgl).
    python examples/train_multi_seed.py --algo ddpgl --seeds 4 --epoch 2 --grouped
--per-alpha A [--per-beta B] [--per-no-weight-norm] (--algo sacl / ddpgl, every mode): prioritised replay -- every seed's buffer is a
HipPrioritizedVectorReplayBuffer, its sum tree on the device.  --grouped: the seeds' prioritised updates share every launch, the
solo prioritised update's sequence once per update for all seeds (13 launches for fused seeds; tools/bench_group_sac.py --per A,B).
CVPO hands no TD error back to a buffer: --algo cvpo refuses the flags.
    python examples/train_multi_seed.py --algo sacl --seeds 8 --epoch 2 --grouped --per-alpha 0.6 --per-beta 0.4
--hidden-sizes 64x48x32 (every mode): the networks' hidden layers.  Anything but two layers of at most 256 units makes layered
contexts; --grouped --algo ppol takes them as well: a layered minibatch step is 2 L + 5 launches whatever the number of seeds
and the actor request of a vector step L + 2 (tools/bench_group_layered.py).
    python examples/train_multi_seed.py --algo ppol --seeds 8 --epoch 2 --grouped --hidden-sizes 256x256x256
--grouped --algo sacl / ddpgl take layered seeds too: a layered replay update is 9 L + 19 launches whatever the number of seeds,
per seed bit-identical to its own update, and the actor request of a vector step L + 2 (tools/bench_group_sac.py --hidden ...,
tools/bench_group_collect.py --hidden ...): at 8 seeds of (256, 256, 256) 1.9x the updates/s of 8 threads and 2.3x the env-steps/s of
collecting seed by seed; grouped updates lose to threads at 2 seeds or fewer, shared collection loses at one seed.
Layered CVPO seeds do not group yet: --grouped --algo cvpo refuses them.
    python examples/train_multi_seed.py --algo sacl --seeds 8 --epoch 2 --grouped --hidden-sizes 64x48x32
--grouped --algo cpo / trpol: ONE thread collects -- the seeds collect in lock step through an EngineCollectGroup over their
on-policy engines (one actor request per vector step, the resident kernel of the PPO-Lag group; layered seeds: L + 2 launches) --
each seed's pre_update_fn sees its cost, then ONE fsrl_amd.policy.TrustPolicyGroup.update runs every seed's own update
(fsrl_tr_begin + fsrl_cpo_learn / fsrl_trpo_learn) on a worker thread per seed, beside each other; no launch is shared on the
update side.  Per seed bit-identical to collecting and updating the seeds one after the other (tools/bench_group_trust.py,
tools/bench_group_collect.py --algo cpo).  Fused and layered --hidden-sizes.
    python examples/train_multi_seed.py --algo cpo --seeds 8 --epoch 2 --grouped
    python examples/train_multi_seed.py --algo trpol --seeds 4 --epoch 2 --grouped --hidden-sizes 64x48x32
--workers W [--busy-us U] (every mode): each seed's envs live in W worker processes (fsrl_amd.env.ShmemVectorEnv), an env step costing U
microseconds of host time.  --grouped then runs a whole collect of all seeds as ONE library call (GroupCollector's native loop ->
fsrl_group_collect_episodes / fsrl_collect_episodes_group): every seed's step command is posted to its workers before the first is
waited for, so k seeds pay one env-step time per vector step, not k (tools/bench_group_collect.py --workers).
    python examples/train_multi_seed.py --algo ppol --seeds 4 --epoch 2 --grouped --workers 2 --busy-us 100
--sweep NAME=v1,v2,... (repeatable; --grouped --algo ppol only; one value per seed): the members of the group are a SWEEP, member i
running with value i of every swept PPOLagAgent keyword (eps_clip, dual_clip, vf_coef, max_grad_norm, target_kl, lr, gae_lambda,
gamma, cost_limit; `none` switches dual_clip / target_kl off) and of batch_size / repeat_per_collect -- still one grouped update
per collect (PolicyGroup.update with a batch size and a pass count per member -> fsrl_group_ppo_update_each).  The members must agree
on whether max_grad_norm is on.  FOCOPS groups are not sweeps.
    python examples/train_multi_seed.py --algo ppol --seeds 4 --epoch 2 --grouped --sweep eps_clip=0.1,0.2,0.2,0.3 --sweep batch_size=128,256,256,512
--task device-linear | device-point-circle (--grouped, every algo it takes): the seeds' envs live on the GPU (fsrl_amd.env.DeviceLinear:
the default task's dynamics; DevicePointCircle), each seed has a DeviceVectorEnv on its engine and a DeviceCollector, and a collect
of all seeds is ONE fsrl_amd.data.GroupDeviceCollector.collect -> fsrl_collect_device_group: every launch carries all seeds'
collects, a workgroup per seed, per seed bit-identical to its own device collect (tools/bench_device_collect.py --ks; DESIGN.md
3.4.1).  The updates go through the same groups as above.  Layered --hidden-sizes are refused by the library at the first collect.
    python examples/train_multi_seed.py --algo ppol --seeds 8 --epoch 2 --grouped --task device-linear
    python examples/train_multi_seed.py --algo sacl --seeds 4 --epoch 2 --grouped --task device-point-circle
--test-episodes N (--grouped; default 0: no evaluation): after every epoch each seed's policy is evaluated for N episodes on test envs
of its own and one line per seed is printed.  Over device tasks every seed has a second DeviceVectorEnv and a store-less
DeviceCollector, and the evaluation of ALL seeds is one GroupDeviceCollector.collect -> fsrl_evaluate_device_group: nothing is
stored and no seed's store, sampler or random stream moves, so the training run is the one without the flag, bit for bit.  Over host
envs the seeds are evaluated one after the other (FastCollector over a host test env).
    python examples/train_multi_seed.py --algo ppol --seeds 8 --epoch 2 --grouped --task device-linear --test-episodes 4
"""
import argparse
import os
import sys
import tempfile
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fsrl_amd.agent import CPOAgent, CVPOAgent, DDPGLagAgent, FOCOPSAgent, PPOLagAgent, SACLagAgent, TRPOLagAgent  # noqa: E402
from fsrl_amd.env import DeviceLinear, DevicePointCircle, PointCircleEnv, ShmemVectorEnv, SyntheticSafetyVectorEnv  # noqa: E402
from fsrl_amd.utils import BaseLogger  # noqa: E402

AGENTS = {"ppol": PPOLagAgent, "cpo": CPOAgent, "trpol": TRPOLagAgent, "focops": FOCOPSAgent, "sacl": SACLagAgent,
          "ddpgl": DDPGLagAgent, "cvpo": CVPOAgent}
def make_env(a, seed):
    """a seed's vector env: in-process, or --workers W worker processes (ShmemVectorEnv; --busy-us: host time of one env step).
    Over worker-process envs a grouped collect is ONE library call and the seeds' workers step at the same time."""
    if a.workers:
        return ShmemVectorEnv(env_num=a.envs, workers=a.workers, obs_dim=8, act_dim=2, episode_len=300, seed=seed, busy_us=a.busy_us)
    return SyntheticSafetyVectorEnv(env_num=a.envs, obs_dim=8, act_dim=2, episode_len=300, seed=seed)


def make_seed(a, seed, **agent_kw):
    """a seed's agent and the vector env it collects from.  --task device-*: the agent is built over a host env of the task's shapes,
    the envs it collects from live on its engine's GPU"""
    host = PointCircleEnv() if a.task == "device-point-circle" else make_env(a, seed)
    logger = BaseLogger(tempfile.mkdtemp(prefix=f"fsrl_amd_s{seed}_"), name=f"{a.algo}-s{seed}")
    agent = AGENTS[a.algo](host, logger, device=a.device, seed=seed, hidden_sizes=a.hidden_sizes, training_num=a.envs, **agent_kw)
    agent.policy.train()
    if a.task == "device-point-circle":
        return agent, DevicePointCircle(agent.policy, a.envs, max_episode_steps=300, seed=seed)
    if a.task == "device-linear":
        return agent, DeviceLinear(agent.policy, like=host, seed=seed)
    return agent, host


def make_collector(a, agent, env, buf):
    from fsrl_amd.data import DeviceCollector, FastCollector
    if a.task.startswith("device-"):
        return DeviceCollector(agent.policy, env, buf)
    return FastCollector(agent.policy, env, buf, exploration_noise=True, device_actor=True)


def make_group_collector(a, group_of, cols):
    """device envs: every seed's whole collect in one looping launch; else lock step through `group_of()`'s shared actor request"""
    from fsrl_amd.data import GroupCollector, GroupDeviceCollector
    if a.task.startswith("device-"):
        return None, GroupDeviceCollector(cols)
    g = group_of()
    return g, GroupCollector(g, cols)


class Evaluator:
    """--test-episodes N: the seeds' test envs and collectors.  Device tasks: a second device env per seed on its engine, store-less
    DeviceCollectors, ONE grouped launch sequence for every seed's evaluation; host tasks: a FastCollector per seed, in turn."""

    def __init__(self, a, agents):
        from fsrl_amd.data import DeviceCollector, FastCollector, GroupDeviceCollector
        self.a, self.agents, self.envs, self.group = a, agents, [], None
        test_num = min(a.envs, max(1, min(a.test_episodes, 2)))
        for seed, ag in enumerate(agents):
            if a.task == "device-point-circle":
                self.envs.append(DevicePointCircle(ag.policy, test_num, max_episode_steps=300, seed=seed + 1000))
            elif a.task == "device-linear":
                like = SyntheticSafetyVectorEnv(env_num=test_num, obs_dim=8, act_dim=2, episode_len=300, seed=seed + 1000)
                self.envs.append(DeviceLinear(ag.policy, like=like, seed=seed + 1000))
            else:
                self.envs.append(SyntheticSafetyVectorEnv(env_num=test_num, obs_dim=8, act_dim=2, episode_len=300, seed=seed + 1000))
        if a.task.startswith("device-"):
            self.cols = [DeviceCollector(ag.policy, env) for ag, env in zip(agents, self.envs)]
            self.group = GroupDeviceCollector(self.cols)
        else:
            self.cols = [FastCollector(ag.policy, env) for ag, env in zip(agents, self.envs)]

    def run(self, epoch):
        for ag in self.agents:
            ag.policy.eval()
        for col in self.cols:
            col.reset_env()
        n = self.a.test_episodes
        stats = self.group.collect(n_episode=n) if self.group is not None else [col.collect(n_episode=n) for col in self.cols]
        for seed, (ag, st) in enumerate(zip(self.agents, stats)):
            ag.policy.train()
            ag.logger.store(**{"test/reward": st["rew"], "test/cost": st["cost"], "test/length": int(st["len"])})
            print(f"epoch {epoch} seed {seed}: test reward {st['rew']:.2f} cost {st['cost']:.2f} length {st['len']:.1f} ({st['n/ep']} episodes)")

    def close(self):
        for env in self.envs:
            if hasattr(env, "close"):
                env.close()


def make_evaluator(a, agents):
    return Evaluator(a, agents) if a.test_episodes > 0 else None


# --sweep: PPOLagAgent keywords (float; `none` where the agent takes None) and the two update arguments (int)
SWEEP_AGENT_KEYS = ("eps_clip", "dual_clip", "vf_coef", "max_grad_norm", "target_kl", "lr", "gae_lambda", "gamma", "cost_limit")
SWEEP_UPDATE_KEYS = ("batch_size", "repeat_per_collect")
SWEEP_NONE_OK = ("dual_clip", "target_kl", "max_grad_norm")


def parse_sweep(specs, k):
    """--sweep NAME=v1,...,vk (repeatable) -> {name: [k values]}; ValueError with the message for ap.error"""
    out = {}
    for spec in specs or []:
        name, eq, vals = spec.partition("=")
        if not eq or name not in SWEEP_AGENT_KEYS + SWEEP_UPDATE_KEYS:
            raise ValueError(f"--sweep {spec}: NAME=v1,v2,... with NAME one of {', '.join(SWEEP_AGENT_KEYS + SWEEP_UPDATE_KEYS)}")
        if name in out:
            raise ValueError(f"--sweep {name}: given twice")
        vals = vals.split(",")
        if len(vals) != k:
            raise ValueError(f"--sweep {name}: {len(vals)} values for {k} seeds (one value per member)")
        try:
            if name in SWEEP_UPDATE_KEYS:
                out[name] = [int(v) for v in vals]
            else:
                out[name] = [None if (v.lower() == "none" and name in SWEEP_NONE_OK) else float(v) for v in vals]
        except ValueError:
            raise ValueError(f"--sweep {spec}: not a number") from None
        if name in SWEEP_UPDATE_KEYS and min(out[name]) < (1 if name == "batch_size" else 0):
            raise ValueError(f"--sweep {name}: batch_size >= 1, repeat_per_collect >= 0")
    return out


GROUPED_ALGOS = ("ppol", "focops", "sacl", "ddpgl", "cvpo", "cpo", "trpol")      # what --grouped takes


def run_grouped_trust(a):
    """k CPO (TRPO-Lag) seeds: lock-step collection from one host thread (a collect group over the seeds' on-policy engines), each
    seed's pre_update_fn, then ONE TrustPolicyGroup.update -- the seeds' own updates on a worker thread each -- and reset_buffer."""
    from fsrl_amd.data import HipVectorReplayBuffer
    from fsrl_amd.engine import EngineCollectGroup
    from fsrl_amd.policy import TrustPolicyGroup
    agents, cols, bufs = [], [], []
    for seed in range(a.seeds):
        agent, env = make_seed(a, seed, cost_limit=10.0)
        buf = HipVectorReplayBuffer(agent.policy.engine, None, a.envs)
        agents.append(agent); bufs.append(buf)
        cols.append(make_collector(a, agent, env, buf))
    cgroup, gcol = make_group_collector(a, lambda: EngineCollectGroup([ag.policy.engine for ag in agents]), cols)
    group = TrustPolicyGroup([ag.policy for ag in agents], collect_group=cgroup)
    evaluator = make_evaluator(a, agents)
    t0, steps, updates = time.time(), 0, 0
    for ep in range(a.epoch):
        budget = 6000
        while budget > 0:
            for ag, st in zip(agents, gcol.collect(n_episode=a.envs)):
                ag.policy.pre_update_fn(stats_train=st)
                ag.logger.store(**{"train/reward": st["rew"], "train/cost": st["cost"]})
                steps += st["n/st"]
            budget -= st["n/st"]
            group.update(bufs, batch_size=99999, repeat=4)
            updates += len(agents)
            for col in cols:
                col.reset_buffer(keep_statistics=True)
        for seed, ag in enumerate(agents):
            print(f"epoch {ep + 1} seed {seed}: reward {ag.logger.get_mean('train/reward'):.2f} "
                  f"cost {ag.logger.get_mean('train/cost'):.2f}")
            ag.logger.write(steps, display=False)
        if evaluator is not None:
            evaluator.run(ep + 1)
    dt = time.time() - t0
    print(f"{a.seeds} seeds x {a.epoch} epochs grouped on {a.device}: {steps / dt:.0f} env-steps/s, {updates / dt:.1f} updates/s "
          f"aggregate in {dt:.1f} s")
    if evaluator is not None:
        evaluator.close()                # device test envs go before their engines too
    group.close()
    if cgroup is not None:
        cgroup.close()
    for col in cols:
        col.env.close()              # a device env goes before the engine it lives on
    for ag in agents:
        ag.policy.engine.close()


def run_grouped_replay(a):
    """k SAC-Lag (CVPO, DDPG-Lag) seeds, one host thread: the seeds collect in lock step (one collect-group call per vector step) and
    run their pre_update_fn (SAC-Lag / DDPG-Lag: the PID multiplier's step; CVPO: the M-step multipliers' reset), then ONE grouped
    update runs each seed's round(update_per_step * n/st) updates (what OffpolicyTrainer.policy_update_fn runs per seed), then each
    seed's post_update_fn.  --per-alpha: every seed's buffer is prioritised (made before the group: its members agree on that)."""
    from fsrl_amd.data import HipPrioritizedVectorReplayBuffer, HipVectorReplayBuffer
    per = prioritized_replay(a)
    from fsrl_amd.engine import EngineCollectGroup
    from fsrl_amd.policy import CVPOPolicyGroup, DDPGPolicyGroup, SACPolicyGroup
    agents, cols, bufs = [], [], []
    for seed in range(a.seeds):
        agent, env = make_seed(a, seed, cost_limit=10.0)
        if per is None:
            buf = HipVectorReplayBuffer(agent.policy.engine, None, a.envs)
        else:
            buf = HipPrioritizedVectorReplayBuffer(agent.policy.engine, None, a.envs, **per)
        agents.append(agent); bufs.append(buf)
        cols.append(make_collector(a, agent, env, buf))
    group = {"sacl": SACPolicyGroup, "ddpgl": DDPGPolicyGroup, "cvpo": CVPOPolicyGroup}[a.algo]([ag.policy for ag in agents])
    cgroup, gcol = make_group_collector(a, lambda: EngineCollectGroup([ag.policy.engine for ag in agents]), cols)
    evaluator = make_evaluator(a, agents)
    update_per_step, t0, steps, updates = 0.2, time.time(), 0, 0
    for ep in range(a.epoch):
        budget = 6000
        while budget > 0:
            n, sts = [], []
            for ag, st in zip(agents, gcol.collect(n_episode=a.envs)):
                sts.append(st)
                ag.policy.pre_update_fn(stats_train=st)
                ag.logger.store(**{"train/reward": st["rew"], "train/cost": st["cost"]})
                steps += st["n/st"]
                n.append(round(update_per_step * st["n/st"]))
            budget -= st["n/st"]
            group.update(bufs, batch_size=256, n_updates=n)
            for ag, st in zip(agents, sts):
                ag.policy.post_update_fn(stats_train=st)
            updates += sum(n)
        for seed, ag in enumerate(agents):
            print(f"epoch {ep + 1} seed {seed}: reward {ag.logger.get_mean('train/reward'):.2f} "
                  f"cost {ag.logger.get_mean('train/cost'):.2f}")
            ag.logger.write(steps, display=False)
        if evaluator is not None:
            evaluator.run(ep + 1)
    dt = time.time() - t0
    print(f"{a.seeds} seeds x {a.epoch} epochs grouped on {a.device}: {steps / dt:.0f} env-steps/s, {updates / dt:.1f} updates/s "
          f"aggregate in {dt:.1f} s")
    if evaluator is not None:
        evaluator.close()                # device test envs go before their engines too
    if cgroup is not None:
        cgroup.close()
    group.close()
    for col in cols:
        col.env.close()              # a device env goes before the engine it lives on
    for ag in agents:
        ag.policy.engine.close()


def run_grouped(a):
    """k PPO-Lag (FOCOPS) seeds, one host thread: collect every seed's episodes in lock step, step each PID multiplier (each
    seed's cost goes to its nu step), ONE grouped update."""
    assert a.algo in GROUPED_ALGOS, "--grouped: PPO-Lagrangian, FOCOPS, SAC-Lagrangian, DDPG-Lagrangian, CVPO, CPO or TRPO-Lagrangian"
    if a.algo in ("sacl", "ddpgl", "cvpo"):
        return run_grouped_replay(a)
    if a.algo in ("cpo", "trpol"):
        return run_grouped_trust(a)
    from fsrl_amd.data import HipVectorReplayBuffer
    from fsrl_amd.policy import PolicyGroup
    agents, cols, bufs = [], [], []
    for seed in range(a.seeds):
        kw = dict(cost_limit=10.0)
        kw.update({name: vals[seed] for name, vals in a.sweep.items() if name in SWEEP_AGENT_KEYS})       # a sweep: member i's own values
        agent, env = make_seed(a, seed, **kw)
        buf = HipVectorReplayBuffer(agent.policy.engine, None, a.envs)
        agents.append(agent); bufs.append(buf)
        cols.append(make_collector(a, agent, env, buf))
    group = PolicyGroup([ag.policy for ag in agents])
    batch_size, repeat = a.sweep.get("batch_size", 256), a.sweep.get("repeat_per_collect", 4)       # ints, or one int per member
    mult = (lambda p: f"nu {float(p._nu):.3f}") if a.algo == "focops" else (lambda p: f"lambda {p.lag_optims[0].get_lag():.3f}")
    _, gcol = make_group_collector(a, lambda: group, cols)
    evaluator = make_evaluator(a, agents)
    t0, steps, updates = time.time(), 0, 0
    for ep in range(a.epoch):
        budget = 6000
        while budget > 0:
            for ag, st in zip(agents, gcol.collect(n_episode=a.envs)):
                ag.policy.pre_update_fn(stats_train=st)
                ag.logger.store(**{"train/reward": st["rew"], "train/cost": st["cost"]})
                steps += st["n/st"]
            budget -= st["n/st"]
            group.update(bufs, batch_size=batch_size, repeat=repeat)
            updates += len(agents)
            for col in cols:
                col.reset_buffer(keep_statistics=True)
        for seed, ag in enumerate(agents):
            print(f"epoch {ep + 1} seed {seed}: reward {ag.logger.get_mean('train/reward'):.2f} "
                  f"cost {ag.logger.get_mean('train/cost'):.2f} {mult(ag.policy)}")
            ag.logger.write(steps, display=False)
        if evaluator is not None:
            evaluator.run(ep + 1)
    dt = time.time() - t0
    print(f"{a.seeds} seeds x {a.epoch} epochs grouped on {a.device}: {steps / dt:.0f} env-steps/s, {updates / dt:.1f} updates/s "
          f"aggregate in {dt:.1f} s")
    if evaluator is not None:
        evaluator.close()                # device test envs go before their engines too
    group.close()
    for col in cols:
        col.env.close()              # a device env goes before the engine it lives on
    for ag in agents:
        ag.policy.engine.close()


def prioritized_replay(a):
    """--per-alpha / --per-beta / --per-no-weight-norm -> the agents' `prioritized_replay` dict, or None"""
    if a.per_alpha is None:
        return None
    return dict(alpha=a.per_alpha, beta=a.per_beta, weight_norm=not a.per_no_weight_norm)


def is_layered(hidden_sizes):
    """the engine's rule: anything but two hidden layers of at most 256 units makes a layered context"""
    return len(hidden_sizes) != 2 or max(hidden_sizes) > 256


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--algo", choices=sorted(AGENTS), default="ppol")
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--epoch", type=int, default=2)
    ap.add_argument("--envs", type=int, default=20)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--task", choices=["linear", "device-linear", "device-point-circle"], default="linear",
                    help="linear: the in-process synthetic env (or --workers); device-*: the seeds' envs live on the GPU and --grouped runs "
                         "every seed's whole collect in one looping launch (GroupDeviceCollector)")
    ap.add_argument("--grouped", action="store_true", help="PPO-Lag / FOCOPS / SAC-Lag / DDPG-Lag / CVPO: lock-step collection and grouped updates from one thread; "
                                                           "CPO / TRPO-Lag: lock-step collection, the seeds' own updates beside each other")
    ap.add_argument("--hidden-sizes", default="128x128", type=lambda t: tuple(int(w) for w in t.lower().split("x")),
                    help="hidden layers of every network, e.g. 64x48x32 (anything but two layers of at most 256 units runs the "
                         "layered kernels; --grouped takes such PPO-Lag, SAC-Lag, DDPG-Lag, CPO and TRPO-Lag seeds too, not FOCOPS or CVPO seeds)")
    ap.add_argument("--workers", type=int, default=0, help="worker processes per seed's env (one ShmemVectorEnv per seed); 0: in-process envs. "
                                                           "--grouped then collects with one library call per collect for all seeds")
    ap.add_argument("--busy-us", type=float, default=0.0, help="--workers: host time of one env step in microseconds (a simulator's stand-in)")
    ap.add_argument("--test-episodes", type=int, default=0,
                    help="--grouped: evaluate every seed for this many episodes after each epoch (0: off); over device tasks all seeds' "
                         "evaluations run in one grouped store-less launch sequence (fsrl_evaluate_device_group)")
    ap.add_argument("--sweep", action="append", default=[], metavar="NAME=v1,v2,...",
                    help="--grouped --algo ppol: member i runs with value i (one per seed) of a PPOLagAgent keyword ("
                         + ", ".join(SWEEP_AGENT_KEYS) + ") or of " + " / ".join(SWEEP_UPDATE_KEYS) + "; repeatable")
    ap.add_argument("--per-alpha", type=float, default=None, help="sacl / ddpgl: prioritised replay with this priority exponent")
    ap.add_argument("--per-beta", type=float, default=None, help="... and this importance-weight exponent (with --per-alpha; default 0.4)")
    ap.add_argument("--per-no-weight-norm", action="store_true", help="... without dividing the weights by the batch maximum (with --per-alpha)")
    a = ap.parse_args(argv)
    if a.per_alpha is None and (a.per_beta is not None or a.per_no_weight_norm):
        ap.error("--per-beta / --per-no-weight-norm: options of prioritised replay, which --per-alpha switches on")
    if a.per_alpha is not None:
        if a.algo not in ("sacl", "ddpgl"):
            ap.error(f"--per-alpha: prioritised replay is built for sacl and ddpgl, not {a.algo}"
                     + (": CVPO's update has no per-row TD error to hand back to the buffer" if a.algo == "cvpo" else ""))
        a.per_beta = 0.4 if a.per_beta is None else a.per_beta
        if a.per_alpha < 0 or a.per_beta < 0:
            ap.error("--per-alpha / --per-beta: >= 0")
    if a.sweep and not (a.grouped and a.algo == "ppol"):
        ap.error("--sweep: PPO-Lagrangian groups only (--grouped --algo ppol); FOCOPS groups keep one set of hyper-parameters")
    try:
        a.sweep = parse_sweep(a.sweep, a.seeds)
    except ValueError as e:
        ap.error(str(e))
    clip = a.sweep.get("max_grad_norm")
    if clip and len({bool(v) for v in clip}) > 1:
        ap.error("--sweep max_grad_norm: the members must agree on whether the clip is on (all values > 0, or all none / 0)")
    if a.test_episodes < 0 or (a.test_episodes and not a.grouped):
        ap.error("--test-episodes: >= 0, with --grouped (a seed of its own evaluates through the agents' learn(test_envs))")
    if a.task != "linear" and not a.grouped:
        ap.error("--task device-*: the grouped device collect of this example (--grouped); one seed's device env: the agents' learn()")
    if a.task != "linear" and a.workers:
        ap.error("--task device-*: the envs live on the GPU, there are no worker processes (--workers 0)")
    if a.task != "linear" and a.envs > 64:
        ap.error("--task device-*: a device env holds at most 64 envs per seed")
    if a.workers < 0 or a.workers > a.envs:
        ap.error("--workers: 0 (in-process envs) .. --envs")
    if isinstance(a.hidden_sizes, str):
        a.hidden_sizes = tuple(int(w) for w in a.hidden_sizes.lower().split("x"))
    if a.grouped and a.algo in ("focops", "cvpo") and is_layered(a.hidden_sizes):
        ap.error(f"--grouped --algo {a.algo}: layered seeds (--hidden-sizes other than two layers of at most 256 units) do not group yet")
    return a


def main():
    a = parse_args()
    out, errs = {}, []
    if a.grouped:
        return run_grouped(a)

    def run(seed):
        env = None
        try:
            env = make_env(a, seed)
            logger = BaseLogger(tempfile.mkdtemp(prefix=f"fsrl_amd_s{seed}_"), name=f"{a.algo}-s{seed}")
            agent = AGENTS[a.algo](env, logger, cost_limit=10.0, device=a.device, seed=seed, hidden_sizes=a.hidden_sizes,
                                   training_num=a.envs)
            kw = dict(epoch=a.epoch, episode_per_collect=a.envs, step_per_epoch=6000, device_actor=True, verbose=False,
                      save_ckpt=False, show_progress=False)
            if a.algo in ("sacl", "ddpgl", "cvpo"):
                if prioritized_replay(a) is not None:
                    kw["prioritized_replay"] = prioritized_replay(a)
                ep, stat, info = agent.learn(env, None, update_per_step=0.2, batch_size=256, **kw)
            else:
                ep, stat, info = agent.learn(env, None, repeat_per_collect=4,
                                             batch_size=256 if a.algo in ("ppol", "focops") else 99999, **kw)
            out[seed] = {k: round(float(v), 3) for k, v in stat.items() if k in ("train/reward", "train/cost", "update/env_step")}
        except Exception as e:      # a failing seed must not hang the others
            errs.append((seed, repr(e)))
        finally:
            if env is not None:
                env.close()

    t0 = time.time()
    threads = [threading.Thread(target=run, args=(s, )) for s in range(a.seeds)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for s in sorted(out):
        print(f"seed {s}: {out[s]}")
    print(f"{len(out)} seeds x {a.epoch} epochs in {time.time() - t0:.1f} s on {a.device}")
    if errs:
        raise SystemExit(f"failed seeds: {errs}")


if __name__ == "__main__":
    main()
