#!/usr/bin/env python
"""env-steps/s of a collect loop (training mode: stochastic actions) on the linear env at obs 8 / act 2, episode length 300:

  (a) device     fsrl_collect_device: actor, noise, map_action, env step, store write and episode bookkeeping in one looping kernel
  (b) in-process FastCollector(device_actor=True) over SyntheticSafetyVectorEnv: the resident actor, one doorbell round trip per vector step
  (c) stepped    FastCollector(device_actor=True) over DeviceVectorEnv.step: the device env as an ordinary vector env (one launch per step)

for 20 and 64 envs at hidden (256, 256) and (64, 64).  Every round times `--calls` collects of env_num episodes per path, the paths
alternate inside a round; the result is the median over the rounds and their spread (max - min).  For (a) also the time per vector
step and per launch, at the default steps per launch and with the whole collect in one launch.

--algo sacl | ddpgl | cvpo runs the same three paths on a replay context of that agent (default: the on-policy leg, output unchanged)
and adds the loop a user runs: a collect of env_num episodes, then round(update_per_step * n/st) updates of --batch-size rows (library
sampler, enqueued, statistics drained once per collect), device collect against FastCollector over the in-process env; env-steps/s.

    python tools/bench_device_collect.py --rounds 3 --out profiles/device_collect.json
    python tools/bench_device_collect.py --algo sacl --rounds 3 --out profiles/device_collect_replay.json

--ks 1,2,4,8 measures grouped seeds instead (on-policy contexts, k seeds on one GPU), aggregate env-steps/s over the k seeds:

  (a) grouped    GroupDeviceCollector: fsrl_collect_device_group, the k collects as the k workgroups of one looping launch
  (b) solo_seq   k solo device collects one after the other, on ungrouped twins
  (c) lock_step  GroupCollector over in-process envs with the EngineGroup's resident actor: one request per vector step for all seeds

--ab-tree DIR (with --ks) also holds the SOLO device collect of this tree against another checkout's (DIR: a built tree, e.g. the
parent commit), the two tools run as processes of their own, alternating; both sets of numbers go to --out.

    python tools/bench_device_collect.py --ks 1,2,4,8 --ab-tree ../parent --rounds 3 --out profiles/device_collect_group.json

--eval measures an EVALUATION of env_num episodes instead (the policy in eval mode, as BaseTrainer.test_step and evaluate() run it),
over a real agent's policy (PPOLagAgent, then SACLagAgent; --algo sacl: the second only), in episodes/s and env-steps/s:

  (a) evaluate   the store-less DeviceCollector(policy, env): fsrl_evaluate_device, nothing stored
  (b) stepped    FastCollector(policy, env): the host torch actor over DeviceVectorEnv.step, what evaluation over a device env was
  (c) collect    DeviceCollector(policy, env, buffer): the storing device collect, same mode

and with --ks the grouped evaluation (GroupDeviceCollector over store-less collectors, fsrl_evaluate_device_group) against k solo
evaluations one after the other, aggregate over the k seeds.

    python tools/bench_device_collect.py --eval --rounds 3 --ks 1,2,4,8 --out profiles/device_eval.json

A --hidden entry written with x (256x256x256, 64x48x32) is a LAYERED context's hidden_sizes; every mode above takes it, and the
collectors route it to fsrl_collect_device_layered / fsrl_evaluate_device_layered (lock_step is then the layered EngineGroup's
lock-step collection, (b) the layered actor's L + 2 launches per vector step).  --layered runs the four legs on such shapes (default
256x256x256 and 64x48x32) in one process -- the three solo paths on-policy and for one replay agent (--algo, default sacl), the
grouped seeds (--ks, default 1,2,4,8) and the evaluations -- and writes them into one file:

    python tools/bench_device_collect.py --layered --rounds 3 --out profiles/device_collect_layered.json
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fsrl_amd import _lib  # noqa: E402
from fsrl_amd.data import DeviceCollector, FastCollector, HipVectorReplayBuffer  # noqa: E402
from fsrl_amd.engine import Engine, EngineConfig, EngineGroup  # noqa: E402
from fsrl_amd.env import Box, DeviceLinear, SyntheticSafetyVectorEnv  # noqa: E402

EPISODE_LEN = 300


class Pol:
    """what the collectors read off a policy: training mode, clip, no scaling (the agents' defaults)"""
    traj_buffer = None
    training, _deterministic_eval = True, True
    action_bound_method, action_scaling = "clip", False

    def __init__(self, eng):
        self.engine = eng
        self.action_space = Box(-1.0, 1.0, (eng.cfg.act_dim, ))


def parse_hidden(text):
    """'256,64' -> [256, 64] (fused: two layers of that width); entries written with x are a layered context's hidden_sizes"""
    return [tuple(int(w) for w in h.split("x")) if "x" in h else int(h) for h in text.split(",")]


def hidden_kw(hidden):
    return dict(hidden_sizes=hidden) if isinstance(hidden, tuple) else dict(hidden=hidden)


def hidden_list(hidden):
    return list(hidden) if isinstance(hidden, tuple) else [hidden, hidden]


def shape_name(c):
    return "x".join(str(w) for w in c["hidden"])


def setup(path, hidden, n, algo="onpolicy"):
    kw = dict(obs_dim=8, act_dim=2, env_num=n, buffer_size=n * 2 * EPISODE_LEN, **hidden_kw(hidden))
    if algo == "onpolicy":
        eng = Engine(EngineConfig(**kw), device=0)
        eng.set_params((0.1 * np.random.default_rng(0).standard_normal(eng.n_params)).astype(np.float32))
    else:
        eng = Engine(EngineConfig(algo=_lib.ALGO_SAC_LAG, **kw), device=0)
        if algo == "cvpo":
            eng.cvpo_init(qc_thres=5.0)
        else:
            eng.sac_init(deterministic=algo == "ddpgl")
        rng = np.random.default_rng(0)
        eng.sac_put_params(0, (0.1 * rng.standard_normal(eng.n_sac_actor)).astype(np.float32))
        eng.sac_put_params(1, (0.1 * rng.standard_normal(eng.n_sac_critics)).astype(np.float32))
        eng.sac_put_params(2, eng.sac_get_params(1)[0])
    host = SyntheticSafetyVectorEnv(env_num=n, obs_dim=8, act_dim=2, episode_len=EPISODE_LEN, seed=1)
    pol, buf = Pol(eng), HipVectorReplayBuffer(eng, n * 2 * EPISODE_LEN, n)
    if path == "in_process":
        return eng, None, FastCollector(pol, host, buf, device_actor=True)
    env = DeviceLinear(eng, like=host, seed=1)
    return eng, env, (DeviceCollector(pol, env, buf) if path == "device" else FastCollector(pol, env, buf, device_actor=True))


def timed(col, n, calls):
    col.reset_buffer()
    col.collect(n_episode=n)                          # warm: code objects, the resident kernel, the staging arrays
    col.reset_buffer()
    rows, t0 = 0, time.perf_counter()
    for _ in range(calls):
        rows += col.collect(n_episode=n)["n/st"]
        col.reset_buffer()
    return rows, time.perf_counter() - t0


def timed_loop(eng, col, n, calls, algo, update_per_step, batch):
    """`calls` x (collect of n episodes, then round(update_per_step * n/st) updates); the store keeps its rows between the collects"""
    def one():
        st = col.collect(n_episode=n)["n/st"]
        k = int(round(update_per_step * st))
        for _ in range(k):
            if algo == "cvpo":
                eng.cvpo_update(batch, sync=False)
            else:
                eng.sac_update(batch, [0.5], 1.0, sync=False)
        eng.sac_drain()
        return st, k
    col.reset_buffer()
    one()
    rows, t0 = 0, time.perf_counter()
    for _ in range(calls):
        st, k = one()
        rows += st
    return rows, time.perf_counter() - t0, k


def setup_group(path, hidden, n, k):
    """k on-policy seeds for one of the grouped paths -> (engines, envs, EngineGroup or None, an object with .collect(n) -> stats per seed)"""
    from fsrl_amd.data import GroupCollector, GroupDeviceCollector
    engs, envs, cols = [], [], []
    for i in range(k):
        eng = Engine(EngineConfig(obs_dim=8, act_dim=2, env_num=n, buffer_size=n * 2 * EPISODE_LEN, **hidden_kw(hidden)), device=0)
        eng.set_params((0.1 * np.random.default_rng(i).standard_normal(eng.n_params)).astype(np.float32))
        host = SyntheticSafetyVectorEnv(env_num=n, obs_dim=8, act_dim=2, episode_len=EPISODE_LEN, seed=1 + i)
        pol, buf = Pol(eng), HipVectorReplayBuffer(eng, n * 2 * EPISODE_LEN, n)
        if path == "lock_step":
            cols.append(FastCollector(pol, host, buf, device_actor=True))
        else:
            envs.append(DeviceLinear(eng, like=host, seed=1 + i))
            cols.append(DeviceCollector(pol, envs[-1], buf))
        engs.append(eng)
    group = EngineGroup(engs) if path != "solo_seq" else None

    class Seq:
        collectors = cols

        def collect(self, n_episode):
            return [c.collect(n_episode=n_episode) for c in cols]
    col = Seq() if path == "solo_seq" else GroupDeviceCollector(cols) if path == "grouped" else GroupCollector(group, cols)
    return engs, envs, group, col


def timed_group(col, n, calls):
    def reset():
        for c in col.collectors:
            c.reset_buffer()
    reset()
    col.collect(n)
    reset()
    rows, t0 = 0, time.perf_counter()
    for _ in range(calls):
        rows += sum(st["n/st"] for st in col.collect(n))
        reset()
    return rows, time.perf_counter() - t0


def summary(rates):
    return dict(median=float(np.median(rates)), spread=float(np.max(rates) - np.min(rates)), rounds=[float(r) for r in rates])


def solo_ab(a):
    """the solo device collect of this tree against the tree at a.ab_tree: each tool in a process of its own, one round per process,
    alternating; per (hidden, env_num) the rates of both"""
    tools = {"tree": os.path.abspath(__file__), "other": os.path.join(os.path.abspath(a.ab_tree), "tools", "bench_device_collect.py")}
    rates = {}
    for _ in range(a.rounds):
        for who, tool in tools.items():
            with tempfile.TemporaryDirectory() as tmp:
                out = os.path.join(tmp, "r.json")
                env = {k: v for k, v in os.environ.items() if k != "FSRL_HIP_LIB"}
                subprocess.run([sys.executable, tool, "--rounds", "1", "--calls", str(a.calls), "--envs", a.envs, "--hidden", a.hidden, "--out", out],
                               check=True, stdout=subprocess.DEVNULL, env=env, cwd=os.path.dirname(os.path.dirname(tool)), timeout=600)
                with open(out) as f:
                    for c in json.load(f)["configs"]:
                        rates.setdefault((shape_name(c), c["env_num"]), {}).setdefault(who, []).append(c["device"]["median"])
    res = []
    for (hidden, n), r in sorted(rates.items(), reverse=True):
        res.append(dict(hidden=[int(w) for w in hidden.split("x")], env_num=n, tree=summary(r["tree"]), other=summary(r["other"])))
        print(json.dumps(res[-1]), flush=True)
    return res


def main_groups(a):
    paths = ("grouped", "solo_seq", "lock_step")
    result = dict(metric="aggregate env-steps/s of k seeds' collects on one GPU, training mode, linear env obs 8 / act 2, episode length 300, "
                         "on-policy contexts", rounds=a.rounds, calls=a.calls, configs=[])
    for hidden in parse_hidden(a.hidden):
        for n in (int(e) for e in a.envs.split(",")):
            for k in (int(x) for x in a.ks.split(",")):
                objs = {p: setup_group(p, hidden, n, k) for p in paths}
                rates = {p: [] for p in paths}
                for _ in range(a.rounds):
                    for p in paths:
                        rows, dt = timed_group(objs[p][3], n, a.calls)
                        rates[p].append(rows / dt)
                cfg = dict(hidden=hidden_list(hidden), env_num=n, k=k, launches_per_collect=objs["grouped"][3].last_launches)
                for p in paths:
                    cfg[p] = summary(rates[p])
                result["configs"].append(cfg)
                print(json.dumps(cfg), flush=True)
                for engs, envs, group, col in objs.values():
                    for env in envs:
                        env.close()
                    if group is not None:
                        group.close()
                    for eng in engs:
                        eng.close()
    if a.ab_tree:
        result["solo_tree_vs_other"] = dict(what="solo fsrl_collect_device, env-steps/s: this tree against the tree it was measured next to (the "
                                                 "parent commit), processes alternating, one round per process", configs=solo_ab(a))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(dict(device_collect_group=[(shape_name(c), c["env_num"], c["k"], round(c["grouped"]["median"]), round(c["solo_seq"]["median"]),
                                                 round(c["lock_step"]["median"])) for c in result["configs"]])))
    return result


class EvalPol(Pol):
    training = False


def setup_eval(hidden, n, algo):
    """a real agent (the host path needs its torch actor) and the three collectors of an evaluation, each over a device env of its own"""
    import tempfile as tf
    from fsrl_amd.agent import PPOLagAgent, SACLagAgent
    from fsrl_amd.utils import BaseLogger
    host = SyntheticSafetyVectorEnv(env_num=n, obs_dim=8, act_dim=2, episode_len=EPISODE_LEN, seed=1)
    Agent = SACLagAgent if algo == "sacl" else PPOLagAgent
    agent = Agent(host, BaseLogger(tf.mkdtemp(prefix="fsrl_amd_bench_"), name="eval"), cost_limit=10, device="cuda:0", seed=1,
                  hidden_sizes=tuple(hidden_list(hidden)), training_num=n, buffer_size=n * 2 * EPISODE_LEN)
    pol = agent.policy
    pol.eval()
    envs = [DeviceLinear(pol, like=host, seed=1) for _ in range(3)]
    buf = HipVectorReplayBuffer(pol.engine, n * 2 * EPISODE_LEN, n)
    cols = dict(evaluate=DeviceCollector(pol, envs[0]), stepped=FastCollector(pol, envs[1]), collect=DeviceCollector(pol, envs[2], buf))
    return agent, envs, cols


def timed_eval(col, n, calls):
    col.collect(n_episode=n)
    rows, eps, t0 = 0, 0, time.perf_counter()
    for _ in range(calls):
        st = col.collect(n_episode=n)
        rows += st["n/st"]; eps += st["n/ep"]
        col.reset_buffer()
    return rows, eps, time.perf_counter() - t0


def main_eval(a):
    assert a.algo in ("onpolicy", "sacl"), "--eval: PPOLagAgent and SACLagAgent (the default), or --algo sacl alone"
    paths = ("evaluate", "stepped", "collect")
    algos = ("onpolicy", "sacl") if a.algo == "onpolicy" else (a.algo, )
    result = dict(metric="an evaluation of env_num episodes, policy in eval mode, linear env obs 8 / act 2, episode length 300: episodes/s and "
                         "env-steps/s", rounds=a.rounds, calls=a.calls, configs=[], groups=[])
    for algo, hidden, n in ((al, h, int(e)) for al in algos for h in parse_hidden(a.hidden) for e in a.envs.split(",")):
        agent, envs, cols = setup_eval(hidden, n, algo)
        steps, eps = {p: [] for p in paths}, {p: [] for p in paths}
        for _ in range(a.rounds):
            for p in paths:
                rows, ne, dt = timed_eval(cols[p], n, a.calls)
                steps[p].append(rows / dt); eps[p].append(ne / dt)
        cfg = dict(algo=algo, hidden=hidden_list(hidden), env_num=n, launches_per_evaluation=cols["evaluate"].last_launches)
        for p in paths:
            cfg[p] = dict(env_steps_per_s=summary(steps[p]), episodes_per_s=summary(eps[p]))
        result["configs"].append(cfg)
        print(json.dumps(cfg), flush=True)
        for env in envs:
            env.close()
        agent.policy.engine.close()
    if a.ks and "onpolicy" in algos:
        from fsrl_amd.data import GroupDeviceCollector
        for hidden in parse_hidden(a.hidden):
            for n in (int(e) for e in a.envs.split(",")):
                for k in (int(x) for x in a.ks.split(",")):
                    sets = {}
                    for p in ("grouped", "solo_seq"):
                        engs, envs, cols = [], [], []
                        for i in range(k):
                            eng = Engine(EngineConfig(obs_dim=8, act_dim=2, env_num=n, buffer_size=n * 2 * EPISODE_LEN, **hidden_kw(hidden)), device=0)
                            eng.set_params((0.1 * np.random.default_rng(i).standard_normal(eng.n_params)).astype(np.float32))
                            host = SyntheticSafetyVectorEnv(env_num=n, obs_dim=8, act_dim=2, episode_len=EPISODE_LEN, seed=1 + i)
                            envs.append(DeviceLinear(eng, like=host, seed=1 + i))
                            cols.append(DeviceCollector(EvalPol(eng), envs[-1]))
                            engs.append(eng)

                        class Seq:
                            collectors = cols

                            def collect(self, n_episode, _cols=cols):
                                return [c.collect(n_episode=n_episode) for c in _cols]
                        sets[p] = (engs, envs, GroupDeviceCollector(cols) if p == "grouped" else Seq())
                    rates = {p: [] for p in sets}
                    for _ in range(a.rounds):
                        for p in sets:
                            rows, dt = timed_group(sets[p][2], n, a.calls)
                            rates[p].append(rows / dt)
                    cfg = dict(hidden=hidden_list(hidden), env_num=n, k=k, grouped=summary(rates["grouped"]), solo_seq=summary(rates["solo_seq"]))
                    result["groups"].append(cfg)
                    print(json.dumps(cfg), flush=True)
                    for engs, envs, _ in sets.values():
                        for env in envs:
                            env.close()
                        for eng in engs:
                            eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(dict(device_eval=[(c["algo"], shape_name(c), c["env_num"]) + tuple(round(c[p]["env_steps_per_s"]["median"]) for p in paths)
                                       for c in result["configs"]])))
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--algo", choices=["onpolicy", "sacl", "ddpgl", "cvpo"], default="onpolicy")
    ap.add_argument("--update-per-step", type=float, default=0.1, help="replay legs: updates per collected env step in the loop figure")
    ap.add_argument("--batch-size", type=int, default=256, help="replay legs: rows per update in the loop figure")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--envs", default="20,64")
    ap.add_argument("--hidden", default="256,64")
    ap.add_argument("--out", default=None)
    ap.add_argument("--ks", default=None, help="group sizes, e.g. 1,2,4,8: measure grouped seeds (on-policy) instead")
    ap.add_argument("--ab-tree", default=None, help="with --ks: another built checkout whose solo device collect this tree's is held against")
    ap.add_argument("--eval", action="store_true", help="measure evaluations: the store-less device evaluation, the host-stepped path it "
                                                        "replaces and a storing collect; with --ks also grouped against solo evaluations")
    ap.add_argument("--layered", action="store_true", help="the four legs on layered shapes (--hidden entries written with x; default "
                                                           "256x256x256,64x48x32) in one process, one --out file")
    a = ap.parse_args()
    if a.layered:
        return main_layered(a)
    if a.eval:
        return main_eval(a)
    if a.ks:
        return main_groups(a)
    return main_solo(a)


def main_layered(a):
    if "x" not in a.hidden:
        a.hidden = "256x256x256,64x48x32"
    assert all(isinstance(h, tuple) for h in parse_hidden(a.hidden)), "--layered: every --hidden entry is written with x"
    out, a.out = a.out, None
    replay = a.algo if a.algo != "onpolicy" else "sacl"
    result = dict(metric="layered device collects and evaluations (fsrl_collect_device_layered / fsrl_evaluate_device_layered) against the "
                         "lock-step and stepped paths, linear env obs 8 / act 2, episode length 300; see the legs", rounds=a.rounds, calls=a.calls)
    a.algo, ks = "onpolicy", a.ks or "1,2,4,8"
    a.ks = None
    result["collect"] = main_solo(a)
    a.algo = replay
    result["collect_replay"] = main_solo(a)
    a.algo, a.ks = "onpolicy", ks
    result["groups"] = main_groups(a)
    result["eval"] = main_eval(a)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
    return result


def main_solo(a):
    paths = ("device", "in_process", "stepped")
    result = dict(metric="env-steps/s of a collect loop, training mode, linear env obs 8 / act 2, episode length 300", rounds=a.rounds,
                  calls=a.calls, configs=[])
    if a.algo != "onpolicy":
        result.update(algo=a.algo, update_per_step=a.update_per_step, batch_size=a.batch_size)
    for hidden in parse_hidden(a.hidden):
        for n in (int(e) for e in a.envs.split(",")):
            objs = {p: setup(p, hidden, n, a.algo) for p in paths}
            rates = {p: [] for p in paths}
            for _ in range(a.rounds):
                for p in paths:
                    rows, dt = timed(objs[p][2], n, a.calls)
                    rates[p].append(rows / dt)
            cfg = dict(hidden=hidden_list(hidden), env_num=n)
            for p in paths:
                cfg[p] = dict(median=float(np.median(rates[p])), spread=float(np.max(rates[p]) - np.min(rates[p])), rounds=[float(r) for r in rates[p]])
            # (a) per vector step and per launch: the default steps per launch, and the whole collect in one launch
            eng, env, col = objs["device"]
            for name, steps in (("default", 0), ("one_launch", EPISODE_LEN)):
                col.max_steps_per_launch = steps
                per_step, per_launch, launches = [], [], 0
                for _ in range(a.rounds):
                    rows, dt = timed(col, n, a.calls)
                    launches = col.last_launches
                    per_step.append(dt / a.calls / EPISODE_LEN * 1e6)
                    per_launch.append(dt / a.calls / launches * 1e6)
                cfg["device_" + name] = dict(launches_per_collect=launches, us_per_vector_step=float(np.median(per_step)),
                                             us_per_launch=float(np.median(per_launch)),
                                             us_per_vector_step_spread=float(np.max(per_step) - np.min(per_step)))
            col.max_steps_per_launch = 0
            if a.algo != "onpolicy":
                # the loop a user runs: collect + updates, the two collectors alternating inside a round
                loop, per_collect = {p: [] for p in ("device", "in_process")}, 0
                for _ in range(a.rounds):
                    for p in loop:
                        rows, dt, per_collect = timed_loop(objs[p][0], objs[p][2], n, a.calls, a.algo, a.update_per_step, a.batch_size)
                        loop[p].append(rows / dt)
                cfg["loop"] = dict(updates_per_collect=per_collect)
                for p in loop:
                    cfg["loop"][p] = dict(median=float(np.median(loop[p])), spread=float(np.max(loop[p]) - np.min(loop[p])),
                                          rounds=[float(r) for r in loop[p]])
            result["configs"].append(cfg)
            print(json.dumps(cfg), flush=True)
            for eng, env, col in objs.values():
                if env is not None:
                    env.close()
                eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(dict(device_collect=[(shape_name(c), c["env_num"], round(c["device"]["median"]), round(c["in_process"]["median"]),
                                           round(c["stepped"]["median"])) for c in result["configs"]])))
    if a.algo != "onpolicy":
        print(json.dumps(dict(algo=a.algo, collect_plus_updates=[(shape_name(c), c["env_num"], c["loop"]["updates_per_collect"],
                                                                  round(c["loop"]["device"]["median"]), round(c["loop"]["in_process"]["median"]))
                                                                 for c in result["configs"]])))
    return result


if __name__ == "__main__":
    main()
