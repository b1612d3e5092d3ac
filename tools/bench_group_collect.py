#!/usr/bin/env python
"""Lock-step collection of a PPO-Lagrangian group (GroupCollector -> fsrl_group_collect_step) against collecting the seeds one after
the other.  k members of 256 x 256, 20 in-process SyntheticSafetyVectorEnv envs each (obs 8, act 2, episodes of 300 steps, one seed per
member).  For every k, in one process and alternating `--rounds` times, aggregate env-steps/s of:
  seq_ungrouped  k ungrouped engines, each FastCollector.collect in turn with its own resident actor (the fair baseline);
  seq_grouped    the members of a group, each FastCollector.collect in turn (what examples/train_multi_seed.py --grouped did: a grouped
                 member has no resident actor, one launch per vector step);
  lockstep       GroupCollector.collect on the same group.
Also: us per grouped actor call at k x 20 rows against one member's 20-row resident call, resident launches per lock-step collect, and
a collect + grouped update loop (aggregate env-steps/s and updates/s).  Prints ONE JSON line.

--algo sacl | ddpgl | cvpo: the replay agents' collect group (GroupCollector over an EngineCollectGroup -> fsrl_collect_group_step).
Modes: seq_ungrouped (each member's own FastCollector with its own resident actor) and lockstep; the same per-call figures and
launches per collect; the loop is lock-step collection + round(0.2 * n/st) updates per seed through SACPolicyGroup / CVPOPolicyGroup
(DDPG-Lag: each seed's own updates, one seed after the other).

--hidden 256x256x256 (--algo sacl | ddpgl | cvpo): layered members.  Their collect group has no resident kernel: a lock-step vector step is
one launch sequence (L + 2 launches) for all members against k (L + 2) member by member, and launches_per_collect counts requests.
With --hidden the DDPG-Lag loop updates through DDPGPolicyGroup as the SAC-Lag loop does through SACPolicyGroup.

--algo cpo | trpol: trust-region seeds in the same collect group (on-policy members: the PPO-Lag group's actor kernel, launched from a
group whose members keep their own streams), fused or --hidden.  The same modes and figures; the loop is lock-step collection + ONE
TrustPolicyGroup.update(repeat=4) per collect (the seeds' own full-batch updates on a thread each) + reset_buffer.

--workers W [--busy-us U] [--native 0|1] (every --algo): the members' envs are worker-process envs (one ShmemVectorEnv of W workers per
member, an env step costing U microseconds of host time) and the legs are
  interpreted     GroupCollector(native_loop=False): one library call per vector step, the members' envs stepped one after the other;
  native          GroupCollector(native_loop=True): the whole collect in one library call (fsrl_group_collect_episodes /
                  fsrl_collect_episodes_group), the members' workers stepping at the same time;
  seq_native      k ungrouped seeds, each one's own FastCollector (fsrl_collect_episodes) in turn.
--native 0 / 1 runs the interpreted / the native leg only.  k x W is capped at 14: the two sets of envs (grouped, ungrouped) never step
at the same time, and a 16-CPU box keeps two CPUs for the collector.

    python tools/bench_group_collect.py [--algo ppol] [--ks 1,2,4,8] [--rounds 3] [--hidden 256x256x256] [--out profiles/x.json]
    python tools/bench_group_collect.py --algo ppol --workers 2 --busy-us 100 --ks 1,2,4 --out profiles/group_episodes_collect.json
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _agents(k, envs, first_seed, device, algo="ppol", hidden=None, workers=0, busy_us=0.0):
    from fsrl_amd.agent import CPOAgent, CVPOAgent, DDPGLagAgent, PPOLagAgent, SACLagAgent, TRPOLagAgent
    Agent = {"ppol": PPOLagAgent, "sacl": SACLagAgent, "ddpgl": DDPGLagAgent, "cvpo": CVPOAgent, "cpo": CPOAgent,
             "trpol": TRPOLagAgent}[algo]
    from fsrl_amd.data import FastCollector, HipVectorReplayBuffer
    from fsrl_amd.env import ShmemVectorEnv, SyntheticSafetyVectorEnv
    from fsrl_amd.utils import BaseLogger
    agents, cols, bufs = [], [], []
    for s in range(first_seed, first_seed + k):
        if workers:
            env = ShmemVectorEnv(env_num=envs, workers=workers, obs_dim=8, act_dim=2, episode_len=300, seed=s, busy_us=busy_us)
        else:
            env = SyntheticSafetyVectorEnv(env_num=envs, obs_dim=8, act_dim=2, episode_len=300, seed=s)
        ag = Agent(env, BaseLogger(tempfile.mkdtemp(prefix=f"fsrl_amd_bgc{s}_"), name=f"s{s}"), cost_limit=10.0, device=device,
                   seed=s, hidden_sizes=hidden or (256, 256), training_num=envs)
        ag.policy.train()
        buf = HipVectorReplayBuffer(ag.policy.engine, None, envs)
        agents.append(ag); bufs.append(buf); cols.append(FastCollector(ag.policy, env, buf, exploration_noise=True, device_actor=True))
    return agents, cols, bufs


def _seq(cols, n_ep):
    steps = 0
    for c in cols:
        steps += c.collect(n_episode=n_ep)["n/st"]
        c.reset_buffer(keep_statistics=True)
    return steps


def _lock(gc, cols, n_ep):
    steps = sum(st["n/st"] for st in gc.collect(n_episode=n_ep))
    for c in cols:
        c.reset_buffer(keep_statistics=True)
    return steps


def _call_us(fn, n):
    for _ in range(20):
        fn()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    return (time.perf_counter() - t) / n * 1e6


def _emit(a, res):
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


def _workers(a):
    """--workers: the members' envs are worker processes; interpreted / native lock-step collection and the seeds' own native collects"""
    from fsrl_amd.data import GroupCollector
    from fsrl_amd.engine import EngineCollectGroup
    from fsrl_amd.policy import PolicyGroup
    n_ep = a.envs
    res = {"algo": a.algo, "envs": a.envs, "workers": a.workers, "busy_us": a.busy_us,
           "hidden": "x".join(str(w) for w in a.hidden) if a.hidden else 256, "rounds": a.rounds, "k": {}}
    legs = ["interpreted", "native", "seq_native"] if a.native is None else [["interpreted", "native"][a.native]]
    for k in [int(x) for x in a.ks.split(",")]:
        assert k * a.workers <= 14, f"k x workers = {k * a.workers}: at most 14 worker processes step at a time on a 16-CPU box"
        solo_agents, solo_cols = [], []
        if "seq_native" in legs:
            solo_agents, solo_cols, _ = _agents(k, a.envs, 0, a.device, a.algo, a.hidden, a.workers, a.busy_us)
        grp_agents, grp_cols, _ = _agents(k, a.envs, 0, a.device, a.algo, a.hidden, a.workers, a.busy_us)
        if a.algo == "ppol":
            group = PolicyGroup([ag.policy for ag in grp_agents])
        else:
            group = EngineCollectGroup([ag.policy.engine for ag in grp_agents])
        gcs = {"interpreted": GroupCollector(group, grp_cols, native_loop=False), "native": GroupCollector(group, grp_cols, native_loop=True)}
        run = {m: (lambda m=m: _seq(solo_cols, n_ep) if m == "seq_native" else _lock(gcs[m], grp_cols, n_ep)) for m in legs}
        t = {m: [] for m in legs}
        for m in legs:                                            # warm-up: code loading, first launches, the workers' first steps
            run[m]()
        for _ in range(a.rounds):
            for m in legs:
                t0 = time.perf_counter()
                st = run[m]()
                t[m].append(st / (time.perf_counter() - t0))
        out = {m: round(float(np.median(v))) for m, v in t.items()}
        out["all"] = {m: [round(x) for x in v] for m, v in t.items()}
        out["spread"] = {m: round(max(v) - min(v)) for m, v in t.items()}
        if "native" in out and "interpreted" in out:
            out["native_over_interpreted"] = round(out["native"] / out["interpreted"], 3)
        if "native" in out and "seq_native" in out:
            out["native_over_seq_native"] = round(out["native"] / out["seq_native"], 3)
        out["rows_per_member_per_collect"] = n_ep * 300
        res["k"][str(k)] = out
        group.close()
        for ag in solo_agents + grp_agents:
            ag.policy.engine.close()
        for c in solo_cols + grp_cols:
            c.env.close()
        print(f"k={k}: {json.dumps(out)}", file=sys.stderr, flush=True)
    _emit(a, res)


def _replay(a):
    """--algo sacl / ddpgl / cvpo: the collect group of the replay agents; --algo cpo / trpol: the same object over on-policy members"""
    from fsrl_amd.data import GroupCollector
    from fsrl_amd.engine import EngineCollectGroup
    from fsrl_amd.policy import CVPOPolicyGroup, DDPGPolicyGroup, SACPolicyGroup, TrustPolicyGroup
    trust = a.algo in ("cpo", "trpol")
    n_ep = a.envs
    res = {"algo": a.algo, "envs": a.envs, "hidden": "x".join(str(w) for w in a.hidden) if a.hidden else 256, "rounds": a.rounds, "k": {}}
    for k in [int(x) for x in a.ks.split(",")]:
        solo_agents, solo_cols, _ = _agents(k, a.envs, 0, a.device, a.algo, a.hidden)
        grp_agents, grp_cols, grp_bufs = _agents(k, a.envs, 0, a.device, a.algo, a.hidden)
        cg = EngineCollectGroup([ag.policy.engine for ag in grp_agents])
        gc = GroupCollector(cg, grp_cols)
        t = {"seq_ungrouped": [], "lockstep": []}
        launches, collects = 0, 0
        _seq(solo_cols, n_ep); _lock(gc, grp_cols, n_ep)          # warm-up: code loading, first launches
        for _ in range(a.rounds):
            for mode in t:
                l0 = cg.actor_resident_stats()["launches"]
                t0 = time.perf_counter()
                if mode == "seq_ungrouped":
                    st = _seq(solo_cols, n_ep)
                else:
                    st = _lock(gc, grp_cols, n_ep)
                    launches += cg.actor_resident_stats()["launches"] - l0
                    collects += 1
                t[mode].append(st / (time.perf_counter() - t0))
        out = {m: round(float(np.median(v))) for m, v in t.items()}
        out["all"] = {m: [round(x) for x in v] for m, v in t.items()}
        out["spread"] = {m: round(max(v) - min(v)) for m, v in t.items()}
        out["lockstep_over_seq_ungrouped"] = round(out["lockstep"] / out["seq_ungrouped"], 3)
        out["launches_per_collect"] = round(launches / max(collects, 1), 2)
        out["rows_per_member_per_collect"] = n_ep * 300
        rng = np.random.default_rng(0)
        obs = rng.standard_normal((a.envs, 8)).astype(np.float32)
        e0 = solo_agents[0].policy.engine
        out["us_member_call"] = round(_call_us(lambda: e0.collect_step(None, obs, False, 1), a.calls), 2)
        e0.actor_release()
        out["us_group_call"] = round(_call_us(lambda: cg.collect_step([None] * k, [obs] * k, False, 1), a.calls), 2)
        cg.actor_release()
        out["group_call_over_member_call"] = round(out["us_group_call"] / out["us_member_call"], 3)
        # collect + update, the training loop's shape (examples/train_multi_seed.py --grouped): update_per_step 0.2
        group_cls = {"sacl": SACPolicyGroup, "cvpo": CVPOPolicyGroup, "ddpgl": DDPGPolicyGroup if a.hidden else None,
                     "cpo": TrustPolicyGroup, "trpol": TrustPolicyGroup}[a.algo]
        group = group_cls([ag.policy for ag in grp_agents], **({"collect_group": cg} if trust else {})) if group_cls else None
        steps, updates = 0, 0
        t0 = time.perf_counter()
        for _ in range(2):
            sts = gc.collect(n_episode=n_ep)
            n = []
            for ag, st in zip(grp_agents, sts):
                ag.policy.pre_update_fn(stats_train=st)
                steps += st["n/st"]
                n.append(1 if trust else round(0.2 * st["n/st"]))
            if trust:
                group.update(grp_bufs, batch_size=99999, repeat=4)
                for c in grp_cols:
                    c.reset_buffer(keep_statistics=True)
            elif group is not None:
                group.update(grp_bufs, batch_size=256, n_updates=n)
            else:
                for ag, buf, n_i in zip(grp_agents, grp_bufs, n):
                    for _ in range(n_i):
                        ag.policy.update(256, buf)
            for ag, st in zip(grp_agents, sts):
                ag.policy.post_update_fn(stats_train=st)
            updates += sum(n)
        dt = time.perf_counter() - t0
        out["loop_env_steps_per_s"] = round(steps / dt)
        out["loop_updates_per_s"] = round(updates / dt, 1)
        res["k"][str(k)] = out
        cg.close()
        if group is not None:
            group.close()
        for ag in solo_agents + grp_agents:
            ag.policy.engine.close()
        print(f"k={k}: {json.dumps(out)}", file=sys.stderr, flush=True)
    _emit(a, res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--algo", choices=("ppol", "sacl", "ddpgl", "cvpo", "cpo", "trpol"), default="ppol")
    ap.add_argument("--ks", default="1,2,4,8")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--envs", type=int, default=20)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--hidden", default=None, type=lambda t: tuple(int(w) for w in t.lower().split("x")),
                    help="--algo sacl | ddpgl | cvpo | cpo | trpol: hidden layers instead of 256x256, e.g. 256x256x256 or 64x48x32 (layered members)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file (profiles/...)")
    ap.add_argument("--workers", type=int, default=0, help="worker processes per member's env (ShmemVectorEnv); 0: in-process envs")
    ap.add_argument("--busy-us", type=float, default=0.0, help="--workers: host time of one env step, microseconds")
    ap.add_argument("--native", type=int, choices=(0, 1), default=None,
                    help="--workers: only the interpreted (0) or the native (1) lock-step leg; default: both and the seeds' own collects")
    a = ap.parse_args()
    assert a.hidden is None or a.algo != "ppol", "--hidden: the layered collect groups (--algo sacl | ddpgl | cvpo | cpo | trpol)"
    if a.workers:
        return _workers(a)
    if a.algo != "ppol":
        return _replay(a)
    from fsrl_amd.data import GroupCollector
    from fsrl_amd.policy import PolicyGroup
    n_ep = a.envs
    res = {"envs": a.envs, "hidden": 256, "rounds": a.rounds, "k": {}}
    for k in [int(x) for x in a.ks.split(",")]:
        solo_agents, solo_cols, _ = _agents(k, a.envs, 0, a.device)
        grp_agents, grp_cols, grp_bufs = _agents(k, a.envs, 0, a.device)
        group = PolicyGroup([ag.policy for ag in grp_agents])
        eg = group.group
        gc = GroupCollector(group, grp_cols)
        t = {"seq_ungrouped": [], "seq_grouped": [], "lockstep": []}
        launches, collects = 0, 0
        _seq(solo_cols, n_ep); _seq(grp_cols, n_ep); _lock(gc, grp_cols, n_ep)          # warm-up: code loading, first launches
        for _ in range(a.rounds):
            for mode in t:
                l0 = eg.actor_resident_stats()["launches"]
                t0 = time.perf_counter()
                if mode == "seq_ungrouped":
                    st = _seq(solo_cols, n_ep)
                elif mode == "seq_grouped":
                    st = _seq(grp_cols, n_ep)
                else:
                    st = _lock(gc, grp_cols, n_ep)
                    launches += eg.actor_resident_stats()["launches"] - l0
                    collects += 1
                t[mode].append(st / (time.perf_counter() - t0))
        out = {m: round(float(np.median(v))) for m, v in t.items()}
        out["all"] = {m: [round(x) for x in v] for m, v in t.items()}
        out["lockstep_over_seq_ungrouped"] = round(out["lockstep"] / out["seq_ungrouped"], 3)
        out["launches_per_collect"] = round(launches / max(collects, 1), 2)
        out["rows_per_member_per_collect"] = n_ep * 300
        # one grouped actor call (k x 20 rows) against one member's own resident 20-row call
        rng = np.random.default_rng(0)
        obs = rng.standard_normal((a.envs, 8)).astype(np.float32)
        e0 = solo_agents[0].policy.engine
        out["us_member_call"] = round(_call_us(lambda: e0.collect_step(None, obs, False, 1), a.calls), 2)
        e0.actor_release()
        out["us_group_call"] = round(_call_us(lambda: eg.collect_step([None] * k, [obs] * k, False, 1), a.calls), 2)
        eg.actor_release()
        out["group_call_over_member_call"] = round(out["us_group_call"] / out["us_member_call"], 3)
        # collect + grouped update, the training loop's shape
        steps, updates = 0, 0
        t0 = time.perf_counter()
        for _ in range(2):
            sts = gc.collect(n_episode=n_ep)
            for ag, st in zip(grp_agents, sts):
                ag.policy.pre_update_fn(stats_train=st)
                steps += st["n/st"]
            group.update(grp_bufs, batch_size=256, repeat=4)
            updates += k
            for c in grp_cols:
                c.reset_buffer(keep_statistics=True)
        dt = time.perf_counter() - t0
        out["loop_env_steps_per_s"] = round(steps / dt)
        out["loop_updates_per_s"] = round(updates / dt, 1)
        res["k"][str(k)] = out
        group.close()
        for ag in solo_agents + grp_agents:
            ag.policy.engine.close()
        print(f"k={k}: {json.dumps(out)}", file=sys.stderr, flush=True)
    _emit(a, res)


if __name__ == "__main__":
    main()
