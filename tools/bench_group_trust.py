#!/usr/bin/env python
"""Trust-region seeds on one GPU: TrustPolicyGroup.update (the members' own full-batch updates on a worker thread each, beside each
other) against the same members updated one after the other and against one context alone.  Nothing is launched jointly on the update
side, so this measures how much of one member's read-back gaps another member's kernels fill -- not a grouped kernel.

BASELINE configs[2] shape: obs 60, act 2, 256 x 256, CPO (or --algo trpol), 20 envs x 300-step episodes = 6 000 rows per member,
repeat 4, one minibatch.  Per k in --ks, alternating `--rounds` times inside one process, aggregate updates/s of
  group        TrustPolicyGroup.update over the k members;
  sequential   policy.update(0, buffer) of the same k members, one after the other (what the parent commit can do from one thread);
  alone        one more context of the same shape updating on its own (k = 1 of `sequential`, measured in the same process);
and the training loop's shape, twice each: lock-step collect + pre_update_fn + group.update + reset_buffer against each member's own
collect + its own update (env-steps/s and updates/s).  Medians, all samples and the spread (max - min) are reported.

Every k runs in a child process of its own under --leg-timeout seconds (a leg that hangs or fails is reported as such and the
others still run).  Prints ONE JSON line and writes a copy to --out (default profiles/trust_group_update.json).

    python tools/bench_group_trust.py [--algo cpo] [--ks 1,2,4,8] [--rounds 3] [--updates 3] [--hidden 256x256]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _members(k, a, first_seed):
    from fsrl_amd.agent import CPOAgent, TRPOLagAgent
    from fsrl_amd.data import FastCollector, HipVectorReplayBuffer
    from fsrl_amd.env import SyntheticSafetyVectorEnv
    from fsrl_amd.env.synthetic import stable_coupling
    from fsrl_amd.utils import BaseLogger
    Agent = {"cpo": CPOAgent, "trpol": TRPOLagAgent}[a.algo]
    agents, cols, bufs = [], [], []
    for s in range(first_seed, first_seed + k):
        # wide observations: the random part of the dynamics scaled so that 300-step episodes stay bounded (synthetic.py)
        env = SyntheticSafetyVectorEnv(env_num=a.envs, obs_dim=a.obs_dim, act_dim=2, episode_len=a.episode_len, seed=s,
                                       coupling=stable_coupling(a.obs_dim))
        ag = Agent(env, BaseLogger(tempfile.mkdtemp(prefix=f"fsrl_amd_bgt{s}_"), name=f"s{s}"), cost_limit=10.0, device=a.device,
                   seed=s, hidden_sizes=a.hidden, training_num=a.envs)
        ag.policy.train()
        buf = HipVectorReplayBuffer(ag.policy.engine, None, a.envs)
        agents.append(ag); bufs.append(buf); cols.append(FastCollector(ag.policy, env, buf, exploration_noise=True, device_actor=True))
    return agents, cols, bufs


def _summary(samples):
    return {"median": round(float(np.median(samples)), 2), "all": [round(float(x), 2) for x in samples],
            "spread": round(float(max(samples) - min(samples)), 2)}


def leg(a, k):
    """one k, in this process"""
    from fsrl_amd.data import GroupCollector
    from fsrl_amd.engine import EngineCollectGroup
    from fsrl_amd.policy import TrustPolicyGroup
    agents, cols, bufs = _members(k, a, 0)
    lone, lone_cols, lone_bufs = _members(1, a, 100)
    cg = EngineCollectGroup([ag.policy.engine for ag in agents])
    gc = GroupCollector(cg, cols)
    group = TrustPolicyGroup([ag.policy for ag in agents], collect_group=cg)
    n_ep = a.envs
    rows = [st["n/st"] for st in gc.collect(n_episode=n_ep)]
    lone_cols[0].collect(n_episode=n_ep)
    for ag in agents + lone:
        ag.policy.pre_update_fn(stats_train={"cost": 12.0})

    def run_group():
        group.update(bufs, batch_size=99999, repeat=a.repeat)
        return k

    def run_seq():
        for ag, b in zip(agents, bufs):
            ag.policy.update(0, b, batch_size=99999, repeat=a.repeat)
        return k

    def run_alone():
        lone[0].policy.update(0, lone_bufs[0], batch_size=99999, repeat=a.repeat)
        return 1

    modes = {"group": run_group, "sequential": run_seq, "alone": run_alone}
    for fn in modes.values():                                   # warm-up: code loading, working sets, the thread pool
        fn()
    t = {m: [] for m in modes}
    for _ in range(a.rounds):
        for m, fn in modes.items():
            t0 = time.perf_counter()
            n = sum(fn() for _ in range(a.updates))
            t[m].append(n / (time.perf_counter() - t0))
    out = {"rows_per_member": rows, "updates_per_s": {m: _summary(v) for m, v in t.items()}}
    med = {m: out["updates_per_s"][m]["median"] for m in modes}
    out["group_over_sequential"] = round(med["group"] / med["sequential"], 3)
    out["group_over_alone"] = round(med["group"] / med["alone"], 3)      # the k members' aggregate against ONE context's rate
    # the training loop's shape: collect, pre_update_fn, update, reset_buffer
    loops = {"lockstep_group": [], "member_by_member": []}
    for _ in range(2):
        for mode in loops:
            for c in cols:
                c.reset_buffer(keep_statistics=True)
            t0 = time.perf_counter()
            sts = gc.collect(n_episode=n_ep) if mode == "lockstep_group" else [c.collect(n_episode=n_ep) for c in cols]
            for ag, st in zip(agents, sts):
                ag.policy.pre_update_fn(stats_train=st)
            if mode == "lockstep_group":
                group.update(bufs, batch_size=99999, repeat=a.repeat)
            else:
                for ag, b in zip(agents, bufs):
                    ag.policy.update(0, b, batch_size=99999, repeat=a.repeat)
            dt = time.perf_counter() - t0
            loops[mode].append((sum(st["n/st"] for st in sts) / dt, k / dt))
    out["loop"] = {m: {"env_steps_per_s": [round(x[0]) for x in v], "updates_per_s": [round(x[1], 2) for x in v]} for m, v in loops.items()}
    group.close(); cg.close()
    for ag in agents + lone:
        ag.policy.engine.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--algo", choices=("cpo", "trpol"), default="cpo")
    ap.add_argument("--ks", default="1,2,4,8")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--updates", type=int, default=3, help="updates per member in one timed sample")
    ap.add_argument("--repeat", type=int, default=4)
    ap.add_argument("--envs", type=int, default=20)
    ap.add_argument("--episode-len", type=int, default=300)
    ap.add_argument("--obs-dim", type=int, default=60)
    ap.add_argument("--hidden", default=(256, 256), type=lambda s: tuple(int(w) for w in s.lower().split("x")))
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--leg-timeout", type=float, default=240.0, help="seconds for one k (its own child process)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trust_group_update.json"))
    ap.add_argument("--leg", type=int, default=0, help=argparse.SUPPRESS)       # child: run this k here, print its JSON
    a = ap.parse_args()
    if a.leg:
        print("LEG " + json.dumps(leg(a, a.leg)), flush=True)
        return
    res = {"algo": a.algo, "obs_dim": a.obs_dim, "hidden": "x".join(str(w) for w in a.hidden), "envs": a.envs,
           "episode_len": a.episode_len, "repeat": a.repeat, "rounds": a.rounds, "updates_per_sample": a.updates, "k": {}}
    passthrough = [x for x in sys.argv[1:]]
    for k in [int(x) for x in a.ks.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), *passthrough, "--leg", str(k)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.leg_timeout)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("LEG ")]
            out = json.loads(lines[-1][4:]) if p.returncode == 0 and lines else {"failed": p.returncode, "stderr_tail": p.stderr[-400:]}
        except subprocess.TimeoutExpired:
            out = {"failed": "time limit", "limit_s": a.leg_timeout}
        res["k"][str(k)] = out
        print(f"k={k}: {json.dumps(out)}", file=sys.stderr, flush=True)
        if "failed" in out:
            break                                               # nothing more is started on the GPU behind a failed leg
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
    if any("failed" in v for v in res["k"].values()):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
