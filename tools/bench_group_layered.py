#!/usr/bin/env python
"""Groups of LAYERED PPO-Lagrangian (or, --algo focops, FOCOPS) seeds on ONE MI355X (hidden_sizes the fused kernels do not cover): grouped updates and lock-step
collection against what a user has without them.  Workload per seed: bench.py's `layered` shape -- obs 8 / act 2 / N = 20 000 /
batch 256 x 4 passes / grad-clip 0.5.  One JSON line per (leg, k).

    python tools/bench_group_layered.py --hidden 256x256x256 --ks 1,2,4,8 [--rounds 5] [--legs update,collect] [--algo ppol|focops]

update leg, three modes on the same build, alternated inside one process (warm-up first, then `rounds` rounds of grouped / threads /
alone; median and min-max of the rounds per mode):
    grouped  k engines in one EngineGroup, one fsrl_group_ppo_update (2 L + 5 launches per minibatch step whatever k)
    threads  k engines, a host thread and a stream each, Engine.ppo_update in every thread (ctypes releases the GIL)
    alone    one engine, Engine.ppo_update
Every timed update starts from the same state, restored from the HBM snapshot as tools/bench_group.py does.
collect leg: k seeds of 20 envs, `--collect-steps` vector steps per round through EngineGroup.collect_step, the shared launch
sequence (L + 2 launches per step) against the member-by-member calls (k (L + 2)), alternated the same way.
--algo focops: the same legs over FOCOPS engines (Engine.focops_update / EngineGroup.focops_update, delta = 1e9 so that no KL early
stop cuts an update short).  --legs once: ONE grouped update of k seeds and nothing else, for a kernel trace of its launches."""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import ACT, BATCH, ENVS, NROWS, OBS, REPEAT, make_inputs  # noqa: E402
from fsrl_amd import _lib  # noqa: E402
from fsrl_amd.engine import Engine, EngineConfig, EngineGroup  # noqa: E402

FOCOPS = False                                          # --algo focops
NU, NU_LOSS = 0.05, -0.5


def _engine(hidden, i, fill=True):
    if FOCOPS:
        e = Engine(EngineConfig(algo=_lib.ALGO_FOCOPS, obs_dim=OBS, act_dim=ACT, hidden_sizes=hidden, n_critics=2, env_num=ENVS,
                                buffer_size=100000, target_kl=None))
        e.focops_init(delta=1e9)
    else:
        e = Engine(EngineConfig(obs_dim=OBS, act_dim=ACT, hidden_sizes=hidden, env_num=ENVS, buffer_size=100000, max_grad_norm=0.5,
                                target_kl=None))
    e.set_params((0.08 * np.random.default_rng(100 + i).standard_normal(e.n_params)).astype(np.float32))
    if fill:
        obs, act, rew, cost, term, trunc = make_inputs(i)
        ids = np.arange(ENVS)
        for t in range(NROWS // ENVS):
            e.push(ids, obs[t], act[t], rew[t], cost[t], term[t], trunc[t], obs[t + 1])
    e.optim_reset(); e.state_snapshot(); e.sync()
    return e


def _solo_update(e, u):
    if FOCOPS:
        return e.focops_update(NU, NU_LOSS, BATCH, REPEAT, seed=u + 1)
    return e.ppo_update([0.75], 1 / 1.75, BATCH, REPEAT, seed=u + 1)


def _group_update(grp, k, u):
    if FOCOPS:
        return grp.focops_update([NU] * k, [NU_LOSS] * k, BATCH, REPEAT, seed=u + 1)
    return grp.ppo_update(np.full((k, 1), 0.75), np.full(k, 1 / 1.75), BATCH, REPEAT, seed=u + 1)


def _spread(times):
    return {"median_ms": float(np.median(times)) * 1e3, "min_ms": float(np.min(times)) * 1e3, "max_ms": float(np.max(times)) * 1e3}


def update_leg(hidden, k, rounds):
    grouped, free = [_engine(hidden, i) for i in range(k)], [_engine(hidden, i) for i in range(k)]
    grp = EngineGroup(grouped)
    steps = [0]

    def solo(e, u):
        e.state_restore()
        st, _ = _solo_update(e, u)
        e.sync()
        steps[0] = st.shape[0]

    def run_grouped(u):
        for e in grouped:
            e.state_restore()
        st, _ = _group_update(grp, k, u)
        for e in grouped:
            e.sync()
        assert all(np.isfinite(s).all() for s in st)

    def run_threads(u):
        ts = [threading.Thread(target=solo, args=(e, u)) for e in free]
        for t in ts:
            t.start()
        for t in ts:
            t.join()

    modes = {"grouped": run_grouped, "threads": run_threads, "alone": lambda u: solo(free[0], u)}
    times = {m: [] for m in modes}
    for u in range(rounds + 1):                         # round 0: warm-up
        for m, f in modes.items():
            t0 = time.perf_counter()
            f(u)
            if u:
                times[m].append(time.perf_counter() - t0)
    out = {"leg": "update", "algo": "focops" if FOCOPS else "ppol", "hidden": list(hidden), "k": k, "rounds": rounds,
           "steps_per_update": steps[0]}
    for m in modes:
        n = 1 if m == "alone" else k
        sp = _spread(times[m])
        out[m] = dict(sp, aggregate_updates_per_s=n / (sp["median_ms"] * 1e-3), us_per_member_step=sp["median_ms"] * 1e3 / steps[0] / n)
    grp.close()
    for e in grouped + free:
        e.close()
    return out


def collect_leg(hidden, k, rounds, n_steps):
    engs = [_engine(hidden, i, fill=False) for i in range(k)]
    grp = EngineGroup(engs)
    rng = np.random.default_rng(0)
    ids = np.arange(ENVS, dtype=np.int32)
    obs = rng.standard_normal((k, ENVS, OBS)).astype(np.float32)
    zeros, no = np.zeros(ENVS), np.zeros(ENVS, bool)

    def run(shared):
        grp.actor_set_resident(shared)
        acts = [np.zeros((ENVS, ACT), np.float32)] * k
        t0 = time.perf_counter()
        for _ in range(n_steps):
            prevs = [(ids, obs[i], acts[i], zeros, zeros, no, no, obs[i]) for i in range(k)]
            acts = [r[0] for r in grp.collect_step(prevs, list(obs))]
        return time.perf_counter() - t0

    times = {"shared": [], "member_by_member": []}
    for u in range(rounds + 1):
        for m in times:
            dt = run(m == "shared")
            if u:
                times[m].append(dt)
    out = {"leg": "collect", "algo": "focops" if FOCOPS else "ppol", "hidden": list(hidden), "k": k, "rounds": rounds,
           "vector_steps": n_steps, "envs_per_seed": ENVS}
    for m, t in times.items():
        sp = _spread(t)
        out[m] = dict(sp, env_steps_per_s=k * ENVS * n_steps / (sp["median_ms"] * 1e-3), us_per_vector_step=sp["median_ms"] * 1e3 / n_steps)
    grp.close()
    for e in engs:
        e.close()
    return out


def once_leg(hidden, k):
    engs = [_engine(hidden, i) for i in range(k)]
    grp = EngineGroup(engs)
    st, _ = _group_update(grp, k, 0)
    for e in engs:
        e.sync()
    grp.close()
    for e in engs:
        e.close()
    return {"leg": "once", "algo": "focops" if FOCOPS else "ppol", "hidden": list(hidden), "k": k,
            "minibatch_steps": [int(s.shape[0]) for s in st], "launches_per_step": 2 * len(hidden) + 5}


def main(argv=None):
    global FOCOPS
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", default="256x256x256", help="hidden layers, e.g. 256x256x256 or 400x300")
    ap.add_argument("--ks", default="1,2,4,8")
    ap.add_argument("--rounds", type=int, default=5, help="timed rounds per mode (at least 5), after one warm-up round")
    ap.add_argument("--legs", default="update,collect")
    ap.add_argument("--collect-steps", type=int, default=300)
    ap.add_argument("--algo", choices=("ppol", "focops"), default="ppol")
    a = ap.parse_args(argv)
    FOCOPS = a.algo == "focops"
    hidden = tuple(int(w) for w in a.hidden.lower().split("x"))
    assert a.rounds >= 5, "at least five rounds per mode"
    for k in (int(x) for x in a.ks.split(",")):
        if "update" in a.legs:
            print(json.dumps(update_leg(hidden, k, a.rounds)), flush=True)
        if "collect" in a.legs:
            print(json.dumps(collect_leg(hidden, k, a.rounds, a.collect_steps)), flush=True)
        if "once" in a.legs:
            print(json.dumps(once_leg(hidden, k)), flush=True)


if __name__ == "__main__":
    main()
