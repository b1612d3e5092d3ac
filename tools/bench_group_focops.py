#!/usr/bin/env python
"""Aggregate FOCOPS updates/s of k independent agents on ONE MI355X, three ways: grouped (one fsrl_group_ppo_update over k FOCOPS
contexts, every launch of the minibatch step carrying all members), k contexts with one host thread each (Engine.focops_update
in parallel), and one context alone.  Per agent: obs 8 / act 2, N = 20 000 rows, batch 256, 4 passes, delta = 1e9 (no KL early
stop cuts an update short); --hidden 256 is the FOCOPS leg of tools/bench_trust.py, --hidden 128 the reference's default.
One JSON line per k.

    python tools/bench_group_focops.py [--hidden 256] [--ks 1 2 4 8] [--updates 6]
    python tools/bench_group_focops.py --hidden 256x256x256 [--ks 1 2 4 8] [--legs update,collect]

--hidden AxBxC (any tuple) makes LAYERED members: tools/bench_group_layered.py's legs with --algo focops (grouped / k threads / one
context alternated in one process, and the collect leg), one JSON line per (leg, k).

Every timed update starts from the same state (initial weights, fresh Adam moments), restored from the HBM snapshot."""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import ACT, BATCH, ENVS, HID, NROWS, OBS, REPEAT, make_inputs, orthogonal_theta  # noqa: E402
from fsrl_amd import _lib  # noqa: E402
from fsrl_amd.engine import Engine, EngineConfig, EngineGroup  # noqa: E402

NU, NU_LOSS = 0.05, -0.5


def engines(k, hidden):
    out = []
    for i in range(k):
        e = Engine(EngineConfig(algo=_lib.ALGO_FOCOPS, obs_dim=OBS, act_dim=ACT, hidden=hidden, n_critics=2, env_num=ENVS,
                                buffer_size=100000, target_kl=None))
        e.focops_init(delta=1e9)
        obs, act, rew, cost, term, trunc = make_inputs(i)
        ids = np.arange(ENVS)
        for t in range(NROWS // ENVS):
            e.push(ids, obs[t], act[t], rew[t], cost[t], term[t], trunc[t], obs[t + 1])
        if hidden == HID:                   # bench.py's initial weights at its shape; the engine's own elsewhere
            e.set_params(orthogonal_theta(i, e.n_params))
        e.optim_reset(); e.state_snapshot()
        e.sync()
        out.append(e)
    return out


def timed(fn, engs, updates):
    fn(0)
    for e in engs:
        e.sync()
    times = []
    for u in range(updates):                # an update ends with its statistics on the host: every update is timed on its own
        for e in engs:                      # same workload every update
            e.state_restore()
        for e in engs:
            e.sync()
        t0 = time.perf_counter()
        fn(u + 1)
        for e in engs:
            e.sync()
        times.append(time.perf_counter() - t0)
    return float(np.median(times))          # the median: the box's CPU quota throttles a process for tens of ms now and then


def run(k, hidden, updates):
    engs = engines(k, hidden)
    grp = EngineGroup(engs)
    res = {}

    def grouped(u):
        st, sp = grp.focops_update([NU] * k, [NU_LOSS] * k, BATCH, REPEAT, seed=u + 1)
        assert all(np.isfinite(s).all() for s in st) and max(sp) == -1
    res["grouped"] = k / timed(grouped, engs, updates)
    grp.close()

    def threaded(u):
        ths = [threading.Thread(target=e.focops_update, args=(NU, NU_LOSS, BATCH, REPEAT), kwargs=dict(seed=u + 1)) for e in engs]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
    res["threaded"] = k / timed(threaded, engs, updates)
    res["one_context"] = 1 / timed(lambda u: engs[0].focops_update(NU, NU_LOSS, BATCH, REPEAT, seed=u + 1), engs[:1], updates)
    for e in engs:
        e.close()
    return {"agents_per_gpu": k, "hidden": hidden, "rows": NROWS, "batch": BATCH, "passes": REPEAT,
            "grouped_updates_per_s": res["grouped"], "threaded_updates_per_s": res["threaded"],
            "one_context_updates_per_s": res["one_context"], "grouped_vs_one_context": res["grouped"] / res["one_context"],
            "grouped_vs_threaded": res["grouped"] / res["threaded"], "timing": "median of %d updates" % updates}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", default="256", help="a width (fused members) or a tuple such as 256x256x256 (layered members)")
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--updates", type=int, default=6)
    ap.add_argument("--legs", default="update,collect", help="layered members: bench_group_layered.py's legs")
    a = ap.parse_args()
    if "x" in a.hidden.lower():
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import bench_group_layered
        bench_group_layered.main(["--algo", "focops", "--hidden", a.hidden, "--ks", ",".join(map(str, a.ks)), "--legs", a.legs,
                                  "--rounds", str(max(a.updates, 5))])
    else:
        for k in a.ks:
            print(json.dumps(run(k, int(a.hidden), a.updates)), flush=True)
