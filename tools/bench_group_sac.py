"""Aggregate SAC-Lagrangian (or, with --algo ddpgl, DDPG-Lagrangian) updates/s of k seeds on one GPU, three ways: grouped (fsrl_sac_group_update: every launch carries all
members), one context alone, and k contexts with one host thread each (train_multi_seed.py's threaded mode).  One JSON line per
(shape, k, mode).

    python tools/bench_group_sac.py [--algo sacl|ddpgl] [--shapes default,configs3] [--ks 1,2,4,8] [--updates 200] [--modes grouped,solo,threaded]

Shapes: default = the reference's sacl_cfg.py (obs 8, act 2, 128 x 128, batch 256, n_step 2); configs3 = BASELINE configs[3]
(obs 33, act 8, 256 x 256, batch 1024, 1 M-row stores).  --algo ddpgl: the same two shapes with sac_init(deterministic=True)
engines (the default shape is also the reference's ddpgl_cfg.py).
--hidden 256x256x256: the shapes' hidden layers replaced by these (anything but two layers of at most 256 units: LAYERED members,
whose grouped update is the layered launch sequence with every member in each launch, bit-identical per member to its own update).

    python tools/bench_group_sac.py --hidden 256x256x256 --shapes default --repeats 3
    python tools/bench_group_sac.py --algo ddpgl --hidden 64x48x32 --shapes default --repeats 3

--per ALPHA,BETA: every context has prioritised replay on (fsrl_per_enable after the fill, weight_norm on): the grouped mode then runs
the grouped prioritised update (the solo prioritised sequence once per update for all members, 13 launches for fused members), the
threaded mode k solo prioritised contexts, the solo mode one.  --rows shrinks the stores (and with them the sum trees' depth).

    python tools/bench_group_sac.py --per 0.6,0.4 --shapes configs3 --repeats 3"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {
    "default": dict(obs=8, act=2, H=128, B=256, n_step=2, rows=20000, env_num=10),
    "configs3": dict(obs=33, act=8, H=256, B=1024, n_step=2, rows=1000000, env_num=10),
}


def _engine(sh, seed, algo="sacl", hidden=None, prio=None):
    import torch
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig
    E = sh["env_num"]
    eng = Engine(EngineConfig(algo=_lib.ALGO_SAC_LAG, obs_dim=sh["obs"], act_dim=sh["act"], hidden_sizes=hidden or (sh["H"], sh["H"]),
                              n_critics=2, env_num=E, buffer_size=sh["rows"], gamma=0.99, target_kl=None))
    if algo == "ddpgl":
        eng.sac_init(deterministic=True, n_step=sh["n_step"])
    else:
        eng.sac_init(n_step=sh["n_step"])
    g = torch.Generator().manual_seed(seed)
    eng.sac_set_params((0.1 * torch.randn(eng.n_sac_actor, generator=g)).numpy(),
                       (0.1 * torch.randn(eng.n_sac_critics, generator=g)).numpy(), 0.0)
    rng = np.random.default_rng(seed)
    per, ids = sh["rows"] // E, np.arange(E)
    chunk = 512
    for t0 in range(0, per, chunk):                    # fill the store (pushes of E rows, batched over time steps)
        n = min(chunk, per - t0)
        o = rng.standard_normal((n, E, sh["obs"])).astype(np.float32)
        a = rng.uniform(-1, 1, (n, E, sh["act"])).astype(np.float32)
        for t in range(n):
            eng.push(ids, o[t], a[t], np.full(E, 0.5), np.zeros(E), np.zeros(E, bool), np.full(E, (t0 + t + 1) % 1000 == 0), o[t])
    if prio:
        eng.per_enable(prio[0], prio[1], True)
    eng.sac_update(sh["B"], [0.3], 1 / 1.3, seed=seed + 1, sync=False)       # key + warm-up
    eng.sac_drain()
    return eng


def _sync(engs):
    for e in engs:
        e.sac_get_params(0)


def run(shape, k, mode, updates, algo="sacl", hidden=None, per=None, rows=None):
    from fsrl_amd.engine import EngineSacGroup
    sh = dict(SHAPES[shape], **({"rows": rows} if rows else {}))
    B = sh["B"]
    engs = [_engine(sh, 10 + i, algo, hidden, per) for i in range(1 if mode == "solo" else k)]
    per_call = 50
    if mode == "grouped":
        g = EngineSacGroup(engs)
        lags, resc = [[0.3]] * k, [1 / 1.3] * k
        g.update(B, [per_call] * k, lags, resc)             # warm-up
        _sync(engs)
        t0 = time.perf_counter()
        done = 0
        while done < updates:
            g.update(B, [per_call] * k, lags, resc)
            done += per_call
            if done % 1000 < per_call:
                for e in engs:
                    e.sac_drain()
        _sync(engs)
        dt = time.perf_counter() - t0
        g.close()
        total = done * k
    else:
        def loop(e, n):
            for u in range(n):
                e.sac_update(B, [0.3], 1 / 1.3, sync=False)
                if u % 1000 == 999:
                    e.sac_drain()
            e.sac_get_params(0)
        for e in engs:
            loop(e, per_call)
        t0 = time.perf_counter()
        if mode == "solo":
            loop(engs[0], updates)
        else:
            th = [threading.Thread(target=loop, args=(e, updates)) for e in engs]
            for t in th:
                t.start()
            for t in th:
                t.join()
        dt = time.perf_counter() - t0
        total = updates * len(engs)
    for e in engs:
        e.close()
    return dict(algo=algo, shape=shape, k=k, mode=mode, batch=B, **({"per": list(per), "rows": sh["rows"]} if per else {}), hidden="x".join(str(w) for w in hidden) if hidden else sh["H"], updates=total, seconds=round(dt, 4),
                updates_per_s=round(total / dt, 1), us_per_member_update=round(dt / total * 1e6, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--algo", choices=("sacl", "ddpgl"), default="sacl")
    ap.add_argument("--shapes", default="default,configs3")
    ap.add_argument("--ks", default="1,2,4,8")
    ap.add_argument("--modes", default="grouped,solo,threaded")
    ap.add_argument("--updates", type=int, default=200, help="updates per member (grouped / threaded) or for the single context")
    ap.add_argument("--repeats", type=int, default=1, help="alternate the modes this many times on the same box")
    ap.add_argument("--hidden", default=None, type=lambda t: tuple(int(w) for w in t.lower().split("x")),
                    help="hidden layers instead of the shape's, e.g. 256x256x256 or 64x48x32 (layered members)")
    ap.add_argument("--per", default=None, metavar="ALPHA,BETA", type=lambda t: tuple(float(x) for x in t.split(",")),
                    help="prioritised replay on every context with these exponents (weight_norm on)")
    ap.add_argument("--rows", type=int, default=None, help="rows of every store instead of the shape's")
    a = ap.parse_args()
    if a.per is not None and len(a.per) != 2:
        ap.error("--per ALPHA,BETA")
    ks = [int(x) for x in a.ks.split(",")]
    for shape in a.shapes.split(","):
        for k in ks:
            for _ in range(a.repeats):
                for mode in a.modes.split(","):
                    if mode == "solo" and k != ks[0]:
                        continue                            # one context alone: measured once per shape
                    print(json.dumps(run(shape, k, mode, a.updates, a.algo, a.hidden, a.per, a.rows)), flush=True)


if __name__ == "__main__":
    main()
