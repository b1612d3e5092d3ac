"""Aggregate CVPO updates/s of k seeds on one GPU, three ways: grouped (fsrl_cvpo_group_update: every launch carries all members),
one context alone, and k contexts with one host thread each (train_multi_seed.py's threaded mode).  One JSON line per
(shape, k, mode, repeat).

    python tools/bench_group_cvpo.py [--shapes default,wide] [--ks 1,2,4,8] [--updates 400] [--modes grouped,solo,threaded]
                                     [--repeats 2] [--cycle 50] [--hidden AxBxC]

Shapes: default = tools/bench_cvpo.py's (the agent's defaults: obs 40, act 2, 128 x 128, batch 256, K = 16 particles, single
critics, n_step 2); wide = 256 x 256, batch 1024, double critics.  Every 50 updates each context runs a collect cycle's
cvpo_post_update / cvpo_pre_update, as tools/bench_cvpo.py does.
The k contexts of a (shape, k) are built and warmed up once (every mode runs 50 untimed updates on them first); then the modes are
ALTERNATED on those contexts, `--repeats` times each (at least twice), so the spread of repeating one mode is in the output next
to the differences between the modes.  Every timed window ends in a device synchronise of every context it used.
--hidden 256x256x256: the shapes' hidden layers replaced by these (anything but two layers of at most 256 units: LAYERED members,
whose grouped update is the layered launch sequence with every member in each launch, bit-identical per member to its own update).

    python tools/bench_group_cvpo.py --hidden 256x256x256 --shapes default --repeats 3"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {
    "default": dict(obs=40, act=2, H=128, B=256, K=16, double=False, rows=20000, env_num=10),
    "wide": dict(obs=40, act=2, H=256, B=1024, K=16, double=True, rows=50000, env_num=10),
}
CYCLE = 50          # updates between two collect cycles (update_per_step 0.2 x 250 steps) = updates per grouped call; --cycle


def _hidden(text):
    """'64x48x32' -> (64, 48, 32)"""
    return tuple(int(w) for w in text.lower().split("x"))


def _engine(sh, seed, hidden=None):
    import torch
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig
    E = sh["env_num"]
    eng = Engine(EngineConfig(algo=_lib.ALGO_SAC_LAG, obs_dim=sh["obs"], act_dim=sh["act"], hidden_sizes=hidden or (sh["H"], sh["H"]),
                              n_critics=2, env_num=E, buffer_size=sh["rows"], gamma=0.98, target_kl=None))
    eng.cvpo_init(0.2, sample_act_num=sh["K"], double_critic=sh["double"])
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
        c = (rng.random((n, E)) < 0.1).astype(np.float64)
        for t in range(n):
            eng.push(ids, o[t], a[t], np.full(E, 0.5), c[t], np.zeros(E, bool), np.full(E, (t0 + t + 1) % 300 == 0), o[t])
    eng.cvpo_post_update(); eng.cvpo_pre_update()
    eng.cvpo_update(sh["B"], seed=seed + 1, sync=False)       # key the Philox stream
    eng.sac_drain()
    return eng


def _cycle(e):
    e.cvpo_post_update(); e.cvpo_pre_update()


def _grouped(g, engs, B, updates):
    done = 0
    while done < updates:
        g.update(B, [CYCLE] * len(engs))
        done += CYCLE
        for e in engs:
            _cycle(e)
        if done % 1000 < CYCLE:
            for e in engs:
                e.sac_drain()
    for e in engs:
        e.sync()
    return done * len(engs)


def _own(e, B, updates):
    for u in range(updates):
        e.cvpo_update(B, sync=False)
        if u % CYCLE == CYCLE - 1:
            _cycle(e)
        if u % 1000 == 999:
            e.sac_drain()
    e.sync()


def _threaded(engs, B, updates):
    th = [threading.Thread(target=_own, args=(e, B, updates)) for e in engs]
    for t in th:
        t.start()
    for t in th:
        t.join()
    return updates * len(engs)


def run(shape, k, modes, updates, repeats, hidden=None):
    from fsrl_amd.engine import EngineCvpoGroup
    sh = SHAPES[shape]
    B = sh["B"]
    engs = [_engine(sh, 10 + i, hidden) for i in range(k)]
    g = EngineCvpoGroup(engs)
    timed = {"grouped": lambda n: _grouped(g, engs, B, n),
             "solo": lambda n: (_own(engs[0], B, n), n)[1],
             "threaded": lambda n: _threaded(engs, B, n)}
    for mode in modes:                                 # warm-up of every mode on this shape
        timed[mode](CYCLE)
    for rep in range(repeats):
        for mode in modes:                             # alternated
            for e in engs:
                e.sac_drain(); e.sync()
            t0 = time.perf_counter()
            total = timed[mode](updates)               # ends in a synchronise of every context it used
            dt = time.perf_counter() - t0
            print(json.dumps(dict(shape=shape, k=k, mode=mode, repeat=rep, batch=B,
                                  hidden="x".join(str(w) for w in hidden) if hidden else sh["H"], particles=sh["K"],
                                  double_critic=sh["double"], updates=total, seconds=round(dt, 4),
                                  updates_per_s=round(total / dt, 1), us_per_member_update=round(dt / total * 1e6, 2),
                                  us_per_call_update=round(dt / (total / (1 if mode == "solo" else k)) * 1e6, 2))), flush=True)
    g.close()
    for e in engs:
        e.close()


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="default,wide")
    ap.add_argument("--ks", default="1,2,4,8")
    ap.add_argument("--modes", default="grouped,solo,threaded")
    ap.add_argument("--updates", type=int, default=400, help="updates per member (grouped / threaded) or for the single context")
    ap.add_argument("--repeats", type=int, default=2, help="alternate the modes this many times (at least 2)")
    ap.add_argument("--cycle", type=int, default=CYCLE, help="updates between two collect cycles = updates per grouped call")
    ap.add_argument("--hidden", default=None, type=_hidden,
                    help="hidden layers instead of the shape's, e.g. 256x256x256 or 64x48x32 (layered members)")
    return ap


def main():
    global CYCLE
    a = build_parser().parse_args()
    CYCLE = max(1, a.cycle)
    modes = a.modes.split(",")
    assert all(m in ("grouped", "solo", "threaded") for m in modes), "modes: grouped, solo, threaded"
    for shape in a.shapes.split(","):
        for k in [int(x) for x in a.ks.split(",")]:
            run(shape, k, modes, a.updates, max(2, a.repeats), a.hidden)


if __name__ == "__main__":
    main()
