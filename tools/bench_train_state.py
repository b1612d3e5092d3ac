#!/usr/bin/env python
"""Training-state I/O at the BASELINE configs[3] shape: SAC-Lagrangian, obs 33, act 8, 256x256, a full 1 M-row replay store.
Times Engine.train_state / load_train_state with and without the store, reports the blob sizes, and -- for scale -- reads the
same rows out through Engine.store_read in chunks, which is the only way to get the store out without the export.
One JSON line; --out also writes it to a file (profiles/train_state_io.json).  `--rows` shrinks the store for a quick run."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fsrl_amd import _lib  # noqa: E402
from fsrl_amd.engine import Engine, EngineConfig  # noqa: E402


def _median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), [round(t, 2) for t in ts]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--envs", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=65536)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    Do, Da, E = 33, 8, a.envs
    T = a.rows // E
    rng = np.random.default_rng(0)

    def engine():
        eng = Engine(EngineConfig(algo=_lib.ALGO_SAC_LAG, obs_dim=Do, act_dim=Da, hidden=256, n_critics=2, env_num=E, buffer_size=a.rows,
                                  target_kl=None))
        eng.sac_init()
        eng.sac_set_params((0.05 * rng.standard_normal(eng.n_sac_actor)).astype(np.float32),
                           (0.05 * rng.standard_normal(eng.n_sac_critics)).astype(np.float32), 0.0)
        return eng
    src, dst = engine(), engine()
    ids = np.arange(E)
    block = 1000                                             # the same random block pushed over and over: the bytes do not matter here
    obs = rng.standard_normal((block + 1, E, Do)).astype(np.float32)
    act = np.tanh(rng.standard_normal((block, E, Da))).astype(np.float32)
    rew, cost = rng.normal(0.5, 0.5, (block, E)), (rng.random((block, E)) < 0.1).astype(np.float64)
    no, yes = np.zeros(E, bool), np.ones(E, bool)
    t0 = time.perf_counter()
    for t in range(T):
        j = t % block
        src.push(ids, obs[j], act[j], rew[j], cost[j], no, yes if j == block - 1 else no, obs[j + 1])
    src.sync()
    fill_s = time.perf_counter() - t0
    for _ in range(3):
        src.sac_update(1024, [0.3], 0.77, seed=1)
    res = {"shape": {"obs": Do, "act": Da, "hidden": 256, "rows": int(len(src)), "sub_buffers": E}, "fill_s": round(fill_s, 2)}
    blob_store, blob_lean = src.train_state(True), src.train_state(False)
    res["bytes_with_store"], res["bytes_without_store"] = len(blob_store), len(blob_lean)
    res["export_store_ms"], res["export_store_runs"] = _median_ms(lambda: src.train_state(True), a.reps)
    res["export_store_array_ms"], res["export_store_array_runs"] = _median_ms(lambda: src.train_state_array(True), a.reps)
    res["export_lean_ms"], res["export_lean_runs"] = _median_ms(lambda: src.train_state(False), a.reps)
    res["import_store_ms"], res["import_store_runs"] = _median_ms(lambda: dst.load_train_state(blob_store), a.reps)
    res["import_lean_ms"], res["import_lean_runs"] = _median_ms(lambda: dst.load_train_state(blob_lean), a.reps)
    res["copy_store_ms"], res["copy_store_runs"] = _median_ms(lambda: dst.copy_train_state_from(src, True), a.reps)
    assert dst.train_state(True) == blob_store, "the imported state does not export to the same bytes"
    idx = src.sample0()

    def read_all():
        for o in range(0, idx.size, a.chunk):
            src.store_read(idx[o:o + a.chunk])
    res["store_read_loop_ms"], res["store_read_loop_runs"] = _median_ms(read_all, a.reps)
    res["store_read_chunk"] = a.chunk
    gb = len(blob_store) / 1e9
    res["export_store_GBps"] = round(gb / (res["export_store_ms"] / 1e3), 2)
    res["import_store_GBps"] = round(gb / (res["import_store_ms"] / 1e3), 2)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return res


if __name__ == "__main__":
    main()
