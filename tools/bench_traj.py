#!/usr/bin/env python
"""What the trajectory tap costs, and what the archive's export path gains (GPU).

    python tools/bench_traj.py [--repeats 3] [--collects 12] [--out profiles/traj_tap.json]
    python tools/bench_traj.py --untapped-only [--tree DIR]      # the untapped leg alone; DIR: another checkout's package (A/B
                                                                  # against a parent commit, whose library has no fsrl_traj_*)
    python tools/bench_traj.py --fill [--out profiles/traj_fill.json]   # the fill leg alone

collect: the native collect of bench.py's end-to-end leg -- 20 envs in 4 worker processes, 300-step episodes, actor on the device,
one library call per collect(n_episode = 20) -- of ONE agent over ONE set of env workers, alternated collect by collect between
untapped and tapped (the buffer is attached before a tapped collect and detached after it, outside the timed region: two twin
agents with their own worker processes differ by more than the tap costs); `repeats` blocks of `collects` collect pairs each.  Reported: collector-only env-steps/s of both per block, the tap's launches
and host-to-device bytes per collect, the launch floor fsrl_launch_floors measures in the same run, and the part of the measured
overhead that launches x floor explains (the extra bytes are a few KB per flush: 4 + 4 act_dim per row).

export: `rows` rows (100 k and 1 M) pushed through a tapped engine; fsrl_traj_export of all of them against fsrl_store_read of the
same rows in chunks of 65 536 slots.

fill: a 1 M-row archive (4000 episodes of 250 rows, obs 33 / act 8) poured into a 1 M-row replay store of 20 sub-buffers by ONE
fsrl_store_fill, against the same rows exported to the host and pushed through Engine.push 20 rows per call (actions inverted in
numpy), against fsrl_train_state_import of a store of that size; alternated, medians of three, wall clock around call + sync.  The
fill's bytes/s count what the kernel reads plus what it writes (about 314 + 313 bytes per row), over that wall clock -- job planning,
the table's copy and the launch included."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def collector(seed, envs=20, workers=4):
    from fsrl_amd.agent import PPOLagAgent
    from fsrl_amd.data import FastCollector, HipVectorReplayBuffer
    from fsrl_amd.env import ShmemVectorEnv
    env = ShmemVectorEnv(env_num=envs, workers=workers, obs_dim=8, act_dim=2, episode_len=300, seed=seed)
    agent = PPOLagAgent(env, cost_limit=10, device="cuda:0", seed=seed, hidden_sizes=(256, 256), max_grad_norm=0.5, training_num=envs)
    agent.policy.train()
    buf = HipVectorReplayBuffer(agent.policy.engine, 100000, envs)
    col = FastCollector(agent.policy, env, buf, exploration_noise=True, device_actor=True, native_loop=True)
    return dict(env=env, agent=agent, col=col, tb=None)


def block(leg, collects, envs=20):
    """`collects` untapped collects -- and, with a buffer, as many tapped ones, alternated -> env-steps/s of each (collector only)"""
    # untapped | tapped through the collector (the buffer looks -- flush, episode table, decisions -- at the end of every collect) |
    # tapped through the engine (the tap alone: nobody looks inside the timed region)
    modes = [None] + ([leg["col"], leg["col"].policy.engine] if leg["tb"] is not None else [])
    t, n = [0.0] * len(modes), [0] * len(modes)
    col = leg["col"]
    for _ in range(collects):
        for i, target in enumerate(modes):
            if target is not None:
                leg["tb"].attach(target)
            t0 = time.perf_counter()
            st = col.collect(n_episode=envs)
            t[i] += time.perf_counter() - t0
            n[i] += st["n/st"]
            if target is not None:
                leg["tb"].detach(target)
            col.reset_buffer(keep_statistics=True)                  # what the on-policy trainer does after every update
    return [n[i] / t[i] for i in range(len(modes))]


def bench_collect(a):
    leg = collector(1)
    if not a.untapped_only:
        from fsrl_amd.data import TrajectoryBuffer
        leg["tb"] = TrajectoryBuffer(leg["col"], max_trajectory=2000, max_episode_len=300, max_rows=1 << 20)
        leg["tb"].detach(leg["col"])
    block(leg, 3)                                                   # warm-up: first launches, worker processes up to speed
    c0 = leg["tb"].counters() if not a.untapped_only else None
    reps = [block(leg, a.collects) for _ in range(a.repeats)]
    out = {"envs": 20, "workers": 4, "episode_len": 300, "collects_per_block": a.collects,
           "untapped_env_steps_per_s": [r[0] for r in reps]}
    if not a.untapped_only:
        c1 = leg["tb"].counters()
        ncol = 2 * a.collects * a.repeats                          # tapped collects: both tapped modes feed the counters
        eng = leg["agent"].policy.engine
        floors = eng.launch_floors(256, 200)
        launches = (c1["launches"] - c0["launches"]) / ncol
        h2d = (c1["h2d_bytes"] - c0["h2d_bytes"]) / ncol
        un, tp, tq = (float(np.mean([r[i] for r in reps])) for i in range(3))
        per_collect_us = (1.0 / tp - 1.0 / un) * 6000 * 1e6
        tap_alone_us = (1.0 / tq - 1.0 / un) * 6000 * 1e6
        floor_us = float(min(floors["fwdbwd"], floors["wgrad"], floors["adam"]))    # one launch behind itself, the cheapest grid
        committed = (c1["committed"] - c0["committed"]) / ncol
        out.update({"tapped_env_steps_per_s": [r[1] for r in reps], "tapped_nobody_looks_env_steps_per_s": [r[2] for r in reps],
                    "overhead_us_per_collect_tap_alone": tap_alone_us, "tap_launches_per_collect": launches,
                    "tap_h2d_bytes_per_collect": h2d, "launch_floor_us": floor_us,
                    "overhead_us_per_collect_measured": per_collect_us,
                    "overhead_us_per_collect_launch_floor_part": launches * floor_us,
                    "episodes_committed_per_collect": committed, "compactions": c1["compactions"]})
    if leg["tb"] is not None:
        leg["tb"].close()
    leg["agent"].policy.engine.close()
    leg["env"].close()
    return out


def bench_export(rows, envs=64, ep_len=125):
    from fsrl_amd.engine import Engine, EngineConfig, TrajArchive
    steps = rows // envs // ep_len * ep_len                        # whole episodes: every stored row is an archived row
    n = steps * envs
    eng = Engine(EngineConfig(obs_dim=8, act_dim=2, hidden=64, env_num=envs, buffer_size=n, target_kl=None))
    arch = TrajArchive(eng, n, n // ep_len + envs, ep_len, 1)
    arch.attach(eng)
    rng = np.random.default_rng(0)
    ids = np.arange(envs)
    obs = rng.standard_normal((envs, 8)).astype(np.float32); act = rng.standard_normal((envs, 2)).astype(np.float32)
    rew, cost, no = rng.standard_normal(envs), np.zeros(envs), np.zeros(envs, bool)
    for t in range(steps):
        eng.push(ids, obs, act, rew, cost, no, np.full(envs, (t + 1) % ep_len == 0), obs)
    arch.flush(); eng.sync()
    t_exp, t_read = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        data = arch.export()
        t_exp.append(time.perf_counter() - t0)
        idx = eng.sample0()
        t0 = time.perf_counter()
        for s in range(0, len(idx), 65536):
            eng.store_read(idx[s:s + 65536])
        t_read.append(time.perf_counter() - t0)
    out = {"rows": int(len(data["rewards"])), "store_rows": int(len(idx)), "export_ms": [1e3 * x for x in t_exp],
           "store_read_chunked_ms": [1e3 * x for x in t_read], "bytes": int(sum(v.nbytes for v in data.values()))}
    arch.close(); eng.close()
    return out


def bench_fill(rows=1_000_000, envs=20, ep_len=250, Do=33, Da=8):
    from fsrl_amd import _lib
    from fsrl_amd.data.traj_buf import inverse_action
    from fsrl_amd.engine import Engine, EngineConfig, TrajArchive
    n_eps = rows // ep_len // envs * envs
    n = n_eps * ep_len

    def engine():
        eng = Engine(EngineConfig(algo=_lib.ALGO_SAC_LAG, obs_dim=Do, act_dim=Da, hidden_sizes=(64, 64), n_critics=2, env_num=envs,
                                  buffer_size=n, target_kl=None))
        eng.sac_init()
        return eng

    a, b = engine(), engine()
    rng = np.random.default_rng(0)
    low, high = np.full(Da, -2.0, np.float32), np.full(Da, 3.0, np.float32)
    term = np.zeros(n, bool); term[ep_len - 1::ep_len] = True
    data = dict(observations=rng.standard_normal((n, Do), np.float32), next_observations=rng.standard_normal((n, Do), np.float32),
                actions=rng.uniform(-2.0, 3.0, (n, Da)).astype(np.float32), rewards=rng.standard_normal(n), costs=np.zeros(n),
                terminals=term, timeouts=np.zeros(n, bool))
    arch = TrajArchive(a, n, n_eps + 1, ep_len, 1, low, high)
    t0 = time.perf_counter()
    assert arch.import_rows(data) == (n_eps, n)
    t_import = time.perf_counter() - t0
    del data
    # lock-step order of the push loop: vector step t of the 20 episodes of block k, one per sub-buffer
    step = (np.arange(envs) * ep_len)[None, :] + np.arange(ep_len)[:, None]                       # [ep_len, envs]
    ids = np.arange(envs)
    t_fill, t_push, t_state = [], [], []
    blob = None
    for _ in range(3):
        a.reset_store(); a.sync()
        t0 = time.perf_counter()
        assert a.store_fill(arch, None, 0, 1, low, high) == n
        a.sync()
        t_fill.append(time.perf_counter() - t0)
        b.reset_store(); b.sync()
        t0 = time.perf_counter()
        d = arch.export()
        act = inverse_action(d["actions"], 1, low, high)
        for k in range(n_eps // envs):
            base = k * envs * ep_len
            for t in range(ep_len):
                r = step[t] + base
                b.push(ids, d["observations"][r], act[r], d["rewards"][r], d["costs"][r], d["terminals"][r], d["timeouts"][r],
                       d["next_observations"][r])
        b.sync()
        t_push.append(time.perf_counter() - t0)
        del d, act
        if blob is None:
            blob = a.train_state_array(with_store=True)
        t0 = time.perf_counter()
        b.load_train_state(blob)
        b.sync()
        t_state.append(time.perf_counter() - t0)
    moved = n * (2 * (2 * Do * 4 + Da * 4 + 16) + 3)
    fill = float(np.median(t_fill))
    out = {"rows": n, "episodes": n_eps, "obs_dim": Do, "act_dim": Da, "sub_buffers": envs, "import_ms": 1e3 * t_import,
           "store_fill_ms": [1e3 * x for x in t_fill], "export_and_push_20_rows_per_call_ms": [1e3 * x for x in t_push],
           "train_state_import_ms": [1e3 * x for x in t_state], "train_state_bytes": int(blob.size),
           "store_fill_median_ms": 1e3 * fill, "export_and_push_median_ms": 1e3 * float(np.median(t_push)),
           "train_state_import_median_ms": 1e3 * float(np.median(t_state)), "fill_bytes_read_plus_written": int(moved),
           "fill_bytes_per_s": moved / fill, "fill_launches": arch.counters()["fill_launches"], "fill_copies": arch.counters()["fill_copies"]}
    arch.close(); a.close(); b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--collects", type=int, default=12)
    ap.add_argument("--untapped-only", action="store_true")
    ap.add_argument("--tree", default=ROOT, help="checkout whose fsrl_amd package (and library) is measured")
    ap.add_argument("--no-export", action="store_true")
    ap.add_argument("--fill", action="store_true", help="the fsrl_store_fill leg alone (profiles/traj_fill.json)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    if a.fill:
        res = {"fill": bench_fill()}
        print(json.dumps(res))
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
        return
    res = {"tree": os.path.relpath(os.path.abspath(a.tree), ROOT), "collect": bench_collect(a)}
    if not a.untapped_only and not a.no_export:
        res["export"] = [bench_export(100_000), bench_export(1_000_000)]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
