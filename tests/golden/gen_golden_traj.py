#!/usr/bin/env python
"""TrajectoryBuffer fixtures from the UNMODIFIED reference (fsrl/data/traj_buf.py).  Build container only.

    python tests/golden/gen_golden_traj.py      # writes tests/golden/traj_filter_cases.npz and traj_store_cases.npz

traj_filter_cases: `TrajectoryBuffer.filter_points(points, target_size)` under `random.seed(seed)` -> the kept indices, for 300
normal points thinned to 100; a clustered set where most cells are empty; a set with several points exactly on both maxima (they
land in an extra cell, traj_buf.py:140-142); target_size equal to the number of points.  Only inputs on which the reference neither
divides by zero (zero spread in a coordinate) nor exhausts its cell list (fewer points than target_size): asserted here.

traj_store_cases: `TrajectoryBuffer.store` driven with scripted single-transition batches, the episode number carried in
observations[:, 0]: which episodes survive, in which order, and `metrics`, for: under capacity; the window; the grid filter firing
twice; random replacement.  The stream is stored as (episode lengths, rewards, costs); `random` / `np.random` are seeded per case.

h5py is not installed here: an empty module stands in (the reference only uses it in save()).  The shim's Batch has no `cat`; the
stand-in below adds it, for this file only."""
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_shim  # noqa: E402

ref_shim.install()
sys.modules.setdefault("h5py", types.ModuleType("h5py"))
from fsrl.data import traj_buf as ref_traj_buf  # noqa: E402


class CatBatch:
    """what traj_buf.py uses of tianshou's Batch: keyword construction, [key], len(), Batch.cat over (possibly empty) batches"""

    def __init__(self, **kw):
        self.__dict__.update({k: np.asarray(v) for k, v in kw.items()})

    def __getitem__(self, k):
        return self.__dict__[k]

    def __len__(self):
        return 0 if not self.__dict__ else len(next(iter(self.__dict__.values())))

    @staticmethod
    def cat(batches):
        full = [b for b in batches if len(b)]
        return CatBatch(**{k: np.concatenate([b[k] for b in full]) for k in full[0].__dict__}) if full else CatBatch()


ref_traj_buf.Batch = CatBatch
RefBuffer = ref_traj_buf.TrajectoryBuffer


def filter_cases():
    rng = np.random.default_rng(20240607)
    cases = {}
    cases["normal"] = (rng.normal([10.0, 5.0], [4.0, 2.0], (300, 2)), 100, 1)
    centres = np.array([[0.0, 0.0], [0.5, 9.0], [9.5, 0.3]])
    clustered = np.concatenate([c + 0.05 * rng.standard_normal((66, 2)) for c in centres] + [np.array([[-3.0, -2.0], [14.0, 12.0]])])
    cases["clustered"] = (clustered, 50, 2)
    lattice = rng.integers(0, 7, (150, 2)).astype(np.float64)
    lattice[:5] = [6.0, 6.0]; lattice[5:9, 0] = 6.0; lattice[9:13, 1] = 6.0          # several points on both maxima
    cases["on_maxima"] = (lattice, 40, 3)
    cases["all_kept"] = (rng.uniform(-1.0, 1.0, (64, 2)), 64, 4)
    out = {"names": np.array(list(cases))}
    for name, (pts, target, seed) in cases.items():
        assert len(pts) >= target and (pts.max(0) > pts.min(0)).all(), name
        random.seed(seed)
        kept = RefBuffer.filter_points(list(pts), target)
        random.seed(seed)
        assert kept == RefBuffer.filter_points(list(pts), target), name
        assert len(kept) == target and len(set(kept)) == target, name
        out[name + "/points"], out[name + "/target"], out[name + "/seed"] = pts, np.int64(target), np.int64(seed)
        out[name + "/kept"] = np.array(kept, np.int64)
        print(f"filter {name}: {len(pts)} -> {target}")
    np.savez_compressed(os.path.join(HERE, "traj_filter_cases.npz"), **out)


def run_store(name, n_episodes, seed, **kw):
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 13, n_episodes)
    lens[1] = 1
    rews = [rng.normal(1.0, 1.0, n) for n in lens]
    costs = [(rng.random(n) < 0.3).astype(np.float64) for n in lens]
    random.seed(seed); np.random.seed(seed)
    tb = RefBuffer(**kw)
    for ep in range(n_episodes):
        for t in range(lens[ep]):
            last = t == lens[ep] - 1
            tb.store(CatBatch(observations=[[float(ep), float(t)]], next_observations=[[float(ep), float(t + 1)]], actions=[[0.0]],
                              rewards=[rews[ep][t]], costs=[costs[ep][t]], terminals=[last and ep % 2 == 0],
                              timeouts=[last and ep % 2 == 1]))
    survivors = np.array([int(traj["observations"][0, 0]) for traj in tb.buffer], np.int64)
    for traj, ep in zip(tb.buffer, survivors):
        assert len(traj) == lens[ep] and (traj["observations"][:, 0] == ep).all()
    out = {"lens": lens.astype(np.int64), "rews": np.concatenate(rews), "costs": np.concatenate(costs), "seed": np.int64(seed),
           "survivors": survivors, "metrics": np.array(tb.metrics, np.float64).reshape(-1, 2), "transitions": np.int64(len(tb))}
    for k, v in kw.items():
        out["kw_" + k] = np.float64(v)
    print(f"store {name}: {n_episodes} episodes -> {len(survivors)} stored, {len(tb)} transitions")
    return {f"{name}/{k}": v for k, v in out.items()}


def store_cases():
    out = {"names": np.array(["under_capacity", "window", "grid_twice", "replace"])}
    out.update(run_store("under_capacity", 6, 11, max_trajectory=10))
    out.update(run_store("window", 14, 12, max_trajectory=20, rmin=2.0, rmax=12.0, cmin=0.0, cmax=3.0))
    r = run_store("grid_twice", 27, 13, max_trajectory=8, use_grid_filter=True, filter_interval=2)
    assert len(r["grid_twice/survivors"]) == 8 + 3          # fired at 16 and again at 16: 27 = 16 + 8 + 3
    out.update(r)
    r = run_store("replace", 14, 14, max_trajectory=5, use_grid_filter=False)
    assert len(r["replace/survivors"]) == 5 and r["replace/survivors"].max() > 4
    out.update(r)
    np.savez_compressed(os.path.join(HERE, "traj_store_cases.npz"), **out)


if __name__ == "__main__":
    filter_cases()
    store_cases()
