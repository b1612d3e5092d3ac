"""Prioritised replay at the sizes a working store has: the inputs of tests/test_gpu_per_big.py, defined once.

tests/test_per_model.py's stores have 32 leaves.  The geometries here are the smallest that reach the branches a 32-leaf tree never
takes (fsrl_amd/csrc/kernels_per.hpp, host_per.inc):

  wide   600 sub-buffers x 8 slots = 4 800 slots, bound 8 192.  More sub-buffers than the sampler's LDS book table holds
         (PER_BOOK_LDS = 512: the books are read from global memory); per_rebuild_kernel's loop over the nodes of a level runs more
         than once (levels of 2 048 and 4 096 nodes, 1 024 threads); rows per sub-buffer drawn from 0 .. 23 (one in eight from 0 .. 7,
         the others from 8 .. 23: a window takes at most 8 rows of a sub-buffer, so 4 096 records need 512 sub-buffers with 8 rows
         to push), so partly filled, exactly full and wrapped sub-buffers lie side by side; sub-buffers 0, 17 and 599 are EMPTY
         (whole zero subtrees, the first and the last leaf run among them) and sub-buffer 300 holds exactly 8 rows.  The pushes go in lock step, every live
         sub-buffer in every call, so a staging window reaches fsrl_ctx::STAGE_CAP = 4 096 records before it flushes: per_ingest's
         loop over the window and per_repair with more leaves than threads.
  deep   2 sub-buffers x 70 000 slots = 140 000 slots, bound 262 144, 300 and 170 rows.  18 levels of repair, and a tree of
         524 288 nodes: per_reset_kernel's grid-stride loop (1 024 x 256 threads) runs twice, the second time over the leaves.
  small  test_per_model's np2_wrap (3 x 7 slots, bound 32): the second member of the mixed group.

Everything is seeded.  tests/test_per_big_host.py asserts on the CPU, with the model alone, the conditions that keep the GPU tests
from being vacuous -- for every (store, priorities, seed, update count, batch) in SAMPLING the model's slots are filled ones, no
comparison of a descent is closer than MARGIN = 1e-9 of the root to a tie, the importance weights of every batch span more than
WEIGHT_SPAN = 0.05, some batch holds a slot twice -- and that the wide store has the sub-buffers it claims.  These are conditions,
not measurements: ROWS_SEED, the priorities' seed and the sampling seeds were picked on the CPU so that they hold (the smallest
margin of the grid is 5.5e-8 of the root)."""
import numpy as np

from test_per_model import ACT_DIM, ALPHA, BETA, OBS_DIM, PerModel
from test_oracle_sampler import Mirror

MARGIN, WEIGHT_SPAN = 1e-9, 0.05
STAGE_CAP = 4096                        # fsrl_ctx::STAGE_CAP (fsrl_hip.hip): the records of one staging window
PER_THREADS, PER_BOOK_LDS = 1024, 512   # kernels_per.hpp
ROWS_SEED = 21
WIDE_EMPTY, WIDE_FULL = (0, 17, 599), 300


class Geometry:
    """a store geometry plus its rollout: what tests/test_gpu_per.py's Rig is built from"""

    def __init__(self, name, E, sub, rows):
        self.name, self.E, self.sub, self.rows = name, int(E), int(sub), np.asarray(rows, np.int64)
        assert self.rows.shape == (self.E, )
        self.slots = self.E * self.sub
        self.bound = 1
        while self.bound < self.slots:
            self.bound *= 2

    def valid(self):
        """the filled slots, in slot order"""
        return np.concatenate([e * self.sub + np.arange(min(r, self.sub)) for e, r in enumerate(self.rows)])

    def rollout(self, seed=1, rows=None):
        """the vector steps that push rows[e] rows into sub-buffer e, in lock step: every live sub-buffer in every call"""
        rng = np.random.default_rng(seed)
        left = (self.rows if rows is None else np.asarray(rows, np.int64)).copy()
        steps = []
        while (left > 0).any():
            ids = np.flatnonzero(left > 0)
            k = len(ids)
            term = rng.random(k) < 0.1
            trunc = (rng.random(k) < 0.1) & ~term
            steps.append((ids.tolist(), rng.standard_normal((k, OBS_DIM)).astype(np.float32),
                          np.tanh(rng.standard_normal((k, ACT_DIM))).astype(np.float32), rng.normal(0, 1, k),
                          (rng.random(k) < 0.3).astype(np.float64), term, trunc, rng.standard_normal((k, OBS_DIM)).astype(np.float32)))
            left[ids] -= 1
        return steps

    def priorities(self, seed=2):
        """non-uniform priorities, one per filled slot, three repeated indices among them (the last entry wins), signs mixed: built
        like test_per_model.priorities"""
        valid = self.valid()
        rng = np.random.default_rng(seed)
        idx = np.concatenate([valid, valid[:3]])
        w = rng.uniform(0.05, 3.0, idx.size) * rng.choice([-1.0, 1.0], idx.size)
        return idx, w


def _wide_rows():
    rng = np.random.default_rng(ROWS_SEED)
    rows = np.where(rng.random(600) < 0.12, rng.integers(0, 8, 600), rng.integers(8, 24, 600))
    rows[list(WIDE_EMPTY)] = 0
    rows[WIDE_FULL] = 8
    return rows


WIDE = Geometry("wide", 600, 8, _wide_rows())
DEEP = Geometry("deep", 2, 70000, [300, 170])
GEOMETRIES = {"wide": WIDE, "deep": DEEP}


def windows(steps, sub, cap=STAGE_CAP):
    """the record counts of the staging windows the pushes `steps` fill, by fsrl_store_push's rule: a window is flushed when it
    holds `cap` records, or when a sub-buffer would put a row into it on top of `sub` rows of its own"""
    out, count, staged = [], 0, {}
    for ids, *_ in steps:
        for e in ids:
            if count == cap or staged.get(e, 0) == sub:
                out.append(count)
                count, staged = 0, {}
            staged[e] = staged.get(e, 0) + 1
            count += 1
    if count:
        out.append(count)
    return out


def wide_host_weights(seed=9, n=5000):
    """fsrl_per_update_weight's operands on the wide store: n entries over its filled slots -- more entries than filled slots and
    than five times the workgroup's threads, the first 300 over 7 slots only, signs mixed"""
    valid = WIDE.valid()
    rng = np.random.default_rng(seed)
    idx = rng.choice(valid, n)
    idx[:300] = rng.choice(valid[::max(1, len(valid) // 7)][:7], 300)
    w = rng.uniform(0.05, 3.0, n) * rng.choice([-1.0, 1.0], n)
    return idx, w


def later_rows(geom, per_sub, seed):
    """`per_sub` more vector steps for every sub-buffer that is not empty (a wrapped or full one overwrites slots)"""
    return geom.rollout(seed, np.where(geom.rows > 0, per_sub, 0))


# ------------------------------------------------------------------------------------------------ what the GPU tests sample with
SAMPLER_SEEDS = (3, 13)
UPDATE_SEED = 2
GROUP_SEED = 1                                          # keys the wide member of the mixed group (the small member: GROUP_SEED + 1)
WIDE_N_STEP, WIDE_BATCHES = 3, (33, 1040, 33)           # per seed of SAMPLER_SEEDS: update counts 0 .. 5
DEEP_N_STEP, DEEP_BATCH, DEEP_UPDATES = 2, 277, 2       # UPDATE_SEED; the training-state test runs 1 + 2 of them
LOSS_N_STEP, LOSS_BATCHES, LOSS_UPDATES = 2, (277, 1040), 3     # UPDATE_SEED, wide store
GROUP_CASES = (("layered", 33, 3), ("fused", 1040, 2))  # the mixed group: keyed by one own update each, then n


def sampling():
    """every (geometry name, seed, update count, batch) a GPU test draws a prioritised sample with"""
    out = []
    count = 0
    for seed in SAMPLER_SEEDS:
        for B in WIDE_BATCHES:
            out.append(("wide", seed, count, B))
            count += 1
    out += [("deep", UPDATE_SEED, u, DEEP_BATCH) for u in range(1 + DEEP_UPDATES)]
    out += [("wide", UPDATE_SEED, u, B) for B in LOSS_BATCHES for u in range(LOSS_UPDATES)]
    out += [("wide", GROUP_SEED, u, B) for _, B, n in GROUP_CASES for u in range(1 + n)]
    return out


SAMPLING = sampling()


def build(geom, alpha=ALPHA, beta=BETA, weight_norm=True, prio=True, seed=1):
    """the mirror of the geometry's store and the model after the pushes (and the priorities)"""
    mirror, model = Mirror(geom.E, geom.sub, OBS_DIM, ACT_DIM), PerModel(geom.slots, alpha, beta, weight_norm)
    for step in geom.rollout(seed):
        model.add(mirror.push(*step))
    if prio:
        model.update_weight(*geom.priorities())
    return mirror, model
