"""The inputs of tests/test_gpu_per_big.py (tests/per_big_problems.py) on the CPU, with the model alone: the conditions that keep the
GPU tests from being vacuous, and the sum tree's invariant at 8 192 and 262 144 leaves."""
import numpy as np
import pytest

import per_big_problems as P
from oracle import sampler as S
from test_per_model import ALPHA, F32_EPS, STORES, PerModel


@pytest.fixture(scope="module")
def built():
    """(mirror, model without priorities, model with them) per geometry, built once and left unchanged"""
    out = {}
    for name, geom in P.GEOMETRIES.items():
        mirror, plain = P.build(geom, prio=False)
        prio = PerModel(geom.slots, ALPHA, P.BETA).load(plain.leaves.copy())
        prio.update_weight(*geom.priorities())
        out[name] = (mirror, plain, prio)
    return out


def _assert_invariant(m):
    """node == left + right over the whole tree, nothing beyond the store's slots"""
    t, n = m.tree, m.bound
    assert np.array_equal(t[1:n], t[2:2 * n:2] + t[3:2 * n:2])
    assert not t[n + m.slots:].any() and t[0] == 0.0


def test_the_geometries_reach_the_sizes_they_are_there_for():
    w, d = P.WIDE, P.DEEP
    assert (w.slots, w.bound, d.slots, d.bound) == (4800, 8192, 140000, 262144)
    assert w.E > P.PER_BOOK_LDS                                       # the sampler's books stay in global memory
    assert w.bound // 2 > P.PER_THREADS                               # per_rebuild_kernel's loop over a level runs more than once
    assert 2 * d.bound > 1024 * 256 and 2 * d.bound - 1024 * 256 == d.bound         # per_reset_kernel: the second stride is the leaves
    assert d.rows.tolist() == [300, 170] and d.rows.sum() < d.slots // 100             # not filled
    assert STORES["np2_wrap"] == (3, 7, [16, 9, 15])                   # the mixed group's second member


def test_the_wide_store_has_the_sub_buffers_it_claims(built):
    w = P.WIDE
    mirror, _, _ = built["wide"]
    assert 0 <= w.rows.min() and w.rows.max() <= 23
    assert all(w.rows[e] == 0 for e in P.WIDE_EMPTY) and w.rows[P.WIDE_FULL] == 8
    part, full, wrapped = (w.rows > 0) & (w.rows < 8), w.rows == 8, w.rows > 8
    assert part.sum() >= 30 and full.sum() >= 10 and wrapped.sum() >= 400 and (w.rows == 0).sum() >= 3
    # side by side: a wrapped sub-buffer next to a partly filled one, and an empty one between filled ones
    assert (wrapped[:-1] & part[1:]).any() and w.rows[16] > 0 and w.rows[18] > 0
    book = mirror.book
    assert np.array_equal(book[:, 0], np.minimum(w.rows, 8)) and np.array_equal(book[:, 1], w.rows % 8)
    assert np.array_equal(mirror.valid(), w.valid())
    heads = book[wrapped, 1]
    assert len(set(heads.tolist())) == 8                              # every write head position among the wrapped ones
    # the zero subtrees: the first and the last 8-leaf run of the store, and the tail of the tree beyond its slots
    m = built["wide"][1]
    for e in P.WIDE_EMPTY:
        assert m.tree[(m.bound + 8 * e) >> 3] == 0.0
    assert m.tree[(m.bound + 8 * 1) >> 3] > 0.0 and not m.tree[m.bound + w.slots:].any()


def test_the_wide_pushes_fill_a_staging_window_to_its_cap():
    win = P.windows(P.WIDE.rollout(), P.WIDE.sub)
    assert win[0] == P.STAGE_CAP and sum(win) == P.WIDE.rows.sum()
    assert sum(n > P.PER_THREADS for n in win) >= 3                   # per_ingest's loop over k, per_repair with n > blockDim.x
    later = P.windows(P.later_rows(P.WIDE, 2, 40), P.WIDE.sub)
    assert later == [2 * (P.WIDE.rows > 0).sum()] and later[0] > P.PER_THREADS
    assert P.windows(P.DEEP.rollout(), P.DEEP.sub) == [470]


def test_the_host_weight_vector_repeats_slots_heavily():
    idx, w = P.wide_host_weights()
    assert idx.size == w.size == 5000 > 4 * P.PER_THREADS and np.isin(idx, P.WIDE.valid()).all()
    u, cnt = np.unique(idx, return_counts=True)
    assert cnt.max() >= 30 and (cnt > 1).sum() >= 500 and (w > 0).sum() > 2000 and (w < 0).sum() > 2000
    # the winner of a repeated slot is not the entry with the largest weight: a kernel that kept the maximum would be seen
    top = u[np.argmax(cnt)]
    pos = np.flatnonzero(idx == top)
    assert abs(w[pos[-1]]) < np.abs(w[pos]).max()
    assert 0.05 <= np.abs(w).min() and np.abs(w).max() <= 3.0


@pytest.mark.parametrize("name", sorted(P.GEOMETRIES))
def test_tree_invariant_through_adds_updates_and_reset(built, name):
    geom = P.GEOMETRIES[name]
    mirror, plain, prio = built[name]
    valid = mirror.valid()
    _assert_invariant(plain)
    assert (plain.leaves[valid] == 1.0).all() and plain.leaves.sum() == len(valid) == plain.total
    _assert_invariant(prio)
    idx, w = geom.priorities()
    assert prio.max_prio == np.abs(w).max() + F32_EPS and prio.min_prio == np.abs(w).min() + F32_EPS
    m = PerModel(geom.slots, ALPHA, P.BETA).load(prio.leaves.copy(), prio.max_prio, prio.min_prio)
    if name == "wide":
        m.update_weight(*P.wide_host_weights())
        _assert_invariant(m)
    m.add(valid[:2])                                     # a push after an update takes the max_prio the update left
    assert (m.leaves[valid[:2]] == m.max_prio**ALPHA).all()
    _assert_invariant(m)
    assert np.count_nonzero(m.leaves) == len(valid)
    m.reset()
    assert not m.tree.any() and m.max_prio == 1.0 and m.min_prio == 1.0


def test_gpu_inputs_land_on_filled_slots_only(built):
    """every (store, priorities, seed, update count, batch) the GPU tests sample with (none samples before the priorities are in:
    a tree of equal leaves has whole-number sums, which a uniform times the root can meet): the slots are filled ones, no comparison
    of a descent is closer than 1e-9 of the root to a tie, the weights span more than 0.05, and a batch holds a slot twice"""
    dup, smallest = False, np.inf
    for name, seed, counter, B in P.SAMPLING:
        mirror, plain, prio = built[name]
        valid = mirror.valid()
        slot, margin = prio.sample(S.key_of(seed), counter, B, with_margin=True)
        assert np.isin(slot, valid).all(), (name, seed, counter, B)
        assert margin.min() > P.MARGIN * prio.total, (name, seed, counter, B, margin.min() / prio.total)
        smallest = min(smallest, margin.min() / prio.total)
        assert np.ptp(prio.weights(slot)) > P.WEIGHT_SPAN, (name, seed, counter, B)
        dup |= len(np.unique(slot)) < B
    print(f"smallest margin of the grid: {smallest:.2e} of the root")
    assert dup


def test_the_descents_step_past_the_empty_sub_buffers(built):
    """slots on both sides of every empty sub-buffer are drawn: the descent has stepped past a zero subtree in both directions"""
    _, _, prio = built["wide"]
    slots = np.concatenate([prio.sample(S.key_of(seed), c, B) for n, seed, c, B in P.SAMPLING if n == "wide"])
    subs = np.unique(slots // 8)
    assert not np.isin(P.WIDE_EMPTY, subs).any()
    assert {1, 16, 18, 598} <= set(subs.tolist())
