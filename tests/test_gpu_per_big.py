"""Prioritised replay on the device at the sizes of a working store, against the exact CPU model of tests/test_per_model.py, at the
bars of tests/test_gpu_per.py (its docstring derives them): leaves and scalars at relative 1e-12, the root exactly the model's sum
over the device's own leaves, sample / chain / end bits element for element, weights at relative 1e-6, new leaves from the device's
own TD averages with numpy's duplicate winner; the weighted update against the float32 restatement at statistics 5e-5 rel + 5e-6, TD
averages 5e-5 rel + 2e-5, parameters 99 % within 5e-6 and all within 5e-4, alpha within 1e-6.

The inputs are tests/per_big_problems.py's (checked on the CPU by tests/test_per_big_host.py): `wide`, 600 x 8 slots with empty, full
and wrapped sub-buffers (bound 8 192, books beyond the sampler's LDS table, staging windows of up to 4 096 records), and `deep`,
2 x 70 000 slots holding 470 rows (bound 262 144: 18 levels, a tree of 524 288 nodes).  Which test runs which branch:

  per_repair over 13 / 18 levels                        every test here / the deep ones
  per_rebuild_kernel's second iteration per level       test_enable_on_the_filled_wide_store, test_store_fill_at_scale,
                                                        test_training_state_carries_the_deep_tree
  per_reset_kernel's grid-stride loop                   test_deep_store_enable_updates_reset_and_recut
  per_ingest_kernel's loop over k, repair with n > 1024 test_wide_leaves_follow_windows_host_weights_pushes_and_reset
  per_sample_body's books in global memory              test_wide_samples_weights_and_new_priorities_equal_the_model (solo),
                                                        test_mixed_group_members_equal_their_solo_twins (per_sample_group_kernel)
  the descent past an empty sub-buffer                  the same two, and the weighted-loss test
  per_update_body, 5 000 host indices                   test_wide_leaves_follow_windows_host_weights_pushes_and_reset
  per_fill_kernel with more jobs than workgroups        test_store_fill_at_scale
  the wgt multiply on 16-row tiles                      test_weighted_updates_match_the_restatement_on_16_row_tiles"""
import numpy as np
import pytest

import per_big_problems as P
from test_gpu_per import KEYS, LAG, RESC, Rig, _check_priorities, _check_sample, _close, rigs  # noqa: F401  (rigs: the fixture)
from test_gpu_per_group import _assert_same, _grouped, _solo, _state
from test_per_model import ACT_DIM, ALPHA, BETA, F32_EPS, OBS_DIM, Mirror, PerModel, oracle_store, priorities, restated_update

pytestmark = pytest.mark.gpu

FUSED, LAYERED = (64, 64), (32, 16, 8)


def _same_tree(x, y):
    return all(np.array_equal(u, v) for u, v in zip(x, y))


# ------------------------------------------------------------------------------------------------ a: wide store, tree maintenance
def test_wide_leaves_follow_windows_host_weights_pushes_and_reset(rigs):  # noqa: F811
    geom = P.WIDE
    r = rigs(geom, fill=False)
    m = PerModel(geom.slots, ALPHA, BETA)
    for step in geom.rollout():                      # no look at the device in between: the windows fill as test_per_big_host counts them
        m.add(r.push(step))
    dev = r.model()
    assert np.array_equal(dev.leaves, m.leaves) and (dev.max_prio, dev.min_prio) == (1.0, 1.0)       # 1 ** alpha is exact
    assert np.array_equal(np.flatnonzero(dev.leaves), geom.valid()) and dev.total == len(geom.valid())
    # 5 000 priorities from the host, slots repeated up to dozens of times
    idx, w = P.wide_host_weights()
    r.eng.per_update_weight(idx, w)
    m.update_weight(idx, w)
    dev = r.model()
    assert _close(dev.leaves, m.leaves) and _close(dev.max_prio, m.max_prio) and _close(dev.min_prio, m.min_prio)
    assert m.max_prio > 1.0 > m.min_prio
    last = np.full(geom.slots, -1)
    last[idx] = np.arange(idx.size)                  # numpy's fancy assignment: the highest position wrote the slot
    hit = np.flatnonzero(last >= 0)
    assert _close(dev.leaves[hit], (np.abs(w[last[hit]]) + F32_EPS)**ALPHA)
    # two more rows per sub-buffer (one window of more than 1 024 records): they take the new max_prio ** alpha, wrapped and full
    # sub-buffers overwrite slots with them
    new = [r.push(step) for step in P.later_rows(geom, 2, 40)]
    for ptr in new:
        m.add(ptr)
    dev = r.model()
    assert _close(dev.leaves, m.leaves) and np.array_equal(np.flatnonzero(dev.leaves), r.mirror.valid())
    assert dev.max_prio == m.max_prio and dev.min_prio == m.min_prio
    new = np.concatenate(new)
    assert new.size > P.PER_THREADS and _close(dev.leaves[new], m.max_prio**ALPHA) and len(np.unique(dev.leaves[new])) == 1
    r.eng.reset_store(False)
    leaves, mx, mn, total = r.eng.per_state()
    assert leaves.size == geom.slots and not leaves.any() and (mx, mn, total) == (1.0, 1.0, 0.0)


# ------------------------------------------------------------------------------------------------ b: wide store, sampling
def test_wide_samples_weights_and_new_priorities_equal_the_model(rigs):  # noqa: F811
    """600 sub-buffers: the prioritised sampler reads the books from global memory; n_step 3 chains over wrapped sub-buffers; the
    noise bit for bit a uniform twin's"""
    geom = P.WIDE
    r, twin = rigs(geom, n_step=P.WIDE_N_STEP), rigs(geom, n_step=P.WIDE_N_STEP, per=None)
    r.eng.per_update_weight(*geom.priorities())
    dup_seen, subs = False, set()
    for seed in P.SAMPLER_SEEDS:
        for B in P.WIDE_BATCHES:
            m = r.model()
            r.update(B, seed=seed)
            twin.update(B, seed=seed)
            idx, _, _, w = _check_sample(r, B, m, twin)
            assert np.ptp(w) > P.WEIGHT_SPAN
            _check_priorities(r, B, m, idx)
            dup_seen |= len(np.unique(idx)) < B
            subs |= set((idx // geom.sub).tolist())
            seed = 0                                    # keeps the key: the update count moves the stream
    assert dup_seen and {1, 16, 18, 598} <= subs and not subs & set(P.WIDE_EMPTY)


# ------------------------------------------------------------------------------------------------ c: deep store
def test_deep_store_enable_updates_reset_and_recut(rigs):  # noqa: F811
    geom = P.DEEP
    r = rigs(geom, n_step=P.DEEP_N_STEP, enable_first=False)            # enabled on the partly filled store
    dev = r.model()
    want = np.zeros(geom.slots)
    want[geom.valid()] = 1.0
    assert np.array_equal(dev.leaves, want) and dev.total == 470.0 and (dev.max_prio, dev.min_prio) == (1.0, 1.0)
    idx, w = geom.priorities()
    r.eng.per_update_weight(idx, w)
    m = PerModel(geom.slots, ALPHA, BETA).load(want)
    m.update_weight(idx, w)
    dev = r.model()
    assert _close(dev.leaves, m.leaves) and _close(dev.max_prio, m.max_prio) and _close(dev.min_prio, m.min_prio)
    for u in range(P.DEEP_UPDATES):                                      # 18 levels of descent and repair
        m = r.model()
        r.update(P.DEEP_BATCH, seed=P.UPDATE_SEED if u == 0 else 0)
        idx, _, _, w = _check_sample(r, P.DEEP_BATCH, m)
        assert np.ptp(w) > P.WEIGHT_SPAN
        _check_priorities(r, P.DEEP_BATCH, m, idx)
    # reset: every one of the 140 000 leaves, the second stride of the reset's loop among them
    r.eng.reset_store(False)
    leaves, mx, mn, total = r.eng.per_state()
    assert leaves.size == 140000 and not leaves.any() and (mx, mn, total) == (1.0, 1.0, 0.0)
    r.mirror = Mirror(geom.E, geom.sub, OBS_DIM, ACT_DIM)
    for step in geom.rollout(seed=3, rows=[5, 3]):
        r.push(step)
    dev = r.model()
    assert np.array_equal(np.flatnonzero(dev.leaves), [0, 1, 2, 3, 4, 70000, 70001, 70002]) and dev.leaves.sum() == 8.0 == dev.total
    # a small geometry, then the deep one again: each time a clean tree
    r.eng.store_configure(2 * 40, 2)
    step = geom.rollout(seed=4, rows=[1, 1])[0]
    r.eng.push(*step)
    leaves, mx, mn, total = r.eng.per_state()
    assert leaves.size == 80 and np.array_equal(np.flatnonzero(leaves), [0, 40]) and total == 2.0 and (leaves[[0, 40]] == 1.0).all()
    r.eng.store_configure(geom.slots, 2)
    leaves, mx, mn, total = r.eng.per_state()
    assert leaves.size == 140000 and not leaves.any() and (mx, mn, total) == (1.0, 1.0, 0.0)
    r.eng.push(*step)
    leaves, _, _, total = r.eng.per_state()
    assert np.array_equal(np.flatnonzero(leaves), [0, 70000]) and total == 2.0


# ------------------------------------------------------------------------------------------------ d: the rebuild at bound 8 192
def test_enable_on_the_filled_wide_store(rigs):  # noqa: F811
    r = rigs(P.WIDE, enable_first=False)
    dev = r.model()                                     # (the root is the model's over these leaves, exactly)
    want = np.zeros(P.WIDE.slots)
    want[r.mirror.valid()] = 1.0
    assert np.array_equal(dev.leaves, want) and dev.total == want.sum() == len(P.WIDE.valid())


# ------------------------------------------------------------------------------------------------ e: store fill at scale
def test_store_fill_at_scale(rigs):  # noqa: F811
    """twin wide contexts with max_prio raised: A is filled from an archive of 1 100 episodes of 1 - 3 rows -- at least one job each
    (store_fill_plan.hpp: a job never spans two episodes), more than the 1 024 workgroups per_fill_kernel is launched with
    (host_per.inc, per_fill) -- B pushed row by row.  Neither the archive (max_episodes is the caller's) nor the job table (grown by
    table_ensure, host_traj.inc) limits the count."""
    from fsrl_amd.engine import TrajArchive
    from test_gpu_store_fill import dataset, push_loop
    geom = P.WIDE
    a, b = rigs(geom), rigs(geom)
    lens = np.random.default_rng(8).integers(1, 4, 1100).tolist()
    data = dataset(OBS_DIM, ACT_DIM, lens, seed=3)
    k = geom.E
    z = np.zeros((k, OBS_DIM), np.float32)
    for r in (a, b):
        r.eng.per_update_weight([geom.valid()[0], geom.valid()[-1]], [2.5, 0.5])
        # close the episodes in progress: a fill refuses a sub-buffer with one open
        r.eng.push(np.arange(k), z, np.zeros((k, ACT_DIM), np.float32), np.zeros(k), np.zeros(k), np.ones(k, bool), np.zeros(k, bool), z)
    arch = TrajArchive(a.eng, 4096, 1200, 16)
    try:
        assert arch.import_rows(data) == (1100, sum(lens))
        assert a.eng.store_fill(arch) == sum(lens)
        push_loop(b.eng, data, range(1100), 0, k, 0, None, None)
        la, lb = a.eng.per_state(), b.eng.per_state()
        assert np.array_equal(la[0], lb[0]) and la[1:] == lb[1:]
        m = PerModel(geom.slots, ALPHA, BETA).load(la[0])
        top = (2.5 + F32_EPS)**ALPHA
        assert la[3] == m.total and _close(la[0].max(), top)
        assert (la[0] == la[0].max()).sum() >= 600 + 1100          # the closing row of every sub-buffer and an episode's last row at least
        assert np.array_equal(a.eng.store_sizes(), b.eng.store_sizes()) and np.count_nonzero(la[0]) == len(a.eng)
    finally:
        arch.close()


# ------------------------------------------------------------------------------------------------ f: the weighted loss on 16-row tiles
@pytest.mark.parametrize("kind,hidden,B", [("sac", FUSED, 277), ("sac", FUSED, 1040), ("ddpg", FUSED, 277), ("ddpg", FUSED, 1040),
                                           ("sac", LAYERED, 277)])
def test_weighted_updates_match_the_restatement_on_16_row_tiles(rigs, kind, hidden, B):  # noqa: F811
    """tests/test_gpu_per.py's test_weighted_updates_match_the_restatement, at its bars, on the wide store at B = 277 (17 full tiles
    and one of 5 rows) and B = 1040.  Fused contexts take 16-row Q tiles when 4 * ceil(B / 16) * n_q exceeds the CU count
    (host_sac.inc, sac_alloc_batch; nothing exposes the decision, so the condition is asserted from the device's properties): on 256
    CUs SAC-Lag (n_q = 4) at both sizes, DDPG-Lag (n_q = 2) at 1040 -- at 277 its 144 workgroups still fit, and it runs 4-row tiles
    with a last tile of one row.  Layered contexts have one tile height.

    The TD averages: a row must meet tests/test_gpu_per.py's bar, 5e-5 rel + 2e-5 against the float32 restatement, or else the
    float64-yardstick rule row by row -- the device no more than 3 x as far from a float64 run of the same updates as the float32
    restatement is.  The bar alone was wrong for fused SAC-Lag here: with these parameters the actor's sigma reaches e^2, tanh
    saturates, and log(1 - tanh^2 + eps) in the target's log-probability (alpha = 1) cancels in float32.  Measured on an MI355X,
    B = 1040, third update: 1 039 rows inside the bar, row 363 at 1.5e-4 against a bar of 8.1e-5 (device 1.2226961, float32
    restatement 1.2225486, float64 1.2189145: 3.78e-3 and 3.63e-3 from float64, ratio 1.04); over all rows the device and the
    restatement both sit up to 0.39 from float64 (mean 1.7e-2) and at most 2.8e-4 from each other.  DDPG-Lag (no log-probability):
    device, restatement and float64 agree to 4e-6."""
    import torch
    if hidden == FUSED:
        n_q = 4 if kind == "sac" else 2
        rows16 = 4 * -(-B // 16) * n_q > torch.cuda.get_device_properties(0).multi_processor_count
        assert rows16 == ((kind, B) != ("ddpg", 277))
    geom = P.WIDE
    r = rigs(geom, kind, hidden, P.LOSS_N_STEP)
    r.eng.per_update_weight(*geom.priorities())
    store, index = oracle_store(r.mirror)
    o = r.oracle
    o64 = type(o)(o.cfg, dtype=torch.float64)               # the yardstick: the same updates in float64
    o64.set_params(o.actor_flat(), o.critics_flat())
    for u in range(P.LOSS_UPDATES):
        m = r.model()
        st = r.update(B, seed=P.UPDATE_SEED if u == 0 else 0)
        idx, et, ep, w = _check_sample(r, B, m)
        assert np.ptp(w) > P.WEIGHT_SPAN                    # the weights are not uniform
        sa, sc, td_ref = restated_update(kind, o, store, index, idx, et, ep, LAG, RESC, w)
        _, _, td_64 = restated_update(kind, o64, store, index, idx, et, ep, LAG, RESC, w)
        want = {**sa, **sc}
        for j, k in enumerate(KEYS):
            if k in want:
                print(f"{kind} {hidden} B={B} update {u} {k}: device {st[j]:.8g} restatement {want[k]:.8g}")
                assert abs(st[j] - want[k]) <= 5e-5 * abs(want[k]) + 5e-6, (u, k, st[j], want[k])
        td, _ = _check_priorities(r, B, m, idx)
        in_bar = np.abs(td - td_ref) <= 5e-5 * np.abs(td_ref) + 2e-5
        d_dev, d_ref = np.abs(td.astype(np.float64) - td_64), np.abs(td_ref.astype(np.float64) - td_64)
        print(f"{kind} {hidden} B={B} update {u} max |td - td_ref| {np.abs(td - td_ref).max():.3e}, rows outside the bar "
              f"{(~in_bar).sum()}, from float64: device {d_dev.max():.3e} restatement {d_ref.max():.3e}")
        assert (in_bar | (d_dev <= 3.0 * d_ref)).all(), (np.flatnonzero(~in_bar), d_dev[~in_bar], d_ref[~in_bar])
        assert in_bar.sum() >= B - 2                        # the yardstick is for the odd ill-conditioned row, not for the batch
    refs = [(0, o.actor_flat()), (1, o.critics_flat()), (2, o.critics_flat(old=True))]
    if kind == "ddpg":
        refs.append((3, o.actor_flat(old=True)))
    for which, ref in refs:
        d = np.abs(r.eng.sac_get_params(which)[0] - ref)
        print(f"{kind} {hidden} B={B} parameters {which}: 99 % {np.quantile(d, 0.99):.3e} max {d.max():.3e}")
        assert np.quantile(d, 0.99) <= 5e-6 and d.max() <= 5e-4, (which, np.quantile(d, 0.99), d.max())
    if kind == "sac":
        assert abs(r.eng.sac_get_params(0)[1] - float(o.alpha)) < 1e-6


# ------------------------------------------------------------------------------------------------ g: training state
def test_training_state_carries_the_deep_tree(rigs):  # noqa: F811
    """export after the priorities and one update, import into a fresh context (another alpha / beta, an empty store): the rebuild
    at bound 262 144; two more updates on both are bit-identical"""
    geom, B = P.DEEP, P.DEEP_BATCH
    a = rigs(geom, n_step=P.DEEP_N_STEP)
    a.eng.per_update_weight(*geom.priorities())
    a.update(B, seed=P.UPDATE_SEED)
    blob = a.eng.train_state(with_store=True)
    b = rigs(geom, n_step=P.DEEP_N_STEP, per=(0.3, 0.1, False), fill=False)
    b.eng.load_train_state(blob)
    assert _same_tree(a.eng.per_state(), b.eng.per_state())
    for u in range(P.DEEP_UPDATES):
        sa, sb = a.update(B), b.update(B)
        assert np.array_equal(sa, sb)
        assert np.array_equal(a.eng.per_last_weights(B), b.eng.per_last_weights(B))
        assert all(np.array_equal(x, y) for x, y in zip(a.eng.sac_last_sample(B), b.eng.sac_last_sample(B)))
        assert _same_tree(a.eng.per_state(), b.eng.per_state())
    for which in (0, 1, 2):
        assert np.array_equal(a.eng.sac_get_params(which)[0], b.eng.sac_get_params(which)[0])
    leaves, mx, mn, total = b.eng.per_state()
    assert total == PerModel(geom.slots, ALPHA, BETA).load(leaves).total and np.count_nonzero(leaves) == 470 and mx > 1.0 > mn


# ------------------------------------------------------------------------------------------------ h: mixed group
def _member(i, store, hidden, B, per):
    """member i on `store` (the wide geometry, or a name of test_per_model.STORES): its own parameters, (alpha, beta, weight_norm),
    priorities and Philox key (one own update)"""
    r = Rig(store, "sac", hidden, n_step=2, per=per)
    try:
        rng = np.random.default_rng(200 + i)
        r.eng.sac_set_params((0.3 * rng.standard_normal(r.eng.n_sac_actor)).astype(np.float32),
                             (0.3 * rng.standard_normal(r.eng.n_sac_critics)).astype(np.float32), float(np.log(0.2 + 0.05 * i)))
        r.eng.per_update_weight(*(priorities(store) if isinstance(store, str) else store.priorities()))
        r.lam, r.resc = 0.1 * (i + 1), 1.0 / (1.0 + 0.1 * (i + 1))
        _solo(r, B, seed=P.GROUP_SEED + i)
    except Exception:
        r.close()
        raise
    return r


@pytest.mark.parametrize("which,B,n_upd", P.GROUP_CASES)
def test_mixed_group_members_equal_their_solo_twins(which, B, n_upd):
    """one launch over a 600 x 8 store (13 levels, books in global memory) and a 3 x 7 one (5 levels, books in LDS), the members'
    (alpha, beta, weight_norm) different: layered members and fused ones above 1024 rows have the solo tile heights
    (tests/test_gpu_per_group.py), so every member is its solo twin bit for bit"""
    from fsrl_amd.engine import EngineSacGroup
    hidden = LAYERED if which == "layered" else FUSED
    stores, pers = [P.WIDE, "np2_wrap"], [(0.6, 0.4, True), (1.0, 0.9, False)]
    made, g = [], None
    try:
        for _ in range(2):
            made.append([_member(i, stores[i], hidden, B, pers[i]) for i in range(2)])
        a, b = made
        g = EngineSacGroup([r.eng for r in a])
        m0 = a[0].model()
        n = [n_upd, n_upd - 1]
        _grouped(g, a, B, n)
        for r, ni in zip(b, n):
            for _ in range(ni):
                _solo(r, B)
        for i in range(2):
            x, y = _state(a[i], B), _state(b[i], B)
            _assert_same(x, y, i)
            assert np.ptp(x[-2]) > 0 and np.abs(x[-1]).max() > 0       # weights that differ, TD averages that are there
        assert not _close(a[0].model().leaves, m0.leaves)              # the wide member's tree moved
    finally:
        if g is not None:
            g.close()
        for rs in made:
            for r in rs:
                r.close()
