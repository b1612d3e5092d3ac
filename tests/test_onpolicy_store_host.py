"""The scenarios of tests/onpolicy_store_problems.py on the host: each one reaches the state it claims to reach, a defect in the
batch order or in the unfinished-tail flags would be seen through the comparison bar, and the float64 oracle the device is
measured against is not itself the loose end (the fp32 oracle sits within a tenth of the bar of it).  Conditions, not
measurements: a scenario that misses one gets another seed or parameter scale, never another bar."""
import numpy as np
import pytest
import torch

import onpolicy_store_problems as P

NAMES = sorted(P.SCENARIOS)
_PLAYED = {}


def _played(name):
    if name not in _PLAYED:
        _PLAYED[name] = P.SCENARIOS[name].play()
    return _PLAYED[name]


def _stages(name):
    return [s for s in _played(name)[0] if len(s.batch)]


def _advs64(scn, batch, rew_norm=False):
    return scn.oracle(torch.float64, rew_norm).process(batch)["advs"].numpy()


@pytest.mark.parametrize("name", NAMES)
def test_scenario_reaches_its_state(name):
    scn = P.SCENARIOS[name]
    stages, adds = _played(name)
    assert stages and any(len(s.batch) for s in stages)
    for s in stages:
        assert np.array_equal(s.book, s.want_book), (s.name, s.book)
        assert len(s.batch) == s.sizes.sum() == s.indices.size == s.valid.size
        if not len(s.batch):
            continue
        b = s.batch
        tails = np.isin(s.indices, s.unfinished)
        few = 1 if len(b) < 16 else 2                         # tiny_sub and the 3-row cut of recut hold 7 and 9 rows
        assert b.terminated.sum() >= few and b.truncated.sum() >= few and tails.sum() >= few, \
            (s.name, int(b.terminated.sum()), int(b.truncated.sum()), int(tails.sum()))
        assert not (b.terminated & b.truncated).any()
        assert b.end_flag[tails].all() and np.array_equal(b.end_flag, b.terminated | b.truncated | tails)
        # the last row of every non-empty sub-buffer's range ends a GAE segment, whatever its flags
        last = np.cumsum(s.sizes[s.sizes > 0]) - 1
        assert b.end_flag[last].all()
    if name in ("wrapped_ragged", "layered_wrapped", "one_critic", "one_critic_layered"):
        assert stages[-1].wrapped.all() and len(set(stages[-1].book[:, 1])) == 3 and (stages[-1].book[:, 1] > 0).all()
    if name == "one_over":
        assert stages[-1].wrapped.tolist() == [False, True] and (stages[-1].sizes == 16).all()
    if name == "tiny_sub":
        assert stages[-1].sizes.tolist() == [3, 3, 1, 0] and stages[-1].wrapped.tolist() == [True, False, False, False]
    if name == "windows":
        off = P.push_offsets(adds)
        assert off[-1] == 8400 > 2 * P.STAGE_CAP
        for cut in (P.STAGE_CAP, 2 * P.STAGE_CAP):            # both window switches fall strictly inside a push call
            assert cut not in off
    if name == "recut":
        assert [(s.sub, s.num) for s in stages] == [(130, 3), (130, 3), (3, 3), (3, 3), (100, 4)]
        assert stages[3].wrapped.all()


@pytest.mark.parametrize("name", ["reset_keep", "reset_drop"])
def test_an_episode_straddles_the_reset_in_every_env(name):
    """the last row before the reset is not done in any env; the first done row after it reports the episode's length and reward
    summed across the reset (keep_statistics) or from the reset on"""
    scn = P.SCENARIOS[name]
    stages, adds = _played(name)
    before, after = stages[0], stages[-1]
    assert before.unfinished.size == scn.E                    # every env's newest row is in flight
    n_before = int(before.sizes.sum())
    rows = np.concatenate([np.stack([a[0] // scn.sub, a[1], a[2]], 1) for a in adds])        # env, ep_rew, ep_len per pushed row
    seen = np.zeros(scn.E, np.int64)
    age = np.zeros(scn.E, np.int64)                           # rows since the last done (or the start)
    first = {}
    for k, (e, ep_rew, ep_len) in enumerate(rows):
        e = int(e)
        seen[e] += 1; age[e] += 1
        if ep_len > 0:
            if k >= n_before and e not in first:
                first[e] = (int(ep_len), int(age[e]), int(seen[e] - 50))
            age[e] = 0
    assert sorted(first) == list(range(scn.E))
    for e, (ep_len, rows_of_episode, rows_after_reset) in first.items():
        assert rows_of_episode > rows_after_reset             # the episode began before the reset
        assert ep_len == (rows_of_episode if name == "reset_keep" else rows_after_reset), (e, first[e])
    assert len(after.batch) == 30 * scn.E and (after.sizes == 30).all()


@pytest.mark.parametrize("name", NAMES)
def test_one_defect_moves_the_advantages_by_100_bars(name):
    scn = P.SCENARIOS[name]
    for s in _stages(name):
        want = _advs64(scn, s.batch)
        bar = P.bar_of(want)
        moved_b = float(np.abs(_advs64(scn, s.batch_without_tails) - want).max())
        assert moved_b >= 100 * bar, (s.name, "tails", moved_b, bar)
        if s.wrapped.any():
            moved_a = float(np.abs(_advs64(scn, s.batch_from_slot0) - want).max())
            assert moved_a >= 100 * bar, (s.name, "slot 0", moved_a, bar)


@pytest.mark.parametrize("rew_norm", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_fp32_oracle_within_a_tenth_of_the_bar_of_float64(name, rew_norm):
    scn = P.SCENARIOS[name]
    for s in _stages(name):
        p32 = scn.oracle(torch.float32, rew_norm).process(s.batch)
        p64 = scn.oracle(torch.float64, rew_norm).process(s.batch)
        for k in P.PRODUCTS:
            a, b = p32[k].numpy().astype(np.float64), p64[k].numpy()
            d = float(np.abs(a - b).max())
            print(f"{name}/{s.name} rew_norm={rew_norm} {k}: fp32 - float64 = {d / P.bar_of(b) * P.BAR:.2e} of scale")
            assert d <= 0.1 * P.bar_of(b), (s.name, k, d, P.bar_of(b))


def test_cpo_case_of_the_wrapped_batch_is_not_borderline():
    """tests/test_gpu_onpolicy_store.py asks the device for the fp32 oracle's branch of CPO's dual solve on wrapped_ragged: the
    fp32 and the float64 oracle take the same one, far from its boundary (B = 2 target_kl - c^2 / S well below 0)"""
    from oracle.trust_region import CPOConfig, CPOOracle
    scn = P.SCENARIOS["wrapped_ragged"]
    s = _stages("wrapped_ragged")[-1]
    first = []
    for dtype in (torch.float32, torch.float64):
        o = CPOOracle(CPOConfig(obs_dim=scn.Do, act_dim=scn.Da, hidden=scn.hidden, max_action=1.5, **P.CPO_KW), dtype=dtype)
        o.set_params(scn.theta0(o.n_params))
        first.append(o.update(s.batch, P.CPO_COST, 1)[1][0][0])
    assert first[0]["loss/optim_case"] == first[1]["loss/optim_case"] == 0
    assert first[0]["loss/optim_B"] < -100 and first[1]["loss/optim_B"] < -100
