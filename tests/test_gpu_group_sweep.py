"""Sweep groups: members of ONE PPO-Lagrangian group with their own hyper-parameters (GroupAgent::hp, kernels_mlp.hpp; the host
frame of host_group.inc) and, through EngineGroup.ppo_update_each, their own minibatch size and number of passes.

Two kinds of comparison, as everywhere in the group tests:
  exact    a LAYERED member's grouped update is its own Engine.ppo_update on a twin engine, bit for bit; a FUSED mixed group is
           bit-identical group against twin group;
  a bar    a fused member against its solo twin: logged rows rtol = atol = 2e-5, parameters atol = 5e-6, the bars of
           tests/test_gpu_group.py::test_members_with_different_batch_lengths_and_shape_checks, at that test's learning rate
           (the EngineConfig default), minibatch size and pass count.  Cases that need a large learning rate run layered.

Members are small: obs 8, act 2, 2 envs, 75 vector steps (150 rows; a ragged member 53: 106 rows), minibatches of 64, 2 passes,
permutations given."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DO, DA, ENVS = 8, 2, 2
LAY = (64, 48, 32)
B, R = 64, 2
ROW_BAR = dict(rtol=2e-5, atol=2e-5)
PARAM_BAR = dict(rtol=0, atol=5e-6)

# every field a sweep may vary, three ways; member 2 also normalises rewards and clips the value loss
MIX = [
    dict(eps_clip=0.2, dual_clip=None, vf_coef=0.25, max_grad_norm=0.5, norm_adv=True, use_lagrangian=True, beta1=0.9, beta2=0.999,
         adam_eps=1e-8),
    dict(eps_clip=0.1, dual_clip=1.12, vf_coef=0.5, max_grad_norm=0.3, norm_adv=False, use_lagrangian=False, beta1=0.8, beta2=0.99,
         adam_eps=1e-5),
    dict(eps_clip=0.3, dual_clip=1.5, vf_coef=1.0, max_grad_norm=1.0, norm_adv=True, use_lagrangian=True, beta1=0.95, beta2=0.9,
         adam_eps=1e-6, rew_norm=True, value_clip=True),
]
# learning rates of the layered (exact) cases: large, so that within the update's four steps ratios leave 1 +- eps_clip, pass the dual
# clip, values leave their clip range and the gradient norm passes every member's max_grad_norm (checked on the CPU with
# oracle/ppo_lag.py, and on the device by the sensitivity condition of the test itself)
LAY_LR = [2e-2, 5e-2, 5e-2]
LAGS, RESC = [[0.2], [0.5], [0.9]], [1 / 1.2, 1 / 1.5, 1 / 1.9]


def rollout(T, seed, n_params):
    """parameters and T vector steps of synthetic transitions, in push order"""
    r = np.random.default_rng(seed)
    theta = (0.1 * r.standard_normal(n_params)).astype(np.float32)
    obs = r.standard_normal((T + 1, ENVS, DO)).astype(np.float32)
    act = (0.3 * r.standard_normal((T, ENVS, DA))).astype(np.float32)
    rew = r.normal(0.5, 0.5, (T, ENVS))
    cost = (r.random((T, ENVS)) < 0.1).astype(np.float64)
    return theta, obs, act, rew, cost


def _member(hp, T, seed, hidden=None, H=64, **more):
    """an engine with the hyper-parameters hp (+ more) holding rollout(T, seed); hidden: a layered context's hidden_sizes"""
    from fsrl_amd.engine import Engine, EngineConfig
    kw = dict(obs_dim=DO, act_dim=DA, env_num=ENVS, target_kl=None)
    kw.update(hp); kw.update(more)
    if hidden is not None:
        kw["hidden_sizes"] = hidden
    else:
        kw["hidden"] = H
    e = Engine(EngineConfig(**kw))
    theta, obs, act, rew, cost = rollout(T, seed, e.n_params)
    e.set_params(theta)
    ids = list(range(ENVS))
    for t in range(T):
        e.push(ids, obs[t], act[t], rew[t], cost[t], [False] * ENVS, [t == T - 1] * ENVS, obs[t + 1])
    return e


def _close(*things):
    for t in things:
        for x in (t if isinstance(t, (list, tuple)) else [t]):
            x.close()


def _perms(rows, passes, seed=0):
    rng = np.random.default_rng(seed)
    passes = passes if isinstance(passes, (list, tuple)) else [passes] * len(rows)
    return [[rng.permutation(n) for _ in range(p)] for n, p in zip(rows, passes)]


def _exact(got, want, tag):
    (st, stop, th), (st_w, stop_w, th_w) = got, want
    assert stop == stop_w, (tag, stop, stop_w)
    assert st.shape == st_w.shape, (tag, st.shape, st_w.shape)
    assert np.array_equal(st, st_w), (tag, "logged rows", float(np.abs(st - st_w).max()) if st.size else 0.0)
    assert np.array_equal(th, th_w), (tag, "parameters", float(np.abs(th - th_w).max()))


def _within_bars(got, want, tag):
    (st, stop, th), (st_w, stop_w, th_w) = got, want
    assert stop == stop_w, (tag, stop, stop_w)
    assert st.shape == st_w.shape, (tag, st.shape, st_w.shape)
    print(tag, "rows max |d| %.3g   parameters max |d| %.3g" % (float(np.abs(st - st_w).max()) if st.size else 0.0,
                                                                 float(np.abs(th - th_w).max())))
    np.testing.assert_allclose(st, st_w, err_msg=str(tag), **ROW_BAR)
    np.testing.assert_allclose(th, th_w, err_msg=str(tag), **PARAM_BAR)


def _group_vs_solos(engs, solo, same, lags=LAGS, resc=RESC, batch=B, repeat=R, perms=None, rounds=2, each=False):
    """`rounds` grouped updates against the twins' own updates, every member compared by `same` after each (the second carries the
    Adam moments and step counters).  each: through ppo_update_each with per-member batch / repeat.  -> rows, stopped passes of round 0"""
    from fsrl_amd.engine import EngineGroup
    k = len(engs)
    grp = EngineGroup(engs)
    first = None
    try:
        for rnd in range(rounds):
            if each:
                st, stop = grp.ppo_update_each(np.asarray(lags[:k], np.float64), resc[:k], batch, repeat, perms=perms)
            else:
                st, stop = grp.ppo_update(np.asarray(lags[:k], np.float64), resc[:k], batch, repeat, perms=perms)
            first = first or (st, stop)
            for i, e in enumerate(solo):
                b_i, r_i = (batch[i], repeat[i]) if each else (batch, repeat)
                s1, sp = e.ppo_update(lags[i], resc[i], b_i, r_i, perms=perms[i])
                same((st[i], stop[i], engs[i].get_params()), (s1, sp, e.get_params()), (rnd, i))
    finally:
        grp.close()
    return first


# ------------------------------------------------------------------------------------------------ 1. creation
def test_members_that_differ_in_every_free_field_form_a_group_and_structural_differences_are_named():
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig, EngineGroup
    for hidden in (None, LAY):
        engs = [_member(hp, 4, 10 + i, hidden=hidden, lr=lr, target_kl=tk, recompute_adv=bool(i & 1))
                for i, (hp, lr, tk) in enumerate(zip(MIX, LAY_LR, (None, 0.01, 0.05)))]
        grp = EngineGroup(engs)                    # the parent refuses this: "members must share the PPO hyper-parameters"
        grp.close()
        base = MIX[0]
        a = engs[0]
        bad = [(_member(dict(base, max_grad_norm=None), 0, 1, hidden=hidden), "member 1: members must agree on whether max_grad_norm is on"),
               (_member(base, 0, 1, hidden=hidden, max_action=2.0), "member 1: members must share max_action"),
               (_member(base, 0, 1, hidden=hidden, unbounded=True), "member 1: members must share unbounded"),
               (_member(base, 0, 1, hidden=hidden, n_critics=1), "member 1: members must share n_critics"),
               (_member(base, 0, 1, hidden=(64, 48, 16) if hidden else None, H=128), "member 1: members must have one network shape")]
        for other, why in bad:
            with pytest.raises(AssertionError, match=why):
                EngineGroup([a, other])
        with pytest.raises(AssertionError, match="member 2: members must agree on whether max_grad_norm is on"):
            EngineGroup([a, engs[1], bad[0][0]])
        grp = EngineGroup(engs)                    # the refusals left the members free
        grp.close()
        _close(engs, [o for o, _ in bad])
    # a FOCOPS group is not a sweep: l2_reg must agree, as before
    foc = []
    for l2 in (1e-3, 2e-3):
        e = Engine(EngineConfig(algo=_lib.ALGO_FOCOPS, obs_dim=DO, act_dim=DA, hidden=64, n_critics=2, env_num=ENVS, target_kl=None))
        e.focops_init(l2_reg=l2)
        foc.append(e)
    with pytest.raises(AssertionError, match="l2_reg"):
        EngineGroup(foc)
    # ... and so must the PPO fields of its members' configurations
    e = Engine(EngineConfig(algo=_lib.ALGO_FOCOPS, obs_dim=DO, act_dim=DA, hidden=64, n_critics=2, env_num=ENVS, target_kl=None,
                            eps_clip=0.1))
    e.focops_init()
    with pytest.raises(AssertionError, match="must share the PPO hyper-parameters"):
        EngineGroup([foc[0], e])
    _close(foc, e)


# ------------------------------------------------------------------------------------------------ 2. layered, exact
LAY_T = [53, 75, 75]                               # 106 / 150 / 150 rows


def _lay_members(hps=MIX, lrs=LAY_LR, Ts=LAY_T, **more):
    return [_member(hp, T, 20 + i, hidden=LAY, lr=lr, **more) for i, (hp, lr, T) in enumerate(zip(hps, lrs, Ts))]


def test_layered_mixed_group_is_every_members_own_update_and_every_field_bites():
    engs, solo = _lay_members(), _lay_members()
    perms = _perms([2 * T for T in LAY_T], R)
    _group_vs_solos(engs, solo, _exact, perms=perms)
    want = [e.get_params() for e in solo]
    _close(engs, solo)
    # Sensitivity, as a condition: member i's data and parameters under member 0's hyper-parameters -- all of them, and one field at a
    # time -- end at other parameters, so a build that hands every member the first member's value of ANY field cannot pass the above.
    for i in (1, 2):
        own = dict(MIX[i], lr=LAY_LR[i])
        theirs = dict(MIX[0], lr=LAY_LR[0], rew_norm=False, value_clip=False)
        trials = [("all", dict(theirs))]
        for f in ("eps_clip", "dual_clip", "vf_coef", "max_grad_norm", "norm_adv", "use_lagrangian", "beta1", "beta2", "adam_eps"):
            if own[f] != theirs[f]:
                trials.append((f, dict(own, **{f: theirs[f]})))
        if own.get("value_clip"):
            trials.append(("value_clip", dict(own, value_clip=False)))
        for what, hp in trials:
            lr = hp.pop("lr")
            e = _member(hp, LAY_T[i], 20 + i, hidden=LAY, lr=lr)
            for _ in range(2):
                e.ppo_update(LAGS[i], RESC[i], B, R, perms=perms[i])
            assert not np.array_equal(e.get_params(), want[i]), (i, what, "the update does not depend on it: choose other data")
            e.close()


# ------------------------------------------------------------------------------------------------ 3. layered KL stop
def test_layered_kl_stop_follows_each_members_own_target():
    """member 0 has no target (a build that watches only member 0's target never stops anybody), member 1 stops after pass 0
    (the setting of tests/test_gpu_group_layered.py's KL test), member 2 never does"""
    tk, lr = [None, 0.01, 0.01], [5e-4, 2e-2, 1e-5]
    mk = lambda: [_member(MIX[0], 75, 30 + i, hidden=LAY, target_kl=tk[i], lr=lr[i]) for i in range(3)]
    engs, solo = mk(), mk()
    perms = _perms([150] * 3, 4)
    st, stop = _group_vs_solos(engs, solo, _exact, repeat=4, perms=perms)
    assert stop == [-1, 0, -1], stop
    assert [s.shape[0] for s in st] == [8, 2, 8]
    _close(engs, solo)


# ------------------------------------------------------------------------------------------------ 4. fused, H = 64, k = 3
def _fused_members(hps, Ts, H=64, seed0=40, **more):
    return [_member(hp, T, seed0 + i, H=H, **more) for i, (hp, T) in enumerate(zip(hps, Ts))]


def _fused_twin_groups(mk, rows, batch=B, repeat=R, plans=(-1, -1), lags=None, resc=None, perms=None):
    """two (or more) groups built alike, one per plan, two updates each -> per group (rows 1, rows 2, stopped 1, parameters)"""
    from fsrl_amd.engine import EngineGroup
    k = len(rows)
    lags = np.asarray(lags if lags is not None else np.linspace(0.1, 0.9, k).reshape(k, 1), np.float64)
    resc = resc if resc is not None else [1.0 / (1.0 + float(l)) for l in lags[:, 0]]
    perms = perms if perms is not None else _perms(rows, repeat, seed=3)
    out = []
    for plan in plans:
        engs = mk()
        grp = EngineGroup(engs)
        grp.set_plan(plan)
        st1, stop1 = grp.ppo_update(lags, resc, batch, repeat, perms=perms)
        st2, _ = grp.ppo_update(lags, resc, batch, repeat, perms=perms)
        out.append((st1, st2, stop1, [e.get_params() for e in engs]))
        grp.close()
        _close(engs)
    return out, perms, lags, resc


def _same_bits(a, b, tag):
    for i in range(len(a[3])):
        assert a[2][i] == b[2][i], (tag, i, a[2], b[2])
        assert np.array_equal(a[0][i], b[0][i]) and np.array_equal(a[1][i], b[1][i]), (tag, i, "logged rows")
        assert np.array_equal(a[3][i], b[3][i]), (tag, i, "parameters")


@pytest.mark.parametrize("clip", [True, False])
def test_fused_mixed_group_equals_its_twin_and_meets_the_bars_of_every_solo(clip):
    """clip False: max_grad_norm off on all members -- the 2-launch step, Adam and the KL gate inside the weight-gradient kernel"""
    hps = [dict(hp) if clip else dict(hp, max_grad_norm=None) for hp in MIX]
    Ts = LAY_T
    rows = [2 * T for T in Ts]
    mk = lambda: _fused_members(hps, Ts)
    (ga, gb), perms, lags, resc = _fused_twin_groups(mk, rows)
    _same_bits(ga, gb, "twin")
    assert all(np.isfinite(s).all() for s in ga[0]) and [s.shape[0] for s in ga[0]] == [2, 4, 4]      # 106 rows: one merged minibatch
    # against the solos: rows and parameters after ONE update each, the bars of tests/test_gpu_group.py:125-126
    engs, solo = mk(), mk()
    _group_vs_solos(engs, solo, _within_bars, lags=lags.tolist(), resc=resc, perms=perms, rounds=1)
    _close(engs, solo)


# ------------------------------------------------------------------------------------------------ 5. fused launch forms
def _cycle(hps, k):
    return [dict(hps[i % len(hps)]) for i in range(k)]


def test_fused_tall_mixed_and_sixteen_row_plans_give_the_same_bits_in_a_mixed_group():
    """H = 128, k = 8, one 256-row minibatch each: 8 x 16 tiles x 3 networks exceed the CUs, so the automatic plan runs 32-row tiles
    (ppo_fwd_bwd_group_mix_kernel), plan 4 a mix of both heights, plan 0 the 16-row kernel"""
    k, T = 8, 128
    hps = _cycle(MIX, k)
    mk = lambda: _fused_members(hps, [T] * k, H=128, seed0=60)
    got, _, _, _ = _fused_twin_groups(mk, [2 * T] * k, batch=256, repeat=2, plans=(0, -1, 4))
    assert all(np.isfinite(s).all() and s.shape == (2, 11) for s in got[0][0])
    _same_bits(got[0], got[1], "automatic")
    _same_bits(got[0], got[2], "four tall tiles")
    # and the members did not all get one member's values: members 0 and 3 share hyper-parameters, members 0 and 1 do not; with the
    # same data, parameters, multipliers and permutations a pair's rows agree exactly when its hyper-parameters do
    mk2 = lambda: [_member(hp, T, 60, H=128) for hp in (MIX[0], MIX[1], MIX[0])]
    (g,), _, _, _ = _fused_twin_groups(mk2, [2 * T] * 3, batch=256, repeat=2, plans=(-1,), lags=[[0.4]] * 3, resc=[1 / 1.4] * 3,
                                       perms=_perms([2 * T], 2) * 3)
    assert np.array_equal(g[0][0], g[0][2]) and np.array_equal(g[3][0], g[3][2])
    assert not np.array_equal(g[0][0], g[0][1]) and not np.array_equal(g[3][0], g[3][1])


def test_fused_big_weight_gradient_form_in_a_mixed_group():
    """one 320-row minibatch per member: above 256 rows the grouped weight-gradient kernel takes its chunked (BIG) form"""
    T = 160
    mk = lambda: _fused_members(MIX, [T] * 3, seed0=70)
    (ga, gb), perms, lags, resc = _fused_twin_groups(mk, [2 * T] * 3, batch=320, repeat=2)
    _same_bits(ga, gb, "twin")
    engs, solo = mk(), mk()
    _group_vs_solos(engs, solo, _within_bars, lags=lags.tolist(), resc=resc, batch=320, perms=perms, rounds=1)
    _close(engs, solo)


def test_fused_group_of_one_with_its_own_hyper_parameters_is_its_solo_update():
    """k = 1, one 64-row minibatch: 4-row tiles, and the launch shapes of the solo step -- bit for bit"""
    mk = lambda: _fused_members([MIX[1]], [32], seed0=80)
    engs, solo = mk(), mk()
    st, _ = _group_vs_solos(engs, solo, _exact, lags=[[0.5]], resc=[1 / 1.5], perms=_perms([64], R))
    assert st[0].shape == (2, 11)
    _close(engs, solo)


# ------------------------------------------------------------------------------------------------ 6. fused KL stop
def test_fused_kl_stop_follows_each_members_own_target():
    """At the default learning rate member 0's mean KL per pass is -1e-4, 4e-4, 1e-3 (oracle/ppo_lag.py on the CPU): with a target of
    1e-4 (threshold 1.5e-4) it runs pass 1 and stops after it.  Member 1 has no target, member 2 a target of 1 it never reaches.  No
    pass's mean KL is within a factor 2 of its member's threshold (asserted on the solo runs), so rounding cannot flip a verdict."""
    tk = [1e-4, None, 1.0]
    mk = lambda: [_member(MIX[i], 75, 90 + i, target_kl=tk[i]) for i in range(3)]
    engs, solo = mk(), mk()
    perms = _perms([150] * 3, 3)
    from fsrl_amd.engine import EngineGroup
    grp = EngineGroup(engs)
    st, stop = grp.ppo_update(np.asarray(LAGS, np.float64), RESC, B, 3, perms=perms)
    grp.close()
    for i, e in enumerate(solo):
        s1, sp = e.ppo_update(LAGS[i], RESC[i], B, 3, perms=perms[i])
        kl = s1[:, 5].reshape(-1, 2).astype(np.float64).mean(1)          # per pass: two minibatches
        print("member", i, "mean KL per pass", kl, "stopped", sp)
        if tk[i] is not None:
            thr = 1.5 * tk[i]
            assert all(x >= 2 * thr or x <= thr / 2 for x in kl), (i, kl, thr)
        assert stop[i] == sp and st[i].shape == s1.shape, (i, stop, sp, st[i].shape, s1.shape)
        np.testing.assert_allclose(st[i], s1, **ROW_BAR)
    assert stop == [1, -1, -1] and [s.shape[0] for s in st] == [4, 6, 6], (stop, [s.shape for s in st])
    _close(engs, solo)


# ------------------------------------------------------------------------------------------------ 7. ppo_update_each
EACH_B, EACH_R = [64, 32, 150], [2, 1, 3]


def test_layered_update_each_is_every_members_own_batch_size_and_pass_count():
    engs, solo = _lay_members(Ts=[75] * 3), _lay_members(Ts=[75] * 3)
    perms = _perms([150] * 3, EACH_R)
    st, stop = _group_vs_solos(engs, solo, _exact, batch=EACH_B, repeat=EACH_R, perms=perms, each=True)
    assert [s.shape[0] for s in st] == [2 * 2, 1 * 4, 3 * 1] and stop == [-1] * 3
    _close(engs, solo)


def test_a_member_with_no_pass_sits_the_update_out():
    """repeat 0: no rows, and parameters, Adam moments and step counters untouched -- its NEXT update is that of a twin whose own
    update with repeat 0 did the same (sampled and processed its batch, stepped nothing)"""
    engs, solo = _lay_members(Ts=[75] * 3), _lay_members(Ts=[75] * 3)
    before = engs[1].get_params()
    perms = _perms([150] * 3, [2, 0, 2])
    st, stop = _group_vs_solos(engs, solo, _exact, batch=[64] * 3, repeat=[2, 0, 2], perms=perms, rounds=1, each=True)
    assert st[1].shape == (0, 11) and stop == [-1] * 3 and np.array_equal(engs[1].get_params(), before)
    perms = _perms([150] * 3, [1, 2, 1], seed=1)
    _group_vs_solos(engs, solo, _exact, batch=[64] * 3, repeat=[1, 2, 1], perms=perms, rounds=1, each=True)
    _close(engs, solo)


def test_fused_update_each_meets_the_bars_and_uniform_arrays_are_ppo_update():
    from fsrl_amd.engine import EngineGroup
    mk = lambda: _fused_members(MIX, [75] * 3, seed0=100)
    engs, solo = mk(), mk()
    perms = _perms([150] * 3, EACH_R)
    st, stop = _group_vs_solos(engs, solo, _within_bars, batch=EACH_B, repeat=EACH_R, perms=perms, rounds=1, each=True)
    assert [s.shape[0] for s in st] == [4, 4, 3] and stop == [-1] * 3
    _close(engs, solo)
    # uniform arrays: the bits of ppo_update, fused and layered
    for hidden in (None, LAY):
        mk = lambda: [_member(hp, 75, 110 + i, hidden=hidden) for i, hp in enumerate(MIX)]
        a, b = mk(), mk()
        ga, gb = EngineGroup(a), EngineGroup(b)
        perms = _perms([150] * 3, R)
        for rnd in range(2):
            st_a, stop_a = ga.ppo_update(np.asarray(LAGS), RESC, B, R, perms=perms)
            st_b, stop_b = gb.ppo_update_each(np.asarray(LAGS), RESC, [B] * 3, [R] * 3, perms=perms)
            for i in range(3):
                _exact((st_a[i], stop_a[i], a[i].get_params()), (st_b[i], stop_b[i], b[i].get_params()), (hidden, rnd, i))
        _close(ga, gb, a, b)


# ------------------------------------------------------------------------------------------------ 8. refusal
@pytest.mark.parametrize("hidden", [None, LAY], ids=["fused", "layered"])
def test_a_refused_update_each_leaves_the_group_as_it_was(hidden):
    """the shape of tests/test_gpu_group_refusals.py through ppo_update_each: a permutation that is bad for the LAST member"""
    from fsrl_amd.engine import EngineGroup
    hps = [dict(hp, rew_norm=False, value_clip=False) for hp in MIX]        # (a second begin would update the return statistics again)
    mk = lambda: [_member(hp, 75, 120 + i, hidden=hidden) for i, hp in enumerate(hps)]
    a, b, c = mk(), mk(), mk()
    perms = _perms([150] * 3, EACH_R)
    bad = [[p.copy() for p in m] for m in perms]
    bad[-1][0][3] = 150
    ga, gb, gc = EngineGroup(a), EngineGroup(b), EngineGroup(c)
    try:
        for g in (ga, gc):
            with pytest.raises(AssertionError, match="out of range"):
                g.ppo_update_each(np.asarray(LAGS), RESC, EACH_B, EACH_R, perms=bad)
        for i, e in enumerate(c):
            st, _ = e.ppo_update(LAGS[i], RESC[i], EACH_B[i], EACH_R[i], perms=perms[i])
            assert st.shape[0] > 0 and np.isfinite(st).all(), i
        for rnd in range(2):
            (st_a, stop_a), (st_b, stop_b) = [g.ppo_update_each(np.asarray(LAGS), RESC, EACH_B, EACH_R, perms=perms) for g in (ga, gb)]
            for i in range(3):
                _exact((st_a[i], stop_a[i], a[i].get_params()), (st_b[i], stop_b[i], b[i].get_params()), (rnd, i))
    finally:
        _close(ga, gb, gc, a, b, c)


# ------------------------------------------------------------------------------------------------ 9. facade
class _Rec:
    """a logger that records what the policies hand it (store_rows: the per-step table, as the package's loggers take it)"""

    def __init__(self):
        self.tables, self.stored, self.printed = [], [], []

    def store_rows(self, keys, table):
        self.tables.append((list(keys), np.array(table)))

    def store(self, tab=None, **kw):
        self.stored.append((tab, dict(kw)))

    def print(self, *a, **k):
        self.printed.append(a[0] if a else "")


def test_policy_group_over_a_sweep_is_the_policies_updated_one_by_one(tmp_path):
    """three layered PPOLagrangian policies that differ in eps_clip, target_kl, batch_size and repeat (learning rate 2e-2, so that
    targets are reached): per member the logged tables, messages, gradient_steps and parameters of its own PPOLagrangian.update"""
    from fsrl_amd.agent import PPOLagAgent
    from fsrl_amd.data import HipVectorReplayBuffer
    from fsrl_amd.env import SyntheticSafetyVectorEnv
    from fsrl_amd.policy import PolicyGroup
    from fsrl_amd.utils import BaseLogger
    eps, tkl, bsz, rep = [0.2, 0.1, 0.3], [0.01, 1e-3, 100.0], [64, 32, 150], [3, 4, 2]
    dirs = iter(range(6))

    def make():
        pols, bufs = [], []
        for i in range(3):
            env = SyntheticSafetyVectorEnv(env_num=ENVS, obs_dim=DO, act_dim=DA, episode_len=40, seed=i)
            ag = PPOLagAgent(env, BaseLogger(str(tmp_path / f"m{next(dirs)}"), name="m"), cost_limit=10, device="cuda:0",
                             seed=i, hidden_sizes=LAY, training_num=ENVS, max_grad_norm=0.5, lr=2e-2, eps_clip=eps[i], target_kl=tkl[i])
            p = ag.policy
            p.train()
            p.logger = _Rec()
            e = p.engine
            _, obs, act, rew, cost = rollout(75, 130 + i, 1)
            for t in range(75):
                e.push(list(range(ENVS)), obs[t], act[t], rew[t], cost[t], [False] * ENVS, [t == 74] * ENVS, obs[t + 1])
            pols.append(p); bufs.append(HipVectorReplayBuffer(e, None, ENVS))
            env.close()
        return pols, bufs

    (one, one_bufs), (grp_pols, grp_bufs) = make(), make()
    for a, b in zip(one, grp_pols):
        assert np.array_equal(a.engine.get_params(), b.engine.get_params())
    group = PolicyGroup(grp_pols)
    for rnd in range(2):
        want, perms = [], []
        for i, p in enumerate(one):                                 # PPOLagrangian.learn draws np.random.permutation per pass
            np.random.seed(1000 * rnd + i)
            want.append(p.update(0, one_bufs[i], batch_size=bsz[i], repeat=rep[i]))
            np.random.seed(1000 * rnd + i)
            perms.append([np.random.permutation(150) for _ in range(rep[i])])
        got = group.update(grp_bufs, batch_size=bsz, repeat=rep, perms=perms)
        print("round", rnd, want)
        assert got == want, (rnd, got, want)
        assert len({w["early_stop_pass"] for w in want}) > 1, "the members' targets should end their updates at different passes"
        for i, (a, b) in enumerate(zip(one, grp_pols)):
            assert a.gradient_steps == b.gradient_steps and a.logger.printed == b.logger.printed and a.logger.stored == b.logger.stored, i
            assert len(a.logger.tables) == len(b.logger.tables) == rnd + 1
            (ka, ta), (kb, tb) = a.logger.tables[-1], b.logger.tables[-1]
            assert ka == kb and ta.shape == tb.shape and np.array_equal(ta, tb), (rnd, i)
            assert np.array_equal(a.engine.get_params(), b.engine.get_params()), (rnd, i)
    group.close()
    for p in one + grp_pols:
        p.engine.close()


# ------------------------------------------------------------------------------------------------ the FOCOPS group on the shared frame
def test_a_layered_focops_group_takes_batch_sizes_and_pass_counts_per_member():
    """The FOCOPS update runs inside the same frame (host_group.inc: ogroup_*), so ppo_update_each's minibatch size and pass count per
    member reach it too; a layered FOCOPS member's grouped update is its own Engine.focops_update bit for bit.  (Its hyper-parameters
    stay shared: test 1.)"""
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig, EngineGroup
    nus, nls = [0.1, 0.4, 0.2], [0.5, -1.0, 0.3]

    def mk():
        out = []
        for i in range(3):
            e = Engine(EngineConfig(algo=_lib.ALGO_FOCOPS, obs_dim=DO, act_dim=DA, hidden_sizes=(64, 64, 64), n_critics=2, env_num=ENVS,
                                    target_kl=None))
            e.focops_init(actor_lr=5e-4 * (1 + i), delta=1e9)          # (no KL stop: every member runs its own passes)
            theta, obs, act, rew, cost = rollout(75, 140 + i, e.n_params)
            e.set_params(theta)
            for t in range(75):
                e.push(list(range(ENVS)), obs[t], act[t], rew[t], cost[t], [False] * ENVS, [t == 74] * ENVS, obs[t + 1])
            out.append(e)
        return out

    engs, solo = mk(), mk()
    perms = _perms([150] * 3, EACH_R)
    grp = EngineGroup(engs)
    for rnd in range(2):
        for e, nu, nl in zip(engs, nus, nls):
            _lib.check(e.lib.fsrl_focops_set_nu(e._ctx, nu, nl))
        st, stop = grp.ppo_update_each(np.zeros((3, 1)), np.ones(3), EACH_B, EACH_R, perms=perms)
        for i, e in enumerate(solo):
            s1, sp = e.focops_update(nus[i], nls[i], EACH_B[i], EACH_R[i], perms=perms[i])
            _exact((st[i][:, :_lib.FOCOPS_NSTATS], stop[i], engs[i].get_params()), (s1, sp, e.get_params()), (rnd, i))
        assert [s.shape[0] for s in st] == [4, 4, 3] and stop == [-1] * 3
    _close(grp, engs, solo)
