"""Groups of LAYERED PPO-Lagrangian contexts (fsrl_amd/csrc/host_layered_group.inc, kernels_layered_group.hpp): k seeds whose
`hidden_sizes` are not two layers of at most 256 units share every launch of the layered minibatch step (2 L + 5 launches whatever k)
and one actor launch sequence per vector step.  The grouped kernels inline the single-context bodies and keep every reduction order,
so "equal" here is bit for bit: a member against its SOLO TWIN -- an engine of the same config, parameters, store contents and
permutations updated with Engine.ppo_update -- compared with np.array_equal on the logged rows, the stopped pass and get_params(),
also after a second update (which carries the Adam moments)."""
import numpy as np
import pytest

from helpers import ppo_case
from test_gpu_group import _members
from test_gpu_group_collect import _close, _same_stores, _step_a, _step_b
from test_gpu_ppo import _rescale

pytestmark = pytest.mark.gpu


def _filled(T, seed, hidden, Do=8, Da=2, env_num=2, target_kl=None, lr=5e-4, max_grad_norm=0.5):
    """an engine of the given hidden_sizes with T vector steps of synthetic transitions in its store (T = 0: never pushed to)"""
    from fsrl_amd.engine import Engine, EngineConfig
    e = Engine(EngineConfig(obs_dim=Do, act_dim=Da, hidden_sizes=hidden, env_num=env_num, max_grad_norm=max_grad_norm,
                            target_kl=target_kl, lr=lr))
    r = np.random.default_rng(seed)
    e.set_params((0.1 * r.standard_normal(e.n_params)).astype(np.float32))
    obs = r.standard_normal((T + 1, env_num, Do)).astype(np.float32)
    ids = list(range(env_num))
    for t in range(T):
        e.push(ids, obs[t], 0.3 * r.standard_normal((env_num, Da)).astype(np.float32), r.normal(0.5, 0.5, env_num),
               (r.random(env_num) < 0.1).astype(np.float64), [False] * env_num, [t == T - 1] * env_num, obs[t + 1])
    return e


def _same_update(got, want, tag):
    (st, stop, th), (st_w, stop_w, th_w) = got, want
    assert stop == stop_w, (tag, stop, stop_w)
    assert st.shape == st_w.shape, (tag, st.shape, st_w.shape)
    assert np.array_equal(st, st_w), (tag, "logged rows", float(np.abs(st - st_w).max()))
    assert np.array_equal(th, th_w), (tag, "parameters", float(np.abs(th - th_w).max()))


def _twice(engs, solo, lags, resc, B, R, perms, after_first=None):
    """two grouped updates against two solo updates of the twins, every member against its twin after each; after_first(rows,
    stopped passes): called after the first.  -> the group's first logged rows and stopped passes"""
    from fsrl_amd.engine import EngineGroup
    grp = EngineGroup(engs)
    first = None
    for rnd in range(2):
        st, stop = grp.ppo_update(np.asarray(lags, np.float64).reshape(len(engs), -1), resc, B, R, perms=perms)
        first = first or (st, stop)
        for i, e in enumerate(solo):
            s1, sp = e.ppo_update(lags[i], resc[i], B, R, perms=perms[i])
            _same_update((st[i], stop[i], engs[i].get_params()), (s1, sp, e.get_params()), (rnd, i))
        if rnd == 0 and after_first:
            after_first(st, stop)
    grp.close()
    return first


def _meets_the_fixture(eng, cfg, g):
    """the bars of test_gpu_ppo.test_full_update_vs_golden on the engine that replayed fixture g once; -> the check for _twice"""
    def check(st, stop):
        assert st[0].shape == g["stats"].shape and (stop[0] >= 0) == bool(g["early_stop_msgs"])
        np.testing.assert_allclose(st[0], g["stats"], rtol=2e-5, atol=2e-5)
        tol = 2e-6 * max(1.0, cfg["lr"] / 5e-4)
        err = np.abs(eng.get_params() - g["theta_final"])
        assert err.max() <= 2 * tol and (err > tol).mean() <= 1e-4, (err.max(), int((err > tol).sum()))
        if eng.cfg.rew_norm:
            np.testing.assert_allclose(eng.ret_rms_get(), g["ret_rms_final"], rtol=1e-5, atol=1e-7)
            assert np.array_equal(eng.ret_rms_get()[:, 2], g["ret_rms_final"][:, 2])
    return check


@pytest.mark.parametrize("name,k", [("deep3", 3),             # k = 3: 39 weight-side jobs, more than a kernel-argument table holds
                                    ("one_layer", 2), ("wide", 2), ("deep4_options", 3)])
def test_golden_fixtures_through_a_group(name, k):
    """Member 0 replays the reference's fixture inside a group (the other members: perturbed parameters, their own multipliers and
    permutations): it meets the fixture's tolerances of test_gpu_ppo.test_full_update_vs_golden, and every member equals its twin."""
    cfg, g = ppo_case(name)
    R, B = cfg["repeat"], cfg["batch_size"]
    n = len(g["indices"])
    rng = np.random.default_rng(5)
    perms = [[rng.permutation(n) for _ in range(R)] for _ in range(k)]
    for j, pj in enumerate(g["perms"][:R]):
        perms[0][j] = pj
    solo, _, lags = _members(cfg, g, k)
    engs, _, _ = _members(cfg, g, k)
    _twice(engs, solo, lags, [_rescale(l) for l in lags], B, R, perms, after_first=_meets_the_fixture(engs[0], cfg, g))
    _close(engs, solo)


def test_minibatches_of_1300_rows_through_a_group_of_two():
    """tests/test_gpu_layered.py's large-minibatch case (hidden (64, 48, 32), 2 600 rows, batch 1 300, no gradient clip) with member 0
    on the oracle's inputs and member 1 on perturbed parameters, its own multiplier and permutations: lin_group_kernel past 512 rows.
    Member 0 meets the oracle's bars after the first update, every member equals its solo twin after both."""
    from test_gpu_layered import large_minibatch_bars, large_minibatch_case, large_minibatch_engine
    case = large_minibatch_case()
    n, R = sum(case["rows"]), case["repeat"]
    rng = np.random.default_rng(6)
    thetas = [case["theta"], case["theta"] + (0.01 * rng.standard_normal(case["theta"].size)).astype(np.float32)]
    perms = [list(case["perms"]), [rng.permutation(n) for _ in range(R)]]
    lags = [case["lag"], case["lag"] * 1.5]
    resc = [case["resc"], _rescale(lags[1])]
    engs = [large_minibatch_engine(case, th) for th in thetas]
    solo = [large_minibatch_engine(case, th) for th in thetas]
    _twice(engs, solo, lags, resc, case["B"], R, perms,
           after_first=lambda st, stop: large_minibatch_bars(case, st[0], stop[0], engs[0].get_params()))
    _close(engs, solo)


def test_ragged_shapes_row_counts_and_an_empty_member():
    """obs 17 (rows that are no multiple of 4 floats: the dword-load instantiation), act 3, hidden (33, 100, 7), gradient clip; members
    with 300 / 257 / 143 / 0 rows at batch 64: different step counts, merged last minibatches, a member that never held a row."""
    hidden, rows = (33, 100, 7), [300, 257, 143, 0]
    mk = lambda: [_filled(T, 20 + i, hidden, Do=17, Da=3, env_num=1) for i, T in enumerate(rows)]
    engs, solo = mk(), mk()
    rng = np.random.default_rng(1)
    perms = [[rng.permutation(T) for _ in range(2)] for T in rows]
    lags, resc = [[0.2], [0.5], [0.9], [0.1]], [1 / 1.2, 1 / 1.5, 1 / 1.9, 1 / 1.1]
    st, stop = _twice(engs, solo, lags, resc, 64, 2, perms)
    assert [s.shape[0] for s in st] == [2 * (T // 64) for T in rows] == [8, 8, 4, 0] and stop == [-1] * 4
    _close(engs, solo)


def test_kl_stop_per_member_with_an_empty_member_carrying_a_stale_plan():
    """The setting of test_gpu_group.test_longest_member_stops_on_kl_first_and_an_empty_member_sits_out on hidden (64, 48, 32)."""
    hidden, lens = (64, 48, 32), [700, 200, 500]
    mk = lambda: [_filled(lens[0], 1, hidden, target_kl=0.01, lr=2e-2), _filled(lens[1], 2, hidden, target_kl=0.01, lr=1e-5),
                  _filled(lens[2], 3, hidden, target_kl=0.01, lr=1e-5)]
    engs, solo = mk(), mk()
    for e in (engs[2], solo[2]):
        e.ppo_update([0.3], 1 / 1.3, 64, 1, seed=3)        # leaves a 15-minibatch plan behind ...
        e.reset_store()                                      # ... and then no rows
        assert len(e) == 0
    rng = np.random.default_rng(0)
    perms = [[rng.permutation(2 * T) for _ in range(4)] for T in lens[:2]] + [[np.zeros(0, np.int64) for _ in range(4)]]
    lags, resc = [[0.2], [0.5], [0.9]], [1 / 1.2, 1 / 1.5, 1 / 1.9]
    st, stop = _twice(engs, solo, lags, resc, 128, 4, perms)
    assert stop[0] == 0 and stop[1] == -1 and st[2].shape[0] == 0, (stop, [s.shape for s in st])
    assert st[0].shape[0] == 10 and st[1].shape[0] == 4 * 3
    _close(engs, solo)


def test_sixteen_one_layer_members_wider_than_the_fused_kernels():
    """k = 16 (the most a group takes) of hidden (300, ); 17 are refused; the same grouped update from the same state twice gives the
    same bits."""
    from fsrl_amd.engine import EngineGroup
    hidden, T, who = (300, ), 65, (0, 7, 15)                # 65 vector steps x 2 envs = 130 rows
    engs = [_filled(T, 40 + i, hidden) for i in range(16)]
    solo = [_filled(T, 40 + i, hidden) for i in who]
    extra = _filled(0, 99, hidden)
    with pytest.raises(AssertionError, match="1..16 members"):
        EngineGroup(engs + [extra])
    rng = np.random.default_rng(2)
    perms = [[rng.permutation(2 * T)] for _ in range(16)]
    lags = np.linspace(0.1, 0.9, 16).reshape(16, 1)
    resc = [_rescale(l) for l in lags]
    grp = EngineGroup(engs)
    for e in engs:
        e.state_snapshot()
    st_a, stop_a = grp.ppo_update(lags, resc, 64, 1, perms=perms)
    th_a = [e.get_params() for e in engs]
    for e in engs:
        e.state_restore()
    st_b, stop_b = grp.ppo_update(lags, resc, 64, 1, perms=perms)
    assert stop_a == stop_b == [-1] * 16
    for i, e in enumerate(engs):
        assert st_a[i].shape == (2, 11)
        assert np.array_equal(st_a[i], st_b[i]) and np.array_equal(th_a[i], e.get_params()), i
    for e, i in zip(solo, who):
        s1, sp = e.ppo_update(lags[i], resc[i], 64, 1, perms=perms[i])
        _same_update((st_a[i], stop_a[i], th_a[i]), (s1, sp, e.get_params()), i)
    grp.close()
    _close(engs, solo, extra)


def test_two_force_layered_members_on_a_fused_fixture():
    """force_layered members (a two-layer network through the layered kernels) group like any layered context: fixture c1 within its
    tolerances (tests/test_gpu_layered.py) and equal to the twins."""
    cfg, g = ppo_case("c1")
    R, B, k = cfg["repeat"], cfg["batch_size"], 2
    n = len(g["indices"])
    rng = np.random.default_rng(8)
    perms = [list(g["perms"][:R]), [rng.permutation(n) for _ in range(R)]]
    solo, _, lags = _members(cfg, g, k, force_layered=True)
    engs, _, _ = _members(cfg, g, k, force_layered=True)
    assert all(e.cfg.force_layered for e in engs)
    _twice(engs, solo, lags, [_rescale(l) for l in lags], B, R, perms, after_first=_meets_the_fixture(engs[0], cfg, g))
    _close(engs, solo)


def test_what_is_refused_and_what_survives():
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig, EngineGroup
    Do, Da = 8, 2
    lay = [_filled(75, 5, (64, 48, 32)), _filled(75, 6, (64, 48, 32))]
    ref = _filled(75, 6, (64, 48, 32))
    fused = Engine(EngineConfig(obs_dim=Do, act_dim=Da, hidden=64, env_num=2, max_grad_norm=0.5, target_kl=None))
    forced = Engine(EngineConfig(obs_dim=Do, act_dim=Da, hidden_sizes=(64, 64), force_layered=True, env_num=2, max_grad_norm=0.5,
                                 target_kl=None))
    plain = Engine(EngineConfig(obs_dim=Do, act_dim=Da, hidden_sizes=(64, 64), env_num=2, max_grad_norm=0.5, target_kl=None))
    narrow = _filled(0, 7, (64, 48, 16))
    deeper = _filled(0, 7, (64, 48, 32, 32))

    def foc(**kw):
        e = Engine(EngineConfig(algo=_lib.ALGO_FOCOPS, obs_dim=Do, act_dim=Da, n_critics=2, env_num=2, target_kl=None, **kw))
        e.focops_init()
        return e
    foc_fused, foc_lay = foc(hidden=64), foc(hidden_sizes=(64, 64, 64))
    for bad, why in (([fused, lay[0]], "one network shape"), ([lay[0], fused], "one network shape"),
                     ([lay[0], narrow], "one network shape"), ([lay[0], deeper], "one network shape"),
                     ([forced, plain], "one network shape"), ([lay[0], lay[1], lay[0]], "listed twice"),
                     ([foc_fused, foc_lay], "layered"), ([foc_lay, foc_fused], "layered")):
        with pytest.raises(AssertionError, match=why):
            EngineGroup(bad)
    # destroying member 0 first: the survivor keeps working on its own, the group reports the destroyed member
    grp = EngineGroup(lay)
    grp.set_plan(3)                                         # accepted, no effect on a layered group
    rng = np.random.default_rng(4)
    perms = [[rng.permutation(150)], [rng.permutation(150)]]
    st, _ = grp.ppo_update(np.array([[0.2], [0.4]]), [1 / 1.2, 1 / 1.4], 64, 1, perms=perms)
    s_ref, _ = ref.ppo_update([0.4], 1 / 1.4, 64, 1, perms=perms[1])
    assert np.array_equal(st[1], s_ref)
    oa = rng.standard_normal((2, Do)).astype(np.float32)
    grp.collect_step([None, None], [oa, oa], True)          # the group's collect buffers exist when the member goes
    lay[0].close()
    s_a, _ = lay[1].ppo_update([0.4], 1 / 1.4, 64, 1, perms=perms[1])
    s_b, _ = ref.ppo_update([0.4], 1 / 1.4, 64, 1, perms=perms[1])
    assert np.array_equal(s_a, s_b) and np.array_equal(lay[1].get_params(), ref.get_params())
    with pytest.raises(Exception, match="destroyed"):           # FSRL_ESTATE
        grp.ppo_update(np.array([[0.2], [0.4]]), [1 / 1.2, 1 / 1.4], 64, 1, seed=9)
    with pytest.raises(Exception, match="destroyed"):           # FSRL_ESTATE
        grp.collect_step([None, None], [oa, oa], True)
    grp.close()
    assert np.isfinite(lay[1].collect_step(None, oa, True)[0]).all()
    _close(lay[1], ref, fused, forced, plain, narrow, deeper, foc_fused, foc_lay)


def _collect_members(envs, hidden, Do, Da, seed):
    from fsrl_amd.engine import Engine, EngineConfig
    rng = np.random.default_rng(seed)
    engs = []
    for i, e in enumerate(envs):
        eng = Engine(EngineConfig(obs_dim=Do, act_dim=Da, hidden_sizes=hidden, env_num=e, buffer_size=64 * e, max_grad_norm=0.5,
                                  target_kl=None, max_action=1.5))
        eng.set_params((0.2 * rng.standard_normal(eng.n_params)).astype(np.float32))
        eng.actor_sample(np.zeros((1, Do), np.float32), seed=1000 + i)        # seeds member i's noise stream
        engs.append(eng)
    return engs


def test_lock_step_collection_is_every_members_collect_step():
    """k = 3 members of hidden (64, 48, 32), obs 11, act 3, 4 / 4 / 20 envs (twenty rows: two 16-row tiles): ten grouped calls against
    ungrouped twins calling Engine.collect_step one after the other -- actions, env actions, store pointers, episode outputs and the
    stores; one shared launch sequence per call that has rows, none once the shared path is switched off."""
    from fsrl_amd.engine import EngineGroup
    envs, hidden, Do, Da = (4, 4, 20), (64, 48, 32), 11, 3
    a, b = _collect_members(envs, hidden, Do, Da, 3), _collect_members(envs, hidden, Do, Da, 3)
    gb = EngineGroup(b)
    rng = np.random.default_rng(9)
    low = -1.0 - rng.random((3, Da)).astype(np.float32)
    high = 1.0 + rng.random((3, Da)).astype(np.float32)

    def step(s):
        prevs, oas = [], []
        for i, e in enumerate(envs):
            k = 0 if (s + i) % 4 == 0 else int(rng.integers(1, e + 1))
            ids = np.sort(rng.choice(e, k, replace=False)).astype(np.int32)
            prevs.append(None if k == 0 else (ids, rng.standard_normal((k, Do)).astype(np.float32),
                                              rng.standard_normal((k, Da)).astype(np.float32), rng.standard_normal(k),
                                              (rng.random(k) < 0.2).astype(np.float64), rng.random(k) < 0.1, rng.random(k) < 0.1,
                                              rng.standard_normal((k, Do)).astype(np.float32)))
            none = s == 6 or (s % 3 == 1 and i == s % 3) or (s == 8 and i != 1)      # s = 6: nobody acts
            ka = e if s % 2 else int(rng.integers(1, e + 1))
            oas.append(None if none else rng.standard_normal((ka, Do)).astype(np.float32))
        det, bound = s % 4 == 3, (1, 2, 0)[s % 3]
        lo, hi = (low, high) if s % 2 else (None, None)
        ra, rb = _step_a(a, prevs, oas, det, bound, lo, hi), _step_b(gb, prevs, oas, det, bound, lo, hi)
        for i, (x, y) in enumerate(zip(ra, rb)):
            for j, (u, v) in enumerate(zip(x, y)):
                assert np.array_equal(u, v), (s, i, j)
        return any(o is not None for o in oas)

    n_req = sum(step(s) for s in range(10))
    st = gb.actor_resident_stats()
    assert n_req == 9 and st == dict(launches=n_req, requests=n_req, live=False), (n_req, st)
    gb.actor_release()                                      # nothing to end
    gb.actor_set_resident(False)                            # member by member from here on
    for s in range(10, 14):
        step(s)
    assert gb.actor_resident_stats() == st
    _same_stores(a, b)
    _close(gb, a, b)


def test_three_layered_seeds_through_policy_group_and_group_collector(tmp_path):
    import torch
    from fsrl_amd.agent import PPOLagAgent
    from fsrl_amd.data import FastCollector, GroupCollector, HipVectorReplayBuffer
    from fsrl_amd.env import SyntheticSafetyVectorEnv
    from fsrl_amd.policy import PolicyGroup
    from fsrl_amd.utils import BaseLogger
    agents, cols, bufs = [], [], []
    for s in range(3):
        env = SyntheticSafetyVectorEnv(env_num=4, episode_len=40, seed=s)
        ag = PPOLagAgent(env, BaseLogger(str(tmp_path / f"s{s}"), name=f"s{s}"), cost_limit=10, device="cuda:0", seed=s,
                         hidden_sizes=(64, 64, 32), training_num=4, max_grad_norm=0.5)
        ag.policy.train()
        buf = HipVectorReplayBuffer(ag.policy.engine, None, 4)
        agents.append(ag); bufs.append(buf)
        cols.append(FastCollector(ag.policy, env, buf, exploration_noise=True, device_actor=True))
    theta0 = [ag.policy.engine.get_params().copy() for ag in agents]
    group = PolicyGroup([ag.policy for ag in agents])
    gcol = GroupCollector(group, cols)
    for cycle in range(2):
        for ag, st in zip(agents, gcol.collect(n_episode=4)):
            assert st["n/st"] == 160
            ag.policy.pre_update_fn(stats_train=st)
        group.update(bufs, batch_size=64, repeat=2)
        for col in cols:
            col.reset_buffer(keep_statistics=True)
    st = group.group.actor_resident_stats()
    assert st["requests"] > 0 and st["launches"] == st["requests"] and not st["live"]
    for ag, th0 in zip(agents, theta0):
        th = ag.policy.engine.get_params()
        assert np.isfinite(th).all() and np.abs(th - th0).max() > 1e-4
        sd = ag.policy.state_dict()
        assert tuple(sd["actor.preprocess.model.model.4.weight"].shape) == (32, 64)
        assert all(torch.isfinite(v).all() for v in sd.values() if torch.is_tensor(v) and v.is_floating_point())
    group.close()
    for ag in agents:
        ag.policy.engine.close()
