"""Groups of LAYERED FOCOPS contexts (fsrl_amd/csrc/host_focops_group.inc's layered branch, lay_fb_head_group_kernel): k seeds whose
`hidden_sizes` are not two layers of at most 256 units share every launch of the layered FOCOPS minibatch step (2 L + 5 launches
whatever k) and one actor launch sequence per vector step.  The grouped kernels inline the single-context bodies and keep every
reduction order, and the layered step has no tile-height plan, so "equal" here is bit for bit at every group size: a member against
its SOLO TWIN -- an engine of the same config, parameters, store contents and permutations updated with Engine.focops_update --
compared with np.array_equal on the logged rows, the stopped pass and get_params(), also after a second update (which carries the
Adam moments, both step counters and the psq / sig_stash parity)."""
import numpy as np
import pytest

from helpers import focops_case
from test_gpu_group_collect import _close, _same_stores, _step_a, _step_b
from test_gpu_group_focops import _engine, _nu, _perms

pytestmark = pytest.mark.gpu


def _filled(T, seed, hidden, Do=8, Da=2, env_num=2, **foc):
    """a FOCOPS engine of the given hidden_sizes with T vector steps of synthetic transitions in its store (T = 0: never pushed to)"""
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig
    e = Engine(EngineConfig(algo=_lib.ALGO_FOCOPS, obs_dim=Do, act_dim=Da, hidden_sizes=hidden, n_critics=2, env_num=env_num,
                            target_kl=None))
    e.focops_init(**foc)
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


def _twice(engs, solo, nus, B, R, perms, after_first=None, twins_first=None):
    """two grouped updates against two solo updates of the twins, every member against its twin after each; after_first(rows,
    stopped passes): called after the first grouped update; twins_first(list of (rows, stopped pass)): called on the twins' first
    updates.  -> the group's first logged rows and stopped passes"""
    from fsrl_amd.engine import EngineGroup
    grp = EngineGroup(engs)
    first = None
    for rnd in range(2):
        st, stop = grp.focops_update([x[0] for x in nus], [x[1] for x in nus], B, R, perms=perms)
        first = first or (st, stop)
        want = [e.focops_update(*nus[i], B, R, perms=perms[i]) for i, e in enumerate(solo)]
        if rnd == 0 and twins_first:
            twins_first(want)
        for i, (e, (s1, sp)) in enumerate(zip(solo, want)):
            _same_update((st[i], stop[i], engs[i].get_params()), (s1, sp, e.get_params()), (rnd, i))
        if rnd == 0 and after_first:
            after_first(st, stop)
    grp.close()
    return first


def _meets_the_fixture(eng, cfg, g):
    """the bars of test_gpu_focops.test_focops_update_vs_golden on the engine that replayed fixture g once; -> the check for _twice"""
    def check(st, stop):
        for key in ("rets", "advs", "logp_old"):
            scale = max(1.0, float(np.abs(g[key]).max()))
            np.testing.assert_allclose(eng.batch_get(key), g[key], rtol=0, atol=5e-6 * scale, err_msg=key)
        want = np.concatenate([g["stats_nu"], g["stats_actor"], g["stats_critic"]], 1)
        assert st[0].shape == want.shape and (stop[0] >= 0) == (len(g["perms"]) < cfg["repeat"])
        np.testing.assert_allclose(st[0], want, rtol=3e-5, atol=3e-5)
        d = np.abs(eng.get_params()[g["theta_final_idx"]] - g["theta_final"])
        assert np.quantile(d, 0.999) <= 5e-6 and d.max() <= 2e-3, (np.quantile(d, 0.999), d.max())
    return check


def _fixture_members(cfg, g, k, make=_engine):
    """member 0 as the fixture has it; the others on perturbed parameters with learning rates of their own"""
    return [make(cfg, g, i, **(dict(actor_lr=cfg["actor_lr"] * (1 + i), critic_lr=cfg["critic_lr"] / (1 + i)) if i else {}))
            for i in range(k)]


@pytest.mark.parametrize("name,k", [("deep3", 3), ("wide1", 2)])
def test_golden_fixtures_through_a_group(name, k):
    """Member 0 replays the reference's fixture inside a group (the other members: perturbed parameters, their own nu / nu_loss,
    permutations and learning rates): it meets test_gpu_focops.test_focops_update_vs_golden's bars, every member equals its twin."""
    cfg, g = focops_case(name)
    assert not cfg.get("recompute_advantage")
    R, B = cfg["repeat"], cfg["batch_size"]
    perms = _perms(g, cfg, k, [len(g["indices"])] * k)
    nus = [_nu(g, i) for i in range(k)]
    engs, solo = _fixture_members(cfg, g, k), _fixture_members(cfg, g, k)
    _twice(engs, solo, nus, B, R, perms, after_first=_meets_the_fixture(engs[0], cfg, g))
    _close(engs, solo)


def test_ragged_shapes_row_counts_and_an_empty_member():
    """obs 17 (rows that are no multiple of 4 floats: the dword-load instantiations), act 3, hidden (33, 100, 7), gradient clip;
    members with 300 / 257 / 143 / 0 rows at batch 64: different step counts, merged last minibatches, a member that never held a
    row.  delta is out of reach, so every member runs both passes."""
    hidden, rows = (33, 100, 7), [300, 257, 143, 0]
    mk = lambda: [_filled(T, 20 + i, hidden, Do=17, Da=3, env_num=1, max_grad_norm=0.5, delta=1e9) for i, T in enumerate(rows)]
    engs, solo = mk(), mk()
    rng = np.random.default_rng(1)
    perms = [[rng.permutation(T) for _ in range(2)] for T in rows]
    nus = [(0.1, 0.5), (0.4, -1.0), (0.0, 2.0), (1.0, 0.0)]
    st, stop = _twice(engs, solo, nus, 64, 2, perms)
    assert [s.shape[0] for s in st] == [2 * (T // 64) for T in rows] == [8, 8, 4, 0] and stop == [-1] * 4
    _close(engs, solo)


def test_kl_stop_per_member_with_an_empty_member_carrying_a_stale_plan():
    """hidden (64, 48, 32), 4 passes, one delta for all: member 0's actor learning rate carries it past delta before the last pass
    (asserted on its solo twin), member 1's does not; member 2 carries a stale minibatch plan from an earlier solo update and an
    empty store.  The stopped member sits the later passes out."""
    hidden, lens = (64, 48, 32), [350, 100, 250]
    lrs = [0.1, 1e-5, 1e-5]
    mk = lambda: [_filled(T, 1 + i, hidden, actor_lr=lrs[i]) for i, T in enumerate(lens)]
    engs, solo = mk(), mk()
    for e in (engs[2], solo[2]):
        e.focops_update(0.3, 0.0, 64, 1, seed=3)            # leaves a 7-minibatch plan behind ...
        e.reset_store()                                      # ... and then no rows
        assert len(e) == 0
    rng = np.random.default_rng(0)
    perms = [[rng.permutation(2 * T) for _ in range(4)] for T in lens[:2]] + [[np.zeros(0, np.int64) for _ in range(4)]]
    nus = [(0.2, 1.0), (0.5, -0.5), (0.9, 0.0)]

    def twins(want):
        assert 0 <= want[0][1] < 3 and want[1][1] == -1 and want[2][1] == -1, [w[1] for w in want]

    st, stop = _twice(engs, solo, nus, 128, 4, perms, twins_first=twins)
    assert st[0].shape[0] == (stop[0] + 1) * 5 and st[1].shape[0] == 4 * 1 and st[2].shape[0] == 0, (stop, [s.shape for s in st])
    _close(engs, solo)


def test_minibatches_of_1300_rows_through_a_group_of_two():
    """2 600 rows at batch 1 300 on hidden (64, 48, 32) (the setting of tests/test_gpu_layered.py's large-minibatch case): the
    grouped launches past 512 rows, where the fused FOCOPS group would switch to its split-K plan and the layered one has none."""
    hidden = (64, 48, 32)
    mk = lambda: [_filled(1300, 60 + i, hidden, max_grad_norm=0.0, actor_lr=5e-4 * (1 + i)) for i in range(2)]
    engs, solo = mk(), mk()
    rng = np.random.default_rng(6)
    perms = [[rng.permutation(2600) for _ in range(2)] for _ in range(2)]
    st, stop = _twice(engs, solo, [(0.1, 0.3), (0.6, -0.2)], 1300, 2, perms)
    assert all(s.shape[0] == (2 if sp == 0 else 4) for s, sp in zip(st, stop)), (stop, [s.shape for s in st])
    _close(engs, solo)


def test_sixteen_one_layer_members_wider_than_the_fused_kernels():
    """k = 16 (the most a group takes) of hidden (300, ); 17 are refused; the same grouped update from the same snapshot twice gives
    the same bits; members 0, 7 and 15 equal solo twins."""
    from fsrl_amd.engine import EngineGroup
    hidden, T, who = (300, ), 65, (0, 7, 15)                # 65 vector steps x 2 envs = 130 rows: two minibatches, the parity returns
    engs = [_filled(T, 40 + i, hidden) for i in range(16)]
    solo = [_filled(T, 40 + i, hidden) for i in who]
    extra = _filled(0, 99, hidden)
    with pytest.raises(AssertionError, match="1..16 members"):
        EngineGroup(engs + [extra])
    rng = np.random.default_rng(2)
    perms = [[rng.permutation(2 * T)] for _ in range(16)]
    nus = [(float(x), 1.0 - float(x)) for x in np.linspace(0.05, 0.9, 16)]
    grp = EngineGroup(engs)
    for e in engs:
        e.state_snapshot()
    st_a, stop_a = grp.focops_update([x[0] for x in nus], [x[1] for x in nus], 64, 1, perms=perms)
    th_a = [e.get_params() for e in engs]
    for e in engs:
        e.state_restore()
    st_b, stop_b = grp.focops_update([x[0] for x in nus], [x[1] for x in nus], 64, 1, perms=perms)
    assert stop_a == stop_b
    for i, e in enumerate(engs):
        assert st_a[i].shape == (2, 8)
        assert np.array_equal(st_a[i], st_b[i]) and np.array_equal(th_a[i], e.get_params()), i
    for e, i in zip(solo, who):
        s1, sp = e.focops_update(*nus[i], 64, 1, perms=perms[i])
        _same_update((st_a[i], stop_a[i], th_a[i]), (s1, sp, e.get_params()), i)
    grp.close()
    _close(engs, solo, extra)


def _forced(cfg, g, i=0, force_layered=True, **foc):
    """test_gpu_group_focops._engine with the switch that sends a two-layer network through the layered kernels"""
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig
    eng = Engine(EngineConfig(algo=_lib.ALGO_FOCOPS, obs_dim=cfg["obs_dim"], act_dim=cfg["act_dim"], hidden_sizes=tuple(cfg["hidden"]),
                              force_layered=force_layered, n_critics=2, env_num=cfg["env_num"], max_action=cfg["max_action"],
                              gamma=cfg["gamma"], gae_lambda=cfg["gae_lambda"], norm_adv=cfg["advantage_normalization"],
                              target_kl=None))
    kw = dict(actor_lr=cfg["actor_lr"], critic_lr=cfg["critic_lr"], l2_reg=cfg["l2_reg"], delta=cfg["delta"], eta=cfg["eta"],
              tem_lambda=cfg["tem_lambda"], max_grad_norm=cfg["max_grad_norm"])
    kw.update(foc)
    eng.focops_init(**kw)
    th = g["theta0"] + (0.01 * np.random.default_rng(100 + i).standard_normal(g["theta0"].size)).astype(np.float32) * (i > 0)
    eng.set_params(th)
    rows = g["env_rows"]; off = np.concatenate([[0], np.cumsum(rows)])
    for t in range(rows.max()):
        ids = [e for e in range(len(rows)) if t < rows[e]]
        sel = np.array([off[e] + t for e in ids])
        eng.push(ids, g["buf_obs"][sel], g["buf_act"][sel], g["buf_rew"][sel], g["buf_cost"][sel], g["buf_terminated"][sel],
                 g["buf_truncated"][sel], g["buf_obs_next"][sel])
    return eng


def test_two_force_layered_members_on_a_fused_fixture():
    """force_layered members (a two-layer network through the layered kernels) group like any layered context: fixture `small`
    within its bars and equal to the twins; a forced and a plain member of the same widths do not group."""
    from fsrl_amd.engine import EngineGroup
    cfg, g = focops_case("small")
    R, B, k = cfg["repeat"], cfg["batch_size"], 2
    perms = _perms(g, cfg, k, [len(g["indices"])] * k)
    nus = [_nu(g, i) for i in range(k)]
    engs, solo = _fixture_members(cfg, g, k, _forced), _fixture_members(cfg, g, k, _forced)
    assert all(e.cfg.force_layered for e in engs)
    plain = _engine(cfg, g, 1)
    with pytest.raises(AssertionError, match="one network shape"):
        EngineGroup([engs[0], plain])
    _twice(engs, solo, nus, B, R, perms, after_first=_meets_the_fixture(engs[0], cfg, g))
    _close(engs, solo, plain)


def test_forced_and_plain_two_layer_members_wider_than_the_fused_kernels_are_two_shapes():
    """both layered (320 units are more than the fused kernels hold), the same widths, force_layered differs: one network shape is
    the widths AND the switch"""
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig, EngineGroup

    def foc(**kw):
        e = Engine(EngineConfig(algo=_lib.ALGO_FOCOPS, obs_dim=8, act_dim=2, n_critics=2, env_num=2, target_kl=None, **kw))
        e.focops_init()
        return e
    forced, plain = foc(hidden_sizes=(320, 64), force_layered=True), foc(hidden_sizes=(320, 64))
    with pytest.raises(AssertionError, match="one network shape"):
        EngineGroup([forced, plain])
    _close(forced, plain)


def test_what_is_refused_and_what_survives():
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig, EngineGroup
    Do = 8
    hidden = (64, 48, 32)
    lay = [_filled(75, 5, hidden), _filled(75, 6, hidden)]
    ref = _filled(75, 6, hidden)
    narrow, deeper = _filled(0, 7, (64, 48, 16)), _filled(0, 7, (64, 48, 32, 32))
    other_l2 = _filled(0, 8, hidden, l2_reg=1e-2)

    def foc(**kw):
        e = Engine(EngineConfig(algo=_lib.ALGO_FOCOPS, obs_dim=Do, act_dim=2, n_critics=2, env_num=2, target_kl=None, **kw))
        e.focops_init()
        return e
    fused = foc(hidden=64)
    for bad, why in (([fused, lay[0]], "layered"), ([lay[0], fused], "layered"), ([lay[0], narrow], "one network shape"),
                     ([lay[0], deeper], "one network shape"), ([lay[0], other_l2], "l2_reg"),
                     ([lay[0], lay[1], lay[0]], "listed twice")):
        with pytest.raises(AssertionError, match=why):
            EngineGroup(bad)
    # a shared hyper-parameter changed between create and update is caught at the update
    grp = EngineGroup(lay)
    lay[1].focops_init(l2_reg=2e-3)
    with pytest.raises(Exception, match="l2_reg"):
        grp.focops_update([0.2, 0.4], [0.0, 0.1], 64, 1, seed=1)
    lay[1].focops_init()
    # destroying member 0 first: the survivor keeps working on its own, the group reports the destroyed member
    grp.set_plan(3)                                         # accepted, no effect on a layered group
    rng = np.random.default_rng(4)
    perms = [[rng.permutation(150)], [rng.permutation(150)]]
    st, sp = grp.focops_update([0.2, 0.4], [0.0, 0.1], 64, 1, perms=perms)
    s_ref, sp_ref = ref.focops_update(0.4, 0.1, 64, 1, perms=perms[1])
    assert sp[1] == sp_ref and np.array_equal(st[1], s_ref)
    oa = rng.standard_normal((2, Do)).astype(np.float32)
    grp.collect_step([None, None], [oa, oa], True)          # the group's collect buffers exist when the member goes
    lay[0].close()
    s_a, _ = lay[1].focops_update(0.4, 0.1, 64, 1, perms=perms[1])
    s_b, _ = ref.focops_update(0.4, 0.1, 64, 1, perms=perms[1])
    assert np.array_equal(s_a, s_b) and np.array_equal(lay[1].get_params(), ref.get_params())
    with pytest.raises(Exception, match="destroyed"):           # FSRL_ESTATE
        grp.focops_update([0.2, 0.4], [0.0, 0.1], 64, 1, seed=9)
    with pytest.raises(Exception, match="destroyed"):           # FSRL_ESTATE
        grp.collect_step([None, None], [oa, oa], True)
    grp.close()
    assert np.isfinite(lay[1].collect_step(None, oa, True)[0]).all()
    _close(lay[1], ref, narrow, deeper, other_l2, fused)


def _collect_members(envs, hidden, Do, Da, seed):
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig
    rng = np.random.default_rng(seed)
    engs = []
    for i, e in enumerate(envs):
        eng = Engine(EngineConfig(algo=_lib.ALGO_FOCOPS, obs_dim=Do, act_dim=Da, hidden_sizes=hidden, n_critics=2, env_num=e,
                                  buffer_size=64 * e, target_kl=None, max_action=1.5))
        eng.focops_init()
        eng.set_params((0.2 * rng.standard_normal(eng.n_params)).astype(np.float32))
        eng.actor_sample(np.zeros((1, Do), np.float32), seed=1000 + i)        # seeds member i's noise stream
        engs.append(eng)
    return engs


def test_lock_step_collection_is_every_members_collect_step():
    """k = 3 FOCOPS members of hidden (64, 48, 32), obs 11, act 3, 4 / 4 / 20 envs (twenty rows: two 16-row tiles): ten grouped calls
    against ungrouped twins calling Engine.collect_step one after the other -- ragged rows, a step where nobody acts, deterministic
    and stochastic steps, action bounds on and off: actions, env actions, store pointers, episode outputs and the stores; one shared
    launch sequence per call that has rows."""
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
    _same_stores(a, b)
    _close(gb, a, b)


def test_three_layered_seeds_through_policy_group_and_group_collector(tmp_path):
    """Three FOCOPSAgent(hidden_sizes=(64, 64, 32)) seeds through PolicyGroup + GroupCollector for two collect / update cycles against
    identically seeded solo twins with their own FastCollector and policy.update (the twins draw FOCOPS.learn's numpy permutations
    from a seed set before each update; the group is handed the same ones): collect stats, nu, gradient_steps, logger keys and
    parameters are equal."""
    from fsrl_amd.agent import FOCOPSAgent
    from fsrl_amd.data import FastCollector, GroupCollector, HipVectorReplayBuffer
    from fsrl_amd.env import SyntheticSafetyVectorEnv
    from fsrl_amd.policy import PolicyGroup
    from fsrl_amd.policy.focops import FOCOPS_KEYS
    from fsrl_amd.utils import BaseLogger

    class Cap:
        def __init__(self): self.rows = []
        def store(self, tab=None, **kw): self.rows.append(dict(kw))
        def print(self, *a, **k): pass

    def make(tag):
        agents, cols = [], []
        for s in range(3):
            env = SyntheticSafetyVectorEnv(env_num=4, episode_len=40, seed=s)
            ag = FOCOPSAgent(env, BaseLogger(str(tmp_path / f"{tag}{s}"), name=f"{tag}{s}"), cost_limit=10.0, device="cuda:0", seed=s,
                             hidden_sizes=(64, 64, 32), training_num=4)
            ag.policy.train()
            ag.policy.logger = Cap()
            buf = HipVectorReplayBuffer(ag.policy.engine, None, 4)
            agents.append(ag); cols.append(FastCollector(ag.policy, env, buf, exploration_noise=True, device_actor=True))
        return agents, cols

    R, B = 2, 64
    solo_agents, solo_cols = make("solo")
    grp_agents, grp_cols = make("grp")
    group = PolicyGroup([ag.policy for ag in grp_agents])
    gcol = GroupCollector(group, grp_cols)
    for cycle in range(2):
        got = gcol.collect(n_episode=4)
        want = [c.collect(n_episode=4) for c in solo_cols]
        assert got == want, cycle
        for ag, st in zip(solo_agents + grp_agents, want + got):
            assert st["n/st"] == 160
            ag.policy.pre_update_fn(stats_train=st)
        perms = []
        for i, (ag, c) in enumerate(zip(solo_agents, solo_cols)):
            seed = 100 * cycle + i
            rs = np.random.RandomState(seed)                 # the stream np.random.seed(seed) gives FOCOPS.learn
            perms.append([rs.permutation(160) for _ in range(R)])
            np.random.seed(seed)
            ag.policy.update(0, c.buffer, batch_size=B, repeat=R)
        res = group.update([c.buffer for c in grp_cols], batch_size=B, repeat=R, perms=perms)
        for a, b, rg in zip(solo_agents, grp_agents, res):
            assert float(a.policy._nu) == float(b.policy._nu)
            assert a.policy.gradient_steps == b.policy.gradient_steps and rg["gradient_steps"] > 0
            assert [tuple(sorted(r)) for r in a.policy.logger.rows] == [tuple(sorted(r)) for r in b.policy.logger.rows]
            assert set(FOCOPS_KEYS) <= {k for r in b.policy.logger.rows for k in r}
            assert np.array_equal(a.policy.engine.get_params(), b.policy.engine.get_params())
        for col in solo_cols + grp_cols:
            col.reset_buffer(keep_statistics=True)
    st = group.group.actor_resident_stats()
    assert st["requests"] > 0 and st["launches"] == st["requests"] and not st["live"]
    group.close()
    for ag in solo_agents + grp_agents:
        ag.policy.engine.close()
