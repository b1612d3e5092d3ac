"""Grouped SAC-Lagrangian updates (fsrl_sac_group_*) against twin contexts updated alone by fsrl_sac_update: the same parameters,
the same pushed transitions, the same Philox key.

Every launch of a group takes the single-context tile-height rule applied to the whole group's launch (4-row tiles while the group
still fits one round of workgroups).  Wherever that gives the solo run's tile heights -- a group of one, batches whose solo launches
already take 16-row tiles (above 1024 rows, which also covers the split-K weight-gradient path), and small batches whose group still
fits 4-row tiles -- every member is bit-identical to its solo twin, parameters, alpha and statistics rows (EXACT_CASES).

Elsewhere (batch 256 and the actor launches at batch 1024, k > 1) the group runs 16-row tiles where the solo run runs 4-row tiles,
and a row's result changes in its last bits with the tile height (test_tile_height_changes_the_result).  Those members are NOT held
to the golden tolerances of test_gpu_sac.py (99th percentile 5e-6, max 5e-4; rows 5e-5 relative): Adam's first steps are about
lr * sign(g), so parameter entries whose gradient sits at the rounding-noise level move by O(lr) in a direction the last bits
decide.  Measured at 256 wide, batch 256, after 5 updates: 1.6e-5 at the 99th percentile.  The bounds used there are 3e-5 at the
99th percentile, 2e-3 (about 4 lr) at most, and rows to 1e-3 relative + 1e-4 absolute (LOOSE_CASES)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _engine(H, Do, Da, n_step=2, auto_alpha=True, use_lag=True, seed=0, T=150, env_num=4, lr=(5e-4, 1e-3), tau=0.05):
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig
    eng = Engine(EngineConfig(algo=_lib.ALGO_SAC_LAG, obs_dim=Do, act_dim=Da, hidden_sizes=(H, H), n_critics=2,
                              env_num=env_num, buffer_size=env_num * 400, gamma=0.99, target_kl=None))
    eng.sac_init(actor_lr=lr[0], critic_lr=lr[1], tau=tau, n_step=n_step, auto_alpha=auto_alpha, use_lagrangian=use_lag)
    rng = np.random.default_rng(100 + seed)
    eng.sac_set_params(0.1 * rng.standard_normal(eng.n_sac_actor).astype(np.float32),
                       0.1 * rng.standard_normal(eng.n_sac_critics).astype(np.float32), float(np.log(0.2)))
    ids = np.arange(env_num)
    for t in range(T):
        obs = rng.standard_normal((env_num, Do)).astype(np.float32)
        act = np.tanh(rng.standard_normal((env_num, Da))).astype(np.float32)
        term = rng.random(env_num) < 0.03
        trunc = np.full(env_num, (t + 1) % 50 == 0) & ~term
        eng.push(ids, obs, act, rng.normal(0.5, 0.5, env_num), (rng.random(env_num) < 0.2).astype(np.float64), term, trunc,
                 rng.standard_normal((env_num, Do)).astype(np.float32))
    return eng


def _state(eng):
    a, alpha = eng.sac_get_params(0)
    return a, eng.sac_get_params(1)[0], eng.sac_get_params(2)[0], alpha, eng.sac_drain()


def _same(x, y, exact, exact_params=None):
    exact_params = exact if exact_params is None else exact_params
    for j in range(3):
        if exact_params:
            assert np.array_equal(x[j], y[j]), (j, np.abs(x[j] - y[j]).max())
        else:
            # Adam's first steps are ~lr * sign(g): entries whose gradient sits at the rounding-noise level move by O(lr) in a
            # direction the last bits decide (256 wide, batch 256: 1.6e-5 at the 99th percentile after 5 updates)
            d = np.abs(x[j] - y[j])
            assert np.quantile(d, 0.99) <= 3e-5 and d.max() <= 2e-3, (j, np.quantile(d, 0.99), d.max())
    if exact_params:
        assert x[3] == y[3]
    else:
        assert abs(x[3] - y[3]) < 1e-6
    assert x[4].shape == y[4].shape
    if exact:
        assert np.array_equal(x[4], y[4])
    else:
        np.testing.assert_allclose(x[4], y[4], rtol=1e-3, atol=1e-4)     # the rows of parameters that drifted as above


def _run(shape, k, n, lam, use_lag=True, auto_alpha=True, n_step=2):
    """k members (different params, data, store lengths, keys, lambda, learning rates), n[i] grouped updates, against solo twins"""
    from fsrl_amd.engine import EngineSacGroup
    H, Do, Da, B = shape
    mk = lambda i: _engine(H, Do, Da, n_step, auto_alpha, use_lag, seed=i, T=120 + 37 * i, lr=(5e-4 * (1 + 0.1 * i), 1e-3))
    grouped, solo = [mk(i) for i in range(k)], [mk(i) for i in range(k)]
    resc = [1.0 / (1.0 + l) for l in lam]
    for i in range(k):                             # key each member's Philox stream (one own update on both twins)
        for e in (grouped[i], solo[i]):
            e.sac_update(B, [lam[i]] if use_lag else [], resc[i], seed=11 + i, sync=False)
    g = EngineSacGroup(grouped)
    g.update(B, n, [[l] for l in lam] if use_lag else None, resc)
    for i in range(k):
        for _ in range(n[i]):
            solo[i].sac_update(B, [lam[i]] if use_lag else [], resc[i], sync=False)
    out = [(_state(grouped[i]), _state(solo[i])) for i in range(k)]
    g.close()
    for e in grouped + solo:
        e.close()
    return out


DEFAULT = (128, 8, 2, 256)           # the reference's sacl_cfg.py shape
CONFIGS3 = (256, 33, 8, 1024)        # BASELINE configs[3] (smaller store)


@pytest.mark.parametrize("shape", [DEFAULT, CONFIGS3])
def test_group_of_one_is_bit_identical_to_solo(shape):
    (x, y), = _run(shape, 1, [20], [0.4])
    _same(x, y, exact=True)
    assert len(x[4]) == 21


def test_tile_height_changes_the_result():
    """Does a row's result depend on the tile height?  k = 2 with auto-alpha off (nothing feeds the logged sums back into the
    update): at batch 256 the group takes 16-row tiles where the solo twins take 4-row tiles, and the parameters after 6 updates
    differ from the solo run's; at batch 1040, where both take 16-row tiles, the same group is bit-identical.  The difference is
    the tile height's, and it is at the level of float rounding."""
    differ = False
    for x, y in _run(DEFAULT, 2, [6, 6], [0.3, 0.7], auto_alpha=False):
        for j in range(3):
            d = np.abs(x[j] - y[j]).max()
            assert d <= 1e-6
            differ |= d > 0
    assert differ, "16-row and 4-row tiles gave the same bits: the grouped tile rule could keep exactness at every batch"
    for x, y in _run((128, 8, 2, 1040), 2, [6, 6], [0.3, 0.7], auto_alpha=False):
        _same(x, y, exact=True)


EXACT_CASES = [  # H, Do, Da, B, n_step, auto_alpha, use_lagrangian, k: the group takes the solo run's tile height in every launch
    (256, 33, 8, 1040, 3, True, True, 3), (64, 33, 8, 1040, 1, False, True, 8), (128, 8, 2, 1040, 2, True, False, 8),
    (128, 8, 2, 64, 3, True, True, 3), (256, 8, 8, 64, 1, False, False, 3), (64, 8, 2, 32, 2, True, True, 8),
]


@pytest.mark.parametrize("case", EXACT_CASES)
def test_members_are_bit_identical_where_the_tile_heights_agree(case):
    H, Do, Da, B, ns, aa, ul, k = case
    n = [5, 3, 0, 5, 2, 4, 1, 5][:k]
    res = _run((H, Do, Da, B), k, n, [0.1 * (i + 1) for i in range(k)], use_lag=ul, auto_alpha=aa, n_step=ns)
    for i, (x, y) in enumerate(res):
        assert len(x[4]) == n[i] + 1
        _same(x, y, exact=True)


LOOSE_CASES = [  # H, Do, Da, B, n_step, auto_alpha, use_lagrangian: 16-row group tiles against 4-row solo tiles
    (64, 8, 2, 256, 1, True, True), (128, 8, 2, 256, 3, False, True), (256, 8, 2, 256, 1, True, False),
    (64, 33, 8, 1024, 3, True, True), (128, 33, 8, 1024, 1, False, False), (256, 33, 8, 1024, 3, True, True),
    (128, 8, 8, 1024, 1, True, True), (256, 33, 2, 256, 3, False, True),
]


@pytest.mark.parametrize("case", LOOSE_CASES)
@pytest.mark.parametrize("k", [3, 8])
def test_members_match_their_solo_twins(case, k):
    H, Do, Da, B, ns, aa, ul = case
    n = ([5, 3, 0, 5, 2, 4, 1, 5] if k == 8 else [5, 3, 0])
    lam = [0.1 * (i + 1) for i in range(k)]
    res = _run((H, Do, Da, B), k, n, lam, use_lag=ul, auto_alpha=aa, n_step=ns)
    for i, (x, y) in enumerate(res):
        assert len(x[4]) == n[i] + 1
        if n[i] == 0:
            _same(x, y, exact=True)               # a member with no updates is left untouched bit for bit
        else:
            _same(x, y, exact=False)


@pytest.mark.parametrize("plan", [0, 8])
def test_interleaved_own_updates_and_pushes(plan):
    """Own updates between grouped ones, pushes in between (they make a prefetched sample stale), and with plan 8 the side-stream
    prefetch of fsrl_sac_set_plan bit 3 on both members (the solo updates leave a prefetched sample in the other buffer set when a
    grouped call comes).  Batch 64: the group keeps the solo tile heights, so every member stays bit-identical to its twin."""
    from fsrl_amd.engine import EngineSacGroup
    H, Do, Da, B = 128, 8, 2, 64
    a = [_engine(H, Do, Da, seed=i) for i in range(2)]
    b = [_engine(H, Do, Da, seed=i) for i in range(2)]
    for e in a + b:
        e.sac_set_plan(plan)
    lam, resc = [0.2, 0.5], [1 / 1.2, 1 / 1.5]
    g = EngineSacGroup(a)
    rng = np.random.default_rng(5)
    ids = np.arange(4)
    for r in range(3):
        for i in range(2):                         # own updates before the grouped call (plan 8: each leaves a prefetch behind)
            for e in (a[i], b[i]):
                e.sac_update(B, [lam[i]], resc[i], sync=False)
        g.update(B, [3, 2], [[x] for x in lam], resc)
        for i in range(2):
            for _ in range([3, 2][i]):
                b[i].sac_update(B, [lam[i]], resc[i], sync=False)
        for e in (a[0], b[0]):                     # an own update between grouped ones
            e.sac_update(B, [lam[0]], resc[0], sync=False)
        rows = [rng.standard_normal((4, Do)).astype(np.float32) for _ in range(2)]
        for e in (a[1], b[1]):                     # pushes in between: a prefetched sample is stale
            e.push(ids, rows[0], np.zeros((4, Da), np.float32), np.ones(4), np.zeros(4), np.zeros(4, bool), np.zeros(4, bool), rows[1])
    g.close()
    for i in range(2):
        _same(_state(a[i]), _state(b[i]), exact=True)
    for e in a + b:
        e.close()


def test_resident_actor_ends_and_relaunches():
    from fsrl_amd.engine import EngineSacGroup
    H, Do, Da, B = DEFAULT
    a, b = _engine(H, Do, Da, seed=3), _engine(H, Do, Da, seed=3)
    g = EngineSacGroup([a])
    obs = np.random.default_rng(1).standard_normal((4, Do)).astype(np.float32)
    for e in (a, b):
        e.actor_sample(obs[:1], seed=9)                               # key the collectors' streams identically
        e.collect_step(None, obs)
    l0 = a.actor_resident_stats()
    assert l0["live"]
    g.update(B, [4], [[0.3]], [1 / 1.3])
    for _ in range(4):
        b.sac_update(B, [0.3], 1 / 1.3, sync=False)
    assert not a.actor_resident_stats()["live"]
    ra, rb = a.collect_step(None, obs), b.collect_step(None, obs)
    for u, v in zip(ra, rb):
        assert np.array_equal(np.asarray(u), np.asarray(v))
    assert a.actor_resident_stats()["launches"] == l0["launches"] + 1
    g.close(); a.close(); b.close()


def test_rejections_and_teardown():
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig, EngineSacGroup
    H, Do, Da, B = DEFAULT
    a, b = _engine(H, Do, Da, seed=0), _engine(H, Do, Da, seed=1)
    ddpg = Engine(EngineConfig(algo=_lib.ALGO_SAC_LAG, obs_dim=Do, act_dim=Da, hidden_sizes=(H, H), n_critics=2, env_num=4,
                               buffer_size=1600, target_kl=None))
    ddpg.sac_init(deterministic=True)
    cvpo = Engine(EngineConfig(algo=_lib.ALGO_SAC_LAG, obs_dim=Do, act_dim=Da, hidden_sizes=(H, H), n_critics=2, env_num=4,
                               buffer_size=1600, target_kl=None))
    cvpo.cvpo_init(0.1)
    lay = Engine(EngineConfig(algo=_lib.ALGO_SAC_LAG, obs_dim=Do, act_dim=Da, hidden_sizes=(64, 64, 64), n_critics=2, env_num=4,
                              buffer_size=1600, target_kl=None))
    lay.sac_init()
    other = [_engine(64, Do, Da), _engine(H, Do, Da, n_step=3), _engine(H, Do, Da, auto_alpha=False), _engine(H, Do, Da, use_lag=False)]
    why = ["DDPG-Lagrangian", "CVPO", "layered", "listed twice", "one network shape", "n_step", "auto_alpha", "use_lagrangian"]
    for bad, reason in zip(([a, ddpg], [a, cvpo], [a, lay], [a, a], *[[a, o] for o in other]), why):
        with pytest.raises(AssertionError, match=reason):      # FSRL_EINVAL, with the reason in the message
            EngineSacGroup(bad)
    g = EngineSacGroup([a, b])
    with pytest.raises(AssertionError, match="already in a SAC group"):
        EngineSacGroup([b])
    g.update(B, [1, 1], [[0.1], [0.1]], [1.0, 1.0])
    b.close()                                      # a member destroyed before its group
    with pytest.raises(RuntimeError, match="destroyed"):
        g.update(B, [1, 1], [[0.1], [0.1]], [1.0, 1.0])
    g.close()
    for e in [a, ddpg, cvpo, lay] + other:
        e.close()


def test_policy_group_matches_sequential_policy_updates(tmp_path):
    import torch
    from fsrl_amd.agent import SACLagAgent
    from fsrl_amd.data import FastCollector, HipVectorReplayBuffer
    from fsrl_amd.env import SyntheticSafetyVectorEnv
    from fsrl_amd.policy import SACPolicyGroup

    class _Log:
        def __init__(self):
            self.rows = []

        def store(self, tab=None, **kw):
            self.rows.append(sorted(kw.items()))

        def store_rows(self, keys, rows):
            self.rows.append((list(keys), np.asarray(rows).tolist()))

        def print(self, *a):
            pass

    def build(grouped):
        agents, bufs, cols, logs = [], [], [], []
        for s in range(2):
            env = SyntheticSafetyVectorEnv(env_num=4, episode_len=30, seed=10 + s)
            ag = SACLagAgent(env, None, cost_limit=10, device="cuda:0", seed=1 + s, hidden_sizes=(64, 64), training_num=4,
                             buffer_size=2000)
            ag.policy.logger = _Log()
            ag.policy.train()
            buf = HipVectorReplayBuffer(ag.policy.engine, 2000, 4)
            agents.append(ag); bufs.append(buf); logs.append(ag.policy.logger)
            cols.append(FastCollector(ag.policy, env, buf, exploration_noise=True))
        grp = SACPolicyGroup([a.policy for a in agents]) if grouped else None
        for cyc in range(2):
            n = []
            for ag, col in zip(agents, cols):
                ag.policy.engine.actor_sample(np.zeros((1, ag.policy.engine.cfg.obs_dim), np.float32), seed=40 + cyc)
                st = col.collect(n_episode=4)
                ag.policy.pre_update_fn(stats_train={"cost": 15.0 + cyc})
                n.append(round(0.1 * st["n/st"]))
            if grouped:
                grp.update(bufs, 64, n)
            else:
                for ag, buf, ni in zip(agents, bufs, n):
                    for _ in range(ni):
                        ag.policy.update(64, buf)
            for ag in agents:
                ag.policy.post_update_fn(stats_train={"cost": 15.0 + cyc})
        out = [({k: v.detach().cpu().numpy().copy() for k, v in ag.policy.state_dict().items() if torch.is_tensor(v)}, lg.rows)
               for ag, lg in zip(agents, logs)]
        if grp is not None:
            grp.close()
        for ag in agents:
            ag.policy.engine.close()
        return out

    got, want = build(True), build(False)
    for (sg, lg), (sw, lw) in zip(got, want):
        assert sg.keys() == sw.keys()
        for key in sg:
            assert np.array_equal(sg[key], sw[key]), key
        assert lg == lw
