"""Grouped DDPG-Lagrangian updates (fsrl_sac_group_* over deterministic-actor contexts) against twin contexts updated alone by
fsrl_sac_update: the same parameters, the same pushed transitions, the same Philox key.  Members differ in parameters, data, store
length, key, lambda, actor_lr and tau.  The compared state is the actor, the critics, the critics' targets, the TARGET ACTOR
(sac_get_params(3): the one array the SAC-Lag group never had to move -- the forward launch's first half reads it, the actor's Adam
pass moves it by the member's own tau) and the drained statistics rows.

Every launch of a group takes the single-context tile-height rule applied to the whole group's launch, with the group's n_q = 2:
    Q launches    4-row tiles while 4 * tiles * 2 * k <= CUs
    backward      4-row tiles while 4 * tiles * k <= CUs
    forward       as the backward, and 8 * tiles * k <= CUs (two batches in one launch)
The cases are chosen for 256 CUs (on another CU count the module is skipped: the rule would give other tile heights).

Wherever the rule gives the solo run's tile heights, every member is bit-identical to its solo twin (EXACT_CASES; a group of one;
and, under FSRL_TILE16 on members and twins alike, the default shape at k = 8).  DEFAULT at k = 2 is exactly one round
(4 * 16 * 2 * 2 = 256 and 8 * 16 * 2 = 256): the SAC-Lag group, with n_q = 4, is not exact there.

Elsewhere (MIXED_SHAPES: at k = 3 the Q launches and the forward take 16-row tiles while the backward keeps 4-row tiles; at k = 8 the
members take 16-row tiles, the solo twins 4-row tiles) a row's result changes in its last bits with the tile height, and Adam's
first steps, about lr * sign(g), move entries whose gradient sits at the rounding-noise level by O(lr) in a direction the last bits
decide (tests/test_gpu_sac_group.py).  The bounds there are not fitted to the grouped path.  They are twice the distance between
two SOLO twins (same parameters, data and key), one of them created under FSRL_TILE16, after the keying update and 5 more on the
single path: measured on an MI355X for each of the eight member configurations of `_member` at both MIXED_SHAPES, the largest
of the sixteen pairs taken for each kind (the single path is bit-reproducible, so these figures do not move from run to run):

                                     (128, 8, 2, 256)      (256, 33, 8, 256)     bound (2 x the larger, 4th digit rounded up)
    parameters, 99th percentile      7.451e-9              1.4901e-8             2.981e-8
    parameters, maximum              4.619e-7              2.7046e-5             5.410e-5
    rows, absolute                   2.384e-7              4.7684e-7             9.537e-7
    rows, relative to the column     2.459e-7              4.6821e-7             9.365e-7

(member 0 alone: 7.5e-9 / 3.7e-8 / 1.2e-7 / 1.0e-7 and 7.5e-9 / 1.4e-5 / 2.4e-7 / 1.3e-7.)  "parameters": the largest over the
four arrays (actor, critics, critics' targets, target actor).  "rows, absolute": the largest |difference| of a logged value; "rows,
relative": per column, the largest |difference| over the largest |value| of the column, the largest column.  Every kind is asserted
on its own.  The distances are far below the SAC-Lag group's (1.6e-5 at the 99th percentile); lr-sized moves show in the maximum
only.  The measured twins differ in six updates (the keying one too), the grouped members in at most five.  Grouped against
solo on an MI355X, the largest over all members of the four cases below: 7.5e-9, 1.3e-7, 4.8e-7, 2.9e-7 (each is printed)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_CUS = 256                          # the tile-height cases below are derived for this many compute units
P99_BOUND, MAX_BOUND, ROW_ABS_BOUND, ROW_REL_BOUND = 2.981e-8, 5.410e-5, 9.537e-7, 9.365e-7      # module docstring


@pytest.fixture(scope="module", autouse=True)
def _cu_count():
    import torch
    n = torch.cuda.get_device_properties(0).multi_processor_count
    if n != N_CUS:
        pytest.skip("the tile-height cases are derived for %d compute units; this device has %d" % (N_CUS, n))


def _config(H, Do, Da, env_num=4):
    from fsrl_amd import _lib
    from fsrl_amd.engine import EngineConfig
    hs = tuple(H) if isinstance(H, (tuple, list)) else (H, H)
    return EngineConfig(algo=_lib.ALGO_SAC_LAG, obs_dim=Do, act_dim=Da, hidden_sizes=hs, n_critics=2, env_num=env_num,
                        buffer_size=env_num * 400, gamma=0.99, target_kl=None)


def _engine(H, Do, Da, n_step=2, use_lag=True, seed=0, T=150, env_num=4, lr=(5e-4, 1e-3), tau=0.05):
    from fsrl_amd.engine import Engine
    eng = Engine(_config(H, Do, Da, env_num))
    eng.sac_init(actor_lr=lr[0], critic_lr=lr[1], tau=tau, n_step=n_step, use_lagrangian=use_lag, deterministic=True)
    rng = np.random.default_rng(100 + seed)
    eng.sac_set_params(0.1 * rng.standard_normal(eng.n_sac_actor).astype(np.float32),
                       0.1 * rng.standard_normal(eng.n_sac_critics).astype(np.float32), 0.0)
    ids = np.arange(env_num)
    for t in range(T):
        obs = rng.standard_normal((env_num, Do)).astype(np.float32)
        act = np.tanh(rng.standard_normal((env_num, Da))).astype(np.float32)
        term = rng.random(env_num) < 0.03
        trunc = np.full(env_num, (t + 1) % 50 == 0) & ~term
        eng.push(ids, obs, act, rng.normal(0.5, 0.5, env_num), (rng.random(env_num) < 0.2).astype(np.float64), term, trunc,
                 rng.standard_normal((env_num, Do)).astype(np.float32))
    return eng


def _member(shape, i, n_step=2, use_lag=True):
    """member i of a group: its own parameters, data, store length, actor_lr and tau"""
    H, Do, Da, _ = shape
    return _engine(H, Do, Da, n_step, use_lag, seed=i, T=120 + 37 * i, lr=(5e-4 * (1 + 0.1 * i), 1e-3), tau=0.05 * (1 + 0.2 * i))


def _state(eng):
    """actor, critics, critics' targets, target actor, drained rows"""
    return [eng.sac_get_params(w)[0] for w in (0, 1, 2, 3)] + [eng.sac_drain()]


def _distance(x, y):
    """the four kinds of distance between two states (module docstring)"""
    d = [np.abs(x[j] - y[j]) for j in range(4)]
    p99, dmax = max(float(np.quantile(v, 0.99)) for v in d), max(float(v.max()) for v in d)
    r = np.abs(x[4] - y[4])
    col = np.abs(y[4]).max(axis=0)
    rel = float((r.max(axis=0)[col > 0] / col[col > 0]).max())
    return p99, dmax, float(r.max()), rel


def _same(x, y, exact):
    assert x[4].shape == y[4].shape
    if exact:
        for j in range(5):
            assert np.array_equal(x[j], y[j]), (j, np.abs(x[j] - y[j]).max())
        return
    p99, dmax, rabs, rrel = _distance(x, y)
    print("ddpg-group mixed: p99 %.3e max %.3e rows abs %.3e rel %.3e" % (p99, dmax, rabs, rrel))
    assert p99 <= P99_BOUND and dmax <= MAX_BOUND, (p99, dmax)
    assert rabs <= ROW_ABS_BOUND and rrel <= ROW_REL_BOUND, (rabs, rrel)


def _run(shape, k, n, lam, use_lag=True, n_step=2):
    """k members, n[i] grouped updates, against solo twins -> per member (grouped state, solo state, the initial target actor)"""
    from fsrl_amd.engine import EngineSacGroup
    B = shape[3]
    grouped, solo = [_member(shape, i, n_step, use_lag) for i in range(k)], [_member(shape, i, n_step, use_lag) for i in range(k)]
    resc = [1.0 / (1.0 + l) for l in lam]
    at0 = [e.sac_get_params(3)[0] for e in solo]
    for i in range(k):                             # key each member's Philox stream (one own update on both twins)
        for e in (grouped[i], solo[i]):
            e.sac_update(B, [lam[i]] if use_lag else [], resc[i], seed=11 + i, sync=False)
    g = EngineSacGroup(grouped)
    g.update(B, n, [[l] for l in lam] if use_lag else None, resc)
    for i in range(k):
        for _ in range(n[i]):
            solo[i].sac_update(B, [lam[i]] if use_lag else [], resc[i], sync=False)
    out = [(_state(grouped[i]), _state(solo[i]), at0[i]) for i in range(k)]
    g.close()
    for e in grouped + solo:
        e.close()
    return out


N_UPDATES = [5, 3, 0, 5, 2, 4, 1, 5]
DEFAULT = (128, 8, 2, 256)           # the reference's ddpgl_cfg.py shape
WIDE = (256, 112, 16, 100)           # Din = 128 with the widest head; the batch is not a multiple of 16


@pytest.mark.parametrize("shape", [DEFAULT, WIDE])
def test_group_of_one_is_bit_identical_to_solo(shape):
    (x, y, at0), = _run(shape, 1, [20], [0.4])
    _same(x, y, exact=True)
    assert len(x[4]) == 21
    # the comparison of the target actor is not vacuous: it has moved, and it is not the actor
    assert not np.array_equal(x[3], at0) and not np.array_equal(x[3], x[0])


EXACT_CASES = [  # H, Do, Da, B, k, n_step, use_lagrangian: the group takes the solo run's tile height in every launch
    (128, 8, 2, 256, 2, 2, True),        # 4 * 16 * 2 * 2 = 256 and 8 * 16 * 2 = 256: exactly one round
    (64, 8, 2, 64, 8, 3, True),          # 4 * 4 * 2 * 8 = 256 and 8 * 4 * 8 = 256
    (256, 112, 16, 100, 3, 2, True),
    (256, 20, 16, 1040, 3, 1, True),     # 16-row tiles solo and grouped; above 512 rows: the split-K weight gradients
    (128, 33, 8, 1040, 8, 2, False),     # use_lagrangian off, lagrangians=None
    (256, 30, 16, 1, 3, 2, True),        # a batch of one row
]


@pytest.mark.parametrize("case", EXACT_CASES)
def test_members_are_bit_identical_where_the_tile_heights_agree(case):
    H, Do, Da, B, k, ns, ul = case
    n = N_UPDATES[:k]
    res = _run((H, Do, Da, B), k, n, [0.1 * (i + 1) for i in range(k)], use_lag=ul, n_step=ns)
    for i, (x, y, at0) in enumerate(res):
        assert len(x[4]) == n[i] + 1
        _same(x, y, exact=True)


@pytest.mark.parametrize("shape", [DEFAULT, (256, 20, 16, 256)])
def test_eight_members_are_bit_identical_to_sixteen_row_twins(shape, monkeypatch):
    """k = 8 at the workload's own shape: the rule gives 16-row tiles in every launch, which is the single path of a context created
    under FSRL_TILE16 (read at fsrl_ctx_create).  Members and twins are both created under it."""
    monkeypatch.setenv("FSRL_TILE16", "1")
    res = _run(shape, 8, N_UPDATES, [0.1 * (i + 1) for i in range(8)])
    for i, (x, y, at0) in enumerate(res):
        assert len(x[4]) == N_UPDATES[i] + 1
        _same(x, y, exact=True)


MIXED_SHAPES = [DEFAULT, (256, 33, 8, 256)]


@pytest.mark.parametrize("shape", MIXED_SHAPES)
@pytest.mark.parametrize("k", [3, 8])
def test_members_match_their_solo_twins_across_tile_heights(shape, k):
    n = N_UPDATES[:k]
    res = _run(shape, k, n, [0.1 * (i + 1) for i in range(k)])
    for i, (x, y, at0) in enumerate(res):
        assert len(x[4]) == n[i] + 1
        _same(x, y, exact=n[i] == 0)             # a member with no updates is left untouched bit for bit


@pytest.mark.parametrize("plan", [0, 8])
def test_interleaved_own_updates_and_pushes(plan):
    """Own updates before and between grouped ones, pushes in between (they make a prefetched sample stale), and with plan 8 the
    side-stream prefetch of fsrl_sac_set_plan bit 3 on both members.  Batch 64: the group keeps the solo tile heights, so every
    member stays bit-identical to its twin."""
    from fsrl_amd.engine import EngineSacGroup
    shape = (128, 8, 2, 64)
    H, Do, Da, B = shape
    a, b = [_member(shape, i) for i in range(2)], [_member(shape, i) for i in range(2)]
    for e in a + b:
        e.sac_set_plan(plan)
    lam, resc = [0.2, 0.5], [1 / 1.2, 1 / 1.5]
    g = EngineSacGroup(a)
    rng = np.random.default_rng(5)
    ids = np.arange(4)
    for r in range(3):
        for i in range(2):                         # own updates before the grouped call (plan 8: each leaves a prefetch behind)
            for e in (a[i], b[i]):
                e.sac_update(B, [lam[i]], resc[i], seed=21 + i if r == 0 else 0, sync=False)
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
        x, y = _state(a[i]), _state(b[i])
        assert len(x[4]) == 3 * (1 + [3, 2][i]) + (3 if i == 0 else 0)
        _same(x, y, exact=True)
    for e in a + b:
        e.close()


def test_resident_actor_ends_and_relaunches():
    from fsrl_amd.engine import EngineSacGroup
    H, Do, Da, B, E = 128, 8, 16, 64, 9
    a, b = _engine(H, Do, Da, seed=3, env_num=E), _engine(H, Do, Da, seed=3, env_num=E)
    g = EngineSacGroup([a])
    obs = np.random.default_rng(1).standard_normal((E, Do)).astype(np.float32)
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
    assert np.asarray(ra[0]).shape == (E, Da)
    for u, v in zip(ra, rb):
        assert np.array_equal(np.asarray(u), np.asarray(v))
    assert a.actor_resident_stats()["launches"] == l0["launches"] + 1
    g.close(); a.close(); b.close()


def test_rejections_and_teardown():
    from fsrl_amd.engine import Engine, EngineSacGroup
    H, Do, Da, B = DEFAULT
    a, b = _engine(H, Do, Da, seed=0), _engine(H, Do, Da, seed=1)
    sac = Engine(_config(H, Do, Da))
    sac.sac_init()
    cvpo = Engine(_config(H, Do, Da))
    cvpo.cvpo_init(0.1)
    lay = Engine(_config((64, 64, 64), Do, Da))
    lay.sac_init(deterministic=True)
    other = [_engine(64, Do, Da), _engine(H, Do, Da, n_step=3), _engine(H, Do, Da, use_lag=False)]
    bad = [[sac, a], [a, sac], [a, cvpo], [a, lay], [a, a]] + [[a, o] for o in other]
    why = ["DDPG-Lagrangian", "DDPG-Lagrangian", "CVPO", "layered", "listed twice", "one network shape", "n_step", "use_lagrangian"]
    for members, reason in zip(bad, why):
        with pytest.raises(AssertionError, match=reason):      # FSRL_EINVAL, with the reason in the message
            EngineSacGroup(members)
    g = EngineSacGroup([a, b])
    with pytest.raises(AssertionError, match="already in a SAC group"):
        EngineSacGroup([b])
    g.update(B, [1, 1], [[0.1], [0.1]], [1.0, 1.0])
    b.close()                                      # a member destroyed before its group
    with pytest.raises(RuntimeError, match="destroyed"):
        g.update(B, [1, 1], [[0.1], [0.1]], [1.0, 1.0])
    g.close()
    for e in [a, sac, cvpo, lay] + other:
        e.close()


def test_policy_group_matches_sequential_policy_updates(tmp_path):
    import torch
    from fsrl_amd.agent import DDPGLagAgent
    from fsrl_amd.data import FastCollector, HipVectorReplayBuffer
    from fsrl_amd.env import SyntheticSafetyVectorEnv
    from fsrl_amd.policy import DDPGPolicyGroup

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
            ag = DDPGLagAgent(env, None, cost_limit=10, device="cuda:0", seed=1 + s, hidden_sizes=(64, 64), training_num=4,
                              buffer_size=2000)
            ag.policy.logger = _Log()
            ag.policy.train()
            buf = HipVectorReplayBuffer(ag.policy.engine, 2000, 4)
            agents.append(ag); bufs.append(buf); logs.append(ag.policy.logger)
            cols.append(FastCollector(ag.policy, env, buf, exploration_noise=True))
        grp = DDPGPolicyGroup([a.policy for a in agents]) if grouped else None
        for cyc in range(2):
            n = []
            for ag, col in zip(agents, cols):
                ag.policy.engine.actor_sample(np.zeros((1, ag.policy.engine.cfg.obs_dim), np.float32), seed=40 + cyc)
                st = col.collect(n_episode=4)
                ag.policy.pre_update_fn(stats_train={"cost": 15.0 + cyc})
                n.append(round(0.1 * st["n/st"]))
            assert min(n) >= 2
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
        assert any(key.startswith("actor_old.") for key in sg) and any(key.startswith("critics_old.") for key in sg)
        for key in sg:
            assert np.array_equal(sg[key], sw[key]), key
        assert lg == lw and lg
