"""Grouped CVPO updates (fsrl_cvpo_group_*) against twin contexts updated alone by fsrl_cvpo_update: the same parameters, the same
pushed transitions, the same Philox key.  The single-context path is the reference everywhere, never the grouped code.

Every launch of a group takes the single-context tile-height rule applied to the whole group's launch (4-row tiles while the
launch still fits one round of workgroups), per launch kind: Q launches on B rows, single actor launches, the two-batch TARGET +
PARTICLES launch, the Q launch over the K * B particles.
  * Where that gives the solo run's tile heights in every launch (a group of one, batches above 1024 rows, small batches whose
    group still fits) every member is bit-identical to its solo twin (SAME_CASES).
  * Where the group runs sixteen-row tiles in every launch (the default shape from k = 5) every member is bit-identical to a solo
    twin created under FSRL_TILE16, which forces sixteen-row tiles on the single path (test_sixteen_row_groups_...).
  * In between (default shape, k = 3 and 4: some launches 4-row, some 16-row) no exact twin exists.  The tile height changes a
    row's last bits and Adam turns last-bit gradient differences into steps of about lr; the size of that noise is the distance
    between the solo twin and the solo FSRL_TILE16 twin, measured by the test itself on the single path, and the grouped member may
    be at most twice that far from its default solo twin (test_mixed_tile_heights_...; its docstring has the measured figures)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEFAULT = (128, 40, 2, 256)          # tools/bench_cvpo.py: obs 40, act 2, 128 x 128, batch 256 (K 16, single critics)
WIDE = (256, 40, 2, 1024)            # 256 x 256, batch 1024 (double critics in the cases below)
N8 = [5, 3, 0, 5, 2, 4, 1, 5]


def _engine(H, Do, Da, seed=0, T=150, env_num=4, sub=200, tile16=False, **cv):
    """A CVPO context with parameters, data, learning rates, tau and qc_thres of its own.  H: a width or (hidden1, hidden2).
    tile16: created under FSRL_TILE16 (fsrl_ctx_create reads it): sixteen-row tiles in every launch of the single path."""
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig
    hs = tuple(H) if isinstance(H, (tuple, list)) else (H, H)
    old = os.environ.get("FSRL_TILE16")
    if tile16:
        os.environ["FSRL_TILE16"] = "1"
    try:
        eng = Engine(EngineConfig(algo=_lib.ALGO_SAC_LAG, obs_dim=Do, act_dim=Da, hidden_sizes=hs, n_critics=2, env_num=env_num,
                                  buffer_size=env_num * sub, gamma=0.98, target_kl=None))
    finally:
        if tile16:
            if old is None:
                del os.environ["FSRL_TILE16"]
            else:
                os.environ["FSRL_TILE16"] = old
    kw = dict(actor_lr=5e-4 * (1 + 0.1 * seed), critic_lr=1e-3 * (1 + 0.05 * seed), tau=0.05 + 0.01 * seed)
    kw.update(cv)
    eng.cvpo_init(0.1 + 0.02 * seed, **kw)
    rng = np.random.default_rng(100 + seed)
    eng.sac_set_params(0.1 * rng.standard_normal(eng.n_sac_actor).astype(np.float32),
                       0.1 * rng.standard_normal(eng.n_sac_critics).astype(np.float32), 0.0)
    eng.cvpo_post_update()                         # actor_old <- actor
    eng.cvpo_pre_update()
    ids = np.arange(env_num)
    for t in range(T):                             # T > sub: the sub-buffers wrap
        obs = rng.standard_normal((env_num, Do)).astype(np.float32)
        act = np.tanh(rng.standard_normal((env_num, Da))).astype(np.float32)
        term = rng.random(env_num) < 0.03
        trunc = np.full(env_num, (t + 1) % 50 == 0) & ~term
        eng.push(ids, obs, act, rng.normal(0.5, 0.5, env_num), (rng.random(env_num) < 0.2).astype(np.float64), term, trunc,
                 rng.standard_normal((env_num, Do)).astype(np.float32))
    return eng


NAMES = ("actor", "critics", "critics_old", "actor_old", "duals", "rows")


def _state(eng):
    """actor, critics, target critics, actor_old after cvpo_post_update, the four duals, the drained rows"""
    eng.cvpo_post_update()
    return [eng.sac_get_params(w)[0] for w in (0, 1, 2, 3)] + [eng.cvpo_duals(), eng.sac_drain()]


def _same(x, y):
    for j, name in enumerate(NAMES):
        assert x[j].shape == y[j].shape, (name, x[j].shape, y[j].shape)
        assert np.array_equal(x[j], y[j]), (name, np.abs(x[j] - y[j]).max())


KEY_B16 = 1040      # a batch whose single-context launches all take sixteen-row tiles, with or without FSRL_TILE16


def _run(shape, k, cycles, tile16=(False, ), key_B=None, **cv):
    """k members, per cycle n[i] grouped updates, cvpo_post_update / cvpo_pre_update on every context between two cycles; against
    solo twins, one per entry of tile16.  -> per member (grouped state, solo state per entry of tile16).
    key_B: the batch size of the own update that keys each context's Philox stream (default: the shape's).  With FSRL_TILE16 twins
    it is KEY_B16, so that this one update, which the grouped member runs alone under the default rule, is the same arithmetic on
    every twin and only the grouped updates are compared."""
    from fsrl_amd.engine import EngineCvpoGroup
    H, Do, Da, B = shape
    mk = lambda i, t16=False: _engine(H, Do, Da, seed=i, T=120 + 37 * i, tile16=t16, **cv)
    grouped = [mk(i) for i in range(k)]
    solos = [[mk(i, t) for i in range(k)] for t in tile16]
    for i in range(k):                             # key each member's Philox stream (one own update on every twin)
        for e in [grouped[i]] + [s[i] for s in solos]:
            e.cvpo_update(key_B or B, seed=11 + i, sync=False)
    g = EngineCvpoGroup(grouped)
    for c, n in enumerate(cycles):
        if c:
            for e in grouped + [e for s in solos for e in s]:
                e.cvpo_post_update(); e.cvpo_pre_update()
        g.update(B, n)
        for s in solos:
            for i in range(k):
                for _ in range(n[i]):
                    s[i].cvpo_update(B, sync=False)
    out = [(_state(grouped[i]), *[_state(s[i]) for s in solos]) for i in range(k)]
    g.close()
    for e in grouped + [e for s in solos for e in s]:
        e.close()
    return out


@pytest.mark.parametrize("shape,cv", [(DEFAULT, {}), (WIDE, dict(double_critic=True)),
                                      (DEFAULT, dict(estep_iter_num=2, mstep_iter_num=3))])
def test_group_of_one_is_bit_identical_to_solo(shape, cv):
    (x, y), = _run(shape, 1, [[5], [5], [5], [5]], **cv)
    _same(x, y)
    assert x[5].shape == (21, 17)


SAME_CASES = [  # H, Do, Da, B, K, n_step, double_critic, k: the group keeps the solo run's tile height in every launch (256 CUs)
    (256, 33, 8, 1040, 16, 3, True, 3),            # above 1024 rows: sixteen-row tiles everywhere, split-K weight gradients
    (64, 33, 8, 1040, 12, 1, False, 8),            # ... K not a power of two: the E-step's per-state loop
    ((128, 96), 8, 2, 64, 16, 2, False, 8),        # batch 64, single critics, k = 8: all four rules still met; hidden1 != hidden2
    (128, 8, 2, 64, 12, 3, True, 3),               # double critics, 4-row tiles on B rows, 16-row on the particles (solo too)
    (256, 8, 4, 64, 16, 1, False, 4),
    (64, 8, 2, 32, 8, 2, False, 2),                # 4-row tiles in every launch, the particles' included
]


@pytest.mark.parametrize("case", SAME_CASES)
def test_members_are_bit_identical_where_the_tile_heights_agree(case):
    H, Do, Da, B, K, ns, dc, k = case
    n = N8[:k]
    res = _run((H, Do, Da, B), k, [n], sample_act_num=K, n_step=ns, double_critic=dc)
    for i, (x, y) in enumerate(res):
        assert x[5].shape == (n[i] + 1, 17)
        _same(x, y)


@pytest.mark.parametrize("k", [5, 8])
def test_sixteen_row_groups_are_bit_identical_to_tile16_solo_twins(k):
    """default shape from k = 5: sixteen-row tiles in every launch of the group = the single path under FSRL_TILE16"""
    n = N8[:k]
    res = _run(DEFAULT, k, [n, n[::-1]], tile16=(True, ), key_B=KEY_B16)
    for i, (x, y) in enumerate(res):
        assert x[5].shape == (n[i] + n[k - 1 - i] + 1, 17)
        _same(x, y)


def _dist(xs, ys):
    """pooled over the members of a case: per class the 99th percentile and the maximum of the absolute differences; the largest
    relative row difference.  A row entry's difference is taken relative to the largest magnitude its statistic reaches in the
    member's rows, not to the entry itself: mstep_loss_kl = dual_mu (kl_mu - eps_mu) + dual_std (kl_std - eps_std) and the
    multipliers right behind cvpo_pre_update pass through zero, so an entry's own magnitude is no scale for its error (measured:
    an entry of 1.8e-6 differing by 6e-11 is 3.4e-5 of itself and 2.4e-7 of its column)."""
    out = {}
    for j, name in enumerate(NAMES[:5]):
        d = np.concatenate([np.abs(x[j] - y[j]).ravel() for x, y in zip(xs, ys)])
        out[name] = (float(np.quantile(d, 0.99)), float(d.max()))
    r = np.concatenate([(np.abs(x[5] - y[5]) / np.maximum(np.abs(y[5]).max(axis=0, keepdims=True), 1e-30)).ravel()
                        for x, y in zip(xs, ys)])
    out["rows"] = (float(r.max()), )
    return out


@pytest.mark.parametrize("k", [3, 4])
def test_mixed_tile_heights_stay_within_twice_the_tile_noise(k):
    """default shape, k = 3 / 4: the group's Q launches and its two-batch actor launch run sixteen-row tiles, its single actor
    launches (MFWD, MBWD) four-row tiles, so neither solo twin is exact.  Bound: twice the distance between the default solo
    twin and the FSRL_TILE16 solo twin after the same updates, computed here on the single path.  A member with no updates is
    untouched bit for bit.
    Measured on an MI355X, 30 / 20 / 0 (/ 30) updates, pooled over the members with updates; 99th percentile / maximum of
    |difference|, grouped against solo | solo against solo FSRL_TILE16 (the test prints them: `cvpo-group mixed k=...`):
      k = 3  actor 3.0e-8 / 1.2e-7 | 3.0e-8 / 8.9e-8   critics 1.5e-8 / 6.7e-8 | the same   duals 4.2e-7 | 1.1e-6   rows 1.8e-5 | 2.4e-5
      k = 4  actor 1.2e-6 / 2.2e-5 | 1.2e-6 / 2.2e-5   critics 4.7e-5 / 1.3e-3 | the same   duals 1.2e-4 | 1.2e-4   rows 1.36e-3 | 1.36e-3
    (k = 4's fourth member, 30 updates, carries the larger figures: Adam has amplified the last-bit differences to about lr.)
    After 6 / 4 / 0 updates everything sits at one or two units in the last place (parameters at most 6.7e-8 on either side), and a
    row difference taken relative to the ENTRY was 3.4e-5 grouped against 1.4e-5 between the twins -- one mstep_loss_kl of 1.8e-6
    differing by 6e-11; see _dist for why the statistic's scale is used instead."""
    n = [30, 20, 0, 30][:k]
    res = _run(DEFAULT, k, [n], tile16=(False, True), key_B=KEY_B16)
    for i, (x, y, _) in enumerate(res):
        if n[i] == 0:
            _same(x, y)
    act = [r for i, r in enumerate(res) if n[i] > 0]
    noise = _dist([r[1] for r in act], [r[2] for r in act])       # solo against solo FSRL_TILE16: the tile height's own noise
    got = _dist([r[0] for r in act], [r[1] for r in act])         # grouped against solo
    for name in NAMES:
        print(f"cvpo-group mixed k={k} {name}: grouped-vs-solo {got[name]} solo-vs-tile16 {noise[name]}")
    for name in NAMES:
        for a, b in zip(got[name], noise[name]):
            assert a <= 2.0 * b, (name, got[name], noise[name])


def test_last_update_replays_through_the_caller_rng_path():
    """a member's sample and particles of its last grouped update, fed to a solo twin that is one update behind"""
    from fsrl_amd.engine import EngineCvpoGroup
    H, Do, Da, B = 128, 8, 2, 64
    n = [3, 1, 2]
    a = [_engine(H, Do, Da, seed=i, T=120 + 60 * i) for i in range(3)]
    b = [_engine(H, Do, Da, seed=i, T=120 + 60 * i) for i in range(3)]
    for i in range(3):
        for e in (a[i], b[i]):
            e.cvpo_update(B, seed=21 + i, sync=False)
    g = EngineCvpoGroup(a)
    g.update(B, n)
    for i in range(3):
        for _ in range(n[i] - 1):
            b[i].cvpo_update(B, sync=False)
        idx, et, _ = a[i].sac_last_sample(B)
        ek = a[i].cvpo_last_particles(B)
        st = b[i].cvpo_update(B, indices=idx, eps_target=et, eps_particles=ek)
        x, y = _state(a[i]), _state(b[i])
        for j in range(5):
            assert np.array_equal(x[j], y[j]), (i, NAMES[j])
        assert np.array_equal(x[5][-1], st)
    g.close()
    for e in a + b:
        e.close()


def test_interleaved_own_updates_pushes_and_member_calls():
    """own cvpo_update calls, pushes, cvpo_pre_update / cvpo_post_update / cvpo_set_thres between grouped calls (batch 64: the
    group keeps the solo tile heights)"""
    from fsrl_amd.engine import EngineCvpoGroup
    H, Do, Da, B = 128, 8, 2, 64
    a = [_engine(H, Do, Da, seed=i) for i in range(2)]
    b = [_engine(H, Do, Da, seed=i) for i in range(2)]
    for i in range(2):
        for e in (a[i], b[i]):
            e.cvpo_update(B, seed=31 + i, sync=False)
    g = EngineCvpoGroup(a)
    rng = np.random.default_rng(5)
    ids = np.arange(4)
    for r in range(3):
        for i in range(2):                         # own updates before the grouped call
            for e in (a[i], b[i]):
                e.cvpo_update(B, sync=False)
        g.update(B, [3, 2])
        for i in range(2):
            for _ in range([3, 2][i]):
                b[i].cvpo_update(B, sync=False)
        for e in (a[0], b[0]):                     # member calls right behind the grouped call, then an own update
            e.cvpo_post_update(); e.cvpo_pre_update(); e.cvpo_set_thres(0.3 + 0.1 * r)
            e.cvpo_update(B, sync=False)
        rows = [rng.standard_normal((4, Do)).astype(np.float32) for _ in range(2)]
        for e in (a[1], b[1]):                     # pushes in between
            e.push(ids, rows[0], np.zeros((4, Da), np.float32), np.ones(4), np.ones(4), np.zeros(4, bool), np.zeros(4, bool), rows[1])
            e.cvpo_pre_update()
    g.close()
    for i in range(2):
        _same(_state(a[i]), _state(b[i]))
    for e in a + b:
        e.close()


def test_resident_actor_ends_and_relaunches():
    from fsrl_amd.engine import EngineCvpoGroup
    H, Do, Da, B = 128, 8, 2, 64
    a, b = _engine(H, Do, Da, seed=3), _engine(H, Do, Da, seed=3)
    for e in (a, b):
        e.cvpo_update(B, seed=5, sync=False)
    g = EngineCvpoGroup([a])
    obs = np.random.default_rng(1).standard_normal((4, Do)).astype(np.float32)
    for e in (a, b):
        e.actor_sample(obs[:1], seed=9)                               # key the collectors' streams identically
        e.collect_step(None, obs)
    l0 = a.actor_resident_stats()
    assert l0["live"]
    g.update(B, [4])
    for _ in range(4):
        b.cvpo_update(B, sync=False)
    assert not a.actor_resident_stats()["live"]
    ra, rb = a.collect_step(None, obs), b.collect_step(None, obs)
    for u, v in zip(ra, rb):
        assert np.array_equal(np.asarray(u), np.asarray(v))
    assert a.actor_resident_stats()["launches"] == l0["launches"] + 1
    g.close(); a.close(); b.close()


def test_rejections_and_teardown():
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig, EngineCvpoGroup, EngineSacGroup
    H, Do, Da, B = 128, 8, 2, 64
    a, b = _engine(H, Do, Da, seed=0), _engine(H, Do, Da, seed=1)
    mk = lambda hs: Engine(EngineConfig(algo=_lib.ALGO_SAC_LAG, obs_dim=Do, act_dim=Da, hidden_sizes=hs, n_critics=2, env_num=4,
                                        buffer_size=800, target_kl=None))
    sac = mk((H, H)); sac.sac_init()
    ddpg = mk((H, H)); ddpg.sac_init(deterministic=True)
    lay = mk((64, 64, 64)); lay.cvpo_init(0.1)
    plan = _engine(H, Do, Da); plan.sac_set_plan(1)
    other = [_engine(64, Do, Da), _engine((128, 96), Do, Da), _engine(H, Do, Da, n_step=3), _engine(H, Do, Da, double_critic=True),
             _engine(H, Do, Da, sample_act_num=8), _engine(H, Do, Da, estep_iter_num=2), _engine(H, Do, Da, mstep_iter_num=2), plan]
    why = ["SAC-Lagrangian", "DDPG-Lagrangian", "layered", "listed twice", "one network shape", "one network shape", "n_step",
           "double_critic", "sample_act_num", "estep_iter_num", "mstep_iter_num", "split-K"]
    for bad, reason in zip(([a, sac], [a, ddpg], [a, lay], [a, a], *[[a, o] for o in other]), why):
        with pytest.raises(AssertionError, match=reason):      # FSRL_EINVAL, with the reason in the message
            EngineCvpoGroup(bad)
    with pytest.raises(AssertionError, match="CVPO"):          # a SAC group still refuses a CVPO member
        EngineSacGroup([sac, a])
    g = EngineCvpoGroup([a, b])
    with pytest.raises(AssertionError, match="already in a CVPO group"):
        EngineCvpoGroup([b])
    with pytest.raises(AssertionError, match="n_updates"):
        g.update(B, [1, -1])
    empty = mk((H, H)); empty.cvpo_init(0.1)
    ge = EngineCvpoGroup([empty])
    ge.update(B, [0])                              # nothing to do: an empty store is no error
    with pytest.raises(AssertionError, match="empty replay store"):
        ge.update(B, [1])
    ge.close()
    b.sac_set_plan(1)                              # re-checked at every update
    with pytest.raises(AssertionError, match="split-K"):
        g.update(B, [1, 1])
    b.sac_set_plan(0)
    g.update(B, [1, 1])
    b.close()                                      # a member destroyed before its group
    with pytest.raises(RuntimeError, match="destroyed"):
        g.update(B, [1, 1])
    g.close()
    for e in [a, sac, ddpg, lay, empty] + other:
        e.close()


def test_policy_group_matches_sequential_policy_updates(tmp_path):
    import torch
    from fsrl_amd.agent import CVPOAgent
    from fsrl_amd.data import FastCollector, HipVectorReplayBuffer
    from fsrl_amd.env import SyntheticSafetyVectorEnv
    from fsrl_amd.policy import CVPOPolicyGroup

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
            ag = CVPOAgent(env, None, cost_limit=10, device="cuda:0", seed=1 + s, hidden_sizes=(64, 64), training_num=4,
                           buffer_size=2000)
            ag.policy.logger = _Log()
            ag.policy.train()
            buf = HipVectorReplayBuffer(ag.policy.engine, 2000, 4)
            agents.append(ag); bufs.append(buf); logs.append(ag.policy.logger)
            cols.append(FastCollector(ag.policy, env, buf, exploration_noise=True))
        grp = CVPOPolicyGroup([a.policy for a in agents]) if grouped else None
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
