"""The device-side replay sampler (library-RNG mode of SAC-Lag, DDPG-Lag, CVPO and their groups) against the exact host model
oracle/sampler.py, which shares no code with the kernels: after a library-RNG update the sampled indices must EQUAL the model's and
the rsample / particle noise must lie within

    |device - float64 model| <= 8 * 2^-24 * max(1, rad)            rad = sqrt(-2 ln u1), the Box-Muller radius of the entry

-- the sum of the documented fp32 bounds of logf, sqrtf, sincospif and the two multiplies with a factor-two margin; a wrong
stream differs by O(1).  Largest ratio measured over this file on an MI355X (ROCm 7.0.2): MEASURED_RATIO below, in units of
2^-24 * max(1, rad), against the bound of 8.

The model is built from a mirror of the store kept by tests/golden/ref_shim.VectorReplayBuffer (sizes, write heads and done flags
AFTER every push), from the key of the last non-zero seed, and from the context's update count: `n_updates` of the library, which
every update of either RNG mode raises by one, a grouped call by n[i], and which no reseed resets.

fsrl_cvpo_init refuses act_dim above 8 (the actor head holds 2 * act_dim outputs in 16 columns) and fsrl_sac_init without
`deterministic` does too, so act_dim 16 is drawn through a DDPG-Lag context and CVPO runs at act_dim 3 and 8."""
import numpy as np
import pytest

from oracle import sampler as S
from test_oracle_sampler import Mirror

pytestmark = pytest.mark.gpu

MEASURED_RATIO = 3.38        # largest |device - model| / (2^-24 * max(1, rad)) seen by this file's checks (bound: 8)
NOISE_BOUND = 8.0
ULP24 = 2.0**-24
SEEN = {"ratio": 0.0}


def _noise_ratio(dev, want, rad):
    r = float((np.abs(np.asarray(dev, np.float64) - want) / (ULP24 * np.maximum(1.0, rad))).max())
    SEEN["ratio"] = max(SEEN["ratio"], r)
    return r


def _engine(kind, Do, Da, E, sub, n_step=2, hidden=(64, 64), K=16, gamma=0.98, max_action=1.0, params=None, log_alpha=0.0,
            plan=None, **init):
    """The one engine build helper: a replay context of `kind` (sac | ddpg | cvpo) with E sub-buffers of `sub` rows."""
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig
    eng = Engine(EngineConfig(algo=_lib.ALGO_SAC_LAG, obs_dim=Do, act_dim=Da, hidden_sizes=tuple(hidden), n_critics=2, env_num=E,
                              buffer_size=E * sub, gamma=gamma, max_action=max_action, target_kl=None))
    try:
        if kind == "cvpo":
            eng.cvpo_init(init.pop("qc_thres", 0.2), n_step=n_step, sample_act_num=K, **init)
        else:
            eng.sac_init(n_step=n_step, deterministic=(kind == "ddpg"), **init)
        if params is None:
            r = np.random.default_rng(0)
            params = ((0.1 * r.standard_normal(eng.n_sac_actor)).astype(np.float32),
                      (0.1 * r.standard_normal(eng.n_sac_critics)).astype(np.float32))
        eng.sac_set_params(params[0], params[1], log_alpha)
        if plan is not None:
            eng.sac_set_plan(plan)
    except Exception:
        eng.close()
        raise
    return eng


class Rig:
    """An engine, the mirror of its store, and what the model needs: the key of the last non-zero seed (the default key before
    any) and the number of updates run so far."""

    def __init__(self, kind, Do, Da, E, sub, K=16, max_action=1.0, **kw):
        self.kind, self.Do, self.Da, self.E, self.sub, self.K, self.amax = kind, Do, Da, E, sub, K, max_action
        self.eng = _engine(kind, Do, Da, E, sub, K=K, max_action=max_action, **kw)
        self.mirror = Mirror(E, sub, Do, Da)
        self.key, self.count = S.key_of(0), 0
        self.lag, self.resc = [0.5], 1 / 1.5
        if kind == "cvpo":
            self.eng.cvpo_pre_update()

    def close(self):
        if self.eng is not None:
            self.eng.close()
            self.eng = None

    # ---- store
    def push(self, ids, obs, act, rew, cost, term, trunc, nxt):
        ptr, *_ = self.eng.push(ids, obs, act, rew, cost, term, trunc, nxt)
        assert np.array_equal(ptr, self.mirror.push(ids, obs, act, rew, cost, term, trunc, nxt))      # the slot the reference's buffer takes

    def push_random(self, rng, ids, t=0):
        k = len(ids)
        term = rng.random(k) < 0.06
        act = self.amax * np.tanh(rng.standard_normal((k, self.Da)))
        self.push(ids, rng.standard_normal((k, self.Do)).astype(np.float32), act.astype(np.float32), rng.normal(0, 1, k),
                  (rng.random(k) < 0.3).astype(np.float64), term, np.full(k, t % 13 == 12) & ~term,
                  rng.standard_normal((k, self.Do)).astype(np.float32))

    def fill(self, rng, rows, lag_env=None):
        """rows[e] rows into sub-buffer e in lock step (more than `sub`: it wraps); lag_env sits out every 7th step"""
        left = np.array(rows, np.int64)
        t = 0
        while (left > 0).any():
            ids = [e for e in range(self.E) if left[e] > 0 and not (e == lag_env and t % 7 == 0)]
            if ids:
                self.push_random(rng, ids, t)
                left[ids] -= 1
            t += 1
        return self

    # ---- updates
    def update(self, B, seed=0, sync=False):
        """one library-RNG update"""
        if seed:
            self.key = S.key_of(seed)
        st = self.eng.cvpo_update(B, seed=seed, sync=sync) if self.kind == "cvpo" else \
            self.eng.sac_update(B, self.lag, self.resc, seed=seed, sync=sync)
        self.count += 1
        return st

    def model(self, B, counter=None):
        """indices, eps_target, eps_pi (+ radii) of the update with this counter (default: the last one run)"""
        c = self.count - 1 if counter is None else counter
        idx = S.sample_indices(self.key, c, B, self.mirror.sizes, self.sub)
        return (idx, ) + S.noise(self.key, c, B, self.Da, with_rad=True)

    def check(self, B, tag=None):
        """the last update's sample against the model built from the store as it is now"""
        idx, et, ep = self.eng.sac_last_sample(B)
        w_idx, w_t, w_p, r_t, r_p = self.model(B)
        assert np.array_equal(idx, w_idx), (tag, self.count - 1, np.flatnonzero(idx != w_idx)[:8], idx[:8], w_idx[:8])
        for name, dev, want, rad in (("eps_target", et, w_t, r_t), ("eps_pi", ep, w_p, r_p)):
            r = _noise_ratio(dev, want, rad)
            assert r <= NOISE_BOUND, (tag, name, self.count - 1, r)
        if self.kind == "cvpo":
            ek = self.eng.cvpo_last_particles(B)
            w_k, r_k = S.particles(self.key, self.count - 1, B, self.Da, self.K, with_rad=True)
            assert ek.shape == w_k.shape
            r = _noise_ratio(ek, w_k, r_k)
            assert r <= NOISE_BOUND, (tag, "particles", self.count - 1, r)


@pytest.fixture
def make():
    made = []

    def _make(*a, **k):
        made.append(Rig(*a, **k))
        return made[-1]
    yield _make
    for r in made:
        r.close()
    print(f"largest noise ratio so far: {SEEN['ratio']:.3f} (bound {NOISE_BOUND})")


ROWS4 = [200, 150, 180, 170]


# ------------------------------------------------------------------------------------------------ SAC launch plans
@pytest.mark.parametrize("batch,plan", [(256, p) for p in (0, 32, 16, 2, 6, 8, 40)] + [(1024, p) for p in (0, 32, 48, 2)])
def test_sac_plans_draw_the_models_sample_at_every_update(make, batch, plan):
    """every copy of the draw code -- stand-alone sampler (2, 6), sample + gather launch (16, 48), the tile kernel's own (0, 32),
    rider blocks (0 at batch 1024), side-stream prefetch (8, 40): the sample of EVERY one of 6 updates is the model's"""
    rig = make("sac", 12, 8, 4, 256, n_step=2, plan=plan).fill(np.random.default_rng(1), ROWS4)
    for u in range(6):
        rig.update(batch, seed=7 if u == 0 else 0)
        rig.check(batch, (plan, u))
    assert np.isfinite(rig.eng.sac_drain()).all()


# ------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("Da", [1, 2, 3, 8, 16])
def test_batches_and_action_widths(make, Da):
    """batches 1, 100, 333 (more than the 105 stored rows) and 1040 at odd and even action widths; n_step 3 over ragged
    sub-buffers.  act_dim 16 through a DDPG-Lag context (see the module docstring)."""
    kind = "ddpg" if Da > 8 else "sac"
    rig = make(kind, 9, Da, 2, 128, n_step=3).fill(np.random.default_rng(2), [60, 45])
    for B in (1, 100, 333, 1040):
        for u in range(2):
            rig.update(B, seed=3 if rig.count == 0 else 0)
            rig.check(B, (Da, B, u))


@pytest.mark.parametrize("plan", [0, 32, 48, 2])
def test_600_sub_buffers_beyond_the_lds_table(make, plan):
    """600 sub-buffers (the samplers keep 512 books in LDS and read global memory beyond), 1 .. 40 rows each, n_step 3, batch 1024"""
    E, sub, B = 600, 64, 1024
    rows = np.random.default_rng(3).integers(1, 41, E)
    rig = make("sac", 11, 3, E, sub, n_step=3, plan=plan).fill(np.random.default_rng(4), rows)
    assert np.array_equal(rig.mirror.sizes, rows)
    for u in range(3):
        rig.update(B, seed=5 if u == 0 else 0)
        rig.check(B, (plan, u))


# ------------------------------------------------------------------------------------------------ pushes between updates
@pytest.mark.parametrize("batch", [256, 1024])
@pytest.mark.parametrize("plan", [0, 8, 32])
def test_pushes_between_updates_are_seen_by_the_next_sample(make, plan, batch):
    """rows pushed between two updates, one of them wrapping a sub-buffer: the next sample is drawn against the store AFTER the
    push -- a sample prefetched on the side stream (plan 8) or by rider blocks (plan 0 at batch 1024) before it is stale"""
    E, sub = 3, 64
    rng = np.random.default_rng(6)
    rig = make("sac", 7, 3, E, sub, n_step=3, plan=plan).fill(rng, [64, 62, 30])
    t = 100
    for u, pushes in enumerate([[], [], [[0, 1, 2]], [], [[0, 1, 2], [0, 1], [1]], [], [[2]], [[0, 1, 2]] * 3, []]):
        for ids in pushes:                                   # env 0 wraps at the first push, env 1 at the third
            rig.push_random(rng, ids, t)
            t += 1
        rig.update(batch, seed=9 if u == 0 else 0)
        rig.check(batch, (plan, batch, u))
    assert rig.mirror.sizes.tolist() == [64, 64, 36] and rig.mirror.book[0, 1] == 6 and rig.mirror.book[1, 1] == 5


# ------------------------------------------------------------------------------------------------ reseeding, caller RNG
@pytest.mark.parametrize("plan", [0, 8])
def test_reseeding_and_caller_rng_updates_keep_the_count(make, plan):
    """The counter is the context's update count (`n_updates`): +1 per update of EITHER RNG mode, never reset; a non-zero seed
    replaces the key from that update on and a zero seed keeps it; a context that was never seeded draws from the default key."""
    B = 256
    rng = np.random.default_rng(8)
    rig = make("sac", 7, 3, 4, 256, n_step=2, plan=plan).fill(rng, ROWS4)
    assert rig.key == S.DEFAULT_KEY
    rig.update(B); rig.check(B, "never seeded, count 0")
    rig.update(B); rig.check(B, "never seeded, count 1")
    rig.update(B, seed=5); rig.check(B, "seeded at count 2")
    assert rig.key == S.key_of(5) and rig.count == 3
    valid = rig.mirror.valid()
    for _ in range(2):                                       # caller-RNG updates in between: the count moves on
        z = rng.standard_normal((B, 3)).astype(np.float32)
        rig.eng.sac_update(B, rig.lag, rig.resc, indices=rng.choice(valid, B), eps_target=z, eps_pi=z)
        rig.count += 1
    rig.update(B); rig.check(B, "library RNG at count 5, after two caller-RNG updates")
    assert rig.count == 6
    rig.update(B, seed=9); rig.check(B, "reseeded at count 6")
    rig.update(B); rig.check(B, "count 7 under the second key")
    rig.update(B, seed=5); rig.check(B, "the first seed again at count 8: its key, not its stream's start")
    first = S.sample_indices(S.key_of(5), 2, B, rig.mirror.sizes, rig.sub)
    assert not np.array_equal(rig.eng.sac_last_sample(B)[0], first)


# ------------------------------------------------------------------------------------------------ DDPG-Lag, CVPO
@pytest.mark.parametrize("batch", [256, 1024])
def test_ddpg_plans_draw_the_models_sample(make, batch):
    """the plans of test_ddpg_launch_plans_are_bit_identical at act_dim 16 (8 noise pairs per row: 128 noise lanes per 16 rows)"""
    for plan in (0, 32, 64, 16, 6, 2, 8, 40, 14, 22):
        rig = make("ddpg", 20, 16, 4, 256, n_step=2, hidden=(128, 128), plan=plan).fill(np.random.default_rng(11), ROWS4)
        for u in range(4):
            if u == 2:
                rig.push_random(np.random.default_rng(12), [0, 1, 2, 3], 5)
            rig.update(batch, seed=7 if u == 0 else 0)
            rig.check(batch, (plan, u))
        rig.close()


@pytest.mark.parametrize("K,Da", [(4, 3), (16, 8), (4, 8), (16, 3)])
def test_cvpo_plans_draw_the_models_sample_and_particles(make, K, Da):
    """the plans of test_cvpo_launch_plans_are_bit_identical: indices, target noise and the K particle blocks of every update"""
    for plan in (0, 2, 4, 6):
        for B in (48, 256):
            rig = make("cvpo", 10, Da, 3, 128, n_step=3, K=K, plan=plan).fill(np.random.default_rng(13), [128, 100, 37])
            for u in range(4):
                if u == 2:
                    rig.push_random(np.random.default_rng(14), [0, 1, 2], 5)      # env 0 wraps
                rig.update(B, seed=9 if u == 0 else 0)
                rig.check(B, (plan, B, u))
            rig.close()


def test_cvpo_refuses_act_dim_16():
    from fsrl_amd import _lib
    with pytest.raises((_lib.FsrlHipError, AssertionError)):
        _engine("cvpo", 10, 16, 2, 64).close()


# ------------------------------------------------------------------------------------------------ groups
GROUP_N = {3: [4, 0, 2], 8: [5, 3, 0, 5, 2, 4, 1, 5]}


@pytest.mark.parametrize("k", [3, 8])
@pytest.mark.parametrize("kind", ["sac", "cvpo"])
def test_group_members_draw_their_own_streams(make, kind, k):
    """EngineSacGroup / EngineCvpoGroup: after a grouped call every member's last sample is the model's at ITS key and ITS update
    count (n[i] differs per member, 0 included); own updates between grouped calls continue the same count; rows pushed into a
    member between two calls are seen by its next grouped sample"""
    from fsrl_amd.engine import EngineCvpoGroup, EngineSacGroup
    B, n = 256, GROUP_N[k]
    rigs = [make(kind, 10, 3, 4, 200, n_step=3, K=4).fill(np.random.default_rng(20 + i), [120 + 37 * i] * 4, lag_env=i % 4)
            for i in range(k)]
    for i, r in enumerate(rigs):                             # key each member's stream with an own update
        r.update(B, seed=11 + i)
        r.check(B, ("own", i))
    assert len({r.key for r in rigs}) == k
    g = (EngineCvpoGroup if kind == "cvpo" else EngineSacGroup)([r.eng for r in rigs])

    def grouped(nn):
        if kind == "cvpo":
            g.update(B, nn)
        else:
            g.update(B, nn, [rigs[0].lag] * k, [rigs[0].resc] * k)
        for i, r in enumerate(rigs):
            r.count += nn[i]
            r.check(B, ("grouped", nn, i))
    try:
        grouped(n)
        assert [r.count for r in rigs] == [1 + x for x in n]
        for i, r in enumerate(rigs[::2]):                    # own updates continue the count
            r.update(B)
            r.check(B, ("own after group", i))
        rigs[0].push_random(np.random.default_rng(30), [0, 1, 2, 3], 3)
        assert n[::-1][0] > 0
        grouped(n[::-1])
        grouped([1] * k)
    finally:
        g.close()
    for r in rigs:
        assert np.isfinite(r.eng.sac_drain()).all()


# ------------------------------------------------------------------------------------------------ end to end on a wrapped store
WRAPPED = dict(E=3, sub=40, rows=[100, 86, 93], lag_env=1, n_step=3)        # ragged write heads, 2.15 .. 2.5 times round
SAC_KEYS = ["loss/rescaling", "loss/lagrangian", "loss/actor_safety", "loss/alpha_loss", "loss/alpha_value",
            "loss/actor_rew", "loss/actor_total", "loss/q0", "loss/q1", "loss/q_total"]


def _wrapped_index(rig):
    from oracle.sac_lag import ReplayIndex
    m = rig.mirror
    assert (m.sizes == rig.sub).all() and len(set(m.book[:, 1].tolist())) == rig.E
    return m.store(), ReplayIndex(None, rig.sub, m.done, heads=m.book)


def test_sac_end_to_end_on_a_wrapped_store_vs_oracle(make):
    """library-RNG SAC-Lag updates on a wrapped store against SACLagOracle fed the MODEL's indices and noise (ReplayIndex with
    write heads).  Bounds: test_sac_variants_vs_oracle's."""
    from oracle.sac_lag import SACConfig, SACLagOracle
    Do, Da, H, B, w = 7, 3, 64, 100, WRAPPED
    rng = np.random.default_rng(Do + 10 * Da)
    o = SACLagOracle(SACConfig(obs_dim=Do, act_dim=Da, hidden=(H, H), gamma=0.98, n_step=w["n_step"], tau=0.1, alpha=0.05,
                               auto_alpha=True, use_lagrangian=True))
    tha = (0.2 * rng.standard_normal(o.n_actor)).astype(np.float32)
    thc = (0.2 * rng.standard_normal(2 * o.n_critic)).astype(np.float32)
    o.set_params(tha, thc, -0.5)
    rig = make("sac", Do, Da, w["E"], w["sub"], n_step=w["n_step"], hidden=(H, H), gamma=0.98, params=(tha, thc), log_alpha=-0.5,
               alpha=0.05, tau=0.1).fill(rng, w["rows"], w["lag_env"])
    rig.lag, rig.resc = [0.3], 1 / 1.3
    store, index = _wrapped_index(rig)
    for u in range(3):
        st = rig.update(B, seed=21 if u == 0 else 0, sync=True)
        rig.check(B, u)
        idx, et, ep, _, _ = rig.model(B)
        sa, sc, _ = o.update(store, index, idx, et, ep, rig.lag, rig.resc)
        want = {**sa, **sc}
        for j, kname in enumerate(SAC_KEYS):
            if kname in want:
                v = float(want[kname])
                assert abs(st[j] - v) <= 1e-4 * abs(v) + 1e-5, (u, kname, st[j], v)
    for got, ref in ((rig.eng.sac_get_params(0)[0], o.actor_flat()), (rig.eng.sac_get_params(1)[0], o.critics_flat()),
                     (rig.eng.sac_get_params(2)[0], o.critics_flat(old=True))):
        d = np.abs(got - ref)
        assert np.quantile(d, 0.99) <= 5e-6 and d.max() <= 3 * 1e-3, (np.quantile(d, 0.99), d.max())


def test_ddpg_end_to_end_on_a_wrapped_store_vs_oracle(make):
    """the same for DDPG-Lag (the indices alone matter: the deterministic actor takes no noise).  Bounds:
    test_ddpg_variants_vs_oracle's."""
    from oracle.ddpg_lag import DDPGConfig, DDPGLagOracle
    Do, Da, H, B, w, amax = 9, 13, 64, 100, WRAPPED, 2.0
    rng = np.random.default_rng(Do + 10 * Da)
    o = DDPGLagOracle(DDPGConfig(obs_dim=Do, act_dim=Da, hidden=(H, H), max_action=amax, gamma=0.98, n_step=w["n_step"], tau=0.1,
                                 actor_lr=1e-3, critic_lr=1e-3, use_lagrangian=True))

    def init(spec):
        return np.concatenate([(rng.standard_normal(shp) / np.sqrt(shp[1]) if len(shp) == 2 else 0.1 * rng.standard_normal(shp)).ravel()
                               for shp in spec.values()]).astype(np.float32)
    tha, thc = init(o.aspec), np.concatenate([init(o.cspec), init(o.cspec)])
    o.set_params(tha, thc)
    rig = make("ddpg", Do, Da, w["E"], w["sub"], n_step=w["n_step"], hidden=(H, H), gamma=0.98, max_action=amax, params=(tha, thc),
               actor_lr=1e-3, critic_lr=1e-3, tau=0.1).fill(rng, w["rows"], w["lag_env"])
    rig.lag, rig.resc = np.array([0.3]), 1 / 1.3
    store, index = _wrapped_index(rig)
    for u in range(3):
        st = rig.update(B, seed=22 if u == 0 else 0, sync=True)
        rig.check(B, u)
        sa, sc, _ = o.update(store, index, rig.model(B)[0], rig.lag, rig.resc)
        want = {**sa, **sc}
        for j, kname in enumerate(SAC_KEYS):
            if kname in want:
                v = float(want[kname])
                assert abs(st[j] - v) <= 1e-4 * abs(v) + 1e-5, (u, kname, st[j], v)
    for which, ref in ((0, o.actor_flat()), (3, o.actor_flat(old=True)), (1, o.critics_flat()), (2, o.critics_flat(old=True))):
        d = np.abs(rig.eng.sac_get_params(which)[0] - ref)
        assert np.quantile(d, 0.99) <= 5e-6 and d.max() <= 3 * 1e-3, (which, np.quantile(d, 0.99), d.max())


def test_cvpo_end_to_end_on_a_wrapped_store_vs_oracle(make):
    """the same for CVPO: indices, target noise and the K particle blocks from the model.  Bounds: test_cvpo_variants_vs_oracle's."""
    from oracle.cvpo import CVPOConfig, CVPOOracle
    Do, Da, H, B, K, w = 7, 3, 64, 100, 16, WRAPPED
    rng = np.random.default_rng(Do + 10 * Da)
    ocfg = CVPOConfig(obs_dim=Do, act_dim=Da, hidden=(H, H), max_action=1.0, gamma=0.97, n_step=w["n_step"], tau=0.1,
                      double_critic=False, sample_act_num=K, estep_iter_num=1, mstep_iter_num=1, cost_limit=0.5,
                      max_episode_steps=50, mstep_kl_mu=1e-4, mstep_kl_std=1e-5, actor_lr=1e-3)
    o = CVPOOracle(ocfg)
    n_a = sum(int(np.prod(s)) for s in o.aspec.values()); n_c = sum(int(np.prod(s)) for s in o.cspec.values())
    tha = (0.2 * rng.standard_normal(n_a)).astype(np.float32)
    thc = (0.2 * rng.standard_normal(2 * n_c)).astype(np.float32)
    o.set_params(tha, thc)
    rig = make("cvpo", Do, Da, w["E"], w["sub"], n_step=w["n_step"], hidden=(H, H), K=K, gamma=0.97, params=(tha, thc),
               qc_thres=ocfg.qc_thres, actor_lr=1e-3, tau=0.1, double_critic=False, estep_iter_num=1, mstep_iter_num=1,
               mstep_kl_mu=1e-4, mstep_kl_std=1e-5).fill(rng, w["rows"], w["lag_env"])
    store, index = _wrapped_index(rig)
    keys = ["loss/estep_loss", "estep/dual0", "estep/dual1", "mstep/mstep_kl_mu", "mstep/mstep_kl_std", "mstep/mstep_loss_kl",
            "mstep/mstep_loss_mle", "mstep/mstep_loss_total", "mstep/mstep_dual_mu", "mstep/mstep_dual_std", "mstep/entropy",
            "loss/loss_q0", "estep/val_q0", "loss/loss_q1", "estep/val_q1", "estep/thres_q1", "loss/q_total"]
    for cyc in range(2):
        o.pre_update()
        if cyc:
            rig.eng.cvpo_pre_update()                        # (the rig ran the first one)
        for u in range(2):
            st = rig.update(B, seed=23 if rig.count == 0 else 0, sync=True)
            rig.check(B, (cyc, u))
            idx, et, _, _, _ = rig.model(B)
            ek = S.particles(rig.key, rig.count - 1, B, Da, K)
            want, _, _ = o.update(store, index, idx, et.astype(np.float32), ek.astype(np.float32))
            for j, kname in enumerate(keys):
                v = float(want[kname])
                assert abs(st[j] - v) <= 2e-4 * abs(v) + 2e-5, (cyc, u, kname, st[j], v)
            d = rig.eng.cvpo_duals()
            np.testing.assert_allclose(d, [o.estep_dual[0].item(), o.estep_dual[1].item(), o.mstep_dual_mu.item(),
                                           o.mstep_dual_std.item()], rtol=2e-4, atol=2e-5)
        o.post_update(); rig.eng.cvpo_post_update()
    for got, ref in ((rig.eng.sac_get_params(0)[0], o.actor_flat()), (rig.eng.sac_get_params(3)[0], o.actor_flat(old=True)),
                     (rig.eng.sac_get_params(1)[0], o.critics_flat()), (rig.eng.sac_get_params(2)[0], o.critics_flat(old=True))):
        d = np.abs(got - ref)
        assert np.quantile(d, 0.99) <= 1e-5 and d.max() <= 5e-3, (np.quantile(d, 0.99), d.max())
