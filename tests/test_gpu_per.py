"""Prioritised replay on the device (fsrl_per_*, kernels_per.hpp) against the exact CPU model of tests/test_per_model.py.

Device pow may differ from numpy's by an ulp, so leaves are compared at relative 1e-12 and every later check starts from the
device's OWN leaves (fsrl_per_state): loaded into the model, they must give the device's sample element for element, its importance
weights within relative 1e-6 (one float32 rounding is 6e-8; pow in float64 adds nothing visible), and -- fed the TD averages the
device formed (fsrl_per_last_td) -- its new leaves and scalars at 1e-12 again, with numpy's duplicate winner.  The root must equal
the model's sum tree over the device's leaves exactly: every node is one IEEE add.

The weighted update itself is held against the float32 torch restatement (validated against the oracles with w = 1 in
test_per_model.py) at the bars tests/test_gpu_sac.py uses for the unweighted update: statistics 5e-5 rel + 5e-6 abs, parameters after
three updates 99 % within 5e-6 and all within 5e-4, alpha within 1e-6.  The TD averages are compared at 5e-5 rel + 2e-5 abs: each of
the up to four Q values and two targets behind one is an fp32 chain of at most 64-term dot products on values of magnitude <= 10,
about sqrt(64) * 6e-8 * 10 = 5e-6 apiece.

Stores: 4 x 8 slots and 3 x 7 slots (21: bound 32), partly filled and wrapped; n_step 1 and 2; batches 16 and 33, 1040 for the sample
alone (more rows than the sampling workgroup has threads)."""
import numpy as np
import pytest

from oracle import sampler as S
from test_per_model import (ACT_DIM, ALPHA, BETA, F32_EPS, OBS_DIM, SAMPLER_SEEDS, STORES, UPDATE_SEED, Mirror, PerModel, make_oracle,
                            oracle_store, priorities, restated_update, rollout)

pytestmark = pytest.mark.gpu

KEYS = ["loss/rescaling", "loss/lagrangian", "loss/actor_safety", "loss/alpha_loss", "loss/alpha_value",
        "loss/actor_rew", "loss/actor_total", "loss/q0", "loss/q1", "loss/q_total"]
LAG, RESC = [0.5], 1 / 1.5
NOISE_BOUND = 8.0 * 2.0**-24            # tests/test_gpu_sampler.py: |device - float64 model| <= 8 * 2^-24 * max(1, rad)


class Rig:
    """a replay context of `kind` on store `name`, the mirror of its rows, the oracle with the same parameters; `name` is a key of
    test_per_model.STORES, or a geometry with a rollout of its own (.name, .E, .sub, .rollout(): tests/per_big_problems.py)"""

    def __init__(self, name, kind="sac", hidden=(64, 64), n_step=2, per=(ALPHA, BETA, True), fill=True, enable_first=True):
        from fsrl_amd import _lib
        from fsrl_amd.engine import Engine, EngineConfig
        self.kind, self.n_step = kind, n_step
        if isinstance(name, str):
            self.name, (self.E, self.sub, _), steps = name, STORES[name], lambda: rollout(name)
        else:
            self.name, self.E, self.sub, steps = name.name, name.E, name.sub, name.rollout
        self.oracle, a, c = make_oracle(kind, hidden, n_step)
        ocfg = self.oracle.cfg
        self.eng = Engine(EngineConfig(algo=_lib.ALGO_SAC_LAG, obs_dim=OBS_DIM, act_dim=ACT_DIM, hidden_sizes=tuple(hidden), n_critics=2,
                                       env_num=self.E, buffer_size=self.E * self.sub, gamma=ocfg.gamma, target_kl=None))
        try:
            if kind == "sac":
                self.eng.sac_init(actor_lr=ocfg.actor_lr, critic_lr=ocfg.critic_lr, alpha_lr=ocfg.alpha_lr, tau=ocfg.tau, alpha=ocfg.alpha,
                                  n_step=n_step, auto_alpha=ocfg.auto_alpha)
            else:
                self.eng.sac_init(actor_lr=ocfg.actor_lr, critic_lr=ocfg.critic_lr, tau=ocfg.tau, n_step=n_step, deterministic=True)
            self.eng.sac_set_params(a, c, 0.0)
            self.mirror = Mirror(self.E, self.sub, OBS_DIM, ACT_DIM)
            self.key, self.count = S.key_of(0), 0
            self.per = per
            if per and enable_first:
                self.eng.per_enable(*per)
            if fill:
                for step in steps():
                    self.push(step)
            if per and not enable_first:
                self.eng.per_enable(*per)
        except Exception:
            self.eng.close()
            raise

    def close(self):
        self.eng.close()

    def push(self, step):
        ptr, *_ = self.eng.push(*step)
        assert np.array_equal(ptr, self.mirror.push(*step))
        return ptr

    def model(self):
        """the model loaded with the device's own leaves and scalars; the root must be the model's, exactly"""
        leaves, mx, mn, total = self.eng.per_state()
        m = PerModel(self.E * self.sub, *self.per).load(leaves, mx, mn)
        assert total == m.total, (total, m.total)
        return m

    def update(self, B, seed=0, **kw):
        if seed:
            self.key = S.key_of(seed)
        st = self.eng.sac_update(B, LAG, RESC, seed=seed, **kw)
        self.count += 1
        return st


@pytest.fixture
def rigs():
    made = []

    def make(*a, **kw):
        made.append(Rig(*a, **kw))
        return made[-1]
    yield make
    for r in made:
        r.close()


def _close(a, b, rel=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool((np.abs(a - b) <= rel * np.abs(b)).all())


# ------------------------------------------------------------------------------------------------ 1: leaves
@pytest.mark.parametrize("name", sorted(STORES))
def test_leaves_follow_pushes_updates_and_resets(rigs, name):
    r = rigs(name, fill=False)
    m = PerModel(r.E * r.sub, ALPHA, BETA)
    steps = rollout(name)
    half = len(steps) // 2
    for step in steps[:half]:
        m.add(r.push(step))
    dev = r.model()
    assert np.array_equal(dev.leaves, m.leaves) and (dev.max_prio, dev.min_prio) == (1.0, 1.0)       # 1 ** alpha is exact
    # priorities from the host: a repeated index among them, max_prio above 1 afterwards
    valid = r.mirror.valid()
    idx = np.concatenate([valid, valid[:2]])
    w = np.random.default_rng(7).uniform(0.05, 3.0, idx.size) * np.where(np.arange(idx.size) % 2, -1.0, 1.0)
    r.eng.per_update_weight(idx, w)
    m.update_weight(idx, w)
    dev = r.model()
    assert _close(dev.leaves, m.leaves) and _close(dev.max_prio, m.max_prio) and _close(dev.min_prio, m.min_prio)
    assert m.max_prio > 1.0 > m.min_prio
    # rows pushed after it take max_prio ** alpha with the max_prio it left (the wrapped stores overwrite slots here)
    for step in steps[half:]:
        m.add(r.push(step))
    dev = r.model()
    assert _close(dev.leaves, m.leaves) and (dev.leaves > 0).sum() == len(r.mirror.valid())
    assert dev.max_prio == m.max_prio and dev.min_prio == m.min_prio
    # reset: an empty tree, both scalars back at 1; configure: the tree of the new geometry
    r.eng.reset_store(False)
    leaves, mx, mn, total = r.eng.per_state()
    assert not leaves.any() and (mx, mn, total) == (1.0, 1.0, 0.0)
    r.eng.store_configure(2 * 5, 2)
    r.eng.push([1, 0], *[x[:2] for x in steps[0][1:]])
    leaves, mx, mn, total = r.eng.per_state()
    assert leaves.size == 10 and np.array_equal(np.flatnonzero(leaves), [0, 5]) and total == 2.0 and (leaves[[0, 5]] == 1.0).all()


def test_enable_on_a_filled_store_gives_stored_rows_the_initial_priority(rigs):
    r = rigs("np2_wrap", enable_first=False)
    dev = r.model()
    want = np.zeros(21)
    want[r.mirror.valid()] = 1.0
    assert np.array_equal(dev.leaves, want) and dev.total == want.sum()


def test_store_fill_gives_poured_rows_the_priority_of_a_push(rigs):
    """twin contexts with max_prio raised: A is filled from an archive, B pushed row by row (the model of fsrl_store_fill)"""
    from test_gpu_store_fill import archive_of, dataset, push_loop
    a, b = rigs("p2_part"), rigs("p2_part")
    data = dataset(OBS_DIM, ACT_DIM, [3, 5, 2, 4], seed=3)
    for r in (a, b):
        r.eng.per_update_weight([0, 9], [2.5, 0.5])
        for e in range(r.E):                # close the episodes in progress: a fill refuses a sub-buffer with one open
            z = np.zeros((1, OBS_DIM), np.float32)
            r.eng.push([e], z, np.zeros((1, ACT_DIM), np.float32), [0.0], [0.0], [True], [False], z)
    arch = archive_of(a.eng, data)
    assert a.eng.store_fill(arch) == 14
    push_loop(b.eng, data, range(4), 0, a.E, 0, None, None)
    la, lb = a.eng.per_state(), b.eng.per_state()
    assert np.array_equal(la[0], lb[0]) and la[1:] == lb[1:]
    m = PerModel(32, ALPHA, BETA).load(la[0])
    assert la[3] == m.total and _close(la[0].max(), (2.5 + F32_EPS)**ALPHA)
    assert (la[0] == la[0].max()).sum() >= 14 - 8       # every poured row that was not overwritten again carries it
    arch.close()


# ------------------------------------------------------------------------------------------------ 2 + 3: sample, weights, priorities
def _check_sample(r, B, m, twin=None):
    """the last update's sample against the model `m` (the device's leaves from BEFORE the update) -> (idx, eps_t, eps_p, w)"""
    idx, et, ep = r.eng.sac_last_sample(B)
    want = m.sample(r.key, r.count - 1, B)
    assert np.isin(want, r.mirror.valid()).all()                     # the condition on the inputs (test_per_model.py), on the device's leaves
    assert np.array_equal(idx, want), (np.flatnonzero(idx != want)[:8], idx[:8], want[:8])
    chain, end = r.eng.sac_last_chain(B, r.n_step)
    w_chain, w_end, _ = S.chains(idx, r.n_step, r.mirror.book, r.mirror.done, r.sub)
    assert np.array_equal(chain, w_chain) and np.array_equal(end.astype(bool), w_end)
    w_t, w_p, r_t, r_p = S.noise(r.key, r.count - 1, B, ACT_DIM, with_rad=True)
    for dev, ref, rad in ((et, w_t, r_t), (ep, w_p, r_p)):
        assert (np.abs(dev - ref) <= NOISE_BOUND * np.maximum(1.0, rad)).all()
    if twin is not None:            # ... and bit for bit the uniform sampler's noise at the same key and update count
        _, tt, tp = twin.eng.sac_last_sample(B)
        assert np.array_equal(et, tt) and np.array_equal(ep, tp)
    w = r.eng.per_last_weights(B)
    assert _close(w, m.weights(idx), 1e-6) and w.max() == 1.0
    return idx, et, ep, w


def _check_priorities(r, B, m, idx):
    """the leaves after the update against the model fed the TD averages the device formed"""
    td = r.eng.per_last_td(B)
    m.update_weight(idx, td)
    dev = r.model()
    assert _close(dev.leaves, m.leaves) and _close(dev.max_prio, m.max_prio) and _close(dev.min_prio, m.min_prio)
    u, cnt = np.unique(idx, return_counts=True)
    for s in u[cnt > 1]:            # numpy's fancy assignment: the highest batch position wrote the slot
        last = np.flatnonzero(idx == s)[-1]
        assert _close(dev.leaves[s], (abs(float(td[last])) + F32_EPS)**r.per[0])
    return td, dev


@pytest.mark.parametrize("name,n_step", [("p2_part", 2), ("p2_wrap", 1), ("np2_part", 1), ("np2_wrap", 2)])
def test_sample_weights_and_new_priorities_equal_the_model(rigs, name, n_step):
    r, twin = rigs(name, n_step=n_step), rigs(name, n_step=n_step, per=None)
    r.eng.per_update_weight(*priorities(name))
    dup_seen = False
    for seed in SAMPLER_SEEDS:
        for B in (16, 33, 1040):
            m = r.model()
            r.update(B, seed=seed)
            twin.update(B, seed=seed)
            idx, *_ = _check_sample(r, B, m, twin)
            _check_priorities(r, B, m, idx)
            dup_seen |= len(np.unique(idx)) < B
            seed = 0                                        # keeps the key: the update count moves the stream
    assert dup_seen


def test_caller_given_indices_take_their_weights_from_the_leaves_and_update_them(rigs):
    """parity mode on a prioritised context: the twin replays the library-RNG sample through the caller-RNG arguments"""
    a, b = rigs("np2_wrap"), rigs("np2_wrap")
    for r in (a, b):
        r.eng.per_update_weight(*priorities("np2_wrap"))
    for u in range(2):
        sa = a.update(33, seed=UPDATE_SEED if u == 0 else 0)
        idx, et, ep = a.eng.sac_last_sample(33)
        sb = b.update(33, indices=idx, eps_target=et, eps_pi=ep)
        assert np.array_equal(sa, sb) and np.array_equal(a.eng.per_last_weights(33), b.eng.per_last_weights(33))
    assert all(np.array_equal(x, y) for x, y in zip(a.eng.per_state(), b.eng.per_state()))
    for which in (0, 1, 2):
        assert np.array_equal(a.eng.sac_get_params(which)[0], b.eng.sac_get_params(which)[0])


def test_set_beta_and_weight_norm_off(rigs):
    r = rigs("p2_wrap", per=(ALPHA, BETA, False))
    r.eng.per_update_weight(*priorities("p2_wrap"))
    r.eng.per_set_beta(0.9)
    r.per = (ALPHA, 0.9, False)
    m = r.model()
    r.update(33, seed=UPDATE_SEED)
    idx, *_ = r.eng.sac_last_sample(33)
    w = r.eng.per_last_weights(33)
    assert _close(w, m.weights(idx), 1e-6) and w.max() != 1.0 and np.ptp(w) > 0.1


# ------------------------------------------------------------------------------------------------ 4: all weights 1
@pytest.mark.parametrize("kind,hidden,name,alpha,n_upd", [("sac", (64, 64), "p2_wrap", ALPHA, 1), ("sac", (64, 64), "np2_part", 0.0, 3),
                                                         ("sac", (32, 16, 8), "np2_wrap", 0.0, 3), ("ddpg", (64, 64), "p2_part", 0.0, 3),
                                                         ("ddpg", (32, 16, 8), "p2_wrap", ALPHA, 1)])
def test_unit_weights_are_bit_identical_to_the_uniform_update(rigs, kind, hidden, name, alpha, n_upd):
    """a fresh store has equal leaves, so with weight_norm every weight is 1 (alpha = 0 keeps it so over later updates): the
    prioritised update must give the bits of a twin without PER that is handed the same indices and noise"""
    r = rigs(name, kind, hidden, per=(alpha, BETA, True))
    twin = rigs(name, kind, hidden, per=None)
    for u in range(n_upd):
        st = r.update(33, seed=UPDATE_SEED if u == 0 else 0)
        idx, et, ep = r.eng.sac_last_sample(33)
        assert (r.eng.per_last_weights(33) == 1.0).all()
        assert np.array_equal(st, twin.update(33, indices=idx, eps_target=et, eps_pi=ep))
    for which in (0, 1, 2) + ((3, ) if kind == "ddpg" else ()):
        assert np.array_equal(r.eng.sac_get_params(which)[0], twin.eng.sac_get_params(which)[0])


# ------------------------------------------------------------------------------------------------ 5: the weighted update
@pytest.mark.parametrize("kind,hidden,name,n_step,B", [("sac", (64, 64), "p2_wrap", 2, 33), ("sac", (32, 16, 8), "np2_wrap", 1, 16),
                                                      ("ddpg", (64, 64), "np2_part", 2, 16), ("ddpg", (32, 16, 8), "p2_part", 1, 33)])
def test_weighted_updates_match_the_restatement(rigs, kind, hidden, name, n_step, B):
    r = rigs(name, kind, hidden, n_step)
    r.eng.per_update_weight(*priorities(name))
    store, index = oracle_store(r.mirror)
    o = r.oracle
    for u in range(3):
        m = r.model()
        st = r.update(B, seed=UPDATE_SEED if u == 0 else 0)
        idx, et, ep, w = _check_sample(r, B, m)
        assert np.ptp(w) > 0.05                              # the weights are not uniform
        sa, sc, td_ref = restated_update(kind, o, store, index, idx, et, ep, LAG, RESC, w)
        want = {**sa, **sc}
        for j, k in enumerate(KEYS):
            if k in want:
                assert abs(st[j] - want[k]) <= 5e-5 * abs(want[k]) + 5e-6, (u, k, st[j], want[k])
        td, _ = _check_priorities(r, B, m, idx)
        assert (np.abs(td - td_ref) <= 5e-5 * np.abs(td_ref) + 2e-5).all(), np.abs(td - td_ref).max()
    refs = [(0, o.actor_flat()), (1, o.critics_flat()), (2, o.critics_flat(old=True))]
    if kind == "ddpg":
        refs.append((3, o.actor_flat(old=True)))
    for which, ref in refs:
        d = np.abs(r.eng.sac_get_params(which)[0] - ref)
        assert np.quantile(d, 0.99) <= 5e-6 and d.max() <= 5e-4, (which, np.quantile(d, 0.99), d.max())
    if kind == "sac":
        assert abs(r.eng.sac_get_params(0)[1] - float(o.alpha)) < 1e-6


# ------------------------------------------------------------------------------------------------ 7: refusals
def test_refusals_name_their_reason(rigs):
    from fsrl_amd.engine import EngineCvpoGroup, EngineSacGroup
    cv = rigs("p2_part", per=None, fill=False)
    cv.eng.cvpo_init(0.2)
    with pytest.raises(AssertionError, match="CVPO"):
        cv.eng.per_enable(ALPHA, BETA)
    a, b = rigs("p2_part"), rigs("p2_part", per=None)
    with pytest.raises(AssertionError, match="member 0 has prioritised replay on"):
        EngineSacGroup([a.eng, b.eng])
    with pytest.raises(AssertionError, match="member 1 has prioritised replay on"):
        EngineSacGroup([b.eng, a.eng])
    with pytest.raises(AssertionError, match="prioritised replay"):
        EngineCvpoGroup([a.eng])
    with pytest.raises(AssertionError, match="prioritised replay"):
        a.eng.cvpo_init(0.2)
    g = EngineSacGroup([b.eng])
    with pytest.raises(AssertionError, match="already in a group"):
        b.eng.per_enable(ALPHA, BETA)
    g.close()
    b.eng.per_enable(ALPHA, BETA)                          # out of the group again: allowed
    with pytest.raises(AssertionError, match="out of range"):
        b.eng.per_update_weight([32], [1.0])
    with pytest.raises(Exception, match="fsrl_per_enable first"):
        cv.eng.per_state()


# ------------------------------------------------------------------------------------------------ 8: training state
@pytest.mark.parametrize("kind,hidden,name", [("sac", (64, 64), "np2_wrap"), ("ddpg", (32, 16, 8), "p2_part")])
def test_training_state_carries_the_tree(rigs, kind, hidden, name):
    """export after two prioritised updates, import into a fresh context (another alpha / beta, an empty store): the next three
    updates and the trees after them are the uninterrupted run's, bit for bit; blobs and contexts that disagree are refused"""
    a = rigs(name, kind, hidden)
    a.eng.per_update_weight(*priorities(name))
    a.eng.per_set_beta(0.7)
    for u in range(2):
        a.update(33, seed=UPDATE_SEED if u == 0 else 0)
    blob = a.eng.train_state(with_store=True)
    b = rigs(name, kind, hidden, per=(0.3, 0.1, False), fill=False)
    b.eng.load_train_state(blob)
    assert all(np.array_equal(x, y) for x, y in zip(a.eng.per_state(), b.eng.per_state()))
    for u in range(3):
        sa, sb = a.update(33), b.update(33)
        assert np.array_equal(sa, sb)
        assert np.array_equal(a.eng.per_last_weights(33), b.eng.per_last_weights(33))
        assert all(np.array_equal(x, y) for x, y in zip(a.eng.sac_last_sample(33), b.eng.sac_last_sample(33)))
    assert all(np.array_equal(x, y) for x, y in zip(a.eng.per_state(), b.eng.per_state()))
    for which in (0, 1, 2):
        assert np.array_equal(a.eng.sac_get_params(which)[0], b.eng.sac_get_params(which)[0])
    # the same blob again is the same bytes; a context without PER keeps the size it always had
    assert a.eng.train_state(with_store=True) == b.eng.train_state(with_store=True)
    plain = rigs(name, kind, hidden, per=None)
    with pytest.raises(AssertionError, match="prioritised-replay state and this context has it off"):
        plain.eng.load_train_state(blob)
    with pytest.raises(AssertionError, match="this context has prioritised replay on"):
        b.eng.load_train_state(plain.eng.train_state(with_store=True))
    n_plain, n_per = len(plain.eng.train_state(with_store=False)), len(a.eng.train_state(with_store=False))
    assert n_per == n_plain + 16 + 48                       # one more section: its head (tag, length) and PerHead, no leaves
    # without the store only the options travel: b's own tree stays
    before = b.eng.per_state()
    a.eng.per_set_beta(0.2)
    b.eng.load_train_state(a.eng.train_state(with_store=False))
    assert all(np.array_equal(x, y) for x, y in zip(before, b.eng.per_state()))
    a.update(16), b.update(16)
    assert np.array_equal(a.eng.per_last_weights(16), b.eng.per_last_weights(16))
    # device-to-device copy: the tree goes along, a destination without PER is refused
    c = rigs(name, kind, hidden, per=(0.9, 0.9, True), fill=False)
    c.eng.copy_train_state_from(a.eng)
    assert all(np.array_equal(x, y) for x, y in zip(a.eng.per_state(), c.eng.per_state()))
    assert np.array_equal(a.update(33), c.update(33))
    with pytest.raises(AssertionError, match="prioritised replay is on in the source and off in the destination"):
        plain.eng.copy_train_state_from(a.eng)


# ------------------------------------------------------------------------------------------------ the Python surface
def test_prioritized_buffer_proxy_is_tianshous_interface(rigs):
    from fsrl_amd.data import HipPrioritizedVectorReplayBuffer
    r = rigs("np2_part", per=None, fill=False)
    buf = HipPrioritizedVectorReplayBuffer(r.eng, 21, 3, alpha=0.5, beta=0.4)
    r.per = (0.5, 0.4, True)
    for step in rollout("np2_part"):
        r.push(step)
    valid = r.mirror.valid()
    import torch
    buf.update_weight(valid[:4], torch.tensor([4.0, -0.25, 1.0, 9.0]))
    m = PerModel(21, 0.5, 0.4)
    m.add(valid)
    m.update_weight(valid[:4], [4.0, -0.25, 1.0, 9.0])
    assert _close(r.model().leaves, m.leaves)
    assert _close(buf.get_weight(valid[:6]), (m.leaves[valid[:6]] / m.min_prio)**-0.4)
    buf.set_beta(1.0)
    assert _close(buf.get_weight(valid[:6]), (m.leaves[valid[:6]] / m.min_prio)**-1.0)
    buf.reset()
    assert not r.eng.per_state()[0].any() and len(buf) == 0


def test_agents_learn_with_prioritized_replay(tmp_path):
    from fsrl_amd.agent import CVPOAgent, DDPGLagAgent, SACLagAgent
    from fsrl_amd.env import SyntheticSafetyVectorEnv
    from fsrl_amd.utils import BaseLogger
    for cls in (SACLagAgent, DDPGLagAgent):
        train = SyntheticSafetyVectorEnv(env_num=4, episode_len=40, seed=1)
        agent = cls(train, BaseLogger(str(tmp_path / cls.__name__), name="p"), cost_limit=10, device="cuda:0", seed=3, hidden_sizes=(64, 64),
                    training_num=4, buffer_size=4000)
        a0, _ = agent.policy.engine.sac_get_params(0)
        ep, stat, _ = agent.learn(train, None, epoch=1, episode_per_collect=4, step_per_epoch=320, update_per_step=0.2, batch_size=64,
                                  verbose=False, save_ckpt=False, prioritized_replay=dict(alpha=0.6, beta=0.4))
        assert ep == 1 and np.isfinite(list(stat.values())).all() and "loss/q_total" in stat
        leaves, mx, mn, total = agent.policy.engine.per_state()
        assert (leaves > 0).sum() == len(agent.policy.engine) and mx > 1.0 > mn > 0.0 and len(np.unique(leaves)) > 10
        assert np.abs(agent.policy.engine.sac_get_params(0)[0] - a0).max() > 1e-4
        with pytest.raises(ValueError, match="alpha, beta"):
            agent.learn(train, None, epoch=1, prioritized_replay=dict(alpha=0.6))
    env = SyntheticSafetyVectorEnv(env_num=4, episode_len=40, seed=1)
    cv = CVPOAgent(env, None, cost_limit=10, device="cuda:0", seed=3, hidden_sizes=(64, 64), training_num=4, buffer_size=4000)
    with pytest.raises(NotImplementedError, match="SACLagAgent and DDPGLagAgent"):
        cv.learn(env, None, epoch=1, prioritized_replay=dict(alpha=0.6, beta=0.4))
