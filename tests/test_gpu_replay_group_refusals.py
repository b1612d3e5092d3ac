"""A refused grouped replay update changes nothing.  The fused SAC-Lag, the layered SAC-Lag and the CVPO update validate a call in
one shared frame (host_sac_group.inc: rgroup_begin) before anything is enqueued or any member's counters move: after a refusal
every member is still bit-identical to a solo twin that was never in a group, and the next accepted call is what it would have
been without the refusal.  The single-context updates are the reference; every comparison is exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

Do, Da, B = 8, 2, 32
PATHS = {  # hidden_sizes, CVPO options (None: SAC-Lag)
    "fused_sacl": ((64, 64), None),
    "layered_sacl": ((64, 48, 32), None),
    "cvpo": ((64, 64), dict(sample_act_num=4, mstep_iter_num=2)),
}
LAM = [0.1, 0.2]
RESC = [1.0 / (1.0 + l) for l in LAM]


def _member(path, seed, T=150, env_num=4):
    """a context of `path` with parameters and T pushed vector steps of its own (T = 0: an empty store)"""
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig
    hs, cv = PATHS[path]
    eng = Engine(EngineConfig(algo=_lib.ALGO_SAC_LAG, obs_dim=Do, act_dim=Da, hidden_sizes=hs, n_critics=2, env_num=env_num,
                              buffer_size=env_num * 400, gamma=0.99, target_kl=None))
    rng = np.random.default_rng(100 + seed)
    if cv is None:
        eng.sac_init(actor_lr=5e-4 * (1 + 0.1 * seed), critic_lr=1e-3, tau=0.05, n_step=2, auto_alpha=True, use_lagrangian=True)
    else:
        eng.cvpo_init(0.1 + 0.02 * seed, actor_lr=5e-4 * (1 + 0.1 * seed), critic_lr=1e-3, tau=0.05, **cv)
    eng.sac_set_params(0.1 * rng.standard_normal(eng.n_sac_actor).astype(np.float32),
                       0.1 * rng.standard_normal(eng.n_sac_critics).astype(np.float32), float(np.log(0.2)) if cv is None else 0.0)
    if cv is not None:
        eng.cvpo_post_update()                     # actor_old <- actor
        eng.cvpo_pre_update()
    ids = np.arange(env_num)
    for t in range(T):
        obs = rng.standard_normal((env_num, Do)).astype(np.float32)
        act = np.tanh(rng.standard_normal((env_num, Da))).astype(np.float32)
        term = rng.random(env_num) < 0.03
        trunc = np.full(env_num, (t + 1) % 50 == 0) & ~term
        eng.push(ids, obs, act, rng.normal(0.5, 0.5, env_num), (rng.random(env_num) < 0.2).astype(np.float64), term, trunc,
                 rng.standard_normal((env_num, Do)).astype(np.float32))
    return eng


def _own_update(path, eng, i, seed=0):
    if PATHS[path][1] is None:
        eng.sac_update(B, [LAM[i]], RESC[i], seed=seed, sync=False)
    else:
        eng.cvpo_update(B, seed=seed, sync=False)


def _group(path, engines):
    from fsrl_amd.engine import EngineCvpoGroup, EngineSacGroup
    return EngineSacGroup(engines) if PATHS[path][1] is None else EngineCvpoGroup(engines)


def _group_update(path, g, n):
    if PATHS[path][1] is None:
        g.update(B, n, [[l] for l in LAM[:len(n)]], RESC[:len(n)])
    else:
        g.update(B, n)


def _assert_same(path, x, y, rows):
    """actor, critics, target critics; alpha (SAC-Lag) or the four duals (CVPO); the drained rows, `rows` of them"""
    for w in (0, 1, 2):
        assert np.array_equal(x.sac_get_params(w)[0], y.sac_get_params(w)[0]), (path, w)
    if PATHS[path][1] is None:
        assert x.sac_get_params(0)[1] == y.sac_get_params(0)[1], path
    else:
        assert np.array_equal(x.cvpo_duals(), y.cvpo_duals()), path
    rx, ry = x.sac_drain(), y.sac_drain()
    assert len(rx) == len(ry) == rows, (path, len(rx), len(ry), rows)
    assert np.array_equal(rx, ry), path


@pytest.mark.parametrize("path", list(PATHS))
def test_a_refused_grouped_update_changes_nothing(path):
    grouped, solo = [_member(path, i, T=150 + 37 * i) for i in range(2)], [_member(path, i, T=150 + 37 * i) for i in range(2)]
    # a second group: member 0 with a solo twin, member 1 with an empty store
    other, other_twin = [_member(path, 0), _member(path, 1, T=0)], _member(path, 0)
    everything = grouped + solo + other + [other_twin]
    for i in range(2):                             # key each member's Philox stream (one own update on both twins)
        for e in (grouped[i], solo[i]):
            _own_update(path, e, i, seed=11 + i)
    for e in (other[0], other_twin):
        _own_update(path, e, 0, seed=11)
    g, g2 = _group(path, grouped), _group(path, other)
    try:
        with pytest.raises(AssertionError, match=r"n_updates\[1\] < 0"):
            _group_update(path, g, [2, -1])
        with pytest.raises(AssertionError, match="member 1: empty replay store"):
            _group_update(path, g2, [2, 1])
        _assert_same(path, other[0], other_twin, rows=1)           # nothing ran: the keying update's row alone
        # recovery: the first group's next call is what it would have been without the refusal
        n = [2, 1]
        _group_update(path, g, n)
        for i in range(2):
            for _ in range(n[i]):
                _own_update(path, solo[i], i)
            _assert_same(path, grouped[i], solo[i], rows=1 + n[i])
    finally:
        g.close(); g2.close()
        for e in everything:
            e.close()


@pytest.mark.parametrize("path", ["fused_sacl", "layered_sacl"])
@pytest.mark.parametrize("k", [1, 2])
def test_a_sac_group_refuses_a_member_reinitialised_as_cvpo(path, k):
    """cvpo_init re-creates a grouped member's state without telling its group: the SAC group's next update names that member and
    runs nothing, also where the re-initialised member is member 0 (the one the group's kind is read from) or the only one"""
    engs = [_member(path, i, T=20) for i in range(k)]
    g = _group(path, engs)
    try:
        engs[0].cvpo_init(0.1)
        with pytest.raises(AssertionError, match="member 0 is no longer a context of the group's kind and shape"):
            _group_update(path, g, [1] * k)
    finally:
        g.close()
        for e in engs:
            e.close()
