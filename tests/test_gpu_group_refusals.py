"""A refused grouped on-policy update leaves the group as it was.  The PPO-Lagrangian and the FOCOPS group, fused and layered, run
inside one frame (host_group.inc: ogroup_*); a permutation that is bad for the LAST member is found in pass 0, after every member
has been through fsrl_ppo_begin and the members before it through their batch preparation.  The call raises and names the perm,
every member then accepts its own update (no member is left "inside an update"), and the group's next two updates are bit for bit
those of a twin group that never saw the refusal: logged rows, stopped passes and parameters, the second update carrying the Adam
moments and step counters.  Group against twin group, so the comparison is exact for the fused PPO group too (whose tile heights
differ from a solo run's).  rew_norm stays off: with it a second fsrl_ppo_begin updates the return statistics again."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K, ENVS, T, B, R = 2, 2, 75, 64, 2
N = ENVS * T
PATHS = {  # algorithm, hidden_sizes
    "ppol_fused": ("ppol", (64, 64)),
    "ppol_layered": ("ppol", (64, 48, 32)),
    "focops_fused": ("focops", (64, 64)),
    "focops_layered": ("focops", (64, 64, 64)),
}
LAGS, RESC = [[0.2], [0.5]], [1 / 1.2, 1 / 1.5]
NUS, NU_LOSSES = [0.1, 0.4], [0.5, -1.0]


def _member(path, seed, Do=8, Da=2):
    """an engine of `path` with parameters and T vector steps of synthetic transitions of its own (the _filled pattern of
    tests/test_gpu_group_layered.py)"""
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig
    algo, hidden = PATHS[path]
    if algo == "ppol":
        e = Engine(EngineConfig(obs_dim=Do, act_dim=Da, hidden_sizes=hidden, env_num=ENVS, max_grad_norm=0.5, target_kl=None,
                                rew_norm=False))
    else:
        e = Engine(EngineConfig(algo=_lib.ALGO_FOCOPS, obs_dim=Do, act_dim=Da, hidden_sizes=hidden, n_critics=2, env_num=ENVS,
                                target_kl=None, rew_norm=False))
        e.focops_init(actor_lr=5e-4 * (1 + seed))
    r = np.random.default_rng(40 + seed)
    e.set_params((0.1 * r.standard_normal(e.n_params)).astype(np.float32))
    obs = r.standard_normal((T + 1, ENVS, Do)).astype(np.float32)
    ids = list(range(ENVS))
    for t in range(T):
        e.push(ids, obs[t], 0.3 * r.standard_normal((ENVS, Da)).astype(np.float32), r.normal(0.5, 0.5, ENVS),
               (r.random(ENVS) < 0.1).astype(np.float64), [False] * ENVS, [t == T - 1] * ENVS, obs[t + 1])
    assert len(e) == N
    return e


def _group_update(path, grp, perms):
    if PATHS[path][0] == "ppol":
        return grp.ppo_update(LAGS, RESC, B, R, perms=perms)
    return grp.focops_update(NUS, NU_LOSSES, B, R, perms=perms)


def _own_update(path, e, i, perm):
    if PATHS[path][0] == "ppol":
        return e.ppo_update(LAGS[i], RESC[i], B, R, perms=perm)
    return e.focops_update(NUS[i], NU_LOSSES[i], B, R, perms=perm)


def _bad_perms(perms, fault):
    """`perms` with the LAST member's pass-0 permutation spoiled; member 0's stay valid"""
    bad = [[p.copy() for p in member] for member in perms]
    if fault == "out of range":
        bad[-1][0][3] = N                          # an index equal to n
    else:
        bad[-1][0][3] = bad[-1][0][2]              # a repeated index
    return bad


@pytest.mark.parametrize("fault", ["out of range", "not a permutation"])
@pytest.mark.parametrize("path", list(PATHS))
def test_a_refused_grouped_update_leaves_the_group_as_it_was(path, fault):
    from fsrl_amd.engine import EngineGroup
    mk = lambda: [_member(path, i) for i in range(K)]
    a, b, c = mk(), mk(), mk()                     # a: refused, then compared with b, which never is; c: refused, then own updates
    rng = np.random.default_rng(7)
    perms = [[rng.permutation(N) for _ in range(R)] for _ in range(K)]
    bad = _bad_perms(perms, fault)
    ga, gb, gc = EngineGroup(a), EngineGroup(b), EngineGroup(c)
    try:
        for g in (ga, gc):
            with pytest.raises(AssertionError, match=fault):
                _group_update(path, g, bad)
        for i, e in enumerate(c):                  # in_update was cleared on every member: no "inside an update" refusal
            st, stop = _own_update(path, e, i, perms[i])
            assert st.shape[0] > 0 and np.isfinite(st).all(), (path, i, st.shape, stop)
        for rnd in range(2):
            (st_a, stop_a), (st_b, stop_b) = _group_update(path, ga, perms), _group_update(path, gb, perms)
            for i in range(K):
                tag = (path, fault, rnd, i)
                assert stop_a[i] == stop_b[i], (tag, stop_a, stop_b)
                assert st_a[i].shape == st_b[i].shape and st_a[i].shape[0] > 0, (tag, st_a[i].shape, st_b[i].shape)
                assert np.array_equal(st_a[i], st_b[i]), (tag, "logged rows", float(np.abs(st_a[i] - st_b[i]).max()))
                th_a, th_b = a[i].get_params(), b[i].get_params()
                assert np.array_equal(th_a, th_b), (tag, "parameters", float(np.abs(th_a - th_b).max()))
    finally:
        for g in (ga, gb, gc):
            g.close()
        for e in a + b + c:
            e.close()
