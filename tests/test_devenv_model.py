"""The host model of the device environments (tests/devenv_model.py) against the host envs it restates, and the properties the GPU
tests lean on: the float64 point-circle model is toy.PointCircleEnv, the linear model is SyntheticSafetyVectorEnv with the noise
injected, the collect loop yields exactly n_episode episodes with the counters DESIGN.md 3.4.1 describes, and on the inputs the GPU
tests inject the discontinuity rule leaves out a small share of the rows only.  No GPU."""
import numpy as np
import pytest

import devenv_model as dm
from fsrl_amd.env.synthetic import SyntheticSafetyVectorEnv
from fsrl_amd.env.toy import PointCircleEnv

F32, F64 = np.float32, np.float64


def test_point_circle_float64_is_the_toy_env_step_for_step():
    env = PointCircleEnv(max_episode_steps=50, radius=0.4, x_lim=0.3, dt=0.1)
    env.reset(seed=3)
    state = np.concatenate([env.pos, env.vel])[None, :]
    rng = np.random.default_rng(1)
    costs = terms = 0
    for t in range(50):
        act = rng.uniform(-1.4, 1.4, 2) if t < 20 else rng.uniform(0.8, 1.4, 2)       # wander, then run off: r crosses 4 radius
        obs, rew, term, trunc, info = env.step(act)
        r = dm.point_step(state, act[None, :], 0.4, 0.3, 0.1, F64)
        state = r["state"]
        np.testing.assert_allclose(state[0], np.concatenate([env.pos, env.vel]), rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose(r["rew"][0], rew, rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(r["obs_next"][0].astype(F32), obs, rtol=3e-7, atol=1e-7)
        assert r["cost"][0] == info["cost"] and bool(r["terminated"][0]) == term
        costs += info["cost"]; terms += term
    assert costs > 0 and terms > 0                 # both branches were walked


def test_point_circle_reset_draws_are_uniform_on_the_grid_and_centred():
    key = dm.key_of(7)
    st, obs = dm.point_reset(key, np.arange(64), np.arange(64) % 5, 1.5, 1.0, F64)
    assert np.all(st[:, :2] >= -0.5) and np.all(st[:, :2] < 0.5) and np.all(st[:, 2:] == 0)
    assert np.all((st[:, :2] + 0.5) * 16777216.0 == np.round((st[:, :2] + 0.5) * 16777216.0))
    st32, _ = dm.point_reset(key, np.arange(64), np.arange(64) % 5, 1.5, 1.0, F32)
    assert np.array_equal(st32.astype(F64), st)        # u - 0.5 is exact in float32: the restatement IS the float64 value
    assert len(np.unique(st[:, 0])) == 64


@pytest.mark.parametrize("Do,Da", [(8, 2), (33, 8)])
def test_linear_model_is_the_synthetic_env_with_its_noise_injected(Do, Da):
    from fsrl_amd.env.synthetic import stable_coupling
    host = SyntheticSafetyVectorEnv(env_num=9, obs_dim=Do, act_dim=Da, episode_len=5, coupling=stable_coupling(Do), cost_threshold=0.6)
    host.reset()
    rng = np.random.default_rng(2)
    noise = rng.standard_normal((9, Do)).astype(F32)

    class Fixed:
        def standard_normal(self, shape):
            assert tuple(shape) == noise.shape
            return noise.astype(F64)
    state = host.state.copy()
    act = rng.uniform(-1, 1, (9, Da)).astype(F32)
    host.rng = Fixed()
    s, rew, term, trunc, info = host.step(act)
    for dtype, tol in ((F32, 2e-6), (F64, 2e-6)):
        r = dm.linear_step(state, act, host.A, host.B, noise, 0.6, dtype)
        np.testing.assert_allclose(r["obs_next"], s, rtol=tol, atol=tol)
        np.testing.assert_allclose(r["rew"], rew, rtol=tol, atol=tol)
        near = np.abs(np.abs(s[:, 1]) - 0.6) < 1e-4
        assert np.array_equal(r["cost"][~near], info["cost"][~near]) and not r["terminated"].any()
    # ascending sums: the float32 restatement is the explicit loop, element for element
    j = 3
    acc = F32(0)
    for i in range(Do):
        acc = F32(acc + F32(state[0, i] * host.A[i, j]))
    accb = F32(0)
    for k in range(Da):
        accb = F32(accb + F32(act[0, k] * host.B[k, j]))
    want = F32(F32(acc + accb) + F32(F32(0.05) * noise[0, j]))
    assert dm.linear_step(state, act, host.A, host.B, noise, 0.6, F32)["obs_next"][0, j] == want


def test_normals_float32_restatement_sits_at_float32_rounding_from_float64():
    key = dm.key_of(11)
    env, d = np.arange(64)[:, None], np.arange(33)[None, :]
    n64 = dm.normal(key, env, 4, 2, dm.STREAM_STEP, d, F64)
    n32 = dm.normal(key, env, 4, 2, dm.STREAM_STEP, d, F32)
    scale = dm.normal_scale(key, env, 4, 2, dm.STREAM_STEP, d)
    assert np.max(np.abs(n32 - n64) / scale) < 8 * np.finfo(F32).eps
    assert abs(n64.mean()) < 0.1 and 0.9 < n64.std() < 1.1
    # streams, ordinals, steps and envs are independent coordinates of the counter
    assert not np.array_equal(n64, dm.normal(key, env, 4, 2, dm.STREAM_ACT, d, F64))
    assert not np.array_equal(n64, dm.normal(key, env, 5, 2, dm.STREAM_STEP, d, F64))
    assert not np.array_equal(n64, dm.normal(key, env, 4, 3, dm.STREAM_STEP, d, F64))
    assert not np.array_equal(n64, dm.normal(dm.key_of(12), env, 4, 2, dm.STREAM_STEP, d, F64))
    assert not np.array_equal(n64[0], n64[1])


@pytest.mark.parametrize("env_num,n_episode", [(1, 3), (5, 3), (5, 5), (5, 12), (17, 40), (64, 70)])
def test_collect_loop_yields_exactly_n_episode_episodes(env_num, n_episode):
    env = dm.ModelEnv(dm.POINT_CIRCLE, env_num, 7, 3, (0.2, 0.3, 0.1), 6, 2, dtype=F32)
    env.reset()
    rng = np.random.default_rng(0)
    rows, episodes, steps = dm.collect(env, n_episode, lambda obs, ids: rng.uniform(-1, 1, (len(ids), 2)).astype(F32))
    assert episodes == n_episode == sum(r[3] for r in rows)
    # rows of one env are chronological: t counts up inside an ordinal, the ordinal steps by one where an episode ended
    for e in range(env_num):
        mine = [r for r in rows if r[0] == e]
        for a, b in zip(mine, mine[1:]):
            assert (b[1], b[2]) == ((a[1] + 1, 0) if a[3] else (a[1], a[2] + 1))
        assert all(r[2] < 7 for r in mine) and all(r[3] for r in mine if r[2] == 6)
    assert np.all(env.t == 0) and np.all(env.ordinal >= 2)      # every env was reset at the end


def test_collect_loop_does_not_depend_on_the_other_envs_or_on_n_episode():
    """env 0's first episode is the same rows whatever runs next to it"""
    def first_episode(env_num, n_episode):
        env = dm.ModelEnv(dm.LINEAR, env_num, 7, 9, (0.7, ), 8, 2, *_ab(8, 2), dtype=F32)
        env.reset()
        seen = []

        def policy(obs, ids):
            if 0 in ids and env.ordinal[0] == 1:
                seen.append(obs[list(ids).index(0)].copy())
            return np.tanh(obs[:, :2])
        dm.collect(env, n_episode, policy)
        return np.array(seen)
    a, b = first_episode(1, 1), first_episode(17, 30)
    assert a.shape == (7, 8) and np.array_equal(a, b)


def _ab(Do, Da):
    h = SyntheticSafetyVectorEnv(env_num=1, obs_dim=Do, act_dim=Da)
    return h.A, h.B


@pytest.mark.parametrize("name", ["point_circle", "linear_8_2", "linear_33_8"])
def test_injected_inputs_reach_every_branch_and_stay_under_the_band_cap(name):
    """what tests/test_gpu_devcollect.py injects: costs and terminations both occur, rows sit just inside AND just outside every
    threshold, and the share of rows within BAND of a threshold -- computed with the float32 restatement alone -- is inside the cap"""
    case = dm.env_alone_cases()[name]
    r32, r64 = dm.env_alone_expected(case, F32), dm.env_alone_expected(case, F64)
    share, near = dm.band_share(r32)
    print(name, "rows within the band:", share)
    assert share <= dm.BAND_CAP
    assert 0 < r32["cost"].sum() < case["env_num"]
    if case["kind"] == dm.POINT_CIRCLE:
        assert 0 < r32["terminated"].sum() < case["env_num"]
    assert r32["truncated"].any() and not r32["truncated"].all()
    for var, thr, scale in r32["margins"].values():
        rel = (var - thr) / thr
        assert ((rel > 0) & (rel < 2e-3)).any() and ((rel < 0) & (rel > -2e-3)).any(), name
    # outside the band both models decide alike
    assert np.array_equal(r32["cost"][~near], r64["cost"][~near]) and np.array_equal(r32["terminated"][~near], r64["terminated"][~near])
    d32 = np.max(np.abs(r32["obs_next"].astype(F64) - r64["obs_next"]) / r32["obs_scale"])
    assert d32 < 16 * np.finfo(F32).eps
