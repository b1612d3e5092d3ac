"""The replay agents' action formulas of tests/devenv_replay_model.py, float32 against float64, on injected (m, sigma, eps): the
yardstick tests/test_gpu_devcollect_replay.py measures the device with.  No GPU.

The bars come from the arithmetic, with EPS = 2^-23 (unit roundoff EPS / 2) and scale = max(1, |m| + |sigma eps|):
  m + sigma eps     the product's rounding is at most EPS / 2 |sigma eps|, the sum's EPS / 2 |m + sigma eps|: EPS x scale together
  tanh of it        tanh contracts (|tanh'| <= 1), so the argument's error passes at most unchanged; numpy's float32 tanh itself is
                    taken as good to 4 ulp of a value below 1, i.e. 2 EPS: 3 EPS x scale together
  exp(clamp(l))     the clamp is exact; numpy's float32 exp taken as good to 4 ulp: relative 4 EPS
  max_action tanh   4 ulp of tanh and one rounding of the product: relative 3 EPS at |tanh| >= 1/2, absolute 3 EPS max_action below
Saturation (|m + sigma eps| up to 40) is where a scale that forgot the terms' magnitudes would be too small by a factor of 40."""
import numpy as np
import pytest

import devenv_replay_model as rm

F32, F64 = np.float32, np.float64
EPS = float(np.finfo(F32).eps)
SLACK = 1.0 + 1e-6                  # the second-order terms of the bounds above


def inputs():
    rng = np.random.default_rng(20261021)
    n = 4096
    m = rng.uniform(-3, 3, (n, 8)).astype(F32)
    log_sigma = rng.uniform(-25, 4, (n, 8)).astype(F32)           # both clamps are crossed
    eps = rng.standard_normal((n, 8)).astype(F32)
    eps[::7] *= F32(5.0)                                          # the tails of a normal: |eps| up to ~ 20
    m[::5] = rng.uniform(-40, 40, m[::5].shape).astype(F32)       # saturated tanh: |m + sigma eps| up to 40 and beyond
    m[0, :4], log_sigma[0, :4], eps[0, :4] = (40.0, -40.0, 33.0, 0.0), 2.0, (0.0, 0.0, 0.9473, 5.4)    # |u| = 40 exactly, from either term
    return m, log_sigma, eps


def test_log_sigma_clamps_and_exp():
    _, log_sigma, _ = inputs()
    s32, s64 = rm.head_sigma(log_sigma, F32), rm.head_sigma(log_sigma, F64)
    assert s32.dtype == F32 and s64.dtype == F64
    lo, hi = log_sigma <= -20, log_sigma >= 2
    assert lo.sum() > 100 and hi.sum() > 100 and (~lo & ~hi).sum() > 100
    assert np.all(s64[lo] == np.exp(-20.0)) and np.all(s64[hi] == np.exp(2.0))
    assert np.all(s32[lo] == np.exp(F32(-20.0))) and np.all(s32[hi] == np.exp(F32(2.0)))
    rel = np.abs(s32.astype(F64) - s64) / s64
    print(f"sigma: float32 restatement {rel.max():.3e} relative from float64")
    assert rel.max() <= 4 * EPS


@pytest.mark.parametrize("max_action", [1.0, 2.5])
def test_head_mean(max_action):
    raw = np.random.default_rng(3).uniform(-6, 6, 5000).astype(F32)
    assert np.array_equal(rm.head_mean(raw, max_action, False, F32), raw) and rm.head_mean(raw, max_action, False, F64).dtype == F64
    m32, m64 = rm.head_mean(raw, max_action, True, F32), rm.head_mean(raw, max_action, True, F64)
    d = np.abs(m32.astype(F64) - m64) / (max_action * np.maximum(np.abs(np.tanh(raw.astype(F64))), 0.5))
    print(f"mean: float32 restatement {d.max():.3e} from float64")
    assert m32.dtype == F32 and d.max() <= 3 * EPS * SLACK and np.abs(m64).max() <= max_action


@pytest.mark.parametrize("agent", rm.AGENTS)
@pytest.mark.parametrize("deterministic", [False, True])
def test_action_float32_against_float64(agent, deterministic):
    m, log_sigma, eps = inputs()
    sigma = rm.head_sigma(log_sigma, F32) if agent != "ddpgl" else np.full_like(m, 0.1)
    a32, a64 = rm.action(agent, m, sigma, eps, deterministic, F32), rm.action(agent, m, sigma, eps, deterministic, F64)
    assert a32.dtype == F32 and a64.dtype == F64
    scale = rm.action_scale(m, sigma, eps, deterministic)
    u = np.abs(m.astype(F64) + (0 if deterministic else sigma.astype(F64) * eps.astype(F64)))
    assert u.max() >= 40 and np.all(scale >= np.maximum(1.0, u) * (1 - 1e-12))        # the scale covers the value it scales
    d = np.abs(a32.astype(F64) - a64) / scale
    print(f"{agent} deterministic={deterministic}: float32 restatement {d.max():.3e} from float64 in units of the scale")
    if agent == "sacl":
        assert np.abs(a64).max() <= 1.0 and np.all(np.abs(a32[u >= 40]) == 1.0)        # saturated: exactly +-1 in float32
        assert d.max() <= 3 * EPS * SLACK
    elif deterministic:
        assert np.array_equal(a32.astype(F64), a64)                                    # the mean itself: no arithmetic
    else:
        assert d.max() <= EPS * SLACK
    # deterministic ignores sigma and eps
    if deterministic:
        assert np.array_equal(a32, rm.action(agent, m, 0 * sigma, 0 * eps, False, F32))


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("agent,kind,n,n_ep", rm.CASES)
def test_closed_loop_rows_stay_out_of_the_discontinuity_band(agent, kind, n, n_ep, deterministic):
    """The cases, seeds and actor parameters of tests/test_gpu_devcollect_replay.py's row-by-row test, run here as a closed loop of the
    float32 model with the oracles' CPU actors: the share of rows whose cost / terminated decision lies within the band must stay
    under dm.BAND_CAP -- the condition under which the GPU test may compare discontinuous outputs at all."""
    import devenv_model as dm
    Do, Da = rm.SHAPES[kind]
    if kind == "pc":
        env = dm.ModelEnv(dm.POINT_CIRCLE, n, 7, rm.ENV_SEED, (rm.PC["radius"], rm.PC["x_lim"], rm.PC["dt"]), Do, Da, dtype=F32)
    else:
        host = rm.linear_host(kind, n)
        env = dm.ModelEnv(dm.LINEAR, n, 7, rm.ENV_SEED, (0.7, ), Do, Da, host.A, host.B, dtype=F32)
    actor, _ = rm.cpu_actor(agent, kind)
    steps = []
    step = env.step
    env.step = lambda act, ids=None: steps.append(step(act, ids)) or steps[-1]

    def policy(obs, ids):
        m, sigma = actor(obs)
        return dm.map_action(rm.action(agent, m, sigma, env.action_noise(ids, F32), deterministic, F32), 1)
    env.reset()
    rows, episodes, n_steps = dm.collect(env, n_ep, policy)
    assert episodes >= n_ep and len(steps) == n_steps and sum(len(s["rew"]) for s in steps) == len(rows)
    near = np.concatenate([dm.band_share(s)[1] for s in steps])
    print(f"{agent} {kind} n={n} deterministic={deterministic}: {len(rows)} rows, within the band {near.mean():.4f}")
    assert near.mean() <= dm.BAND_CAP
    if kind == "pc":
        assert sum(s["cost"].sum() for s in steps) > 0 and sum(s["terminated"].sum() for s in steps) > 0
