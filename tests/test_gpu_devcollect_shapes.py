"""Whole collects on the GPU (fsrl_collect_device) at the widths, shape edges and head modes that the 64-wide tests of
tests/test_gpu_devcollect.py and tests/test_gpu_devcollect_replay.py do not reach, row by row against the float64 model
(tests/devenv_model.py, tests/devenv_replay_model.py) by the shared body of tests/devcollect_rows.py.

The cases are devenv_replay_model.ALL_CASES; tests/test_devcollect_shapes_model.py asserts their preconditions without a GPU (rows
out of the discontinuity band; inputs that tell a wrong head formula from the true one by 100 bounds):
  * hidden 128 and 256 for every head (on-policy, SAC-Lag, CVPO, DDPG-Lag), one padded fused width (100, 72) -> 128;
  * the edges of the collect's own staging loop: obs 16 | 17 (the LDS-FMA | MFMA first layer), obs 64 with 64 envs at 256 wide (four
    full tiles, 16 * Do == the workgroup's 1024 threads), act 1 (the magic == 0 branch of the division by Da), the 16-column DDPG-Lag
    and Gaussian head rows at 256 wide;
  * the head options: max_action 1.5, both `unbounded` modes of the on-policy head, of SAC-Lag and of CVPO, exploration_sigma.
Episodes are cut at 7 steps; at most 64 envs and 70 episodes.  No new tolerance: continuous outputs by the float64-yardstick rule of
DESIGN.md 6, discontinuous ones equal outside the band, deterministic collects against the existing path bit for bit.  Every case
prints its distances; the figures measured on an MI355X are in DESIGN.md 3.4.1."""
import numpy as np
import pytest

import devenv_replay_model as rm
import test_gpu_devcollect as on
import test_gpu_devcollect_replay as rp
from devcollect_rows import action_draws, check_action, check_collect_rows

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64


def build(case, seed=rm.ENV_SEED, rows_per_env=200, per=None):
    """-> (engine, device env) of a case of devenv_replay_model: the helpers' make() with the case's width and head options"""
    agent, kind, n, n_ep, H, opts = case
    cfg = {k: opts[k] for k in ("max_action", "hidden_sizes") if k in opts}
    if agent == "onpolicy":
        eng, env = on.make(kind, n, H=H, rows_per_env=rows_per_env, seed=seed, oracle_params=True, unbounded=bool(opts.get("unbounded", False)), **cfg)
        assert eng.n_params == rm.cpu_onpolicy_actor(kind, rm.case_hidden(case))[1]
    else:
        eng, env = rp.make(agent, kind, n, H=H, rows_per_env=rows_per_env, seed=seed, per=per, unbounded=opts.get("unbounded"),
                           exploration_sigma=opts.get("exploration_sigma", rm.EXPLORATION_SIGMA), **cfg)
        assert eng.n_sac_actor == rm.cpu_actor(agent, kind, rm.case_hidden(case))[1]
        if agent != "ddpgl":
            assert eng.actor_unbounded is (opts["unbounded"] if opts.get("unbounded") is not None else agent == "sacl")
    return eng, env


# ------------------------------------------------------------------------------------------------ 1. row by row
@pytest.mark.parametrize("deterministic", [False, True], ids=["training", "deterministic"])
@pytest.mark.parametrize("case", rm.ALL_CASES, ids=rm.case_id)
def test_collect_row_by_row_against_the_model(case, deterministic):
    """(mu, sigma) of a stored row are what the batch forward gives for its observation (Engine.actor_forward /
    Engine.sac_actor_forward, held to the oracles and a host mirror at these widths and modes by tests/test_gpu_actor_modes.py and
    the update tests); the noise, the action formula and the transition are the model's.  The on-policy head in training mode is
    measured in units of the noise, as tests/test_gpu_devcollect.py measures it; everything else in units of the action.

    One case was moved.  DDPG-Lag with max_action 1.5 on obs 20 / act 16 passed in training mode and in deterministic mode sat at
    2.4e-7, two one-ulp floors, on a mean in [0.75, 1): a deterministic action is the mean, which this test takes from the host as
    exact (restatement distance 0), while 1.5 tanh(head) is a float32 evaluation on both sides -- the float32 restatement of the mean
    alone is 1.2 floors from float64 where |tanh| >= 0.5 (tests/test_devcollect_shapes_model.py shows it on the CPU).  A property of
    the inputs, not of the collect: max_action 1.5 runs on obs 8 / act 2 (CVPO and DDPG-Lag sit at 1.19e-7 there, the floor exactly),
    the 16-column rows at max_action 1."""
    agent, kind, n, n_ep, H, opts = case
    eng, env = build(case)
    env.reset()
    _, t0, ord0 = env.get_state()
    assert np.all(t0 == 0) and np.all(ord0 == 1)
    res = eng.collect_device(env._h, n_ep, deterministic=deterministic, bound_method=1)
    what = f"{rm.case_id(case)} {'deterministic' if deterministic else 'training'}"

    def action(rows, e, ordinal, t, key):
        if agent != "onpolicy":
            return rp.replay_action_check(eng, agent, deterministic, what, rows, e, ordinal, t, key)
        mu, sigma = eng.actor_forward(rows["obs"])
        eps64, eps32, nscale = action_draws(rows, e, ordinal, t, key, eng.cfg.act_dim)
        return check_action("onpolicy", rows["act"], mu, sigma, eps64, eps32, deterministic, nscale, what + (" act" if deterministic else " action noise"))
    rows, dist = check_collect_rows(eng, env, ord0, res, n_ep, kind, rm.ENV_SEED, what, action)
    print(f"{what}: {len(rows['rew'])} rows, cost rows {rows['cost'].sum():.0f}, largest |act| {np.abs(rows['act']).max():.3f}")
    assert rows["cost"].sum() > 0
    if opts.get("max_action", 1.0) > 1.0 and agent != "sacl" and not deterministic:
        # bound_method 1 on stored actions beyond +-1: the clip branch of the device's map_action ran on collect-produced rows, and
        # obs_next / rew above were held to the model's clipped action
        assert np.abs(rows["act"]).max() > 1.0
    env.close(); eng.close()


# ------------------------------------------------------------------------------------------------ 2. deterministic collects
@pytest.mark.parametrize("kind,n,episodes,bound,low_high,H,cfg", [
    ("lin8", 17, (20, 9), "clip", (-2.0, 0.5), 128, {}),
    ("lin8", 17, (20, 9), "clip", (-2.0, 0.5), 256, {}),
    ("lin64", 64, (70, 64), "", None, 256, {}),                              # four full tiles of obs 64: 16 * Do == 1024 threads
    ("lin17", 16, (16, 30), "clip", None, 128, {}),
    ("lin2", 5, (3, 12), "clip", None, 64, {}),                              # act 1
    ("lin8", 17, (20, 9), "clip", None, 64, {"max_action": 1.5}),
    ("lin8", 17, (20, 9), "", (-0.5, 1.5), 64, {"max_action": 1.5, "unbounded": True}),
    ("pc", 5, (3, 12), "clip", None, 256, {"unbounded": True}),
], ids=lambda v: str(v).replace(" ", "") if isinstance(v, dict) else None)
def test_deterministic_collect_is_the_existing_path_bit_for_bit(kind, n, episodes, bound, low_high, H, cfg):
    """the assertions of tests/test_gpu_devcollect.py's test of this name, at 128 and 256 wide and with the head options set"""
    on.deterministic_collect_twins(kind, n, episodes, bound, low_high, H=H, **cfg)
