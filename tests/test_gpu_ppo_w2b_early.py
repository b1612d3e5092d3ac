"""The single-agent PPO step with the early part of the backward W2 fragment issued from inside the forward pass
(ppo_fwd_bwd_kernel<H, 4 | 8, true>, kernels_mlp.hpp: W2bEarly) against the one-burst instantiation of the same kernel
(a context created under FSRL_NO_W2B_EARLY launches it).  The change moves loads, not arithmetic: the same addresses, the same
values, the same dz1 MFMA sequence -- so the logged statistics and the parameters after two passes are compared bit for bit.
The comparison means something only if the library under test reads FSRL_NO_W2B_EARLY in fsrl_ctx_create (the shipped build does,
outside its probe-only block) and has both instantiations to launch (tests/test_code_object_w2b_early.py); a library that ignored
the variable would compare the early-issue kernel with itself.

Shapes, the smallest at which each branch can go wrong (about 600 rows, two passes):
  * hidden 256 and 128: 16 and 8 waves, 16 and 8 rows of the backward fragment;
  * obs_dim 8 (W1 in LDS, layer 1 on FMA) and 40 (W1 from L2: layer 1 issues vector-memory loads of its own in front of the
    early rows);
  * batch 64: whole 4-row tiles only; batch 50: a tile with 2 valid rows and tiles with none inside the last 16-row group;
  * one batch that takes the 8-row tiles on the device at hand, from its CU count by ppo_tile_plan's rule
    (networks x tiles x 4 > CUs >= networks x tiles x 2; 352 rows on 256 CUs);
  * max_grad_norm 0.5 (three launches per step) and None (the weight-gradient launch applies Adam: two launches), both behind
    the same fused kernel."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_NETS = 3           # actor + two critics (EngineConfig's default n_critics)
ENVS, T = 4, 150     # 600 rows (the 8-row case: two whole minibatches, 704 rows on 256 CUs)


def _engine(no_early, **kw):
    """A PPO-Lagrangian context; no_early: created under FSRL_NO_W2B_EARLY (fsrl_ctx_create reads it once)."""
    from fsrl_amd.engine import Engine, EngineConfig
    old = os.environ.get("FSRL_NO_W2B_EARLY")
    if no_early:
        os.environ["FSRL_NO_W2B_EARLY"] = "1"
    else:
        os.environ.pop("FSRL_NO_W2B_EARLY", None)
    try:
        return Engine(EngineConfig(env_num=ENVS, target_kl=None, **kw), device=0)
    finally:
        if old is None:
            os.environ.pop("FSRL_NO_W2B_EARLY", None)
        else:
            os.environ["FSRL_NO_W2B_EARLY"] = old


def _batch8():
    """a minibatch size whose fused launch runs 8-row tiles on this device (ppo_tile_plan, host_ppo.inc)"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = cus // (4 * N_NETS) + 1                  # the first count of 16-row tiles that 4-row tiles no longer fit
    assert N_NETS * tiles * 4 > cus >= N_NETS * tiles * 2, (cus, tiles)
    return 16 * tiles


def _run(H, Do, batch, mgn, T=T):
    Da = 2
    rng = np.random.default_rng(7)
    obs = rng.standard_normal((T + 1, ENVS, Do)).astype(np.float32)
    act = (0.3 * rng.standard_normal((T, ENVS, Da))).astype(np.float32)
    rew = rng.normal(0.5, 0.5, (T, ENVS))
    cost = (rng.random((T, ENVS)) < 0.1).astype(np.float64)
    trunc = np.zeros((T, ENVS), bool); trunc[74::75] = True
    term = np.zeros((T, ENVS), bool)
    perms = [rng.permutation(T * ENVS) for _ in range(2)]
    theta = None
    out = []
    for no_early in (False, True):
        eng = _engine(no_early, obs_dim=Do, act_dim=Da, hidden=H, max_grad_norm=mgn)
        if theta is None:
            theta = (0.1 * np.random.default_rng(3).standard_normal(eng.n_params)).astype(np.float32)
        eng.set_params(theta)
        ids = np.arange(ENVS)
        for t in range(T):
            eng.push(ids, obs[t], act[t], rew[t], cost[t], term[t], trunc[t], obs[t + 1])
        stats, _ = eng.ppo_update(np.array([0.5]), 1.0 / 1.5, batch, 2, perms=perms)
        out.append((stats.copy(), eng.get_params().copy()))
        eng.close()
    return out


def _check(out, steps):
    (s_new, p_new), (s_old, p_old) = out
    assert s_new.shape == s_old.shape == (steps, 11), (s_new.shape, s_old.shape, steps)
    assert np.isfinite(s_new).all() and np.isfinite(p_new).all()
    assert np.array_equal(s_new, s_old), (float(np.abs(s_new - s_old).max()), int((s_new != s_old).sum()))
    assert np.array_equal(p_new, p_old), (float(np.abs(p_new - p_old).max()), int((p_new != p_old).sum()))
    assert not np.array_equal(p_new, np.zeros_like(p_new))


@pytest.mark.parametrize("mgn", [0.5, None])
@pytest.mark.parametrize("batch", [64, 50])
@pytest.mark.parametrize("Do", [8, 40])
@pytest.mark.parametrize("H", [256, 128])
def test_four_row_tiles_bit_identical_to_the_one_burst_kernel(H, Do, batch, mgn):
    _check(_run(H, Do, batch, mgn), 2 * (ENVS * T // batch))      # a short last minibatch is merged into the one before it


@pytest.mark.parametrize("mgn", [0.5, None])
@pytest.mark.parametrize("Do", [8, 40])
@pytest.mark.parametrize("H", [256, 128])
def test_eight_row_tiles_bit_identical_to_the_one_burst_kernel(H, Do, mgn):
    batch = _batch8()
    _check(_run(H, Do, batch, mgn, T=2 * batch // ENVS), 4)       # two whole minibatches per pass: every step runs 8-row tiles
