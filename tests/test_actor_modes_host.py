"""The actor-mean option of the stochastic replay agents (fsrl_sac_config.actor_mean / fsrl_cvpo_config.actor_mean), host side:
the fixtures of tests/golden/gen_golden_actor_modes.py load, carry the sensitivity figure their generator asserted, and the torch
mirror of ActorProb reproduces the means the reference recorded in the fixture's mode."""
import json

import numpy as np
import pytest
import torch

from helpers import load_npz

SAC_FIXTURES = ["sac_bounded_small", "sac_bounded_c4", "sac_bounded_deep3"]
CVPO_FIXTURES = ["cvpo_unbounded_small", "cvpo_unbounded_double", "cvpo_unbounded_deep3"]
SHAPES = {"sac_bounded_small": (6, 3, [64, 64], 64, 1.0), "sac_bounded_c4": (33, 8, [128, 128], 100, 2.0),
          "sac_bounded_deep3": (6, 3, [48, 64, 40], 64, 2.0), "cvpo_unbounded_small": (6, 3, [64, 64], 64, 1.0),
          "cvpo_unbounded_double": (8, 2, [64, 64], 100, 2.0), "cvpo_unbounded_deep3": (6, 3, [48, 64, 40], 64, 1.0)}


def _case(name):
    g = load_npz(name + ".npz")
    return g, json.loads(str(g["cfg_json"]))


@pytest.mark.parametrize("name", SAC_FIXTURES + CVPO_FIXTURES)
def test_fixture_loads_in_the_new_mode_at_the_stated_shape(name):
    g, cfg = _case(name)
    sac = name.startswith("sac_")
    assert cfg["unbounded"] is (not sac)                 # the mode the other generators do not record
    assert (cfg["obs_dim"], cfg["act_dim"], cfg["hidden"], cfg["batch_size"], cfg["max_action"]) == SHAPES[name]
    n = cfg["n_updates"] if sac else cfg["cycles"] * cfg["updates_per_cycle"]
    assert g["indices"].shape == (n, cfg["batch_size"]) and g["eps_target"].shape == (n, cfg["batch_size"], cfg["act_dim"])
    if sac:
        assert g["eps_pi"].shape == g["eps_target"].shape and g["stats_actor"].shape[0] == n
    else:
        assert g["eps_particles"].shape == (n, cfg["sample_act_num"], cfg["batch_size"], cfg["act_dim"]) and g["stats"].shape[0] == n
    if name == "sac_bounded_small":
        assert cfg["auto_alpha"] and n == 6
    if name == "cvpo_unbounded_double":
        assert cfg["double_critic"] and cfg["estep_iter_num"] == 2 and cfg["mstep_iter_num"] == 2 and cfg["sample_act_num"] == 8 \
            and cfg["n_step"] == 3
    if name == "cvpo_unbounded_small":
        assert not cfg["double_critic"] and cfg["cycles"] == 2


@pytest.mark.parametrize("name", SAC_FIXTURES + CVPO_FIXTURES)
def test_fixture_records_that_the_other_mode_would_miss_the_bar(name):
    """the reference, run in the other mode from the same parameters, store, indices and noise, moves a compared logged quantity of
    the first two updates by at least 10 x what the GPU test allows, and ends at other actor parameters"""
    g, cfg = _case(name)
    s = cfg["sensitivity"]
    sac = name.startswith("sac_")
    assert s["key"] in (("loss/actor_total", ) if sac else ("mstep/mstep_loss_mle", "mstep/mstep_kl_mu")) and s["update"] in (0, 1)
    keys = [str(k) for k in (g["stats_actor_keys"] if sac else g["stats_keys"])]
    x = float((g["stats_actor"] if sac else g["stats"])[s["update"], keys.index(s["key"])])
    bar = (5e-5 * abs(x) + 5e-6) if sac else (1e-4 * abs(x) + 1e-5)          # the bars of test_gpu_actor_modes.py, recomputed
    print(f"{name}: {s['key']} of update {s['update']} = {x:.6g}, the other mode is {s['distance']:.3e} away = {s['distance'] / bar:.0f} x "
          f"the bar; final actor parameters {s['theta_actor_final_maxdiff']:.3e} apart")
    assert abs(bar - s["bar"]) <= 1e-12 and s["distance"] >= 10.0 * bar and abs(s["ratio"] - s["distance"] / bar) <= 1e-6 * s["ratio"]
    assert s["theta_actor_final_maxdiff"] > 0.0


@pytest.mark.parametrize("name", SAC_FIXTURES + CVPO_FIXTURES)
def test_torch_mirror_reproduces_the_recorded_means(name):
    from fsrl_amd.policy import SACLagrangian
    from fsrl_amd.utils.net import ActorProb, Net
    g, cfg = _case(name)
    Do, Da, h = cfg["obs_dim"], cfg["act_dim"], tuple(cfg["hidden"])
    means = {}
    for unbounded in (cfg["unbounded"], not cfg["unbounded"]):
        actor = ActorProb(Net((Do, ), hidden_sizes=h), (Da, ), max_action=cfg["max_action"], conditioned_sigma=True, unbounded=unbounded)
        SACLagrangian._unflat([actor], g["theta_actor0"])
        with torch.no_grad():
            (mu, sigma), _ = actor(g["mean_obs"])
        means[unbounded] = mu.numpy()
        if unbounded is cfg["unbounded"]:
            assert g["mean_mu"].shape == (8, Da)
            np.testing.assert_allclose(mu.numpy(), g["mean_mu"], rtol=0, atol=1e-6)
            np.testing.assert_allclose(sigma.numpy(), g["mean_sigma"], rtol=1e-6, atol=0)
    assert np.abs(means[True] - means[False]).max() > 1e-3        # the recorded rows tell the two modes apart
    assert np.abs(means[False]).max() <= cfg["max_action"]


def test_config_structs_end_in_the_new_field():
    import ctypes as C
    from fsrl_amd import _lib
    for cls in (_lib.SacConfig, _lib.CvpoConfig):
        name, typ = cls._fields_[-1]
        assert name == "actor_mean" and typ is C.c_int32
        assert cls().actor_mean == 0                     # a zero-initialised struct: the kind's present behaviour
    assert (_lib.ACTOR_MEAN_DEFAULT, _lib.ACTOR_MEAN_UNBOUNDED, _lib.ACTOR_MEAN_TANH) == (0, 1, 2)
    assert [_lib.actor_mean_code(u) for u in (None, True, False)] == [0, 1, 2]
