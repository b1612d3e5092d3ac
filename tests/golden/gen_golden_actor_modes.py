#!/usr/bin/env python
"""Golden vectors G12: SACLagrangian.update and CVPO.update from the UNMODIFIED reference with the Gaussian actor's mean in the
mode the other generators do not record -- SAC-Lag with ActorProb(unbounded=False) (mu = max_action * tanh(head), what every
sacl_cfg.py config trains with) and CVPO with ActorProb(unbounded=True) (mu = head, cvpo_cfg.py MujocoBaseCfg).  Build container only.

    python tests/golden/gen_golden_actor_modes.py

The runs are gen_golden_sac.gen / gen_golden_cvpo.gen themselves (same stores, parameter initialisation, recorded indices and
noise, same file formats: see their docstrings); only the ActorProb they construct is given another `unbounded` / `max_action`.

    fixture                      agent    obs/act  hidden         batch  mode and extras
    sac_bounded_small.npz        SAC-Lag   6 / 3   (64, 64)         64   unbounded=False, max_action 1.0, auto_alpha, 6 updates
    sac_bounded_c4.npz           SAC-Lag  33 / 8   (128, 128)      100   unbounded=False, max_action 2.0: ragged last tile, full-width head;
                                                                         the final critics / target critics as every 8th entry (theta_final_stride)
    sac_bounded_deep3.npz        SAC-Lag   6 / 3   (48, 64, 40)     64   unbounded=False, max_action 2.0: a layered context
    cvpo_unbounded_small.npz     CVPO      6 / 3   (64, 64)         64   unbounded=True, SingleCritic, 2 cycles
    cvpo_unbounded_double.npz    CVPO      8 / 2   (64, 64)        100   unbounded=True, double_critic, 2 E-step / 2 M-step iterations, K = 8, n_step 3
    cvpo_unbounded_deep3.npz     CVPO      6 / 3   (48, 64, 40)     64   unbounded=True: a layered context
(the CVPO runs use the tight mstep_kl_* / actor_lr of cvpo_deep3, which keep the M-step multipliers off zero)

On top of the generators' own entries every fixture carries
    cfg_json             + "unbounded", the actor's "max_action", and "sensitivity": {"key", "update", "distance", "bar", "ratio",
                           "theta_actor_final_maxdiff"} (below)
    mean_obs, mean_mu, mean_sigma    the first rows of st_obs and the reference actor's (mu, sigma) on them at theta_actor0
Sensitivity: the reference is run a second time in the OTHER mode from the same initial parameters, store, indices and noise
(asserted equal).  Over the first two updates the logged quantity named by "key" (SAC: loss/actor_total; CVPO: mstep/mstep_loss_mle
or mstep/mstep_kl_mu) differs between the two runs by "distance" >= 10 x "bar", where bar is what the GPU test allows for that value
(SAC: 5e-5 |x| + 5e-6; CVPO: 1e-4 |x| + 1e-5), and the final actor parameters differ: a device that ignored the option would fail
the golden test.  Asserted here before a file is written, and printed.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden_cvpo  # noqa: E402  (installs ref_shim)
import gen_golden_sac  # noqa: E402
import ref_shim  # noqa: E402

N_MEANS = 8


def run(mod, mode_unbounded, mode_max, name, *args, **kw):
    """mod.gen(name, ...) with its ActorProb built in the given mode; -> the dict it would have written (nothing is written)"""
    box = {}

    def actor_prob(net, shape, max_action=None, conditioned_sigma=False, unbounded=None, _m=mode_max, _u=mode_unbounded):
        return ref_shim.ActorProb(net, shape, max_action=_m, conditioned_sigma=conditioned_sigma, unbounded=_u)

    def capture(path, **out):
        box["path"], box["out"] = path, out

    keep_actor, keep_save = mod.ActorProb, np.savez_compressed
    mod.ActorProb, np.savez_compressed = actor_prob, capture
    try:
        mod.gen(name, *args, **kw)
    finally:
        mod.ActorProb, np.savez_compressed = keep_actor, keep_save
    return box["path"], box["out"]


def actor_means(cfg, theta, obs, unbounded, max_action):
    actor = ref_shim.ActorProb(ref_shim.Net((cfg["obs_dim"], ), hidden_sizes=tuple(cfg["hidden"])), (cfg["act_dim"], ),
                               max_action=max_action, conditioned_sigma=True, unbounded=unbounded)
    flat, off = torch.from_numpy(theta), 0
    with torch.no_grad():
        for p in actor.parameters():
            p.copy_(flat[off:off + p.numel()].view_as(p)); off += p.numel()
        assert off == flat.numel()
        (mu, sigma), _ = actor(torch.as_tensor(obs))
    return mu.numpy().copy(), sigma.numpy().copy()


def logged(out, key):
    if "stats_keys" in out:                                       # CVPO: one merged row per update
        return out["stats"][:, [str(k) for k in out["stats_keys"]].index(key)]
    return out["stats_actor"][:, [str(k) for k in out["stats_actor_keys"]].index(key)]


def fixture(mod, kind, unbounded, max_action, name, *args, critics_stride=1, **kw):
    """critics_stride (SAC): theta_critics_final / theta_critics_old_final keep every critics_stride-th entry and the fixture carries
    `theta_final_stride`, as gen_golden_cvpo's wide cases do: what keeps four 128-wide Q-networks under the size limit"""
    if kind == "cvpo":
        kw = dict(kw, max_action=max_action)                      # gen_golden_cvpo also scales the action space and the stored actions
    path, out = run(mod, unbounded, max_action, name, *args, **kw)
    _, other = run(mod, not unbounded, max_action, name, *args, **kw)
    same = ["theta_actor0", "theta_critics0", "indices", "eps_target", "st_obs", "st_act"] + \
           (["eps_pi"] if kind == "sac" else ["eps_particles"])
    for k in same:
        assert np.array_equal(out[k], other[k]), k
    rel, ab = (5e-5, 5e-6) if kind == "sac" else (1e-4, 1e-5)
    best = None
    for key in (("loss/actor_total", ) if kind == "sac" else ("mstep/mstep_loss_mle", "mstep/mstep_kl_mu")):
        a, b = logged(out, key), logged(other, key)
        for u in range(2):
            bar = rel * abs(a[u]) + ab
            cand = dict(key=key, update=u, distance=float(abs(a[u] - b[u])), bar=float(bar), ratio=float(abs(a[u] - b[u]) / bar))
            if best is None or cand["ratio"] > best["ratio"]:
                best = cand
    best["theta_actor_final_maxdiff"] = float(np.abs(out["theta_actor_final"] - other["theta_actor_final"]).max())
    assert best["ratio"] >= 10.0 and best["theta_actor_final_maxdiff"] > 0.0, (name, best)
    cfg = json.loads(str(out["cfg_json"]))
    cfg.update(unbounded=bool(unbounded), max_action=float(max_action), sensitivity=best)
    out["cfg_json"] = np.array(json.dumps(cfg))
    if critics_stride != 1:
        for k in ("theta_critics_final", "theta_critics_old_final"):
            out[k] = out[k][::critics_stride].copy()
        out["theta_final_stride"] = np.array(critics_stride)
    out["mean_obs"] = out["st_obs"][:N_MEANS].copy()
    out["mean_mu"], out["mean_sigma"] = actor_means(cfg, out["theta_actor0"], out["mean_obs"], unbounded, max_action)
    np.savez_compressed(path, **out)
    print(f"G12 {os.path.basename(path)}: {best['key']} of update {best['update']} moves by {best['distance']:.3e} between the modes = "
          f"{best['ratio']:.0f} x the bar {best['bar']:.2e}; final actor parameters by up to {best['theta_actor_final_maxdiff']:.3e}")


if __name__ == "__main__":
    torch.set_num_threads(4)
    eps = [[60, 50, -17], [70, 55], [40, 40, 40, -9]]
    sac, cvpo = gen_golden_sac, gen_golden_cvpo
    fixture(sac, "sac", False, 1.0, "bounded_small", 6, 3, (64, 64), 3, eps, batch_size=64, n_updates=6, seed=130, n_step=2)
    fixture(sac, "sac", False, 2.0, "bounded_c4", 33, 8, (128, 128), 4, [[120, 80], [100, -60], [90, 70], [150]], batch_size=100,
            n_updates=4, seed=132, n_step=2, critics_stride=8)
    fixture(sac, "sac", False, 2.0, "bounded_deep3", 6, 3, (48, 64, 40), 3, eps, batch_size=64, n_updates=5, seed=136, n_step=2)
    tight = dict(cost_limit=0.3, mstep_kl_mu=2e-4, mstep_kl_std=2e-6, actor_lr=2e-3)
    fixture(cvpo, "cvpo", True, 1.0, "unbounded_small", 6, 3, (64, 64), 3, eps, batch_size=64, cycles=2, updates_per_cycle=4, seed=150,
            **tight)
    fixture(cvpo, "cvpo", True, 2.0, "unbounded_double", 8, 2, (64, 64), 3, eps, batch_size=100, cycles=2, updates_per_cycle=3, seed=152,
            n_step=3, double_critic=True, mstep_iter_num=2, estep_iter_num=2, sample_act_num=8, **tight)
    fixture(cvpo, "cvpo", True, 1.0, "unbounded_deep3", 6, 3, (48, 64, 40), 3, eps, batch_size=64, cycles=2, updates_per_cycle=4, seed=157,
            **tight)
