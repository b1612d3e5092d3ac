"""The on-policy loss head (kernels_mlp.hpp ppo_fwd_bwd_body, kernels_layered.hpp lay_head) at theta != theta_old, where every
branch of it is live: ratio inside / above / below 1 +- eps_clip with either sign of the advantage, the dual-clip region, and the
value clip's clamp mask and "which square wins" choice.  tests/test_gpu_ppo.py::test_minibatch_gradient_vs_autograd runs at
theta = theta_old (every ratio exactly 1, every v - v_old exactly 0).

Protocol (test_gpu_focops_shapes.py's): upload theta_old, ppo_begin (records log pi_old, v_old, returns, advantages), upload theta,
one ppo_pass at lr 0, ppo_end, get_grads(): the LAST minibatch's gradient at theta.  Reference: float64 autograd of
PPOLagOracle._minibatch_losses on that chunk with process() run at theta_old.  Compared: the whole gradient vector at the bar of the
existing gradient tests (rtol 1e-4, atol 2e-6 max(1, max |g|)) and the step's logged actor_rew / actor_safety / kl / vf0 / vf1 at
test_full_update_vs_golden's row bar (2e-5 rel + 2e-5 abs).  Either bar would widen to twice the fp32 oracle's own distance from
float64 where that is larger (elementwise); it is not, anywhere.

The problems and their branch censuses come from tests/branch_problems.py (asserted on the CPU by test_branch_problems_host.py and
again here).  Census of the compared minibatch (float64 oracle), the fp32 oracle's distance from float64 (as test_branch_problems_host.py prints it) and the device's from
float64, in units of the project's bars (gradient: worst element; row: worst entry):

    case                         rows  in+  in-  hi+  hi-  lo+  lo- dual | v_in raw clip (reward) | v_in raw clip (cost) | margin  | oracle: grad  row  | device: grad  row
    w64_dual_vclip                215   50   35   30   16   48   30    6 |  110   52   53        |  106   32   77      | 2.0e-3  |  0.015  0.006      |  0.010  0.005
    w128_da1_rawadv_vclip         389   99   77   31   17   82   83    - |  145  157   87        |  220  156   13      | 2.1e-3  |  0.006  0.005      |  0.004  0.002
    w256_da16_unbounded_dual      203   18   18   49    8   47   35   28 |    -    -    -        |    -    -    -      | 2.5e-3  |  0.100  0.015      |  0.153  0.009
    w128_tall_dual_vclip_nolag    717  168  157  104   31  109  103   45 |  267   91  359        |  244  323  150      | 2.3e-3  |  0.015  0.003      |  0.012  0.008  (both plans)
    w256_auto_tall_dual_vclip    1607  346  241  174   75  378  312   81 |  793  620  194        |  364  222 1021      | 2.0e-3  |  0.021  0.005     |  0.007  0.009
    layered_dual_vclip            253   49   50   46   15   25   47   21 |  211   26   16        |  110  135    8      | 2.1e-3  |  0.036  0.008      |  0.027  0.007

Bars above the project's: none (the fp32 oracle sits within 0.1 project bars of float64 in every case, the device within 0.16)."""
import numpy as np
import pytest

import branch_problems as bp

pytestmark = pytest.mark.gpu

_PROBLEMS = {}


def _problem(name):
    """built once per session and left unchanged (two tile plans share it)"""
    if name not in _PROBLEMS:
        _PROBLEMS[name] = bp.ppo_problem(name)
    return _PROBLEMS[name]


def _engine(p):
    from fsrl_amd.engine import Engine, EngineConfig
    c, cfg = p["case"], p["cfg"]
    rows = c["rows"]
    eng = Engine(EngineConfig(obs_dim=c["Do"], act_dim=c["Da"], hidden_sizes=tuple(c["hidden"]), n_critics=2, env_num=len(rows),
                              buffer_size=len(rows) * 2048, max_action=cfg.max_action, eps_clip=cfg.eps_clip, dual_clip=cfg.dual_clip,
                              vf_coef=cfg.vf_coef, max_grad_norm=cfg.max_grad_norm, target_kl=None,
                              norm_adv=cfg.advantage_normalization, use_lagrangian=cfg.use_lagrangian, lr=0.0,
                              unbounded=cfg.unbounded, rew_norm=cfg.reward_normalization, value_clip=cfg.value_clip))
    cols = p["cols"]
    for t in range(max(rows)):                            # lock-step, envs drop out as they run dry
        ids = [e for e in range(len(rows)) if t < rows[e]]
        eng.push(ids, *[np.stack([cols[k][e][t] for e in ids]) for k in ("obs", "act", "rew", "cost", "term", "trunc", "obs_next")])
    return eng


def _params():
    return [pytest.param(n, plan, id=f"{n}-plan{plan}") for n, c in bp.PPO_CASES.items() for plan in c.get("plans", (-1, ))]


@pytest.mark.parametrize("name,plan", _params())
def test_ppo_head_gradient_and_row_away_from_theta_old_vs_float64_autograd(name, plan):
    p = _problem(name)
    bp.check_census(p["census"], p["margin"], bp.ppo_claims(p["case"]), name)
    eng = _engine(p)
    if p["cfg"].reward_normalization:
        eng.ret_rms_set(bp.RET_RMS0)
    eng.ppo_set_plan(plan)
    eng.set_params(p["theta_old"])
    assert eng.ppo_begin(p["lag"], p["resc"], p["case"]["B"]) == len(p["data"])
    eng.set_params(p["theta"])
    eng.ppo_pass(p["perm"])
    stats = eng.ppo_end_stats(p["n_steps"])
    assert stats.shape[0] == p["n_steps"] and np.array_equal(eng.get_params(), p["theta"])
    got = eng.get_grads().astype(np.float64)
    row = stats[-1, list(bp.ROW_COLS)].astype(np.float64)
    eng.close()
    g64, g32, row64, row32 = p["g64"], p["g32"], p["row64"], p["row32"]
    gbar, rbar = bp.ppo_bars(p)
    print(f"{name} plan {plan}: gradient {(np.abs(got - g64) / gbar).max():.3f} x bar (fp32 oracle {(np.abs(g32 - g64) / gbar).max():.3f}), "
          f"row {(np.abs(row - row64) / rbar).max():.3f} x bar (fp32 oracle {(np.abs(row32 - row64) / rbar).max():.3f})")
    print(bp.census_line(name, p["census"], p["margin"]))
    # twice the fp32 oracle's own distance where that exceeds the project's bar (nowhere, see the module docstring)
    gtol, rtol = np.maximum(gbar, 2 * np.abs(g32 - g64)), np.maximum(rbar, 2 * np.abs(row32 - row64))
    bad = np.flatnonzero(np.abs(got - g64) > gtol)
    assert bad.size == 0, (name, f"{bad.size} of {got.size} gradient entries", int(bad[0]), got[bad[0]], g64[bad[0]])
    for k, a, b, t in zip(bp.ROW_KEYS, row, row64, rtol):
        assert abs(a - b) <= t, (name, k, a, b)
