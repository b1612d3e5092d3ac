"""The clamp and saturation branches of the replay agents' loss heads against the CPU oracles: SAC-Lag's actor head
(kernels_sac.hpp, layered: kernels_layered_sac.hpp) -- `pass`, the gradient mask of clamp(log sigma, -20, 2), and the 1 - a^2 + eps
correction where tanh saturates; DDPG-Lag's 1 - th^2; CVPO's M-step head (kernels_cvpo.hpp, layered: kernels_layered_sac.hpp) --
the same log-sigma mask and the var > 1e-6 mask of gaussian_kl's clamp_min.  Every other replay test draws fan-in scaled
parameters that keep the heads off these branches.

Caller-RNG mode (indices and noise injected).  tests/branch_problems.py builds an actor whose chosen action columns sit in chosen
regimes ("upper": the sampled rows straddle log sigma = 2; "lower": every row below -20; "sat+-": |u| >= 12; "smallvar": sigma^2 <
1e-6 inside the clamp), proves it with the float64 oracle (test_branch_problems_host.py on the CPU, and again here), and runs the
fp32 oracle and its float64 twin.

* Exact-zero regimes (`*_zero`, `*_sat`, CVPO): ONE update, compared with the fp32 oracle at the project's bars (SAC / DDPG rows
  1e-4 rel + 1e-5 abs, parameters q99 <= 5e-6 and max <= 3e-3; CVPO rows and duals 2e-4 rel + 2e-5 abs, parameters q99 <= 1e-5 and
  max <= 5e-3), nothing widened.  float64 is no yardstick here: it sees 1 - a^2 = 3e-12 where float32 sees 0, Adam turns that into
  a full lr step (the fp32 oracle's actor sits 5e-4 from its float64 run after one update, on the saturated columns' rows), and from the second update on
  the critic losses drift by 8 - 22 bars.  Also, bit for bit, what the fp32 oracle shows on the CPU: the W_sig / b_sig row of a
  column below the lower clamp is unchanged by the update, the W_mu / b_mu row of a saturated column is unchanged, every other head
  row has moved.  And EVERY head row of every column against the fp32 oracle's, as a max over the row, at the project's bulk figure
  (5e-6 SAC / DDPG, 1e-5 CVPO; branch_problems.check_head_rows says why the whole-vector bars cannot see a wrong row): this is what
  holds CVPO's small-variance column, whose sigma row is moved by the likelihood term alone.
* Mixed upper clamp (`*_mixed`): three updates, bars of tests/test_gpu_layered_replay.py (the project's, or twice the fp32
  oracle's own distance from float64 where larger); the census holds at every update.
* One grouped SAC-Lag update, k = 3, the members' actors in three different regimes: every member bit-identical to its solo twin
  (the mask is taken per member).

Not covered: exact ties of min(Q1, Q2) (SAC-Lag, CVPO's double critic) or of PPO's min(s1, s2).  Bitwise-equal values with unequal
gradients cannot be constructed robustly across summation orders.

Census (float64 oracle, CPU; regime column: rows above the upper clamp at s_t / at s_t+n per update, of the batch), the fp32 oracle
against float64 (CPU), the bar that follows, and the device against the fp32 oracle (MI355X).  rows: worst logged entry in units of the
project's bar; parameters: worst vector's max and q99.

    case                 batch  regimes (column: regime)                  census                            | oracle vs f64: rows  max     | bar     | device: rows  max      q99
    sac/h64_zero            48  0 lower, 1 sat+, 2 sat-                   lower 96/96, |u| >= 13.8 sat       |  0.017  5.0e-4 (sat rows)  | project |  0.001  6.0e-8  1.5e-8
    sac/h64_mixed           48  1 upper                                   24/23, 26/38, 25/31 of 48          |  0.002  1.5e-7             | project |  0.002  1.2e-7  3.0e-8
    sac/h256_zero          100  0 lower, 1 sat+, 2 sat-                   lower 200/200                      |  0.017  5.0e-4 (sat rows)  | project |  0.001  1.2e-7  7.5e-9
    sac/h256_mixed         100  3 upper                                   22/23, 54/50, 73/73 of 100         |  0.005  3.7e-6             | project |  0.004  3.2e-6  1.5e-8
    sac/splitk_zero         72  0 lower, 1 sat+, 2 sat-   (sac_set_plan 1) lower 144/144                     |  0.017  5.0e-4 (sat rows)  | project |  0.001  6.0e-8  1.5e-8
    sac/splitk_mixed        72  0 upper                   (sac_set_plan 1) 29/33, 45/28, 50/39 of 72         |  0.003  2.7e-7             | project |  0.003  7.5e-7  1.5e-8
    sac/layered_zero        48  0 lower, 1 sat+, 2 sat-                   lower 96/96                        |  0.017  5.0e-4 (sat rows)  | project |  0.001  6.0e-8  1.5e-8
    sac/layered_mixed       48  2 upper                                   22/15, 22/25, 23/28 of 48          |  0.002  1.6e-7             | project |  0.002  1.2e-7  3.0e-8
    ddpg/h64_sat            48  1 sat+, 2 sat-                            |head| = 14                        |  0.001  9.5e-7             | project |  0.001  1.2e-7  1.5e-8
    ddpg/layered_sat        48  0 sat-, 3 sat+                            |head| = 14                        |  0.001  9.5e-7             | project |  0.001  6.0e-8  1.5e-8
    cvpo/h64_single         48  0 lower, 2 smallvar  K 4                  var < 1e-6: 96/96, dual_std 0.1    |  0.001  4.0e-7             | project |  0.001  5.8e-7  1.5e-8
    cvpo/h64_double         48  1 lower, 3 smallvar  K 6, double critic   var < 1e-6: 96/96, dual_std 0.1    |  0.002  4.0e-7             | project |  0.001  1.2e-7  1.5e-8
    cvpo/layered_single     48  0 smallvar, 3 lower  K 4                  var < 1e-6: 96/96, dual_std 0.1    |  0.001  4.0e-7             | project |  0.001  6.0e-8  1.5e-8

Sensitivity, measured once on an MI355X with one line of a kernel changed (tests that then fail):
    `* pass` dropped in the fused SAC-Lag head        sac h64 / h256 / splitk `_zero` and `_mixed`, the grouped case, sac_clamped x 2
                                                     (and three of test_gpu_shapes.py's SAC variants)
    `* pass` dropped in the layered SAC-Lag head      sac/layered_zero, sac/layered_mixed (nothing else in the suite)
    `var > 1e-6f` made unconditional, fused CVPO      cvpo/h64_single, cvpo/h64_double (nothing else in the suite)

Bars above the project's: none.  (The zero cases are compared with the fp32 oracle, so its distance from float64 does not enter; in
the mixed cases that distance is under 0.01 project bars.)"""
import numpy as np
import pytest

import branch_problems as bp

pytestmark = pytest.mark.gpu

WHICH = {"actor": 0, "critics": 1, "critics_old": 2, "actor_old": 3}


def _push(eng, p):
    """the problem's store, in lock step (env e holds rows[e] rows from slot e * SUB on)"""
    rows, st = p["case"]["rows"], p["store"]
    for t in range(max(rows)):
        ids = [e for e in range(len(rows)) if t < rows[e]]
        at = np.array([e * bp.SUB + t for e in ids])
        eng.push(ids, st["obs"][at], st["act"][at], st["rew"][at], st["cost"][at], st["terminated"][at], st["truncated"][at],
                 st["obs_next"][at])


def _run_device(p):
    """the problem's updates on a fresh context -> (logged rows, final vectors) in the oracles' format"""
    from test_gpu_layered_replay import _engine
    kind, c = p["kind"], p["case"]
    eng = _engine(kind, c)
    if c.get("plan"):
        eng.sac_set_plan(c["plan"])
    eng.sac_set_params(p["tha"], p["thc"], -0.5 if kind == "sac" else 0.0)
    if kind == "cvpo":
        eng.sac_put_params(3, p["tha_old"])
        eng.cvpo_pre_update()
    _push(eng, p)
    B, rows = c["B"], []
    for inp in p["inputs"]:
        if kind == "sac":
            rows.append(eng.sac_update(B, p["lag"], 1 / 1.3, indices=inp["idx"], eps_target=inp["et"], eps_pi=inp["ep"]).copy())
        elif kind == "ddpg":
            zero = np.zeros((B, c["Da"]), np.float32)
            rows.append(eng.sac_update(B, p["lag"], 1 / 1.3, indices=inp["idx"], eps_target=zero, eps_pi=zero).copy())
        else:
            st = eng.cvpo_update(B, indices=inp["idx"], eps_target=inp["et"], eps_particles=inp["ek"]).copy()
            rows.append((st, eng.cvpo_duals().copy()))
    final = {k: eng.sac_get_params(WHICH[k])[0] for k in p["final"][0] if k != "alpha"}
    if kind == "sac":
        final["alpha"] = eng.sac_get_params(0)[1]
    eng.close()
    return rows, final


def _report(p, rows, final):
    kind = p["kind"]
    for u, (cen, margin) in enumerate(p["census"]):
        print(bp.census_line(f"{kind}/{p['name']} update {u}", cen, margin))
    w, vec, at = bp.replay_distance(kind, rows, final, p["rows"][0], p["final"][0])
    ow, ovec, _ = bp.replay_distance(kind, p["rows"][0], p["final"][0], p["rows"][1], p["final"][1])
    print(f"{kind}/{p['name']}: device vs fp32 oracle rows {w:.3f} x bar at {at[:2]}, max {max(v[0] for v in vec.values()):.1e} "
          f"q99 {max(v[1] for v in vec.values()):.1e} | fp32 oracle vs float64 rows {ow:.3f}, max {max(v[0] for v in ovec.values()):.1e} "
          f"q99 {max(v[1] for v in ovec.values()):.1e}")
    return w, vec, at


def _cases(kind, exact_zero):
    return [n for n, c in bp.REPLAY_CASES[kind].items() if (c["updates"] == 1) == exact_zero]


@pytest.mark.parametrize("kind,name", [(k, n) for k in bp.REPLAY_CASES for n in _cases(k, True)])
def test_exact_zero_regimes_one_update_vs_fp32_oracle_and_frozen_rows(kind, name):
    p = bp.replay_problem_with_regimes(kind, name)
    bp.check_replay_census(p)
    bp.check_frozen_rows(p, p["final"][0]["actor"], "fp32 oracle")
    rows, final = _run_device(p)
    w, vec, at = _report(p, rows, final)
    assert w <= 1.0, (kind, name, at)
    q99, mx = bp.VEC_BAR[kind]
    for k, (dmax, dq) in vec.items():
        assert dmax <= mx and dq <= q99, (kind, name, k, dmax, dq)
    bp.check_frozen_rows(p, final["actor"], "device")
    hr = bp.head_row_distances(p, final["actor"], p["final"][0]["actor"])
    print(f"{kind}/{name}: head rows vs fp32 oracle, worst {max(hr.values()):.1e} (bar {bp.HEAD_ROW_BAR[kind]:.0e}) at {max(hr, key=hr.get)}")
    bp.check_head_rows(p, final["actor"], "device")


@pytest.mark.parametrize("name", _cases("sac", False))
def test_mixed_upper_clamp_three_updates_vs_oracle(name):
    from test_gpu_layered_replay import _check
    p = bp.replay_problem_with_regimes("sac", name)
    bp.check_replay_census(p)
    rows, final = _run_device(p)
    _report(p, rows, final)
    _check("sac", name, p["case"], p["rows"] + [rows], p["final"] + [final], 2)


def test_grouped_sac_members_in_three_regimes_are_bit_identical_to_their_solo_twins():
    """k = 3 at a shape where the group takes the solo run's tile heights (test_gpu_sac_group.py EXACT_CASES: 128 wide, batch 64):
    member 0's column 0 straddles the upper clamp, member 1's sits below the lower clamp, member 2's columns saturate tanh.  Device
    RNG (a group has no caller-RNG mode), so no float64 census: the regimes hold by construction for any noise (lower: every row;
    saturated: |b_mu| = 14 against sigma = e^-3), and member 0's clamped share is read back from the solo twin's actor."""
    from fsrl_amd.engine import EngineSacGroup
    import torch
    from oracle.sac_lag import SACConfig, SACLagOracle, actor_spec
    from test_gpu_sac_group import _engine, _same, _state
    H, Do, Da, B = 128, 8, 2, 64
    spec = actor_spec(Do, Da, (H, H))
    regimes = [{0: "upper"}, {0: "lower"}, {0: "sat+", 1: "sat-"}]
    lam = [0.1, 0.2, 0.3]
    resc = [1.0 / (1.0 + l) for l in lam]
    grouped, solo = [], []
    obs = np.random.default_rng(0).standard_normal((256, Do)).astype(np.float32)
    for i in range(3):
        pair = [_engine(H, Do, Da, seed=i, T=120 + 37 * i) for _ in range(2)]
        tha = bp._set_regimes("sac", pair[0].sac_get_params(0)[0], spec, regimes[i])
        if i == 0:        # 0.1 N(0, 1) parameters: the log sigma head barely varies -- widen the row and centre it on the clamp
            sg = bp.head_rows("sac", spec, 0)[1]
            tha[sg[:-1]] *= 20.0
            o = SACLagOracle(SACConfig(obs_dim=Do, act_dim=Da, hidden=(H, H)), dtype=torch.float64)
            o.set_params(tha, np.zeros(2 * o.n_critic, np.float32))
            tha[sg[-1]] -= np.float32(np.median(bp._heads64("sac", o, o.actor, obs)[1][:, 0]) - 2.0)
        for e in pair:
            e.sac_put_params(0, tha)
            e.sac_update(B, [lam[i]], resc[i], seed=11 + i, sync=False)        # keys the member's Philox stream
        grouped.append(pair[0]); solo.append(pair[1])
    sig = solo[0].sac_actor_forward(obs)[1][:, 0]
    share = float((sig >= np.float32(np.exp(2.0)) * (1 - 1e-6)).mean())
    assert 0.2 <= share <= 0.8, share
    assert (solo[1].sac_actor_forward(obs)[1][:, 0] < 1e-8).all()
    n = [3, 3, 3]
    g = EngineSacGroup(grouped)
    g.update(B, n, [[l] for l in lam], resc)
    for i in range(3):
        for _ in range(n[i]):
            solo[i].sac_update(B, [lam[i]], resc[i], sync=False)
    out = [(_state(grouped[i]), _state(solo[i])) for i in range(3)]
    g.close()
    for e in grouped + solo:
        e.close()
    for x, y in out:
        assert len(x[4]) == 4
        _same(x, y, exact=True)
    # the regimes did shape the members' updates: member 1's sigma row of column 0 never moved, member 2's mean rows never moved
    mu0, sg0 = bp.head_rows("sac", spec, 0)
    mu1, _ = bp.head_rows("sac", spec, 1)
    a1, a2 = out[1][0][0], out[2][0][0]
    assert (a1[sg0[:-1]] == 0).all() and a1[sg0[-1]] == np.float32(-25.0)
    assert (a2[mu0[:-1]] == 0).all() and a2[mu0[-1]] == np.float32(14.0) and (a2[mu1[:-1]] == 0).all() and a2[mu1[-1]] == np.float32(-14.0)
