"""The CVPO update on the device with its duals away from their lower clamps (tests/cvpo_dual_problems.py): eta at either clamp,
lambda growing, at its cap and at its floor, the M-step multipliers at their cap, three E-step iterations with the per-iteration
overwrite of q[0] carrying weight -- on single and double critics, fused 64 / 256 wide, a layered context, every path of the
E-step kernel, and in a group of three members in three different regimes.

The device is compared with the fp32 oracle on the same inputs (caller-RNG mode): the logged row and cvpo_duals() after every
update, every parameter vector at the end; bars helpers.ROW_BAR["cvpo"] / VEC_BAR["cvpo"], or twice the fp32 oracle's distance from
its float64 run where that is larger.  The regime's conditions (cvpo_dual_problems.check_regime) are asserted on the DEVICE's log.

Measured on an MI355X (the tests print these lines): worst logged entry in units of its bar, then max / q99 of |device - oracle|
per parameter vector.

rows: worst logged entry or dual over the updates as |device - oracle| / bar (1.0 = the bar); oracle: the fp32 oracle's own worst
entry against float64 in project bars (every bar the rule yields is therefore the project's own); vectors: max / q99 of
|device - oracle| (bars 5e-3 / 1e-5); actor_old is exact everywhere but after post_update (two_cycles: 6.0e-08 / 1.5e-08).

    case                             rows   worst entry                     oracle   actor max/q99    critics          critics_old     
    eta_hi                          0.001 (update 2 estep/val_q0          )  0.002   3.0e-08/1.5e-08  3.0e-08/7.5e-09  6.0e-08/3.0e-08 
    eta_lo                          0.000 (update 0 loss/q_total          )  0.000   7.8e-08/3.7e-09  3.0e-08/1.9e-09  6.0e-08/1.5e-08 
    lam_lo                          0.002 (update 2 mstep/mstep_dual_std  )  0.001   5.6e-08/1.5e-08  3.0e-08/7.5e-09  6.0e-08/3.0e-08 
    both_moving                     0.001 (update 0 estep/dual1           )  0.001   6.0e-08/1.5e-08  6.0e-08/7.5e-09  6.0e-08/3.0e-08 
    mdual_hi                        0.001 (update 3 duals[3]              )  0.001   6.0e-08/1.5e-08  3.0e-08/7.5e-09  6.0e-08/3.0e-08 
    costly_capped                   0.001 (update 0 duals[2]              )  0.001   6.0e-08/1.5e-08  3.0e-08/7.5e-09  6.0e-08/3.0e-08 
    costly_it3/h64_single           0.004 (update 2 estep/dual0           )  0.002   1.2e-07/1.5e-08  3.0e-08/7.5e-09  6.0e-08/3.0e-08 
    costly_it3/h64_double           0.011 (update 1 estep/dual0           )  0.003   4.0e-07/3.0e-08  3.2e-06/7.5e-09  8.7e-07/3.0e-08 
    costly_it3/h256_b1040_double    0.002 (update 2 mstep/mstep_kl_mu     )  0.002   6.0e-07/1.5e-08  4.4e-07/7.5e-09  1.2e-07/1.5e-08 
    costly_it3/layered              0.005 (update 1 mstep/mstep_dual_std  )  0.003   1.6e-07/3.0e-08  3.4e-07/7.5e-09  1.2e-07/3.0e-08 
    costly_it3/two_cycles           0.006 (update 3 mstep/mstep_dual_mu   )  0.006   6.0e-08/1.5e-08  3.0e-08/7.5e-09  6.0e-08/3.0e-08 
    costly_it3/k2_b600              0.009 (update 1 mstep/mstep_dual_std  )  0.002   8.9e-08/3.0e-08  1.3e-07/7.5e-09  1.8e-07/3.0e-08 
    costly_it3/k8_b128              0.034 (update 0 estep/dual0           )  0.012   6.3e-07/5.3e-08  1.3e-07/7.5e-09  1.2e-07/3.0e-08 
    costly_it3/k32_b40              0.025 (update 1 estep/dual0           )  0.002   1.7e-07/3.0e-08  6.7e-08/7.5e-09  1.2e-07/3.0e-08 
    costly_it3/k64_b17              0.013 (update 1 estep/dual0           )  0.002   2.7e-07/3.0e-08  6.0e-08/7.5e-09  1.2e-07/3.0e-08 
    costly_it3/k3_b48               0.011 (update 1 estep/dual0           )  0.004   1.2e-07/3.0e-08  3.2e-06/7.5e-09  8.7e-07/3.0e-08 
    costly_it3/k33_b1100            0.011 (update 2 estep/dual0           )  0.010   4.8e-07/3.0e-08  3.0e-08/7.5e-09  6.0e-08/3.0e-08 
    costly_it3/k63_b20              0.028 (update 1 estep/dual0           )  0.021   2.0e-06/4.5e-08  3.0e-08/7.5e-09  6.0e-08/3.0e-08 

What the device logged per update: eta_hi eta = 1 / 1 / 1; eta_lo eta = lambda = 1.192e-06; lam_lo lambda = 1.192e-06 throughout,
eta 0.98 / 0.9603 / 0.9404; both_moving (eta, lambda) = (0.4, 0.6), (1.192e-06, 1.1), (1.192e-06, 1.1); mdual_hi logged multipliers
0, 0 / 0.0653, 0.0734 / 0.15, 0.15 / 0.15, 0.15 with 0.242, 0.244 stored at the end; costly_capped eta 0.45 throughout, lambda
0.2998 / 0.45 / 0.45; costly_it3 lambda 0.30 / 0.59 .. 0.60 / 0.88 .. 0.91 on every context and path (two_cycles: to 1.204),
eta between 0.52 and 1.40.
Group of three (costly_it3, eta_hi, lam_lo settings): member 0's lambda 0.30 -> 1.85, member 1's eta 1.0, member 2's lambda
1.192e-06 in every row, at both shapes.
"""
import numpy as np
import pytest

import cvpo_dual_problems as dp

pytestmark = pytest.mark.gpu


def _engine(name):
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig
    c = dp.case_of(name)
    cfg = dp.cvpo_config(c, dp.CASES[name][1])
    E = len(dp.ROWS)
    eng = Engine(EngineConfig(algo=_lib.ALGO_SAC_LAG, obs_dim=c["Do"], act_dim=c["Da"], hidden_sizes=tuple(c["hidden"]), n_critics=2,
                              env_num=E, buffer_size=E * dp.SUB, gamma=dp.GAMMA, target_kl=None))
    eng.cvpo_init(cfg.qc_thres, **dp.init_kwargs(cfg))
    return eng


@pytest.mark.parametrize("name", list(dp.CASES))
def test_cvpo_duals_vs_oracle(name):
    eng = _engine(name)
    p = dp.run_case(name, [eng])
    eng.close()
    dp.check_regime(name, dp.trace(p["rows"][1]), p["w64"])
    tr = dp.trace(p["rows"][2])
    print(dp.trace_line(f"{name} (device)", tr))
    dp.check(p, 2)
    dp.check_regime(name, tr, None, "device")


# H, Do, Da, B, K of two of test_gpu_cvpo_group.py's SAME_CASES, the group size, and whether every context is created under
# FSRL_TILE16.  At the second shape the particle launch (K B = 256 rows) fits one round of four-row tiles only up to k = 2; a group
# keeps the member's own tile height in that launch (host_cvpo_group.inc), so k = 3 is bit-identical too -- it was one unit in the
# last place off (actor 7.5e-8, duals 9.5e-7) while the group sized that launch by k.  The last two entries are the same shape at the
# SAME_CASES group size and with sixteen-row tiles everywhere.
GROUP_CASES = [(((128, 96), 8, 2, 64, 16), 3, False), ((64, 8, 2, 32, 8), 3, False), ((64, 8, 2, 32, 8), 2, False),
               ((64, 8, 2, 32, 8), 3, True)]


@pytest.mark.parametrize("shape,k,tile16", GROUP_CASES)
def test_group_members_in_different_regimes_are_bit_identical_to_solo(shape, k, tile16):
    """EngineCvpoGroup, library RNG, two cycles: the members share the launch structure (three E-step and two M-step iterations, K,
    n_step) and differ in dual rates, caps, KL bounds and qc_thres -- costly_it3, eta_hi, lam_lo (k = 2: the first two).  Every member
    is bit for bit its solo twin, and each member's log shows its regime."""
    from fsrl_amd.engine import EngineCvpoGroup
    from oracle.cvpo import EPS10
    from test_gpu_cvpo_group import _engine as member, _same, _state
    H, Do, Da, B, K = shape
    shared = dict(sample_act_num=K, estep_iter_num=3, mstep_iter_num=2)
    own = [dict(estep_dual_lr=0.1), dict(dp.ETA_HI), dict()][:k]
    thres = [-0.5, None, 100.0][:k]

    def mk(i):
        e = member(H, Do, Da, seed=i, T=120 + 37 * i, tile16=tile16, **shared, **own[i])
        if thres[i] is not None:
            e.cvpo_set_thres(thres[i])
        return e
    grouped, solo = [mk(i) for i in range(k)], [mk(i) for i in range(k)]
    for i in range(k):                                 # key each member's Philox stream
        for e in (grouped[i], solo[i]):
            e.cvpo_update(B, seed=11 + i, sync=False)
    g = EngineCvpoGroup(grouped)
    cycles = [[3, 2, 3][:k], [2, 3, 1][:k]]
    for c, n in enumerate(cycles):
        if c:
            for e in grouped + solo:
                e.cvpo_post_update(); e.cvpo_pre_update()
        g.update(B, n)
        for i in range(k):
            for _ in range(n[i]):
                solo[i].cvpo_update(B, sync=False)
    states = [(_state(grouped[i]), _state(solo[i])) for i in range(k)]
    g.close()
    for e in grouped + solo:
        e.close()
    eta = [s[1][5][:, 1] for s in states]                 # the solo twins' logs: the regimes
    lam = [s[1][5][:, 2] for s in states]
    print("group", shape, k, "lambda of member 0:", lam[0], "eta of member 1:", eta[1], "lambda of member 2:", lam[2] if k > 2 else None)
    assert np.all(lam[0] >= 0.1) and lam[0][-1] >= 1.0, lam[0]
    assert np.all(eta[1] == 1.0), eta[1]
    assert k < 3 or np.all(lam[2] == np.float32(EPS10)), lam[2]
    for i, (x, y) in enumerate(states):
        assert x[5].shape == (cycles[0][i] + cycles[1][i] + 1, 17)
        for j, nm in enumerate(("actor", "critics", "critics_old", "actor_old", "duals", "rows")):
            print(f"group {shape} k={k} member {i} {nm}: max |grouped - solo| {np.abs(x[j] - y[j]).max():.3g}")
    for x, y in states:
        _same(x, y)


@pytest.mark.parametrize("K", [0, 65])
def test_cvpo_init_refuses_a_particle_count_outside_1_to_64(K):
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig
    eng = Engine(EngineConfig(algo=_lib.ALGO_SAC_LAG, obs_dim=4, act_dim=2, hidden=64, n_critics=2, env_num=1, buffer_size=64,
                              target_kl=None))
    with pytest.raises(AssertionError, match="sample_act_num"):
        eng.cvpo_init(0.1, sample_act_num=K)
    eng.cvpo_init(0.1, sample_act_num=64 if K > 64 else 1)              # the limit itself is fine
    eng.close()
