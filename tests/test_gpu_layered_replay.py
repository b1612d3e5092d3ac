"""Solo LAYERED replay agents (SAC-Lag, DDPG-Lag, CVPO on `hidden_sizes` that are not two layers of at most 256 units:
kernels_layered.hpp, kernels_layered_sac.hpp, host_layered.inc, the layered branches of host_sac.inc / host_cvpo.inc) against
their CPU oracles (oracle/sac_lag.py, oracle/ddpg_lag.py, oracle/cvpo.py) on random problems -- the path the grouped layered tests
(tests/test_gpu_sac_group_layered.py) compare themselves with bit for bit, at the shapes they lean on, at the documented limits
(FSRL_MAX_HIDDEN layers, FSRL_MAX_WIDTH units, obs_dim + act_dim = FSRL_MAX_OBS), at widths below a float4, on a single row, and
in ONE context whose working set grows (`regrow`: the row stride of the working set is then no longer the batch).

Protocol: fan-in scaled parameters (W ~ N(0, 1 / fan_in), b ~ 0.1 N(0, 1)), three updates in caller-RNG mode (indices and noise
injected), the logged row of every update, every parameter vector at the end (actor, critics, target critics, DDPG's target /
CVPO's old actor), alpha, CVPO's duals after every update.  CVPO: updates 1 and 2 in one collect cycle, post_update (actor_old <-
actor), update 3 in the next, so the last update runs with actor_old != actor.

Bars.  The project's own (tests/test_gpu_shapes.py, test_gpu_ddpg.py, test_gpu_cvpo.py): SAC / DDPG rows 1e-4 rel + 1e-5 abs,
parameters q99 <= 5e-6 and max <= 3e-3; CVPO rows and duals 2e-4 rel + 2e-5 abs, parameters q99 <= 1e-5 and max <= 5e-3.  They were
set on two-layer networks of 64 - 256 units, so every comparison takes the larger of that bar and TWICE THE fp32 ORACLE'S OWN
DISTANCE FROM ITS float64 RUN of the same case (the oracles' `dtype` argument; the rule of test_gpu_trust.py::
test_cpo_learn_vs_golden): per logged entry for rows, duals and alpha; per vector (max, and q99) for parameters.  Nothing is
widened from the device's output.  On the tiny networks (`narrow`, `one_particle_narrow`: 20 - 40 parameters) a q99 is no
quantile: the max bound alone; their data seeds (SEEDS below) were picked on the CPU, among 0 .. 7, so that every Linear keeps a
live gradient (a dead one-unit layer would leave most tensors unchanged) and the fp32 oracle sits inside the project bar against
float64.
SAC-Lag's head is sigma = exp(Linear): with fan-in scaled parameters a few of the hundreds of samples u = mu + sigma eps of a large
batch reach the saturated tail of tanh, where 1 - tanh(u)^2 falls below 1e-6 and the fp32 ORACLE itself leaves its float64 run
by 10 - 90 project bars (seed 0 of `wide1`: min (1 - a^2) = 3e-12, loss/q1 off by 8.5e-3 rel).  That tail is ill-conditioned in
either implementation and not what this file is about, so the three SAC cases with the largest batches / widest layers (`wide1`,
`width_4096`, `din128`) take the first data seed (SEEDS) at which the fp32 oracle -- the oracle, not the device -- is inside
the project bar against float64 with room to spare; the rule above still applies to them.

fp32 oracle against its float64 run (CPU), the bar that follows, and the device against the fp32 oracle (MI355X), worst over the
three updates / the parameter vectors.  rows: |a - b| / (rel |b| + abs) with the project's rel / abs, so 1.0 is the project bar;
params: max |a - b| (project: 3e-3 SAC / DDPG, 5e-3 CVPO) and q99 (5e-6 / 1e-5).

    case                             oracle vs f64: rows   max      q99    | bar: rows max     q99    | device: rows max    q99
    sac/ragged                                   0.001  8.5e-08  4.4e-08  |  1.00  3.0e-03  5.0e-06  |  0.001  6.0e-08  3.0e-08
    sac/wide1                (seed 37)           0.025  1.8e-07  8.5e-08  |  1.00  3.0e-03  5.0e-06  |  0.002  1.2e-07  6.0e-08
    sac/narrow               (seed 1)            0.002  3.6e-07     -     |  1.00  3.0e-03     -     |  0.001  6.0e-08     -
    sac/din128               (seed 6)            0.012  3.9e-07  3.6e-08  |  1.00  3.0e-03  5.0e-06  |  0.002  3.9e-07  2.2e-08
    sac/eight_layers                             0.007  2.3e-07  6.7e-08  |  1.00  3.0e-03  5.0e-06  |  0.005  1.2e-07  3.0e-08
    sac/width_4096           (seed 1)            0.055  1.3e-05  8.5e-08  |  1.00  3.0e-03  5.0e-06  |  0.024  1.4e-05  6.0e-08
    sac/forced               layered             0.002  1.6e-07  4.8e-08  |  1.00  3.0e-03  5.0e-06  |  0.002  1.2e-07  3.0e-08
                             fused                                        |  1.00  3.0e-03  5.0e-06  |  0.002  1.2e-07  3.0e-08
                             layered vs fused                             |  2.00  6.0e-03  1.0e-05  |  0.001  1.0e-07  7.5e-09
    sac/regrow                                   0.123  1.1e-06  6.8e-08  |  1.00  3.0e-03  5.0e-06  |  0.006  6.4e-07  3.0e-08
    ddpg/eight_layers                            0.001  7.6e-06  7.9e-08  |  1.00  3.0e-03  5.0e-06  |  0.001  1.3e-05  3.0e-08
    ddpg/narrow              (seed 6)            0.001  3.0e-07     -     |  1.00  3.0e-03     -     |  0.000  1.2e-07     -
    ddpg/regrow                                  0.003  2.2e-07  5.1e-08  |  1.00  3.0e-03  5.0e-06  |  0.001  1.9e-07  3.0e-08
    cvpo/eight_layers_double                     0.002  1.8e-07  7.1e-08  |  1.00  5.0e-03  1.0e-05  |  0.002  1.2e-07  3.0e-08
    cvpo/eight_layers_single                     0.004  7.3e-07  7.0e-08  |  1.00  5.0e-03  1.0e-05  |  0.003  6.6e-07  3.0e-08
    cvpo/one_particle_narrow (seed 2)            0.451  2.4e-07     -     |  1.00  5.0e-03     -     |  0.574  2.4e-07     -
    cvpo/particles_many_tiles                    0.004  1.5e-07  4.5e-08  |  1.00  5.0e-03  1.0e-05  |  0.004  2.1e-07  1.5e-08
    cvpo/regrow                                  0.003  4.0e-07  5.0e-08  |  1.00  5.0e-03  1.0e-05  |  0.003  1.4e-07  3.0e-08
    collector actor (1 / 17 / 33 rows): mean <= 0.023 of its bar, sigma <= 0.22 of its bar (SAC-Lag, DDPG-Lag, CVPO)

Bars above the project's: none.  At these seeds the fp32 oracle is within half a project bar of its float64 run in every entry of
every case, so every bar the rule yields is the project's own (the largest oracle distances: the M-step dual of the one-particle
case, whose Adam step divides a difference of two nearly equal KL terms, at 0.45 bars; one critic entry of the 4 096-wide layer at
1.3e-5, Adam moving an entry whose gradient is rounding noise).  The device sits as close to the fp32 oracle as the oracle to
float64.
"""
import numpy as np
import pytest
import torch

from helpers import (CVPO_KEYS, ROW_BAR, SAC_KEYS, VEC_BAR, fan_in_params, replay_problem)  # noqa: F401
from helpers import replay_cvpo_cfg as _cvpo_cfg
from helpers import replay_oracles as _oracles
from helpers import replay_row_items as _row_items
from helpers import replay_vectors as _vectors

pytestmark = pytest.mark.gpu

EIGHT = (24, 17, 32, 9, 40, 4, 28, 12)       # FSRL_MAX_HIDDEN ragged layers: one below a float4, one of 4, none a multiple of 16 twice
SUB = 256                                     # rows of a sub-buffer

# B: one batch size, or the three of the `regrow` cases.  Defaults: n_step 2, learned alpha, Lagrangian term, data seed 0.
SAC_CASES = {
    # the grouped test's shape: no float4 operand anywhere (obs 33, widths 50 / 30), one 16-row tile plus a 4-row tail, all 16 head
    # columns [mu | log sigma] through the a_len = 16 rows
    "ragged": dict(Do=33, Da=8, hidden=(50, 30), rows=[40, 17], B=20, n_step=3, auto_alpha=False),
    # the grouped test's other shape: one layer, 17 row tiles
    "wide1": dict(Do=8, Da=2, hidden=(320, ), rows=[150, 150], B=272, use_lag=False),
    # Din = 2, layers narrower than a float4, a one-unit layer, one batch row, Da = 1 (the row sums over one lane)
    "narrow": dict(Do=1, Da=1, hidden=(3, 1, 2), rows=[33], B=1, tiny=True),
    # dQ / d[obs | act] (lay_bwd_dz_k with dx_in: the l = -1 launch) at FSRL_MAX_OBS: two column tiles, the action columns 120 .. 127
    # read back by the actor's head
    "din128": dict(Do=120, Da=8, hidden=(40, 72, 24), rows=[70, 50], B=100),
    # 4 Q-networks x 9 Linears = 36 weight-side jobs: more than one launch's table holds (lay_wgrad_k sends whole networks)
    "eight_layers": dict(Do=20, Da=8, hidden=EIGHT, rows=[70, 50], B=64),
    "width_4096": dict(Do=8, Da=2, hidden=(4096, ), rows=[70, 50], B=64),                 # FSRL_MAX_WIDTH
    # the fused kernels' own network through the layered ones: against the oracle AND against the fused context
    "forced": dict(Do=8, Da=2, hidden=(64, 64), rows=[70, 50], B=64, force=True),
    # the working set grows at the second update: from then on its row stride (out, dout, DXQ, Bq) is 208, not the batch
    "regrow": dict(Do=8, Da=2, hidden=(64, 48, 32), rows=[70, 50], B=[32, 208, 32]),
}
DDPG_CASES = {
    "eight_layers": dict(Do=20, Da=16, hidden=EIGHT, rows=[70, 50], B=64),                # 18 jobs; 16 raw head columns
    "narrow": dict(Do=1, Da=1, hidden=(3, 1, 2), rows=[33], B=1, tiny=True),
    "regrow": dict(Do=8, Da=2, hidden=(64, 48, 32), rows=[70, 50], B=[32, 208, 32]),
}
CVPO_CASES = {
    # DoubleCritic: 36 weight-side jobs; the E-step's K x B particle rows in the Q working set
    "eight_layers_double": dict(Do=12, Da=4, hidden=EIGHT, rows=[70, 50], B=64, K=8, double=True),
    "eight_layers_single": dict(Do=12, Da=4, hidden=EIGHT, rows=[70, 50], B=64, K=8),     # n_q = 2
    "one_particle_narrow": dict(Do=1, Da=1, hidden=(3, 1, 2), rows=[33], B=1, K=1, tiny=True),
    # 4 096 particle rows: 64 row tiles x 3 column tiles x 4 networks = 768 workgroups in the first-layer launch.  lay_launch
    # (host_layered.inc) gives a launch of more than 2 x n_cus active workgroups 8 waves each (nw = 2), of more than 4 x n_cus 4
    # waves (nw = 1): on the 256 compute units of an MI355X 768 selects nw = 2, which no other replay test reaches
    "particles_many_tiles": dict(Do=12, Da=4, hidden=(130, 70), rows=[70, 50], B=64, K=64, double=True),
    "regrow": dict(Do=8, Da=2, hidden=(64, 48, 32), rows=[70, 50], B=[16, 100, 16], K=16),      # the XK / QK / Wk strides change
}
# data seeds picked on the CPU from the oracle alone (see the module docstring); every other case: 0
SEEDS = {("sac", "narrow"): 1, ("ddpg", "narrow"): 6, ("cvpo", "one_particle_narrow"): 2,
         ("sac", "wide1"): 37, ("sac", "width_4096"): 1, ("sac", "din128"): 6}


def _batches(c):
    return list(c["B"]) if isinstance(c["B"], (list, tuple)) else [c["B"]] * 3


def _engine(kind, c, force=None):
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig
    E = len(c["rows"])
    eng = Engine(EngineConfig(algo=_lib.ALGO_SAC_LAG, obs_dim=c["Do"], act_dim=c["Da"], hidden_sizes=tuple(c["hidden"]), n_critics=2,
                              env_num=E, buffer_size=E * SUB, gamma=0.97 if kind == "cvpo" else 0.98, target_kl=None,
                              force_layered=bool(c.get("force")) if force is None else force))
    if kind == "sac":
        eng.sac_init(n_step=c.get("n_step", 2), auto_alpha=c.get("auto_alpha", True), alpha=0.05, use_lagrangian=c.get("use_lag", True),
                     tau=0.1)
    elif kind == "ddpg":
        eng.sac_init(actor_lr=1e-3, critic_lr=1e-3, tau=0.1, n_step=2, use_lagrangian=True, deterministic=True)
    else:
        eng.cvpo_init(_cvpo_cfg(c).qc_thres, actor_lr=1e-3, tau=0.1, n_step=2, double_critic=c.get("double", False),
                      sample_act_num=c["K"], estep_iter_num=1, mstep_iter_num=1, mstep_kl_mu=1e-4, mstep_kl_std=1e-5)
    return eng


WHICH = {"actor": 0, "critics": 1, "critics_old": 2, "actor_old": 3}


def run_case(kind, name, engines=()):
    """One case on the fp32 oracle, the float64 oracle and every engine of `engines` (contexts of _engine(kind, case)): the same
    parameters, store, indices and noise.  -> (case, per run a list of three logged rows (dict / device row; CVPO: + `duals`), per run the
    final vectors and alpha); runs ordered fp32 oracle, float64 oracle, engines..."""
    c = {"sac": SAC_CASES, "ddpg": DDPG_CASES, "cvpo": CVPO_CASES}[kind][name]
    rng = np.random.default_rng(SEEDS.get((kind, name), 0))
    Do, Da = c["Do"], c["Da"]
    o32, o64 = _oracles(kind, c)
    tha = fan_in_params(rng, o32.aspec)
    thc = np.concatenate([fan_in_params(rng, o32.cspec), fan_in_params(rng, o32.cspec)])
    for o in (o32, o64):
        o.set_params(tha, thc, -0.5) if kind == "sac" else o.set_params(tha, thc)
    for e in engines:
        e.sac_set_params(tha, thc, -0.5 if kind == "sac" else 0.0)
    squash = (lambda z: np.clip(z, -1.0, 1.0)) if kind == "cvpo" else np.tanh
    store, index, valid = replay_problem(rng, engines, c["rows"], Do, Da, squash, SUB)
    lag = [0.3] if c.get("use_lag", True) else []
    rows = [[] for _ in range(2 + len(engines))]
    for u, B in enumerate(_batches(c)):
        idx = rng.choice(valid, B)
        et = rng.standard_normal((B, Da)).astype(np.float32)
        if kind == "sac":
            ep = rng.standard_normal((B, Da)).astype(np.float32)
            for o, out in ((o32, rows[0]), (o64, rows[1])):
                sa, sc, _ = o.update(store, index, idx, et, ep, lag if lag else [0.0], 1 / 1.3)
                out.append({**sa, **sc})
            for e, out in zip(engines, rows[2:]):
                out.append(e.sac_update(B, lag, 1 / 1.3, indices=idx, eps_target=et, eps_pi=ep).copy())
        elif kind == "ddpg":
            zero = np.zeros((B, Da), np.float32)
            for o, out in ((o32, rows[0]), (o64, rows[1])):
                sa, sc, _ = o.update(store, index, idx, np.array(lag), 1 / 1.3)
                out.append({**sa, **sc})
            for e, out in zip(engines, rows[2:]):
                out.append(e.sac_update(B, lag, 1 / 1.3, indices=idx, eps_target=zero, eps_pi=zero).copy())
        else:
            ek = rng.standard_normal((c["K"], B, Da)).astype(np.float32)
            if u in (0, 2):                         # updates 1, 2 | post_update | update 3
                for o in (o32, o64):
                    o.pre_update()
                for e in engines:
                    e.cvpo_pre_update()
            for o, out in ((o32, rows[0]), (o64, rows[1])):
                st, _, _ = o.update(store, index, idx, et, ek)
                out.append({**st, "duals": np.array([o.estep_dual[0].item(), o.estep_dual[1].item(), o.mstep_dual_mu.item(),
                                                     o.mstep_dual_std.item()])})
            for e, out in zip(engines, rows[2:]):
                st = e.cvpo_update(B, indices=idx, eps_target=et, eps_particles=ek).copy()
                out.append((st, e.cvpo_duals().copy()))
            if u == 1:
                for o in (o32, o64):
                    o.post_update()
                for e in engines:
                    e.cvpo_post_update()
    final = []
    for o in (o32, o64):
        v = _vectors(kind, o)
        if kind == "sac":
            v["alpha"] = float(o.alpha)
        final.append(v)
    for e in engines:
        v = {k: e.sac_get_params(WHICH[k])[0] for k in final[0] if k != "alpha"}
        if kind == "sac":
            v["alpha"] = e.sac_get_params(0)[1]
        final.append(v)
    return c, rows, final


def row_figures(kind, a, b, y):
    """per update and key: (|a - b|, the bar) with the bar = max(project bar on b, 2 |b - y|); b the fp32 oracle, y its float64 run"""
    rel, ab = ROW_BAR[kind]
    out = []
    for u in range(len(b)):
        A, Bv, Y = _row_items(kind, a[u]), _row_items(kind, b[u]), _row_items(kind, y[u])
        for k, w in Bv.items():
            out.append((u, k, A[k], w, abs(A[k] - w), max(rel * abs(w) + ab, 2.0 * abs(w - Y.get(k, w))), rel * abs(w) + ab))
    return out


def vec_figures(kind, a, b, y):
    """per vector: (max |a - b|, q99 |a - b|, bar on the max, bar on the q99), bars = max(project, twice the oracle's own distance)"""
    q99, mx = VEC_BAR[kind]
    out = {}
    for k in b:
        if k == "alpha":
            continue
        d, yd = np.abs(a[k] - b[k]), np.abs(b[k] - y[k])
        out[k] = (float(d.max()), float(np.quantile(d, 0.99)), max(mx, 2.0 * float(yd.max())), max(q99, 2.0 * float(np.quantile(yd, 0.99))),
                  int(d.argmax()))
    return out


def _check(kind, name, c, rows, final, run, factor=1.0, against=0):
    """run `run` against run `against` (0: the fp32 oracle) at `factor` times the case's bars; the figures are printed first"""
    figs = row_figures(kind, rows[run], rows[against], rows[1])
    worst = max(figs, key=lambda f: f[4] / f[6])
    print(f"{kind}/{name} run {run} vs {against}: rows worst {worst[4] / worst[6]:.3f} x project bar at update {worst[0]} {worst[1]} "
          f"(got {worst[2]:.9g}, want {worst[3]:.9g})")
    vf = vec_figures(kind, final[run], final[against], final[1])
    for k, (dmax, dq, bmax, bq, at) in vf.items():
        print(f"{kind}/{name} run {run} vs {against}: {k:12s} max {dmax:.3e} (bar {bmax:.3e})  q99 {dq:.3e} (bar {bq:.3e})")
    for u, k, got, want, d, bar, _ in figs:
        assert d <= factor * bar, (name, u, k, got, want)
    if kind == "sac":
        rel, ab = ROW_BAR[kind]
        got, want = final[run]["alpha"], final[against]["alpha"]
        assert abs(got - want) <= factor * max(rel * abs(want) + ab, 2.0 * abs(final[0]["alpha"] - final[1]["alpha"])), \
            (name, "final", "alpha", got, want)
    for k, (dmax, dq, bmax, bq, at) in vf.items():
        got, want = float(final[run][k][at]), float(final[against][k][at])
        assert dmax <= factor * bmax, (name, "final", f"{k}[{at}]", got, want)
        if not c.get("tiny"):
            assert dq <= factor * bq, (name, "final", f"{k} q99", dq, bq)


@pytest.mark.parametrize("name", [n for n in SAC_CASES if n != "forced"])
def test_layered_sac_vs_oracle(name):
    eng = _engine("sac", SAC_CASES[name])
    c, rows, final = run_case("sac", name, [eng])
    eng.close()
    _check("sac", name, c, rows, final, 2)


def test_forced_layered_sac_vs_oracle_and_vs_the_fused_context():
    """hidden (64, 64) through the fused kernels and, with force_layered, through one GEMM launch per Linear, on the same inputs:
    both within the case's bars of the oracle, and within twice the bars of each other (as
    test_gpu_layered.py::test_two_layer_network_through_the_layered_kernels does for PPO-Lag)."""
    fused, layered = _engine("sac", SAC_CASES["forced"], force=False), _engine("sac", SAC_CASES["forced"], force=True)
    c, rows, final = run_case("sac", "forced", [fused, layered])
    fused.close(); layered.close()
    _check("sac", "forced", c, rows, final, 2)
    _check("sac", "forced", c, rows, final, 3)
    _check("sac", "forced", c, rows, final, 3, factor=2.0, against=2)


@pytest.mark.parametrize("name", list(DDPG_CASES))
def test_layered_ddpg_vs_oracle(name):
    eng = _engine("ddpg", DDPG_CASES[name])
    c, rows, final = run_case("ddpg", name, [eng])
    eng.close()
    _check("ddpg", name, c, rows, final, 2)


@pytest.mark.parametrize("name", list(CVPO_CASES))
def test_layered_cvpo_vs_oracle(name):
    eng = _engine("cvpo", CVPO_CASES[name])
    c, rows, final = run_case("cvpo", name, [eng])
    eng.close()
    _check("cvpo", name, c, rows, final, 2)


COLLECT = {   # the collector's actor (sac_actor_launch's layered branch, lay_raw_out_kernel) per kind: Do, Da, hidden
    "sac": dict(Do=33, Da=8, hidden=(50, 30), rows=[1]),            # 16 raw columns [mu | log sigma], dword loads
    "ddpg": dict(Do=20, Da=16, hidden=EIGHT, rows=[1]),             # 16 raw columns of the mean head alone
    "cvpo": dict(Do=12, Da=4, hidden=(130, 70), rows=[1], K=4),     # 8 raw columns
}


def _actor_heads(kind, o, obs):
    """the oracle's actor on `obs` in the oracle's precision: (mean as fsrl_sac_actor_forward reports it, sigma)"""
    import torch.nn.functional as F
    from oracle.sac_lag import SIGMA_MAX, SIGMA_MIN, _trunk
    x = torch.as_tensor(obs, dtype=o.dtype)
    with torch.no_grad():
        if kind == "ddpg":
            return o.pi(o.actor, x).numpy(), None
        if kind == "cvpo":
            mu, sigma = o.pi(o.actor, x)
            return mu.numpy(), sigma.numpy()
        p = o.actor                                 # SAC-Lag: the raw mean head; tanh is applied to the SAMPLE
        h = _trunk(p, x, len(o.cfg.hidden))
        return (F.linear(h, p["Wmu"], p["bmu"]).numpy(),
                torch.clamp(F.linear(h, p["Wsig"], p["bsig"]), min=SIGMA_MIN, max=SIGMA_MAX).exp().numpy())


@pytest.mark.parametrize("kind", list(COLLECT))
def test_collector_actor_of_a_layered_replay_context(kind):
    """fsrl_sac_actor_forward / fsrl_actor_sample on 1, 17 and 33 rows (one row; a tile plus one row; two tiles plus one) against
    the oracle's actor on the same parameters.  Bars of test_gpu_layered.py::test_collector_actor_of_a_layered_context (mean 1e-5
    rel + 1e-5 abs, sigma 1e-6 + 1e-6), or twice the fp32 oracle's distance from its float64 run where that is larger.  The
    deterministic sample IS the mean: exactly for DDPG-Lag and CVPO; SAC-Lag squashes on the host, tanh(mean) to two float32 ulps of 1
    (two libms, each within an ulp)."""
    c = COLLECT[kind]
    eng = _engine(kind, c)
    o32, o64 = _oracles(kind, c)
    rng = np.random.default_rng(5)
    tha = fan_in_params(rng, o32.aspec)
    thc = np.concatenate([fan_in_params(rng, o32.cspec), fan_in_params(rng, o32.cspec)])
    for o in (o32, o64):
        o.set_params(tha, thc)
    eng.sac_set_params(tha, thc, 0.0)
    for k in (1, 17, 33):
        obs = rng.standard_normal((k, c["Do"])).astype(np.float32)
        mu, sigma = eng.sac_actor_forward(obs)
        (m32, s32), (m64, s64) = _actor_heads(kind, o32, obs), _actor_heads(kind, o64, obs)
        bar = np.maximum(1e-5 * np.abs(m32) + 1e-5, 2.0 * np.abs(m32 - m64))
        print(f"{kind} k={k}: mean worst {(np.abs(mu - m32) / bar).max():.3f} x bar")
        at = np.unravel_index((np.abs(mu - m32) / bar).argmax(), mu.shape)
        assert (np.abs(mu - m32) <= bar).all(), (kind, k, f"mean{at}", float(mu[at]), float(m32[at]))
        if kind == "ddpg":
            assert np.array_equal(sigma, np.full_like(sigma, 0.1))         # the exploration noise's std
        else:
            bar = np.maximum(1e-6 * np.abs(s32) + 1e-6, 2.0 * np.abs(s32 - s64))
            print(f"{kind} k={k}: sigma worst {(np.abs(sigma - s32) / bar).max():.3f} x bar")
            at = np.unravel_index((np.abs(sigma - s32) / bar).argmax(), sigma.shape)
            assert (np.abs(sigma - s32) <= bar).all(), (kind, k, f"sigma{at}", float(sigma[at]), float(s32[at]))
        a = eng.actor_sample(obs, deterministic=True)
        if kind == "sac":
            np.testing.assert_allclose(a, np.tanh(mu.astype(np.float64)), rtol=0, atol=2.4e-7)
        else:
            assert np.array_equal(a, mu), (kind, k)
    eng.close()
