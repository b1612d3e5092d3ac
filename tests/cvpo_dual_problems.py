"""CVPO problems that move the E-step duals (eta, lambda) and the M-step multipliers off their lower clamps, and prove it.

Everywhere else in the suite lambda sits at its lower clamp (1.19e-6) or below 0.1: the cost side of the E-step (which member of a
DoubleCritic's pair, the overwrite of q[0] by q[0] - lambda q[1] in every iteration, the clamp after the loop and not inside it)
and the cap of the M-step multipliers do not show in any compared figure.  Here every case is a REGIME of the duals, reached through
fsrl_cvpo_config alone, with the conditions the float64 oracle must show (tests/test_cvpo_dual_problems_host.py asserts them on the
CPU; tests/test_gpu_cvpo_duals.py builds its inputs here and compares the device with the fp32 oracle):

  eta_hi       estep_kl 0, estep_dual_max 1: g_eta = -KL(p || uniform) <= 0, the unclamped step goes up, eta = 1 (upper clamp) always
  eta_lo       estep_kl 5, estep_dual_lr 2, one update: both unclamped duals negative, eta = lambda = EPS10, one-hot weights; every
               row's two largest combined values differ by >= 1e-3 >= 800 eta, so neither precision gives a fractional weight
  lam_lo       qc_thres 100: lambda = EPS10 in every update (the regime of the rest of the suite: the contrast case)
  both_moving  qc_thres -100, estep_kl 5, estep_dual_lr 0.6, estep_dual_max 1.1: (eta, lambda) = (0.4, 0.6), then (EPS10, 1.1)
  mdual_hi     mstep_kl_mu 1e-9, mstep_kl_std 1e-10, mstep_dual_max 0.15, four updates in one collect cycle: logged multipliers 0,
               then inside (0, 0.15), then 0.15 / 0.15 with the stored (unclipped) values above the cap
  costly_capped  costly_it3's settings under estep_dual_max 0.45: eta = 0.45 after update 1, lambda = 0.45 from update 2
  costly_it3   qc_thres -0.5, estep_dual_lr 0.1, three E-step iterations, two M-step iterations: lambda >= 0.1 from the first update;
               run on single / double critics, 64 and 256 wide (B 1040: sixteen-row tiles, split-K weight gradients), a layered
               context, and a (K, B) sweep over every path of the E-step kernel (lane path: one, exactly one, several rounds, ragged last
               round; per-state loop: fewer and more states than threads)

Protocol: fan-in scaled parameters, caller-RNG mode, actor_old = actor at the start, cvpo_pre_update once, then the updates with
no post_update between them.  Compared: the logged row and the four duals after every update, actor / actor_old / critics / target
critics at the end.  Bars: helpers.ROW_BAR["cvpo"] / VEC_BAR["cvpo"], or twice the fp32 oracle's own distance from its float64 run
where that is larger (the rule of tests/test_gpu_layered_replay.py).

SENSITIVITY (CPU, test_cvpo_dual_problems_host.py::test_mutant_breaks_the_bars): fp32 copies of the oracle with ONE defect each
are held to the device's bars against the unmutated fp32 oracle and must fail them.  Worst logged entry in units of its bar
(1.0 = the bar; the device itself sits at 0.001 .. 0.034, tests/test_gpu_cvpo_duals.py) and the actor's q99 in units of its bar, on a
case the GPU test runs:

    mutant                                                      case                       ratio
    (a) cost value from the first net of the DoubleCritic pair  costly_it3/h64_double      292 (update 3 loss/estep_loss; actor q99 228)
    (b) q[0] not overwritten between the E-step iterations      costly_it3/h64_single      952 (update 3 estep/dual0; actor q99 472)
    (c) the clamp applied after every E-step iteration          costly_capped              12.7 (update 3 mstep/mstep_kl_mu; actor q99 27)
    (d) the M-step multipliers used unclipped                   mdual_hi                   1884 (update 4 mstep/mstep_dual_std; actor q99 15)
    (e) the E-step Adam moments zeroed by pre_update            costly_it3/two_cycles      693 (update 3 estep/dual0; actor q99 33)
"""
import numpy as np
import torch

from helpers import ROW_BAR, VEC_BAR, fan_in_params, load_npz, replay_problem, replay_row_items, replay_vectors
from oracle.cvpo import EPS10, CVPOConfig, CVPOOracle

SUB = 256
ROWS = [100, 90]
BASE = dict(Do=7, Da=3, hidden=(64, 64), B=48, K=4, double=False, updates=3, cycles=1, seed=0)

COSTLY = dict(qc_thres=-0.5, estep_dual_lr=0.1, estep_iter_num=3, mstep_iter_num=2)
ETA_HI = dict(estep_kl=0.0, estep_dual_max=1.0)
LAM_LO = dict(qc_thres=100.0)

# name -> (case overrides, config overrides).  qc_thres is not a field of the oracle's config: cvpo_config turns it into the
# cost_limit that gives it.
CASES = {
    "eta_hi": (dict(), ETA_HI),
    "eta_lo": (dict(updates=1), dict(estep_kl=5.0, estep_dual_lr=2.0)),
    "lam_lo": (dict(), LAM_LO),
    "both_moving": (dict(), dict(qc_thres=-100.0, estep_kl=5.0, estep_dual_lr=0.6, estep_dual_max=1.1)),
    "mdual_hi": (dict(updates=4), dict(mstep_kl_mu=1e-9, mstep_kl_std=1e-10, mstep_dual_max=0.15)),
    # the E-step's clamp is applied after the loop: from 1.0 eta walks down THROUGH the cap (0.45) inside the first update's loop and
    # lambda walks up through it inside the second's, each iteration overwriting q[0] with the unclamped lambda
    "costly_capped": (dict(), dict(COSTLY, estep_dual_max=0.45)),
    # ---- costly_it3 on every kind of context
    "costly_it3/h64_single": (dict(), COSTLY),
    "costly_it3/h64_double": (dict(double=True), COSTLY),
    "costly_it3/h256_b1040_double": (dict(hidden=(256, 256), B=1040, double=True), COSTLY),     # 16-row tiles, split-K weight gradients
    "costly_it3/layered": (dict(hidden=(48, 40, 24)), COSTLY),
    # two collect cycles of two updates: pre_update resets the M-step duals and their Adam state, NOT the E-step's
    "costly_it3/two_cycles": (dict(updates=2, cycles=2), COSTLY),
    # ---- costly_it3 over the E-step kernel's paths: K a power of two <= 64 = one lane per (state, particle), 1024 per round
    "costly_it3/k2_b600": (dict(K=2, B=600), COSTLY),                       # lane path, two rounds, ragged last
    "costly_it3/k8_b128": (dict(K=8, B=128, double=True), COSTLY),          # lane path, K B = 1024 exactly
    "costly_it3/k32_b40": (dict(K=32, B=40), COSTLY),                       # lane path, ragged last round
    "costly_it3/k64_b17": (dict(K=64, B=17), COSTLY),                       # lane path, a state per wave, ragged last round
    "costly_it3/k3_b48": (dict(K=3, B=48, double=True), COSTLY),            # per-state loop
    "costly_it3/k33_b1100": (dict(K=33, B=1100), COSTLY),                   # per-state loop, more states than threads
    "costly_it3/k63_b20": (dict(K=63, B=20), COSTLY),                       # per-state loop
}
REGIMES = ("eta_hi", "eta_lo", "lam_lo", "both_moving", "mdual_hi", "costly_capped")
COSTLY_CONTEXTS = tuple(n for n in CASES if n.startswith("costly_it3/") and "/k" not in n)
COSTLY_SWEEP = tuple(n for n in CASES if n.startswith("costly_it3/k"))
GAMMA, T_MAX = 0.97, 50


def case_of(name):
    return {**BASE, **CASES[name][0]}


def cvpo_config(c, knobs):
    """the oracle's config of a case: tests/helpers.py::replay_cvpo_cfg's settings with the regime's knobs on top"""
    kn = dict(knobs)
    kw = dict(obs_dim=c["Do"], act_dim=c["Da"], hidden=tuple(c["hidden"]), max_action=1.0, gamma=GAMMA, n_step=2, tau=0.1,
              double_critic=c["double"], sample_act_num=c["K"], estep_iter_num=1, mstep_iter_num=1, cost_limit=0.5,
              max_episode_steps=T_MAX, mstep_kl_mu=1e-4, mstep_kl_std=1e-5, actor_lr=1e-3)
    if "qc_thres" in kn:                              # qc_thres = cost_limit (1 - g^T) / (1 - g) / T   (cvpo.py:138-141)
        kw["cost_limit"] = kn.pop("qc_thres") * T_MAX * (1 - GAMMA) / (1 - GAMMA**T_MAX)
    kw.update(kn)
    return CVPOConfig(**kw)


INIT_KEYS = ("actor_lr", "critic_lr", "tau", "n_step", "double_critic", "sample_act_num", "estep_iter_num", "mstep_iter_num", "estep_kl",
             "estep_dual_max", "estep_dual_lr", "mstep_kl_mu", "mstep_kl_std", "mstep_dual_max", "mstep_dual_lr")


def init_kwargs(cfg):
    """Engine.cvpo_init's keyword arguments of an oracle config (qc_thres goes first, positionally)"""
    return {k: getattr(cfg, k) for k in INIT_KEYS}


# ------------------------------------------------------------------------------------------------ the sensitivity mutants
class MutantCVPO(CVPOOracle):
    """the oracle with one defect (`mutation`: a letter of the module docstring's table)"""
    mutation = None

    def estep_cost_q(self, obs_k, act_k):
        if self.mutation == "a":
            return self.q_list(self.critics[1], obs_k, act_k)[0]
        return super().estep_cost_q(obs_k, act_k)

    def estep_duals(self, q, stats):
        if self.mutation not in ("b", "c"):
            return super().estep_duals(q, stats)
        cfg = self.cfg
        K = q[0].shape[1]
        for it in range(cfg.estep_iter_num):
            self.estep_optim.zero_grad()
            eta = self.estep_dual[0]
            combined = q[0] - self.estep_dual[1] * q[1]
            loss = eta * cfg.estep_kl + self.estep_dual[1] * cfg.qc_thres
            loss = loss + eta * torch.mean(torch.logsumexp(combined / eta, dim=1) - np.log(K))
            loss.backward()
            self.estep_optim.step()
            if self.mutation != "b":
                q[0] = combined.detach()
            if self.mutation == "c":
                self.estep_dual.data.clamp_(min=EPS10, max=cfg.estep_dual_max)
            if it == 0:
                stats["loss/estep_loss"] = loss.item()
        self.estep_dual.data.clamp_(min=EPS10, max=cfg.estep_dual_max)

    def mstep_multipliers(self):
        if self.mutation == "d":
            return self.mstep_dual_mu.item(), self.mstep_dual_std.item()
        return super().mstep_multipliers()

    def pre_update(self):
        super().pre_update()
        if self.mutation == "e":
            self.estep_optim = torch.optim.Adam([self.estep_dual], lr=self.cfg.estep_dual_lr)


def mutant(cfg, letter):
    o = MutantCVPO(cfg)
    o.mutation = letter
    return o


# ------------------------------------------------------------------------------------------------ running a case
def _duals(o):
    return np.array([o.estep_dual[0].item(), o.estep_dual[1].item(), o.mstep_dual_mu.item(), o.mstep_dual_std.item()])


def run_case(name, engines=(), extra=()):
    """One case on the fp32 oracle, the float64 oracle, every oracle `extra(cfg)` returns (mutants) and every engine of `engines`
    (contexts of test_gpu_cvpo_duals._engine): the same parameters, store, indices and noise.
    A case of several cycles runs its updates once per collect cycle, post_update / pre_update between two cycles.
    -> dict: case, cfg, per run the rows [(dict | device row) with the duals] and the final vectors, the last update's weights of the
    float64 oracle [K,B] and its combined values (q0 - lambda q1 as the weights see them) [B,K]; runs ordered fp32, float64, extra..,
    engines.."""
    torch.set_num_threads(4)
    c = case_of(name)
    cfg = cvpo_config(c, CASES[name][1])
    rng = np.random.default_rng(c["seed"])
    oracles = [CVPOOracle(cfg), CVPOOracle(cfg, dtype=torch.float64)] + list(extra(cfg) if extra else ())
    o32 = oracles[0]
    tha = fan_in_params(rng, o32.aspec)
    thc = np.concatenate([fan_in_params(rng, o32.cspec), fan_in_params(rng, o32.cspec)])
    for o in oracles:
        o.set_params(tha, thc)
    for e in engines:
        e.sac_set_params(tha, thc, 0.0)
    store, index, valid = replay_problem(rng, engines, ROWS, c["Do"], c["Da"], lambda z: np.clip(z, -1.0, 1.0), SUB)
    rows = [[] for _ in range(len(oracles) + len(engines))]
    B, K, Da = c["B"], c["K"], c["Da"]
    w64 = c64 = None
    for cyc in range(c["cycles"]):
        if cyc:
            for o in oracles:
                o.post_update()
            for e in engines:
                e.cvpo_post_update()
        for o in oracles:
            o.pre_update()
        for e in engines:
            e.cvpo_pre_update()
        for u in range(c["updates"]):
            idx = rng.choice(valid, B)
            et = rng.standard_normal((B, Da)).astype(np.float32)
            ek = rng.standard_normal((K, B, Da)).astype(np.float32)
            for o, out in zip(oracles, rows):
                st, _, w = o.update(store, index, idx, et, ek)
                out.append({**st, "duals": _duals(o)})
                if o is oracles[1]:
                    w64, c64 = w.numpy(), o.combined.numpy()
            for e, out in zip(engines, rows[len(oracles):]):
                st = e.cvpo_update(B, indices=idx, eps_target=et, eps_particles=ek).copy()
                out.append((st, e.cvpo_duals().copy()))
    final = [replay_vectors("cvpo", o) for o in oracles]
    which = {"actor": 0, "critics": 1, "critics_old": 2, "actor_old": 3}
    for e in engines:
        final.append({k: e.sac_get_params(which[k])[0] for k in final[0]})
    return dict(name=name, case=c, cfg=cfg, rows=rows, final=final, w64=w64, c64=c64)


def trace(rows):
    """per update of a run: (eta, lambda, logged dual_mu, logged dual_std, stored dual_mu, stored dual_std)"""
    out = []
    for r in rows:
        it = replay_row_items("cvpo", r)
        out.append((it["estep/dual0"], it["estep/dual1"], it["mstep/mstep_dual_mu"], it["mstep/mstep_dual_std"], it["duals[2]"],
                    it["duals[3]"]))
    return np.array(out)


def trace_line(name, tr):
    return f"{name:30s} " + "  ".join(f"[eta {t[0]:.4g} lam {t[1]:.4g} mu {t[2]:.3g}/{t[4]:.3g} std {t[3]:.3g}/{t[5]:.3g}]" for t in tr)


def check_regime(name, tr, w=None, who="float64 oracle"):
    """the conditions of the module docstring on a run's trace (`w`: eta_lo's weights [K,B])"""
    e10 = np.float32(EPS10)
    eta, lam = tr[:, 0], tr[:, 1]
    at = lambda x, v: np.all(np.asarray(x, np.float32) == np.float32(v))  # noqa: E731  the clamps are exact in float32
    if name == "eta_hi":
        assert at(eta, 1.0), (who, name, eta)
    elif name == "eta_lo":
        assert len(tr) == 1 and at(eta, e10) and at(lam, e10), (who, name, eta, lam)
        if w is not None:
            assert np.all((w == 0.0) | (w == 1.0)) and np.all(w.sum(0) == 1.0), (who, name, "fractional weights")
    elif name == "lam_lo":
        assert at(lam, e10), (who, name, lam)
    elif name == "both_moving":
        np.testing.assert_allclose(tr[0, :2], [0.4, 0.6], rtol=1e-5, err_msg=f"{who} {name}")
        assert at(eta[1:], e10) and at(lam[1:], 1.1), (who, name, eta, lam)
    elif name == "mdual_hi":
        assert len(tr) == 4 and np.all(tr[0, 2:4] == 0.0), (who, name, tr[:, 2:4])
        assert np.all((tr[1, 2:4] > 0.03) & (tr[1, 2:4] < 0.12)), (who, name, tr[1])
        assert at(tr[2:, 2:4], 0.15) and np.all(tr[2:, 4:6] > 0.15), (who, name, tr[2:])
        assert np.all(tr[3, 4:6] > 0.2), (who, name, "stored multipliers", tr[3, 4:6])
    elif name == "costly_capped":
        assert at(eta[0], 0.45) and at(lam[1:], 0.45) and 0.1 <= lam[0] < 0.45, (who, name, eta, lam)
    else:
        assert name.startswith("costly_it3/"), name
        assert np.all(lam >= 0.1), (who, name, lam)


def row_gap(p):
    """the smallest distance between a state's two largest combined values q0 - lambda q1 of the last update (float64 oracle)"""
    top = np.sort(p["c64"], axis=1)[:, -2:]
    return float((top[:, 1] - top[:, 0]).min())


# ------------------------------------------------------------------------------------------------ distances and bars
def row_figures(a, b, y):
    """per update and entry: (u, key, got, want, |a - b|, bar, project bar); bar = max(project bar on b, 2 |b - y|), b the fp32
    oracle, y its float64 run"""
    rel, ab = ROW_BAR["cvpo"]
    out = []
    for u in range(len(b)):
        A, Bv, Y = (replay_row_items("cvpo", r[u]) for r in (a, b, y))
        for k, w in Bv.items():
            out.append((u, k, A[k], w, abs(A[k] - w), max(rel * abs(w) + ab, 2.0 * abs(w - Y[k])), rel * abs(w) + ab))
    return out


def vec_figures(a, b, y):
    """per vector: (max |a - b|, q99, bar on the max, bar on the q99, argmax)"""
    q99, mx = VEC_BAR["cvpo"]
    out = {}
    for k in b:
        d, yd = np.abs(a[k] - b[k]), np.abs(b[k] - y[k])
        out[k] = (float(d.max()), float(np.quantile(d, 0.99)), max(mx, 2.0 * float(yd.max())), max(q99, 2.0 * float(np.quantile(yd, 0.99))),
                  int(d.argmax()))
    return out


def distance(p, run, against=0):
    """run `run` of a problem against run `against` in units of the case's bars: (worst logged entry, where, worst vector figure,
    where, the fp32 oracle's own worst logged entry against float64 in PROJECT bars)"""
    figs = row_figures(p["rows"][run], p["rows"][against], p["rows"][1])
    worst = max(figs, key=lambda f: f[4] / f[5])
    vf = vec_figures(p["final"][run], p["final"][against], p["final"][1])
    vworst, vat = 0.0, None
    for k, (dmax, dq, bmax, bq, _) in vf.items():
        for r, what in ((dmax / bmax, "max"), (dq / bq, "q99")):
            if r > vworst:
                vworst, vat = r, (k, what)
    own = max(row_figures(p["rows"][0], p["rows"][1], p["rows"][1]), key=lambda f: f[4] / f[6])
    return worst[4] / worst[5], worst[:4], vworst, vat, own[4] / own[6]


def check(p, run, who="device"):
    """prints the figures, then holds run `run` to the case's bars against the fp32 oracle"""
    name = p["name"]
    r, at, vr, vat, own = distance(p, run)
    vf = vec_figures(p["final"][run], p["final"][0], p["final"][1])
    print(f"{name:30s} {who}: rows {r:.3f} x bar at update {at[0]} {at[1]} (got {at[2]:.9g}, want {at[3]:.9g}); fp32 oracle vs float64 "
          f"{own:.3f} x project bar; " + " ".join(f"{k} {v[0]:.1e}/{v[1]:.1e}" for k, v in vf.items()))
    for u, k, got, want, d, bar, _ in row_figures(p["rows"][run], p["rows"][0], p["rows"][1]):
        assert d <= bar, (who, name, u, k, got, want, bar)
    for k, (dmax, dq, bmax, bq, i) in vf.items():
        assert dmax <= bmax, (who, name, f"{k}[{i}]", dmax, bmax)
        assert dq <= bq, (who, name, f"{k} q99", dq, bq)


# ------------------------------------------------------------------------------------------------ the golden fixtures' census
COSTLY_FIXTURES = ("costly_double", "costly_k5", "costly_deep3", "costly_wide")


def costly_census(name, estep_dual, stats_keys, stats, cfg):
    """What a `costly` fixture of tests/golden/gen_golden_cvpo.py must show, asserted by the generator when it writes the fixture and by
    tests/test_oracle_cvpo.py on the committed file.  estep_dual [U,2] after every update, stats [U][keys] the logged rows.
    -> a line of figures"""
    keys = [str(k) for k in stats_keys]
    eta, lam = np.asarray(estep_dual, np.float32).T
    mu, std = (np.asarray(stats, np.float64)[:, keys.index(k)] for k in ("mstep/mstep_dual_mu", "mstep/mstep_dual_std"))
    U, upc = len(eta), cfg["updates_per_cycle"]
    assert (lam >= 0.1).sum() * 2 >= U, (name, "lambda >= 0.1 in fewer than half of the updates", lam)
    assert (eta < 0.25).any(), (name, "eta never below 0.25", eta)
    if name == "costly_double":
        assert lam[0] >= 0.2 and lam[-1] >= 1.5, (name, lam)
    elif name == "costly_k5":
        cap = np.float32(cfg["estep_dual_max"])
        assert cap == np.float32(0.45) and eta[0] == cap and np.all(lam[2:] == cap) and np.all(lam[:2] < cap), (name, eta, lam)
    elif name == "costly_deep3":
        cap = cfg["mstep_dual_max"]
        assert lam.max() >= 2.0, (name, lam)
        for u in (4, 5, 10, 11):
            assert np.float32(mu[u]) == np.float32(cap) and np.float32(std[u]) == np.float32(cap), (name, u, mu, std)
        for u in range(0, U, upc):               # right behind pre_update_fn
            assert mu[u] == 0.0 and std[u] == 0.0, (name, u, mu, std)
    elif name == "costly_wide":
        assert cfg["sample_act_num"] * cfg["batch_size"] == 4096 and cfg["double_critic"], name
    else:
        raise KeyError(name)
    return (f"{name}: eta {eta.min():.3g} .. {eta.max():.3g}, lambda {lam.min():.3g} .. {lam.max():.3g} (>= 0.1 in {(lam >= 0.1).sum()} of "
            f"{U}), logged multipliers up to {mu.max():.3g} / {std.max():.3g}")


def fixture_census(name):
    import json
    g = load_npz(f"cvpo_{name}.npz")
    return costly_census(name, g["estep_dual"], g["stats_keys"], g["stats"], json.loads(str(g["cfg_json"])))
