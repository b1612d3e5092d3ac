"""Layered contexts on the FULL-BATCH (trust-region) path at the sizes, ragged widths and limits where lay_launch
(fsrl_amd/csrc/host_layered.inc) changes the kernel it starts: lin_kernel<FORM, VEC, NW> for FORM = LIN_F / LIN_X / LIN_W with the
float4 and the dword-load instantiation (VEC), 16 / 8 / 4 waves per workgroup (NW = 4 / 2 / 1, chosen from the launch's workgroup
count against the CU count) and the split-K weight side (ksplit ranges of the batch rows, partials at stride n_dev added in float64 by
fb_sum_parts_kernel, adam_range_kernel and cg_pz_kernel).

The pieces -- tr_grad(0 / 1 / 2), tr_eval, tr_hvp, tr_hvp_cached at theta != theta_old (exact Hessian, every R-operator term live) --
are compared with the FLOAT64 evaluation of the oracle (oracle.trust_region.CPOOracle(dtype=torch.float64): torch autograd, double
backward for the products).  Bars: the fused tests' 3e-5 (gradients) / 1e-4 (products) of the vector's largest entry, or twice the
distance of the fp32 oracle's own autograd result from the float64 one on that case where that is larger -- the reference's own
rounding is the yardstick (tests/test_gpu_trust.py), never the device's.  tr_eval: 1e-4 relative + 1e-6 or twice that distance.
The evaluation theta is kept off the kinks of relu (KINK_MARGIN below: what that is about and what was measured without it).

test_learn_through_the_split_path runs whole CPO / TRPO-Lag updates on the split, dword-load case against the fp32 oracle with
the bars of tests/test_gpu_trust.py (observed on the full-batch CPO run: Q 3e-3, S 1e-3, R 9e-3 from the oracle, which itself sits
6e-3, 7e-3 and 3e-2 from float64; final parameters 4e-4 from the oracle's, the float64 run 3e-3).

`launch_variants` / `split_ranges` restate the host's launch rule; test_case_table_reaches_every_variant keeps CASES from silently
losing a variant when a threshold moves.

Measured on an MI355X (256 CUs), worst of the three vectors of a kind, relative to the float64 result's largest entry
(ref = fp32 oracle to float64, dev = device to float64; the device adds its split-K partials in float64 and should not sit
farther out than the fp32 reference does, see tests/test_gpu_fullsize.py):

  case                   N   gradients         products          tr_eval (absolute)
                             ref     dev       ref     dev       ref     dev
  ragged               249   2.2e-06 2.6e-06   3.9e-07 7.9e-07   9.4e-08 4.8e-08
  narrow                37   1.4e-06 3.2e-06   1.5e-07 2.4e-07   1.6e-08 3.4e-08
  split2              1025   2.5e-06 1.1e-06   2.5e-07 5.6e-07   3.2e-07 5.9e-08
  split3              2049   1.6e-05 1.7e-06   7.1e-07 6.0e-07   4.0e-07 4.6e-08
  split3_ragged       2049   3.0e-06 1.3e-06   6.0e-07 7.3e-07   2.3e-07 7.3e-08
  one_row_range      16385   2.5e-06 6.3e-07   2.6e-06 1.4e-07   1.5e-07 5.0e-08
  empty_range        24600   4.3e-06 1.2e-06   2.8e-06 1.1e-07   3.1e-07 9.1e-08
  nw_w2               1100   1.0e-06 1.0e-06   1.1e-06 9.0e-07   1.7e-07 1.1e-08
  nw_w1_fx2           3100   2.0e-06 1.8e-06   1.9e-06 7.9e-07   7.3e-08 6.8e-08
  nw_fx1              4200   2.4e-06 2.4e-06   2.7e-06 8.2e-07   7.5e-08 7.3e-08
  nw_w2_ragged        1100   1.9e-06 1.6e-06   9.2e-07 8.1e-07   5.6e-08 6.5e-08
  nw_w1_fx2_ragged    3100   2.9e-06 3.6e-06   2.8e-06 8.8e-07   8.7e-08 9.5e-08
  nw_fx1_ragged      33000   5.3e-06 7.4e-07   5.6e-06 1.3e-07   2.3e-08 2.0e-08
  eight_layers         300   2.0e-06 1.3e-06   1.1e-07 5.6e-07   4.0e-08 2.4e-08
  width_4096           200   2.1e-06 2.9e-06   4.7e-07 1.0e-06   1.1e-07 4.2e-08
"""
import numpy as np
import pytest
import torch

from test_gpu_shapes import _synthetic

pytestmark = pytest.mark.gpu

LIN_F, LIN_X, LIN_W = "LIN_F", "LIN_X", "LIN_W"
KSPLIT_MAX, DOW, HEAD_LEN = 24, 32, 16        # LAY_KSPLIT_MAX; FSRL_DOW floats per head-gradient row, 16 of them readable (a_len)


def _round_up(a, b):
    return (a + b - 1) // b * b


def split_ranges(rows):
    """host_layered.inc lay_wgrad_k + kernels_layered.hpp lin_kernel: the (first row, row count) of every split-K range of a
    full-batch weight-side launch over `rows` batch rows"""
    ks = max(1, min(KSPLIT_MAX, (rows + 1023) // 1024))
    kchunk = _round_up((rows + ks - 1) // ks, 64)
    out = []
    for s in range(ks):
        kb = min(s * kchunk, rows)
        out.append((kb, min(rows - kb, kchunk)))
    return out


def _vec_ok(ld, length):
    """lay_vec_ok for an operand whose base is 16-byte aligned (every tensor of the parameter vector starts on 256 bytes, every
    working-set buffer on a multiple of 64 floats, observation rows on a multiple of obs_dim floats)"""
    return length <= 0 or (ld % 4 == 0 and length % 4 == 0)


def _launch(form, jobs, ks, n_cus):
    """lay_launch: jobs = [(M, N, K, lda, a_len, ldb)] -> (form, vec, nw, split)"""
    vec, wgs = True, 0
    for M, N, K, lda, a_len, ldb in jobs:
        la = a_len if a_len else (M if form == LIN_W else K)
        lb = K if form == LIN_F else N
        vec = vec and _vec_ok(lda, la) and _vec_ok(ldb, lb if N > 0 else 0)
        wgs += max(1, (N + 63) // 64) * ((M + 63) // 64) * ks
    nw = 4 if wgs <= 2 * n_cus else (2 if wgs <= 4 * n_cus else 1)
    return (form, vec, nw, ks > 1)


def launch_variants(Do, Da, hidden, rows, n_cus, nets=1, split=True):
    """The lin_kernel instantiations one pass of `nets` networks over `rows` rows starts: forward (lay_fwd_k; the R-forward of
    lay_hvp has the same shapes, one job per launch), activation side of the backward pass (lay_bwd_dz_k; the R-backward alike),
    and the one weight-side launch (lay_wgrad_k), split as the full-batch callers ask for it.  nets = 1: the actor alone (head
    Da wide, plus the sigma_param job); 2: the two critics (heads one wide)."""
    L = len(hidden)
    head = Da if nets == 1 else 1
    ins = [Do] + list(hidden)
    outs = list(hidden) + [head]
    seen = set()
    for l in range(L + 1):                                    # Z_l = A W_l^T: A rows x in, W out x in
        seen.add(_launch(LIN_F, [(rows, outs[l], ins[l], ins[l], 0, ins[l])] * nets, 1, n_cus))
    for l in range(L - 1, -1, -1):                            # dZ_l = dZ_{l+1} W_{l+1}: the Linear above hidden layer l
        up_in, up_out = ins[l + 1], outs[l + 1]
        top = l == L - 1
        seen.add(_launch(LIN_X, [(rows, up_in, up_out, DOW if top else up_out, HEAD_LEN if top else 0, up_in)] * nets, 1, n_cus))
    jobs = []
    for _ in range(nets):
        for l in range(L + 1):                                # dW_l = dZ_l^T A_{l-1}: M = out, N = in, K = the batch rows
            jobs.append((outs[l], ins[l], rows, outs[l] if l < L else DOW, 0 if l < L else HEAD_LEN, ins[l]))
        if nets == 1:
            jobs.append((Da, 0, rows, DOW, HEAD_LEN, Do))     # sigma_param: column sums only
    seen.add(_launch(LIN_W, jobs, len(split_ranges(rows)) if split else 1, n_cus))
    return seen


def _spread(n, envs):
    """n rows over `envs` ragged sub-buffers"""
    if envs == 3:
        a, b = n // 2, n // 3
        return [a, b, n - a - b]
    return [n // envs + (1 if e < n % envs else 0) for e in range(envs)]


WIDE = (1024, 1024)
CASES = {  # obs, act, hidden, rows per env, unbounded
    # dword loads everywhere: first layer, middle layers and head off the float4 path; then layers narrower than 4, one of width 1
    "ragged": (17, 3, (33, 50, 7), [130, 99, 20], True),
    "narrow": (5, 2, (3, 1, 2), [37], False),
    # the first split ranges: ks = 2 (second range 449 rows) and ks = 3; a twin that is split and off the float4 path at once
    "split2": (8, 2, (48, 64, 40), _spread(1025, 3), False),
    "split3": (8, 2, (48, 64, 40), _spread(2049, 3), False),
    "split3_ragged": (8, 2, (45, 62, 39), _spread(2049, 3), False),
    # a last range of ONE row (ks = 17, kchunk = 1024) and an EMPTY last range (ks = 24, kchunk = 1088, 23 x 1088 >= N)
    "one_row_range": (6, 2, (20, 12), _spread(16385, 20), False),
    "empty_range": (6, 2, (20, 12), _spread(24600, 20), False),
    # 8 and 4 waves per workgroup on 256 CUs: LIN_W 289 x ks workgroups, LIN_F / LIN_X 16 x ceil(N / 64)
    "nw_w2": (8, 2, WIDE, _spread(1100, 3), False),            # LIN_W 578 -> NW 2
    "nw_w1_fx2": (8, 2, WIDE, _spread(3100, 3), False),        # LIN_W 1 156 -> NW 1; LIN_F / LIN_X 784 -> NW 2
    "nw_fx1": (8, 2, WIDE, _spread(4200, 4), False),           # LIN_F / LIN_X 1 056 -> NW 1
    "nw_w2_ragged": (8, 2, (1022, 1023), _spread(1100, 3), False),
    "nw_w1_fx2_ragged": (8, 2, (1022, 1023), _spread(3100, 3), False),
    "nw_fx1_ragged": (6, 2, (66, 70), _spread(33000, 20), False),   # two column tiles x 516 row tiles = 1 032 -> NW 1, dword loads
    # the documented limits (include/fsrl_hip.h): FSRL_MAX_HIDDEN layers at the widest observation / action, FSRL_MAX_WIDTH units
    "eight_layers": (128, 16, (24, 17, 32, 9, 40, 4, 28, 12), [300], False),
    "width_4096": (8, 2, (4096, ), [200], False),
}
HVP_CACHE_CASE = "split3_ragged"
LEARN_CASE = "split3_ragged"
# The whole-update test asserts the dual-solve branch and the backtrack count EXACTLY, so it needs inputs on which arithmetic, not
# rounding, decides them: the first data seed from 200 on which the fp32 and the float64 oracle agree on both in every row of the
# full-batch and of the minibatched CPO run (on 200 .. 203 the two oracles themselves part ways by a backtrack or a branch).
LEARN_SEED = 204


def _theta(o, rng):
    """-> (theta, per-entry scale): W ~ N(0, 1 / fan_in) so that no width saturates the tanh head, b ~ 0.1 N(0, 1), sigma_param
    around -0.5"""
    parts, scales = [], []
    for spec in o.specs:
        for name, shape in spec.items():
            n = int(np.prod(shape))
            if name == "sigma_param":
                parts.append(-0.5 + 0.1 * rng.standard_normal(n)); scales.append(np.full(n, 0.1))
            elif name.startswith("W"):
                s = 1.0 / np.sqrt(shape[1])
                parts.append(s * rng.standard_normal(n)); scales.append(np.full(n, s))
            else:
                parts.append(0.1 * rng.standard_normal(n)); scales.append(np.full(n, 0.1))
    return np.concatenate(parts).astype(np.float32), np.concatenate(scales)


# relu' jumps at 0: a hidden pre-activation within fp32 rounding of 0 lets the sign -- and with it one batch row's whole
# contribution to that unit's weight row, 1 / sqrt(N) of it -- fall either way in the fp32 oracle, on the device and in float64.
# With up to 8.6 M (row, unit) pairs per case that is no rare event: on the 1024 x 1024 / N = 3 100 inputs as first drawn, unit 196
# of layer 2 had z = -7.8e-8 in row 1 968, the device's gradient sat 4.4e-4 from float64 with ALL of it in that unit's row
# (cosine 1.000000 with the row's input activations) while the fp32 oracle sat at 2e-6; on another seed of the same shape the
# fp32 oracle was the one 6e-4 out and the device at 1e-6.  A comparison of roundings needs inputs off the kinks: the evaluation
# theta's actor biases are nudged until every hidden pre-activation is at least KINK_MARGIN from 0 in float64 -- five times the
# rounding of a 1 024-term fp32 chain of these magnitudes (sqrt(1024) x 2^-24 x |z| ~ 2e-6), and small against the spacing of
# a unit's pre-activations around 0 even at 33 000 rows (7e-5), so a nudge of a few margins always exists.
KINK_MARGIN = 1e-5


def _off_the_kinks(actor, obs):
    """nudge the biases (float32 views into the flat vector, changed in place) of the actor's hidden layers"""
    h = np.asarray(obs, np.float64)
    n_lin = sum(1 for k in actor if k[0] == "W")
    for l in range(1, n_lin):
        b = actor[f"b{l}"]
        pre = h @ actor[f"W{l}"].astype(np.float64).T
        for j in np.flatnonzero(np.abs(pre + b.astype(np.float64)).min(0) < KINK_MARGIN):
            col = pre[:, j]
            near = col[np.abs(col + float(b[j])) < 8 * KINK_MARGIN]
            cands = np.concatenate([-near + 1.5 * KINK_MARGIN, -near - 1.5 * KINK_MARGIN]).astype(np.float32)
            ok = [c for c in cands[np.argsort(np.abs(cands - b[j]))] if np.abs(col + float(c)).min() >= KINK_MARGIN]
            b[j] = ok[0]
        z = pre + b.astype(np.float64)
        assert np.abs(z).min() >= KINK_MARGIN
        h = np.maximum(z, 0.0)


def _inputs(name, seed=None):
    """-> (rollout columns, OnPolicyData, theta at tr_begin, theta moved away from it, three tangents)"""
    from oracle.ppo_lag import OnPolicyData
    from oracle.trust_region import CPOConfig, CPOOracle
    Do, Da, hidden, rows, unbounded = CASES[name]
    rng = np.random.default_rng(100 + list(CASES).index(name) if seed is None else seed)
    cols = _synthetic(rng, rows, Do, Da, 25 if max(rows) < 400 else 250)
    cat = {k: np.concatenate(v) for k, v in cols.items()}
    end = (cat["term"] | cat["trunc"]).copy(); end[np.cumsum(rows) - 1] = True
    data = OnPolicyData(obs=cat["obs"], act=cat["act"], rew=cat["rew"], cost=cat["cost"], terminated=cat["term"],
                        truncated=cat["trunc"], obs_next=cat["obs_next"], end_flag=end)
    o = CPOOracle(CPOConfig(obs_dim=Do, act_dim=Da, hidden=hidden, unbounded=unbounded))
    theta, scale = _theta(o, rng)
    moved = (theta + 0.1 * scale * rng.standard_normal(theta.size)).astype(np.float32)     # theta != theta_old: exact Hessian
    from oracle import layout
    _off_the_kinks(layout.views(moved, o.specs[0])[0], cat["obs"])
    na = layout.spec_size(o.specs[0])
    vs = [rng.standard_normal(na).astype(np.float32) for _ in range(3)]
    return cols, data, theta, moved, vs


_REF = {}


def _reference(name, data, theta, moved, vs):
    """{dtype: {"grad0", "grad1", "grad2", "eval", "hvp": [3]}} of the oracle's autograd in fp32 and in float64, computed once"""
    if name not in _REF:
        from oracle.trust_region import CPOConfig, CPOOracle
        from torch.distributions import Independent, Normal, kl_divergence
        Do, Da, hidden, rows, unbounded = CASES[name]
        torch.set_num_threads(16)
        out = {}
        for dt in (torch.float32, torch.float64):
            o = CPOOracle(CPOConfig(obs_dim=Do, act_dim=Da, hidden=hidden, unbounded=unbounded), dtype=dt)
            o.set_params(theta)
            pb = o.process(data)
            o.set_params(moved)
            dist = o.actor_dist(pb["obs"])
            ratio = torch.exp(dist.log_prob(pb["act"]) - pb["logp_old"])
            obj = torch.mean(ratio * pb["advs"][..., 0])
            csur = torch.mean(ratio * pb["advs"][..., 1])
            kl = kl_divergence(Independent(Normal(pb["mean_old"], pb["std_old"]), 1), dist).mean()
            r = {"grad0": o.flat_grad(obj, retain_graph=True).numpy().astype(np.float64),
                 "grad1": o.flat_grad(-csur, retain_graph=True).numpy().astype(np.float64),
                 "eval": np.array([obj.item(), csur.item(), kl.item()])}
            klg = o.flat_grad(kl, create_graph=True)
            r["grad2"] = klg.detach().numpy().astype(np.float64)
            r["hvp"] = [o.flat_grad(torch.dot(klg, torch.from_numpy(v).to(dt)), retain_graph=True).numpy().astype(np.float64)
                        for v in vs]
            out[dt] = r
        _REF[name] = out
    return _REF[name]


def _engine(name, cols, **over):
    from fsrl_amd.engine import Engine, EngineConfig
    Do, Da, hidden, rows, unbounded = CASES[name]
    cap = _round_up(max(rows), 64)
    eng = Engine(EngineConfig(obs_dim=Do, act_dim=Da, hidden_sizes=hidden, env_num=len(rows), buffer_size=len(rows) * cap,
                              target_kl=None, max_action=1.0, unbounded=unbounded, **over))
    for t in range(max(rows)):                              # lock-step, envs drop out as they run dry
        ids = [e for e in range(len(rows)) if t < rows[e]]
        eng.push(ids, *[np.stack([cols[k][e][t] for e in ids]) for k in ("obs", "act", "rew", "cost", "term", "trunc",
                                                                         "obs_next")])
    return eng


def _dist(a, b64):
    """max-norm distance relative to the float64 vector's largest entry"""
    return float(np.abs(np.asarray(a, np.float64) - b64).max()) / max(float(np.abs(b64).max()), 1e-12)


@pytest.mark.parametrize("name", list(CASES))
def test_pieces_vs_float64_autograd(name):
    cols, data, theta, moved, vs = _inputs(name)
    Do, Da, hidden, rows, unbounded = CASES[name]
    N = sum(rows)
    ref = _reference(name, data, theta, moved, vs)
    r32, r64 = ref[torch.float32], ref[torch.float64]
    eng = _engine(name, cols)
    eng.set_params(theta)
    assert eng.tr_begin(target_kl=0.01, norm_adv=True, cost_limit=10.0) == N
    eng.set_params(moved)
    report, bad = [], []

    def check(what, got, want32, want64, floor):
        e_ref, e_dev = _dist(want32, want64), _dist(got, want64)
        report.append(f"{what}: ref {e_ref:.1e} dev {e_dev:.1e}")
        if not e_dev <= max(floor, 2.0 * e_ref):
            bad.append((what, e_dev, e_ref))
    for w in range(3):
        check(f"grad{w}", eng.tr_grad(w), r32[f"grad{w}"], r64[f"grad{w}"], 3e-5)
    ev = eng.tr_eval()[:3]
    for j, what in enumerate(("objective", "cost surrogate", "kl")):
        tol = max(1e-4 * abs(r64["eval"][j]) + 1e-6, 2.0 * abs(r32["eval"][j] - r64["eval"][j]))
        report.append(f"{what}: ref {abs(r32['eval'][j] - r64['eval'][j]):.1e} dev {abs(ev[j] - r64['eval'][j]):.1e} (absolute)")
        if not abs(ev[j] - r64["eval"][j]) <= tol:
            bad.append((what, float(ev[j]), float(r32["eval"][j]), float(r64["eval"][j])))
    hv = []
    for k, v in enumerate(vs):
        hv.append(eng.tr_hvp(v))
        check(f"hvp{k}", hv[k], r32["hvp"][k], r64["hvp"][k], 1e-4)
    if name == HVP_CACHE_CASE:
        # the cached product (what conjugate gradients call): the same bits as the uncached one at the same theta; after new
        # parameters the promise is stale and the activations are recomputed
        again = eng.tr_hvp_cached(vs[2])
        check("hvp cached", again, r32["hvp"][2], r64["hvp"][2], 1e-4)
        assert np.array_equal(again, hv[2])
        assert np.array_equal(eng.tr_hvp_cached(vs[0]), hv[0])
        eng.set_params(theta)
        stale = eng.tr_hvp_cached(vs[0])
        fresh = eng.tr_hvp(vs[0])
        assert np.array_equal(stale, fresh) and not np.array_equal(stale, hv[0])
    print(f"\n{name} N={N}: " + "; ".join(report))
    eng.close()
    assert not bad, (bad, report)


def test_one_row_and_empty_last_range():
    """the two range cases are what their names say, by the mirrored rule"""
    r = split_ranges(sum(CASES["one_row_range"][3]))
    assert len(r) == 17 and r[-1] == (16384, 1) and all(n == 1024 for _, n in r[:-1])
    r = split_ranges(sum(CASES["empty_range"][3]))
    assert len(r) == 24 and r[-1][1] == 0 and r[-2][1] > 0 and sum(n for _, n in r) == 24600
    assert [n for _, n in split_ranges(1025)] == [576, 449] and len(split_ranges(2049)) == 3


def test_case_table_reaches_every_variant():
    """On this device's CU count the pieces of CASES start every lin_kernel<FORM, VEC, NW> instantiation, the split weight side
    with and without float4 loads, a one-row and an empty split range."""
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    seen = set()
    for Do, Da, hidden, rows, _ in CASES.values():
        seen |= launch_variants(Do, Da, hidden, sum(rows), n_cus)
    want = {(f, v, nw) for f in (LIN_F, LIN_X, LIN_W) for v in (True, False) for nw in (4, 2, 1)}
    have = {s[:3] for s in seen}
    assert len(want) == 18 and want <= have, sorted(want - have)
    assert {v for f, v, nw, split in seen if f == LIN_W and split} == {True, False}
    assert not any(split for f, v, nw, split in seen if f != LIN_W)
    last = [split_ranges(sum(c[3]))[-1][1] for c in CASES.values()]
    assert 1 in last and 0 in last
    # the whole updates of test_learn_through_the_split_path: the critics' launch (two networks) is split and off the float4 path
    Do, Da, hidden, rows, _ = CASES[LEARN_CASE]
    assert (LIN_W, False, 4, True) in launch_variants(Do, Da, hidden, sum(rows), n_cus, nets=2)


CPO_KEYS = ["loss/kl", "loss/entropy", "loss/rew_loss", "loss/cost_loss", "loss/optim_A", "loss/optim_B",
            "loss/optim_C", "loss/optim_Q", "loss/optim_R", "loss/optim_S", "loss/optim_lam",
            "loss/optim_nu", "loss/optim_case", "loss/step_size", "loss/vf0", "loss/vf1", "loss/vf_total"]
TRPO_KEYS = ["loss/rescaling", "loss/lagrangian", "loss/actor_safety", "loss/actor_rew", "loss/actor_total",
             "loss/vf0", "loss/vf1", "loss/vf_total", "loss/kl", "loss/step_size", "loss/entropy"]
CPO_TIGHT = ("loss/vf0", "loss/vf1", "loss/vf_total", "loss/entropy", "loss/cost_loss", "loss/optim_C")
TRPO_TIGHT = ("loss/vf0", "loss/vf1", "loss/vf_total")


def _first_row(keys, tight, loose, got, want, want64):
    """test_gpu_trust.test_cpo_learn_vs_golden's bars on the first logged row: the critic losses (and what else is upstream of
    conjugate gradients) at 2e-5, the rest at `loose` or twice the fp32 reference's own distance from the float64 run"""
    for j, k in enumerate(keys):
        scale = max(abs(want[j]), 1e-3)
        tol = 2e-5 * scale if k in tight else max(loose * scale, 2.0 * abs(want[j] - want64[j]))
        print(f"{k}: dev {got[j]:.7g} ref {want[j]:.7g} float64 {want64[j]:.7g}")
        assert abs(got[j] - want[j]) <= tol + 1e-6, (k, float(got[j]), float(want[j]), float(want64[j]))


def _theta_bars(th, th32, th64, floor_max, floor_mean):
    ref_err = np.abs(th64 - th32)          # how far exact arithmetic lands from the fp32 reference after all repeats
    d = np.abs(th - th32)
    print("theta: dev max / mean", d.max(), d.mean(), " ref max / mean", ref_err.max(), ref_err.mean())
    assert d.max() <= max(floor_max, 2.0 * ref_err.max()) and d.mean() <= max(floor_mean, 2.0 * ref_err.mean()), \
        (d.max(), d.mean(), ref_err.max(), ref_err.mean())


@pytest.mark.parametrize("which", ["cpo", "trpo", "cpo_minibatch"])
def test_learn_through_the_split_path(which):
    """Whole updates on hidden (45, 62, 39), N = 2 049 (three split ranges, dword loads): cpo_learn and trpo_learn for two repeats,
    and cpo_learn in minibatches of 700 / 1 349 rows (the second one split in two), against the fp32 oracle with the assertions of
    tests/test_gpu_trust.py -- the critics' split partials through adam_range_kernel, conjugate gradients over cg_pz_kernel
    with more than one partial."""
    from oracle.trust_region import CPOConfig, CPOOracle, TRPOConfig, TRPOLagOracle
    torch.set_num_threads(4)
    cols, data, theta, _, _ = _inputs(LEARN_CASE, LEARN_SEED)
    Do, Da, hidden, rows, unbounded = CASES[LEARN_CASE]
    N, repeat = sum(rows), 2
    eng = _engine(LEARN_CASE, cols)
    eng.set_params(theta); eng.optim_reset()
    if which == "trpo":
        mk = lambda dt: TRPOLagOracle(TRPOConfig(obs_dim=Do, act_dim=Da, hidden=hidden, optim_critic_iters=3), dtype=dt)  # noqa: E731
        run = lambda o: o.update(data, [0.75], 1 / 1.75, repeat)[1]  # noqa: E731
        assert eng.tr_begin(target_kl=0.001, critic_lr=5e-4, max_backtracks=10, optim_critic_iters=3) == N
        stats = eng.trpo_learn([0.75], 1 / 1.75, repeat)
        keys, row = TRPO_KEYS, (lambda r: r[0])
    else:
        perms = [np.random.default_rng(9 + k).permutation(N) for k in range(repeat)] if which == "cpo_minibatch" else None
        B = 700 if which == "cpo_minibatch" else 99999
        mk = lambda dt: CPOOracle(CPOConfig(obs_dim=Do, act_dim=Da, hidden=hidden, optim_critic_iters=3, max_backtracks=10,  # noqa: E731
                                            cost_limit=10.0, l2_reg=0.001, target_kl=0.01), dtype=dt)
        run = lambda o: o.update(data, 25.0, repeat, perms=perms, batch_size=B)[1]  # noqa: E731
        assert eng.tr_begin(target_kl=0.01, l2_reg=0.001, critic_lr=1e-3, max_backtracks=10, optim_critic_iters=3,
                            cost_limit=10.0) == N
        stats = eng.cpo_learn(25.0, repeat, batch_size=B, perms=perms) if perms else eng.cpo_learn(25.0, repeat)
        keys, row = CPO_KEYS, (lambda r: {**r[0], **r[1]})
    o32, o64 = mk(torch.float32), mk(torch.float64)
    o32.set_params(theta); o64.set_params(theta)
    want = np.array([[float(row(r)[k]) for k in keys] for r in run(o32)])
    want64 = np.array([[float(row(r)[k]) for k in keys] for r in run(o64)])
    print("\ndev", stats, "\nref", want, "\nfloat64", want64)
    assert stats.shape == want.shape == (repeat * (2 if which == "cpo_minibatch" else 1), len(keys))
    si = keys.index("loss/step_size")
    if which == "trpo":
        _first_row(keys, TRPO_TIGHT, 2e-3, stats[0], want[0], want64[0])
        np.testing.assert_allclose(stats, want, rtol=5e-2, atol=2e-3)
        _theta_bars(eng.get_params(), o32.get_params(), o64.get_params(), 1.5e-3, 1e-5)
    else:
        ci = keys.index("loss/optim_case")
        assert np.array_equal(stats[:, ci], want[:, ci])                  # same branch of the dual solve
        np.testing.assert_allclose(stats[0, si], want[0, si], rtol=1e-6)  # same number of backtracks
        for r in range(1, len(stats)):                                    # later rows: the line search may flip at its boundary
            k = np.log(stats[r, si] / want[r, si]) / np.log(0.8)
            assert abs(k) <= (1.05 if r == 1 and which == "cpo" else 4.05), (stats[:, si], want[:, si])
        _first_row(keys, CPO_TIGHT, 8e-3, stats[0], want[0], want64[0])
        if which == "cpo_minibatch":                                      # the critics see the right rows in every minibatch
            np.testing.assert_allclose(stats[:, 14:], want[:, 14:], rtol=2e-4, atol=1e-5)
        _theta_bars(eng.get_params(), o32.get_params(), o64.get_params(), 3e-3, 5e-5)
    eng.close()
