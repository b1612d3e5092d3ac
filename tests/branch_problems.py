"""Problems that put chosen shares of their rows into every branch of the hand-written loss heads, and prove it.

Each constructor returns the inputs of a comparison plus a CENSUS taken with the float64 oracle: how many rows of the compared
minibatch (or batch) sit in each branch, and the smallest relative distance of any row from any branch boundary.
tests/test_branch_problems_host.py asserts the conditions below for every case on the CPU; the GPU tests
(test_gpu_ppo_branches.py, test_gpu_replay_branches.py) build their inputs here and repeat the assertion, so a case cannot
degenerate unnoticed.

  * every branch a case claims holds at least MIN_SHARE of the rows and at least MIN_ROWS rows;
  * no row is closer than MIN_MARGIN (relative) to a boundary: ratio vs 1 - eps, 1 + eps and dual_clip; |v - v_old| vs eps and
    (ret - v)^2 vs (ret - v_clip)^2 on the clamped rows; raw log sigma vs -20 and 2; variance vs 1e-6.

These are conditions, not measurements: seeds and perturbation sizes were picked on the CPU so that they hold."""
import numpy as np
import torch

MIN_SHARE, MIN_ROWS, MIN_MARGIN = 0.02, 3, 1e-3


def check_census(census, margin, claimed, what=""):
    """the conditions of the module docstring; census: branch -> rows, claimed: the branches the case must populate"""
    for group in claimed:
        tot = sum(census[k] for k in group)
        for k in group:
            assert census[k] >= MIN_ROWS and census[k] >= MIN_SHARE * tot, (what, k, census[k], tot)
    assert margin >= MIN_MARGIN, (what, "margin", margin)


def census_line(name, census, margin):
    return f"{name:28s} " + " ".join(f"{k}={v}" for k, v in census.items()) + f"  margin {margin:.2e}"


# ------------------------------------------------------------------------------------------------ on-policy head (PPO-Lag)
POLICY_BRANCHES = ("in+", "in-", "hi+", "hi-", "lo+", "lo-", "dual")   # ratio inside / above / below 1 +- eps x sign of the advantage;
VALUE_BRANCHES = ("v_in", "v_clamp_raw", "v_clamp_clip")                # dual: ratio > dual_clip with a negative advantage (hi- excludes it)
#                                                                        v_clamp_raw: clamped and (ret - v)^2 wins; v_clamp_clip: clamped and the
#                                                                        clipped square wins (no gradient)

# Do, Da, hidden, rows per env, batch, s / sv (theta = theta_old (1 + s N) + 0.01 N; sv: the critics' s), options.  The compared
# minibatch is the LAST chunk of the pass: the remainder merged into a batch, so never a multiple of the batch.  The tile height of
# the forward / backward launch that chunk takes on a 256-CU device (host_ppo.inc): 4 rows while 12 * ceil(rows / 16) <= CUs, 8 while
# 6 * ... <= CUs, else 16, with 32-row tiles in front at 128 / 256 wide where ppo_set_plan asks or 3 * ceil(rows / 16) > CUs.
PPO_CASES = {
    # 4-row tiles at 64 wide, last chunk 215 rows (no multiple of 16, nor of 4)
    "w64_dual_vclip": dict(Do=9, Da=6, hidden=(64, 64), rows=[180, 163], B=128, s=0.12, sv=0.5, dual_clip=1.5, value_clip=True),
    # 8-row tiles at 128 wide (chunk of 389 rows), one action column, raw advantages (zero-mean rewards: both signs), no dual clip
    "w128_da1_rawadv_vclip": dict(Do=17, Da=1, hidden=(128, 128), rows=[350, 339], B=300, s=0.3, sv=0.3, value_clip=True,
                                  norm_adv=False, rew_mean=0.0),
    # 256 wide, all 16 action columns, unbounded head, no value clip, gradient-norm clip on; chunk of 203 rows: 4-row tiles
    "w256_da16_unbounded_dual": dict(Do=12, Da=16, hidden=(256, 256), rows=[170, 161], B=128, s=0.08, dual_clip=1.5, unbounded=True,
                                     max_grad_norm=0.5),
    # 16-row tiles and, with ppo_set_plan(8), eight 32-row tiles in front of them: a chunk of 717 rows at 128 wide; no Lagrangian term
    "w128_tall_dual_vclip_nolag": dict(Do=8, Da=6, hidden=(128, 128), rows=[600, 517], B=400, s=0.12, sv=0.5, dual_clip=1.5,
                                       value_clip=True, use_lag=False, plans=(0, 8)),
    # the size at which the automatic plan takes 32-row tiles (3 x 100 sixteen-row tiles > 256 CUs): a chunk of 1 607 rows at 256 wide
    "w256_auto_tall_dual_vclip": dict(Do=8, Da=6, hidden=(256, 256), rows=[1500, 1507], B=1400, s=0.12, sv=0.5, dual_clip=1.5,
                                      value_clip=True, max_grad_norm=0.5),
    # the layered twin of the head (kernels_layered.hpp), ragged widths, chunk of 253 rows
    "layered_dual_vclip": dict(Do=7, Da=6, hidden=(40, 72, 24), rows=[127, 125, 129], B=128, s=0.12, sv=0.5, dual_clip=1.5,
                               value_clip=True),
}
RET_RMS0 = np.array([[0.4, 2.0, 200.0], [0.1, 0.6, 200.0]])      # preset running return statistics (value clip needs reward normalisation)


def _rollout(seed, rows, Do, Da, ep=40, rew_mean=0.5):
    """rows in push order per env + the same rows env-major with the oracle's end flags"""
    from oracle.ppo_lag import OnPolicyData
    rng = np.random.default_rng(seed)
    cols = {k: [] for k in ("obs", "act", "rew", "cost", "term", "trunc", "obs_next")}
    for T in rows:
        obs = rng.standard_normal((T + 1, Do)).astype(np.float32)
        act = (0.3 * rng.standard_normal((T, Da))).astype(np.float32)
        rew = rng.normal(rew_mean, 0.5, T)
        cost = (rng.random(T) < 0.2).astype(np.float64)
        trunc = np.zeros(T, bool); trunc[ep - 1::ep] = True
        term = np.zeros(T, bool); term[T // 2] = True
        for k, v in zip(cols, (obs[:-1], act, rew, cost, term, trunc, obs[1:])):
            cols[k].append(v)
    cat = {k: np.concatenate(v) for k, v in cols.items()}
    end = (cat["term"] | cat["trunc"]).copy()
    end[np.cumsum(rows) - 1] = True
    data = OnPolicyData(obs=cat["obs"], act=cat["act"], rew=cat["rew"], cost=cat["cost"], terminated=cat["term"],
                        truncated=cat["trunc"], obs_next=cat["obs_next"], end_flag=end)
    return cols, data


def ppo_config(c):
    from oracle.ppo_lag import PPOLagConfig
    vclip = bool(c.get("value_clip"))
    return PPOLagConfig(obs_dim=c["Do"], act_dim=c["Da"], hidden=tuple(c["hidden"]), max_action=1.2, eps_clip=0.2,
                        dual_clip=c.get("dual_clip"), max_grad_norm=c.get("max_grad_norm"), target_kl=1e9,
                        advantage_normalization=c.get("norm_adv", True), use_lagrangian=c.get("use_lag", True), lr=0.0,
                        unbounded=bool(c.get("unbounded")), reward_normalization=vclip, value_clip=vclip)


def _theta_old(o, seed):
    rng = np.random.default_rng(seed)
    parts = []
    for net in o.nets:
        for k, t in net.items():
            if k == "sigma_param":
                parts.append(-0.5 + 0.1 * rng.standard_normal(t.shape))
            elif t.ndim == 2:
                parts.append(rng.standard_normal(t.shape) / np.sqrt(t.shape[1]))
            else:
                parts.append(0.05 * rng.standard_normal(t.shape))
    return np.concatenate([p.reshape(-1) for p in parts]).astype(np.float32)


def _ppo_processed(cfg, dtype, data, theta_old, theta):
    """an oracle in `dtype` with process() run at theta_old and the parameters then set to theta"""
    from oracle.ppo_lag import PPOLagOracle
    o = PPOLagOracle(cfg, dtype=dtype)
    o.set_params(theta_old)
    if cfg.reward_normalization:
        o.ret_rms[:] = RET_RMS0
    pb = o.process(data)
    o.set_params(theta)
    return o, pb


def _ppo_reference(o, pb, chunk, lag, resc):
    """the minibatch's losses and their gradient at the oracle's parameters"""
    loss, _, st = o._minibatch_losses(pb, chunk, lag, resc)
    grads = torch.autograd.grad(loss, o._leaves)
    g = torch.cat([t.reshape(-1) for t in grads]).numpy().astype(np.float64)
    row = np.array([st["loss/actor_rew"], st.get("loss/actor_safety", 0.0), st["loss/kl"], st["loss/vf0"], st["loss/vf1"]])
    return g, row


ROW_KEYS = ("loss/actor_rew", "loss/actor_safety", "loss/kl", "loss/vf0", "loss/vf1")
ROW_COLS = (3, 2, 5, 6, 7)            # their columns in the device's logged row (oracle.ppo_lag.STAT_KEYS)


def ppo_row_state(o, pb):
    """per row of the whole batch at the oracle's current parameters (float64 oracle): ratio, per critic (v - v_old, (ret - v)^2,
    (ret - v_clip)^2), and the row's relative distance from the nearest branch boundary"""
    cfg = o.cfg
    eps = cfg.eps_clip
    with torch.no_grad():
        ratio = (o.actor_dist(pb["obs"]).log_prob(pb["act"]) - pb["logp_old"]).exp().numpy()
        bounds = [1 - eps, 1 + eps] + ([cfg.dual_clip] if cfg.dual_clip else [])
        margin = np.min([np.abs(ratio / b - 1) for b in bounds], 0)
        vals = []
        for i in range(cfg.n_critics if cfg.value_clip else 0):
            v, vo, ret = o.value(i, pb["obs"]).numpy(), pb["values"][:, i].numpy(), pb["rets"][:, i].numpy()
            dv = v - vo
            raw, clip = (ret - v)**2, (ret - (vo + np.clip(dv, -eps, eps)))**2
            vals.append((dv, raw, clip))
            clamped = np.abs(dv) > eps
            margin = np.minimum(margin, np.abs(np.abs(dv) / eps - 1))
            margin = np.where(clamped, np.minimum(margin, np.abs(raw / np.where(clamped, clip, 1.0) - 1)), margin)
    return ratio, vals, margin


def ppo_census(o, pb, chunk):
    """branch populations of the minibatch `chunk` at the float64 oracle's current parameters, and the chunk's smallest margin"""
    cfg = o.cfg
    eps = cfg.eps_clip
    ratio, vals, margin = ppo_row_state(o, pb)
    ratio = ratio[chunk]
    adv = pb["advs"][torch.as_tensor(chunk, dtype=torch.long)][:, 0].numpy()
    if cfg.advantage_normalization:                   # per minibatch, as _minibatch_losses does: the sign is that of a - mean
        adv = adv - adv.mean()
    # (no margin on the advantage's sign: every branch's term and gradient carry the factor A, so they are continuous at A = 0)
    dual = cfg.dual_clip or np.inf
    pos = adv > 0
    hi, lo = ratio > 1 + eps, ratio < 1 - eps
    census = {"in+": int((~hi & ~lo & pos).sum()), "in-": int((~hi & ~lo & ~pos).sum()),
              "hi+": int((hi & pos).sum()), "hi-": int((hi & ~pos & (ratio <= dual)).sum()),
              "lo+": int((lo & pos).sum()), "lo-": int((lo & ~pos).sum()), "dual": int((~pos & (ratio > dual)).sum())}
    for i, (dv, raw, clip) in enumerate(vals):
        dv, raw, clip = dv[chunk], raw[chunk], clip[chunk]
        clamped = np.abs(dv) > eps
        for k, m in (("v_in", ~clamped), ("v_clamp_raw", clamped & (raw > clip)), ("v_clamp_clip", clamped & (raw <= clip))):
            census[f"{k}{i}"] = int(m.sum())
    return census, float(margin[chunk].min())


def ppo_claims(c):
    """the branch groups a case must populate: every policy branch its options leave reachable, every value branch per critic"""
    pol = [b for b in POLICY_BRANCHES if b != "dual" or c.get("dual_clip")]
    out = [pol]
    if c.get("value_clip"):
        out += [[f"{b}{i}" for b in VALUE_BRANCHES] for i in range(2)]
    return out


def ppo_bars(p):
    """the project's bars on a problem's float64 reference: per gradient entry (the existing gradient tests': rtol 1e-4, atol 2e-6
    max(1, max |g|)) and per logged entry (test_full_update_vs_golden's: 2e-5 rel + 2e-5 abs)"""
    g, row = p["g64"], p["row64"]
    return 1e-4 * np.abs(g) + 2e-6 * max(1.0, float(np.abs(g).max())), 2e-5 * np.abs(row) + 2e-5


def ppo_oracle_distance(p):
    """the fp32 oracle's distance from its float64 run in units of those bars: (worst gradient entry, worst logged entry)"""
    gbar, rbar = ppo_bars(p)
    return float((np.abs(p["g32"] - p["g64"]) / gbar).max()), float((np.abs(p["row32"] - p["row64"]) / rbar).max())


SAFE_MARGIN = 2e-3       # rows closer than this to a boundary are kept out of the compared minibatch


def ppo_problem(name):
    """-> dict: the case, rollout (`cols` per env in push order, `data` env-major), theta_old, theta, the permutation and its last
    chunk, lagrangian / rescaling, the float64 reference (gradient `g64`, logged entries `row64`), the fp32 oracle's (`g32`,
    `row32`), and the float64 census of the chunk (`census`, `margin`).  The permutation is a random one in which the few rows within
    SAFE_MARGIN of a boundary come first, so that they land in an earlier minibatch than the compared one."""
    from oracle.ppo_lag import PPOLagOracle, split_chunks
    torch.set_num_threads(4)
    c = PPO_CASES[name]
    seed = 1000 + 7 * c["Do"] + c["Da"] + c.get("seed", 0)
    cols, data = _rollout(seed, c["rows"], c["Do"], c["Da"], rew_mean=c.get("rew_mean", 0.5))
    N = len(data)
    cfg = ppo_config(c)
    rng = np.random.default_rng(seed + 2)
    o = PPOLagOracle(cfg)
    theta_old = _theta_old(o, seed + 1)
    n_actor = sum(t.numel() for t in o.nets[0].values())
    s = np.where(np.arange(theta_old.size) < n_actor, c["s"], c.get("sv", c["s"]))
    theta = (theta_old * (1 + s * rng.standard_normal(theta_old.size)) + 0.01 * rng.standard_normal(theta_old.size))
    theta = theta.astype(np.float32)
    lag, resc = np.array([0.6]), (1 / 1.6 if c.get("use_lag", True) else 1.0)
    o64, pb64 = _ppo_processed(cfg, torch.float64, data, theta_old, theta)
    o32, pb32 = _ppo_processed(cfg, torch.float32, data, theta_old, theta)
    near = ppo_row_state(o64, pb64)[2] < SAFE_MARGIN
    perm = rng.permutation(N)
    perm = np.concatenate([perm[near[perm]], perm[~near[perm]]])
    chunks = split_chunks(N, c["B"], perm)
    chunk = chunks[-1]
    g64, row64 = _ppo_reference(o64, pb64, chunk, lag, resc)
    g32, row32 = _ppo_reference(o32, pb32, chunk, lag, resc)
    census, margin = ppo_census(o64, pb64, chunk)
    census["_near"] = int(near.sum())
    return dict(case=c, cfg=cfg, cols=cols, data=data, theta_old=theta_old, theta=theta, perm=perm, chunk=chunk, lag=lag, resc=resc,
                g64=g64, row64=row64, g32=g32, row32=row32, census=census, margin=margin, n_steps=len(chunks))


# ------------------------------------------------------------------------------------------------ replay heads
# Caller-RNG mode: the sampled indices and the noise are test inputs.  An actor is built whose chosen action columns sit in chosen
# regimes, every other column stays ordinary (fan-in scaled, log sigma around -1 so that no sample reaches the tails of tanh):
#   "upper"     W_sig row doubled, b_sig such that the stored rows' median raw log sigma is 2: the sampled rows straddle the upper clamp
#               (at s_t and s_t+n);
#               the column's noise is scaled by 0.05 so that sigma = e^2 does not throw u into tanh's transition band
#   "lower"     W_sig row 0, b_sig = -25 (every row below the lower clamp: sigma = e^-20, no gradient into the row); W_mu row 0, b_mu 0
#               and NO noise on the column: under sigma = e^-20 a non-zero mean makes u - mu cancel in float32, and non-zero noise sends
#               -+(u - mu) / sigma^2 = 5e8 eps through autograd's float32 sums, which absorbs the column's Q gradient before it cancels
#               (the fp32 oracle's gradient of that mean is then 0 or rounding noise); the mask's row still carries -c * pass
#   "sat+/-"    W_mu row 0, b_mu = +-14, W_sig row 0, b_sig = -3: |u| >= 12 for every sample, tanh(u) = +-1 exactly in float32, so
#               1 - a^2 = 0 and no gradient reaches the W_mu / b_mu row (SAC-Lag: dL/du = 0; DDPG-Lag: 1 - th^2 = 0)
#   "smallvar"  (CVPO) W_sig row 0, b_sig = -8.1 against -8 in the old actor: sigma^2 = 9e-8 < 1e-6 with log sigma INSIDE the clamp --
#               gaussian_kl's clamp_min masks the KL-sigma term while the likelihood term still moves the row
# The indices of every update are drawn among the stored rows whose raw log sigma (float64 oracle, current actor, at s_t and at
# s_t+n) is at least SAFE_MARGIN away from both clamps.  Batches <= 128 rows, stores <= 200 rows.
SUB = 256
ZERO = {0: "lower", 1: "sat+", 2: "sat-"}          # column 3: ordinary
REPLAY_CASES = {
    "sac": {   # exact-zero regimes: one update; mixed upper clamp: three
        "h64_zero": dict(Do=7, Da=4, hidden=(64, 64), rows=[100, 90], B=48, regimes=ZERO, updates=1),
        "h64_mixed": dict(Do=7, Da=4, hidden=(64, 64), rows=[100, 90], B=48, regimes={1: "upper"}, updates=3),
        "h256_zero": dict(Do=7, Da=4, hidden=(256, 256), rows=[100, 90], B=100, regimes=ZERO, updates=1),
        "h256_mixed": dict(Do=7, Da=4, hidden=(256, 256), rows=[100, 90], B=100, regimes={3: "upper"}, updates=3, upper_q=0.75),
        # split-K weight gradients forced at a batch under 512 rows (sac_set_plan(1))
        "splitk_zero": dict(Do=7, Da=4, hidden=(128, 128), rows=[100, 90], B=72, regimes=ZERO, updates=1, plan=1),
        "splitk_mixed": dict(Do=7, Da=4, hidden=(128, 128), rows=[100, 90], B=72, regimes={0: "upper"}, updates=3, plan=1),
        "layered_zero": dict(Do=7, Da=4, hidden=(48, 40, 24), rows=[100, 90], B=48, regimes=ZERO, updates=1),
        "layered_mixed": dict(Do=7, Da=4, hidden=(48, 40, 24), rows=[100, 90], B=48, regimes={2: "upper"}, updates=3),
    },
    "ddpg": {
        "h64_sat": dict(Do=7, Da=4, hidden=(64, 64), rows=[100, 90], B=48, regimes={1: "sat+", 2: "sat-"}, updates=1),
        "layered_sat": dict(Do=7, Da=4, hidden=(48, 40, 24), rows=[100, 90], B=48, regimes={0: "sat-", 3: "sat+"}, updates=1),
    },
    "cvpo": {
        "h64_single": dict(Do=7, Da=4, hidden=(64, 64), rows=[100, 90], B=48, K=4, regimes={0: "lower", 2: "smallvar"}, updates=1),
        "h64_double": dict(Do=7, Da=4, hidden=(64, 64), rows=[100, 90], B=48, K=6, double=True, regimes={1: "lower", 3: "smallvar"},
                           updates=1),
        "layered_single": dict(Do=7, Da=4, hidden=(48, 40, 24), rows=[100, 90], B=48, K=4, regimes={0: "smallvar", 3: "lower"},
                               updates=1),
    },
}


def head_slices(spec):
    """name -> slice of the flat vector, for a parameter spec (name -> shape)"""
    out, off = {}, 0
    for k, shp in spec.items():
        n = int(np.prod(shp))
        out[k] = (slice(off, off + n), shp)
        off += n
    return out


def head_rows(kind, spec, col):
    """flat indices of the mean head's row of action column `col` (weights and bias) and of the log-sigma head's"""
    sl = head_slices(spec)
    def row(wk, bk):
        (ws, shp), (bs, _) = sl[wk], sl[bk]
        return np.concatenate([np.arange(ws.start + col * shp[1], ws.start + (col + 1) * shp[1]), [bs.start + col]])
    if kind == "ddpg":
        L = sum(1 for k in spec if k[0] == "W")
        return row(f"W{L}", f"b{L}"), None
    return row("Wmu", "bmu"), row("Wsig", "bsig")


def _set_regimes(kind, theta, spec, regimes, old=False):
    th = theta.copy()
    for col in range(next(iter(reversed(spec.values())))[0]):
        mu_rows, sg_rows = head_rows(kind, spec, col)
        reg = regimes.get(col, "ordinary")
        if sg_rows is not None:
            if reg == "ordinary":
                th[sg_rows[:-1]] *= 0.5; th[sg_rows[-1]] = -1.0 + th[sg_rows[-1]]
            elif reg == "upper":
                th[sg_rows[:-1]] *= 2.0; th[sg_rows[-1]] = 2.0
            else:
                th[sg_rows[:-1]] = 0.0
                th[sg_rows[-1]] = {"lower": -25.0, "smallvar": -8.0 if old else -8.1}.get(reg, -3.0)
        if reg in ("lower", "sat+", "sat-"):
            th[mu_rows[:-1]] = 0.0
            th[mu_rows[-1]] = {"lower": 0.0, "sat+": 14.0, "sat-": -14.0}[reg]
    return th


def _noise_scale(regimes, Da):
    return np.array([{"upper": 0.05, "lower": 0.0}.get(regimes.get(d), 0.5) for d in range(Da)], np.float32)


def _heads64(kind, o, params, obs):
    """float64 oracle: raw mean head and raw log sigma head of `params` on obs"""
    import torch.nn.functional as F
    from oracle.sac_lag import _trunk
    with torch.no_grad():
        x = torch.as_tensor(obs, dtype=o.dtype)
        if kind == "ddpg":
            from oracle.ddpg_lag import mlp
            return mlp(params, x).numpy(), None
        h = _trunk(params, x, len(o.cfg.hidden))
        return F.linear(h, params["Wmu"], params["bmu"]).numpy(), F.linear(h, params["Wsig"], params["bsig"]).numpy()


def _lraw_margin(lraw):
    return np.minimum(np.abs(lraw / 2.0 - 1), np.abs(lraw / -20.0 - 1))


def replay_problem_with_regimes(kind, name):
    """Runs the case on the fp32 oracle and on its float64 twin.  -> dict: case, initial parameters (`tha`, `thc`, CVPO: `tha_old`),
    `store` / `index`, per update the inputs (`idx`, `et`, `ep` / `ek`), per oracle the logged rows and final vectors
    (`rows`, `final`: [fp32, float64]), the fp32 oracle's actor before and after (`actor0`), and per update the float64 census:
    per column the rows above / inside / below the clamp at s_t (and at s_t+n where the target actor has a sigma head), the
    range of |u|, the smallest relative distance from a boundary."""
    from helpers import fan_in_params, replay_problem
    from helpers import replay_oracles as _oracles, replay_vectors as _vectors
    torch.set_num_threads(4)
    c = REPLAY_CASES[kind][name]
    Do, Da, regimes = c["Do"], c["Da"], c["regimes"]
    rng = np.random.default_rng(c.get("seed", 0) + 17)
    o32, o64 = _oracles(kind, c)
    tha0 = fan_in_params(rng, o32.aspec)
    tha = _set_regimes(kind, tha0, o32.aspec, regimes)
    thc = np.concatenate([fan_in_params(rng, o32.cspec), fan_in_params(rng, o32.cspec)])
    tha_old = None
    for o in (o32, o64):
        o.set_params(tha, thc, -0.5) if kind == "sac" else o.set_params(tha, thc)
    if kind == "cvpo":     # actor_old != actor, or the M-step's KL terms and their duals stay at zero
        tha_old = _set_regimes(kind, (tha0 * (1 + 0.3 * rng.standard_normal(tha0.size))).astype(np.float32), o32.aspec, regimes, old=True)
        sl = head_slices(o32.aspec)
        for o in (o32, o64):
            with torch.no_grad():
                for k, (s_, shp) in sl.items():
                    o.actor_old[k].copy_(torch.as_tensor(tha_old[s_].reshape(shp)).to(o.dtype))
            o.pre_update()
    squash = (lambda z: np.clip(z, -1.0, 1.0)) if kind == "cvpo" else np.tanh
    store, index, valid = replay_problem(rng, (), c["rows"], Do, Da, squash, SUB)
    for d, reg in regimes.items():            # an "upper" column: b_sig such that the stored rows' median raw log sigma is the clamp
        if reg == "upper":
            at = head_rows(kind, o32.aspec, d)[1][-1]
            tha[at] -= np.float32(np.quantile(_heads64(kind, o64, o64.actor, store["obs"][valid])[1][:, d], c.get("upper_q", 0.5)) - 2.0)
            for o in (o32, o64):
                o.set_params(tha, thc, -0.5)
    scale = _noise_scale(regimes, Da)
    lag = [0.3]
    n_step = 2
    inputs, census, rows = [], [], [[], []]
    for u in range(c["updates"]):
        term = valid
        for _ in range(n_step - 1):
            term = index.next(term)
        actor_t = o64.actor_old if kind == "ddpg" else o64.actor          # the actor that acts at s_t+n
        ok = np.ones(valid.size, bool)
        if kind != "ddpg":
            for params, obs in ((o64.actor, store["obs"][valid]), (actor_t, store["obs_next"][term])):
                ok &= (_lraw_margin(_heads64(kind, o64, params, obs)[1]) >= SAFE_MARGIN).all(1)
        pick = rng.choice(np.flatnonzero(ok), c["B"])
        idx, tidx = valid[pick], term[pick]
        et = (scale * rng.standard_normal((c["B"], Da))).astype(np.float32)
        inp = dict(idx=idx, et=et)
        cen, margin = {"_excluded": int((~ok).sum())}, np.inf
        mu, lraw = _heads64(kind, o64, o64.actor, store["obs"][idx])
        if kind == "sac":
            inp["ep"] = ep = (scale * rng.standard_normal((c["B"], Da))).astype(np.float32)
            mun, lrawn = _heads64(kind, o64, actor_t, store["obs_next"][tidx])
            au = np.concatenate([np.abs(mu + ep * np.exp(np.clip(lraw, -20, 2))), np.abs(mun + et * np.exp(np.clip(lrawn, -20, 2)))])
            lr_all = np.concatenate([lraw, lrawn])
        elif kind == "cvpo":
            inp["ek"] = (scale * rng.standard_normal((c["K"], c["B"], Da))).astype(np.float32)
            _, lrawo = _heads64(kind, o64, o64.actor_old, store["obs"][idx])
            _, lrawn = _heads64(kind, o64, actor_t, store["obs_next"][tidx])
            lr_all = np.concatenate([lraw, lrawo, lrawn])
            var = np.exp(2 * np.clip(np.concatenate([lraw, lrawo]), -20, 2))
            margin = min(margin, float(np.abs(var / 1e-6 - 1).min()))
            au = None
        else:
            mun, _ = _heads64(kind, o64, actor_t, store["obs_next"][tidx])
            au, lr_all = np.concatenate([np.abs(mu), np.abs(mun)]), None
        for d in range(Da):
            if lr_all is not None:
                n = c["B"]
                cen[f"c{d}:hi"], cen[f"c{d}:lo"] = int((lraw[:, d] > 2).sum()), int((lr_all[:, d] < -20).sum())
                cen[f"c{d}:hi_n"] = int((lr_all[-n:, d] > 2).sum())
            if kind == "cvpo":
                cen[f"c{d}:var<1e-6"] = int((var[:, d] < 1e-6).sum())
            if au is not None:
                cen[f"c{d}:|u|"] = (round(float(au[:, d].min()), 2), round(float(au[:, d].max()), 2))
        if lr_all is not None:
            margin = min(margin, float(_lraw_margin(lr_all).min()))
        inputs.append(inp)
        for o, out in ((o32, rows[0]), (o64, rows[1])):
            if kind == "sac":
                sa, sc, _ = o.update(store, index, idx, et, inp["ep"], lag, 1 / 1.3)
                out.append({**sa, **sc})
            elif kind == "ddpg":
                sa, sc, _ = o.update(store, index, idx, np.array(lag), 1 / 1.3)
                out.append({**sa, **sc})
            else:
                st, _, _ = o.update(store, index, idx, et, inp["ek"])
                out.append({**st, "duals": np.array([o.estep_dual[0].item(), o.estep_dual[1].item(), o.mstep_dual_mu.item(),
                                                     o.mstep_dual_std.item()])})
        if kind == "cvpo":
            cen["_dual_std"] = rows[1][-1]["mstep/mstep_dual_std"]
        census.append((cen, margin))
    final = []
    for o in (o32, o64):
        v = _vectors(kind, o)
        if kind == "sac":
            v["alpha"] = float(o.alpha)
        final.append(v)
    return dict(kind=kind, name=name, case=c, tha=tha, thc=thc, tha_old=tha_old, store=store, index=index, inputs=inputs, lag=lag,
                rows=rows, final=final, census=census, aspec=o32.aspec)


def check_replay_census(p):
    """every column of every update sits in the regime the case claims (float64 oracle), at least MIN_MARGIN from every boundary"""
    c, kind = p["case"], p["kind"]
    B, what = c["B"], f"{kind}/{p['name']}"
    for u, (cen, margin) in enumerate(p["census"]):
        assert margin >= MIN_MARGIN, (what, u, "margin", margin)
        for d in range(c["Da"]):
            reg = c["regimes"].get(d, "ordinary")
            if kind != "ddpg":
                hi, hi_n, lo = cen[f"c{d}:hi"], cen[f"c{d}:hi_n"], cen[f"c{d}:lo"]
                n_lo = (3 if kind == "cvpo" else 2) * B
                if reg == "upper":           # clamped share 20 .. 80 %, at s_t and at s_t+n
                    assert 0.2 * B <= hi <= 0.8 * B and 0.2 * B <= hi_n <= 0.8 * B and lo == 0, (what, u, d, hi, hi_n, lo)
                    assert min(hi, B - hi, hi_n, B - hi_n) >= MIN_ROWS
                else:
                    assert hi == 0 and hi_n == 0 and lo == (n_lo if reg == "lower" else 0), (what, u, d, reg, hi, hi_n, lo)
            if kind == "cvpo":
                assert cen[f"c{d}:var<1e-6"] == (2 * B if reg in ("lower", "smallvar") else 0), (what, u, d, reg)
            else:
                lo_u, hi_u = cen[f"c{d}:|u|"]
                assert lo_u >= 12.0 if reg in ("sat+", "sat-") else hi_u <= 3.5, (what, u, d, reg, lo_u, hi_u)     # never 3.5 < |u| < 12
        if kind == "cvpo":
            assert cen["_dual_std"] > 0, (what, u, "the KL-sigma term carries no weight: its mask cannot show")


from helpers import ROW_BAR, VEC_BAR  # noqa: E402  the project's bars: rows (rel, abs), parameter vectors (q99, max)


def replay_distance(kind, rows_a, final_a, rows_b, final_b):
    """run a against run b in units of the project's bars: (worst logged entry over the updates, {vector: (max, q99)}, the entry)"""
    from helpers import replay_row_items as _row_items
    rel, ab = ROW_BAR[kind]
    worst, at = 0.0, None
    for u in range(len(rows_b)):
        A, Bv = _row_items(kind, rows_a[u]), _row_items(kind, rows_b[u])
        for k, w in Bv.items():
            r = abs(A[k] - w) / (rel * abs(w) + ab)
            if r > worst:
                worst, at = r, (u, k, A[k], w)
    if kind == "sac":
        r = abs(final_a["alpha"] - final_b["alpha"]) / (rel * abs(final_b["alpha"]) + ab)
        if r > worst:
            worst, at = r, ("final", "alpha", final_a["alpha"], final_b["alpha"])
    vec = {k: (float(np.abs(final_a[k] - final_b[k]).max()), float(np.quantile(np.abs(final_a[k] - final_b[k]), 0.99)))
           for k in final_b if k != "alpha"}
    return worst, vec, at


def check_frozen_rows(p, actor_after, who):
    """bit for bit, after the one update of an exact-zero case: the log-sigma head's row of a column below the lower clamp and the
    mean head's row of a saturated column are unchanged; every other head row has moved (CVPO's small-variance column: its sigma row
    moves by the likelihood term alone, which the comparison with the oracle checks)"""
    c, kind = p["case"], p["kind"]
    before, after = np.asarray(p["tha"], np.float32), np.asarray(actor_after, np.float32)
    for d in range(c["Da"]):
        reg = c["regimes"].get(d, "ordinary")
        mu_rows, sg_rows = head_rows(kind, p["aspec"], d)
        # CVPO's noiseless lower column: every particle IS the mean and mu = mu_old, so neither M-step term moves the mean row
        mu_frozen = reg in ("sat+", "sat-") or (kind == "cvpo" and reg == "lower")
        for rows, frozen, what in ((mu_rows, mu_frozen, "mean"), (sg_rows, reg == "lower", "log sigma")):
            if rows is None:
                continue
            same = np.array_equal(before[rows], after[rows])
            assert same == frozen, (who, f"{kind}/{p['name']}", f"column {d} ({reg})", what, "unchanged" if same else "changed")


HEAD_ROW_BAR = {"sac": 5e-6, "ddpg": 5e-6, "cvpo": 1e-5}


def head_row_distances(p, actor, ref):
    """per action column and head: max |actor - ref| over the head's row of that column (weights and bias)"""
    out = {}
    for d in range(p["case"]["Da"]):
        for rows, what in zip(head_rows(p["kind"], p["aspec"], d), ("mean", "log sigma")):
            if rows is not None:
                out[(d, p["case"]["regimes"].get(d, "ordinary"), what)] = float(np.abs(np.asarray(actor)[rows] - np.asarray(ref)[rows]).max())
    return out


def check_head_rows(p, actor, who):
    """After the ONE update of an exact-zero case every head row of every column agrees with the fp32 oracle's to HEAD_ROW_BAR, as a
    MAX over the row.  The whole-vector bars cannot see a wrong head row: a row is 25 .. 257 of 3 500 .. 70 000 actor entries (under
    the 99th percentile), its weights may be zero (nothing flows back into the trunk), and one Adam step moves an entry by
    lr g / (|g| + 1e-8), so a gradient of the wrong sign is off by 2 lr = 1e-3 .. 2e-3, under the vector's max bar.  With the right
    gradient the step agrees to the rounding of g against |g| + 1e-8.  The bar is the project's own bulk figure (the q99 bar of the
    parameter vectors: 5e-6 SAC / DDPG, 1e-5 CVPO) applied to each row's worst entry: 100 to 400 times under a wrong-signed step."""
    bar = HEAD_ROW_BAR[p["kind"]]
    for key, d in head_row_distances(p, actor, p["final"][0]["actor"]).items():
        assert d <= bar, (who, f"{p['kind']}/{p['name']}", "column %d (%s) %s row" % key, d, bar)
