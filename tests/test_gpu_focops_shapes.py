"""FOCOPS against its oracle away from the golden fixtures, on seeded synthetic rollouts: 256-wide fused networks, wide
observations (W1 staged in LDS only up to 16 columns), 1 .. 16 action columns, zero-padded widths, both tile heights of the
three-launch step, the four-launch split-K step of minibatches over 512 rows, layered contexts, a batch larger than N, a
single-row sub-buffer and one observation column.

* The gradient the minibatch step leaves in G, at theta != theta_old with eta in the middle of the rows' KL(new || old), against
  float64 autograd of the oracle's losses: the KL part of the loss gradient (dmu / so^2, vr - 1, the KL <= eta mask) directly.
* Whole updates (process_fn products, logged rows, the stopped pass, parameters) against the fp32 oracle at test_gpu_focops.py's
  bars, under both step plans."""
import numpy as np
import pytest
import torch

from test_gpu_shapes import _synthetic

pytestmark = pytest.mark.gpu


def _hidden(h):
    return (h, h) if isinstance(h, int) else tuple(h)


def _layered(h):
    hs = _hidden(h)
    return not (len(hs) == 2 and max(hs) <= 256)


def _width(h):
    """the fused kernels' width for two hidden layers of at most 256 units (narrower layers zero-padded)"""
    m = max(_hidden(h))
    return 64 if m <= 64 else 128 if m <= 128 else 256


def _chunk_sizes(n, B):
    from fsrl_amd.policy.ppo_lag import _chunk_sizes
    return _chunk_sizes(n, B)


def _plan(h, n, B, four_launch):
    """-> (fast, [rows4 per minibatch]) as host_focops.inc decides them on this device: the three-launch step while the
    minibatch working set (2 * min(B, N) rows, rounded up to 32) fits 512 rows, 4-row tiles while 4 * tiles * 3 <= CUs"""
    if _layered(h):
        return False, []
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    fast = not four_launch and (2 * min(B, n) + 31) // 32 * 32 <= 512
    return fast, [12 * ((s + 15) // 16) <= cus for s in _chunk_sizes(n, B)]


def _rollout(seed, rows, Do, Da, ep):
    """synthetic rows in push order + the oracle's OnPolicyData (env-major: sample(0) order)"""
    from oracle.ppo_lag import OnPolicyData
    cols = _synthetic(np.random.default_rng(seed), rows, Do, Da, ep)
    cat = {k: np.concatenate(v) for k, v in cols.items()}
    end = (cat["term"] | cat["trunc"]).copy()
    end[np.cumsum(rows) - 1] = True                       # unfinished tails
    data = OnPolicyData(obs=cat["obs"], act=cat["act"], rew=cat["rew"], cost=cat["cost"], terminated=cat["term"],
                        truncated=cat["trunc"], obs_next=cat["obs_next"], end_flag=end)
    return cols, data


def _theta0(o, seed, sigma=-0.5):
    """matrices ~ N(0, 1 / fan_in), biases 0.05 N(0, 1), sigma_param around `sigma`, in the oracle's flat layout"""
    rng = np.random.default_rng(seed)
    parts = []
    for net in o.nets:
        for k, t in net.items():
            if k == "sigma_param":
                parts.append(sigma + 0.1 * rng.standard_normal(t.shape))
            elif t.ndim == 2:
                parts.append(rng.standard_normal(t.shape) / np.sqrt(t.shape[1]))
            else:
                parts.append(0.05 * rng.standard_normal(t.shape))
    return np.concatenate([p.reshape(-1) for p in parts]).astype(np.float32)


def _oracle(Do, Da, h, dtype=torch.float32, **kw):
    from oracle.focops import FOCOPSConfig, FOCOPSOracle
    return FOCOPSOracle(FOCOPSConfig(obs_dim=Do, act_dim=Da, hidden=_hidden(h), **kw), dtype=dtype)


def _engine(Do, Da, h, rows, cols, four_launch=0, max_action=1.0, unbounded=False, norm_adv=True, recompute=False, **foc):
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig
    eng = Engine(EngineConfig(algo=_lib.ALGO_FOCOPS, obs_dim=Do, act_dim=Da, hidden_sizes=_hidden(h), n_critics=2,
                              env_num=len(rows), buffer_size=len(rows) * 2048, max_action=max_action, norm_adv=norm_adv,
                              target_kl=None, unbounded=unbounded, recompute_adv=recompute))
    eng.focops_init(**foc)
    eng.focops_set_plan(four_launch)
    for t in range(max(rows)):                            # lock-step, envs drop out as they run dry
        ids = [e for e in range(len(rows)) if t < rows[e]]
        eng.push(ids, *[np.stack([cols[k][e][t] for e in ids]) for k in ("obs", "act", "rew", "cost", "term", "trunc",
                                                                         "obs_next")])
    return eng


# ----------------------------------------------------------------------------------------------- gradient at theta != theta_old
GRAD_CASES = [  # Do, Da, hidden, rows per env, batch, unbounded
    (33, 6, 128, [300, 257, 143], 64, False),             # wide observations, 4-row tiles
    (17, 5, 256, [300, 300], 256, False),                 # last minibatch of 344 rows: 16-row tiles at 256 wide; act_dim > 4
    (128, 16, 64, [200, 200], 128, True),                 # maximum dimensions, unbounded head
    (40, 8, 256, [200, 180], 128, True),                  # unbounded head at 256 wide, 4-row tiles
    (60, 7, 256, [1300, 1200], 1024, False),              # minibatches over 512 rows: the four-launch step only
    (12, 4, (100, 50), [150, 140], 64, False),            # two unrelated widths, zero-padded to 128
    (7, 5, (40, 72, 24), [127, 125, 129], 64, False),     # layered: G holds all three networks
]


def _grad_params():
    out = []
    for case in GRAD_CASES:
        Do, Da, h, rows, B, _ = case
        plans = (0, 1) if not _layered(h) and min(B, sum(rows)) <= 256 else (0, )
        out += [pytest.param(*case, p, id=f"{Do}x{Da}-{'x'.join(map(str, _hidden(h)))}-B{B}-plan{p}") for p in plans]
    return out


def _eta_in_gap(kl):
    """an eta between two consecutive per-row KLs that masks 20 .. 60 % of the rows, at the widest relative gap there"""
    s = np.sort(np.asarray(kl, np.float64))
    n = s.size
    js = [j for j in range(1, n) if 0.2 <= (n - j) / n <= 0.6 and s[j - 1] > 0]
    j = max(js, key=lambda j: s[j] / s[j - 1])
    eta = float(np.float32(np.sqrt(s[j - 1] * s[j])))
    assert np.abs(s / eta - 1).min() > 1e-3, "no KL gap to put eta in"
    return eta, (n - j) / n


@pytest.mark.parametrize("Do,Da,h,rows,B,unbounded,four_launch", _grad_params())
def test_focops_gradient_away_from_theta_old_vs_float64_autograd(Do, Da, h, rows, B, unbounded, four_launch):
    """lr 0 keeps theta fixed: after one pass G holds the last minibatch's gradient at theta, taken against the old
    distribution recorded at theta_old by ppo_begin.  Actor slice on every plan; the critics' slices where G holds them (the
    three-launch step and layered contexts), with the l2 term the Adam step adds (2 * l2_reg * theta) added here."""
    from fsrl_amd import _lib
    from oracle.ppo_lag import split_chunks
    torch.set_num_threads(4)
    seed = 7 * Do + Da
    cols, data = _rollout(seed, rows, Do, Da, 40)
    N = len(data)
    l2, nu, max_action = 1e-3, 0.35, 1.3
    o = _oracle(Do, Da, h, torch.float64, max_action=max_action, unbounded=unbounded, l2_reg=l2)
    theta_old = _theta0(o, seed + 1)
    rng = np.random.default_rng(seed + 2)
    theta = (theta_old * (1 + 0.1 * rng.standard_normal(theta_old.size)) + 0.01 * rng.standard_normal(theta_old.size))
    theta = theta.astype(np.float32)
    o.set_params(theta_old, nu=nu)
    pb = o.process(data)
    perm = rng.permutation(N)
    chunk = split_chunks(N, B, perm)[-1]
    o.set_params(theta, nu=nu)
    with torch.no_grad():
        _, kl, _ = o.policy_loss(pb, chunk)
    eta, masked = _eta_in_gap(kl.numpy())
    o.fcfg.eta = eta
    loss, _, _ = o.policy_loss(pb, chunk)
    vf, _ = o.critics_loss(pb, chunk)
    leaves = o._leaves
    ga = torch.autograd.grad(loss, leaves, allow_unused=True)
    gc = torch.autograd.grad(vf.sum(), leaves, allow_unused=True)
    og = np.concatenate([(a if a is not None else c).reshape(-1).numpy() for a, c in zip(ga, gc)])

    eng = _engine(Do, Da, h, rows, cols, four_launch, max_action=max_action, unbounded=unbounded, actor_lr=0.0, critic_lr=0.0,
                  l2_reg=l2, eta=eta, max_grad_norm=0.5, delta=1e9)
    _lib.check(eng.lib.fsrl_focops_set_nu(eng._ctx, nu, 0.0))
    eng.set_params(theta_old)
    assert eng.ppo_begin([0.0], 1.0, B) == N
    eng.set_params(theta)
    eng.ppo_pass(perm)
    eng.ppo_end()
    assert np.array_equal(eng.get_params(), theta)
    got = eng.get_grads()
    na = eng.n_actor_params
    fast, _ = _plan(h, N, B, four_launch)
    n_cmp = got.size if (fast or _layered(h)) else na
    got = got[:n_cmp].astype(np.float64)
    got[na:] += 2 * l2 * theta[na:n_cmp]
    want = og[:n_cmp]
    for sl, what in ((slice(0, na), "actor"), (slice(na, n_cmp), "critics")):
        if sl.stop > sl.start:
            np.testing.assert_allclose(got[sl], want[sl], rtol=1e-4, atol=2e-6 * max(1.0, float(np.abs(want[sl]).max())),
                                       err_msg=f"{what} (eta {eta:.4g} masks {masked:.0%} of {len(chunk)} rows)")
    eng.close()


# ----------------------------------------------------------------------------------------------- whole updates
FOCOPS_VARIANTS = [  # Do, Da, hidden, rows per env, batch, repeat, options
    (33, 6, 128, [300, 257, 143], 64, 2, dict()),                                   # wide observations, 4-row tiles
    (128, 16, 64, [200, 200], 128, 2, dict(norm_adv=False)),                        # maximum dimensions, raw advantages
    (17, 1, 256, [300, 300], 256, 2, dict(max_grad_norm=None)),                     # merged 344-row minibatch: 16-row tiles
    (60, 2, 256, [1300, 1200], 1024, 1, dict()),                                    # over 512 rows: four-launch step, 256 wide
    (3, 2, 64, [90, 1, 35], 1000, 3, dict(recompute=True)),                         # batch > N; a single-row sub-buffer
    (12, 4, (100, 50), [150, 140], 64, 2, dict()),                                  # two unrelated widths, padded to 128
    (1, 1, 64, [100, 60], 64, 2, dict()),                                           # one observation column
    (7, 5, (40, 72, 24), [127, 125, 129], 64, 3, dict(delta=0.004, actor_lr=2e-3)),  # layered, ragged; KL stop
    (8, 3, (300, ), [200, 160], 128, 2, dict()),                                    # layered, wider than the fused kernels
    (40, 8, 256, [400, 380], 128, 3, dict(unbounded=True, actor_lr=1e-4)),         # unbounded head at 256 wide
]


def _variant_params():
    out = []
    for v in FOCOPS_VARIANTS:
        Do, Da, h, rows, B, R, _ = v
        plans = (0, ) if _layered(h) else (0, 1)
        out += [pytest.param(*v, p, id=f"{Do}x{Da}-{'x'.join(map(str, _hidden(h)))}-B{B}-plan{p}") for p in plans]
    return out


def run_variant(Do, Da, h, rows, B, R, opts, four_launch):
    """one FOCOPS update of the engine and of the fp32 oracle from the same theta0, nu and permutations
    -> (engine stats, engine stopped pass, engine, oracle process products, oracle rows as stats, oracle stopped pass, oracle)"""
    opts = dict(opts)
    seed = 1000 + 31 * Do + Da
    unbounded, norm_adv, recompute = opts.pop("unbounded", False), opts.pop("norm_adv", True), opts.pop("recompute", False)
    foc = dict(actor_lr=5e-4, critic_lr=1e-3, l2_reg=1e-3, delta=0.02, eta=0.02, tem_lambda=0.95, max_grad_norm=0.5)
    foc.update(opts)
    cols, data = _rollout(seed, rows, Do, Da, 45)
    N = len(data)
    o = _oracle(Do, Da, h, unbounded=unbounded, advantage_normalization=norm_adv, recompute_advantage=recompute, **foc)
    theta0 = _theta0(o, seed + 1)
    o.set_params(theta0, nu=0.3)
    rng = np.random.default_rng(seed + 2)
    perms = [rng.permutation(N) for _ in range(R)]
    pb, orows, ostopped = o.update(data, 25.0, B, R, perms)
    want = np.array([[sn["loss/nu_loss"], sn["loss/nu_value"], sa["loss/actor_loss"], sa["loss/kl"], sa["loss/entropy"],
                      sc["loss/vf0"], sc["loss/vf1"], sc["loss/vf_total"]] for sn, sa, sc in orows])
    eng = _engine(Do, Da, h, rows, cols, four_launch, unbounded=unbounded, norm_adv=norm_adv, recompute=recompute, **foc)
    eng.set_params(theta0)
    stats, stopped = eng.focops_update(want[0, 1], want[0, 0], B, R, perms=perms)
    return stats, stopped, eng, pb, want, ostopped, o


def check_update(stats, stopped, eng, pb, want, ostopped, o, recompute=False, actor_lr=5e-4):
    """test_gpu_focops.py's bars: process products 5e-6 * scale, rows 3e-5, parameters 99.9 % within 5e-6 (x lr / 5e-4), all
    within 2e-3.  pb None: no process products (a grouped update's members have no Engine-side batch length to read them by)"""
    for k in () if pb is None else ("logp_old", ) if recompute else ("rets", "advs", "logp_old"):   # recompute overwrites rets / advs
        ref = pb[k].numpy()
        scale = max(1.0, float(np.abs(ref).max()))
        np.testing.assert_allclose(eng.batch_get(k), ref, rtol=0, atol=5e-6 * scale, err_msg=k)
    assert stopped == ostopped, (stopped, ostopped)
    assert stats.shape == want.shape, (stats.shape, want.shape)
    np.testing.assert_allclose(stats, want, rtol=3e-5, atol=3e-5)
    d = np.abs(eng.get_params() - o.get_params())
    tol = 5e-6 * max(1.0, actor_lr / 5e-4)
    assert np.quantile(d, 0.999) <= tol and d.max() <= 2e-3, (np.quantile(d, 0.999), d.max())


@pytest.mark.parametrize("Do,Da,h,rows,B,R,opts,four_launch", _variant_params())
def test_focops_update_variants_vs_oracle(Do, Da, h, rows, B, R, opts, four_launch):
    torch.set_num_threads(4)
    stats, stopped, eng, pb, want, ostopped, o = run_variant(Do, Da, h, rows, B, R, opts, four_launch)
    check_update(stats, stopped, eng, pb, want, ostopped, o, recompute=opts.get("recompute", False),
                 actor_lr=opts.get("actor_lr", 5e-4))
    eng.close()


def test_focops_variants_reach_every_plan():
    """on this device's CU count the table reaches both tile heights of the three-launch step, the three- and the four-launch
    step with the automatic plan, layered contexts, and every option the update has"""
    seen = set()                          # (width, three-launch step, 4-row tiles) of every minibatch
    for Do, Da, h, rows, B, R, opts in FOCOPS_VARIANTS:
        if not _layered(h):
            fast, rows4 = _plan(h, sum(rows), B, 0)
            seen |= {(_width(h), fast, r) for r in rows4}
    assert {(256, True, True), (256, True, False), (256, False, False)} <= seen, seen
    assert any(_layered(v[2]) for v in FOCOPS_VARIANTS) and any(_width(v[2]) == 256 and not _layered(v[2]) for v in FOCOPS_VARIANTS)
    opts = [v[6] for v in FOCOPS_VARIANTS]
    for key, val in (("norm_adv", False), ("max_grad_norm", None), ("recompute", True), ("unbounded", True)):
        assert any(key in o and o[key] == val for o in opts), key
    assert sum("eta" not in o for o in opts) >= 2 and any("delta" in o for o in opts)
