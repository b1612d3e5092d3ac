"""Layered behaviour cloning on the device (fsrl_bc_update_layered) against tests/test_gpu_bc.py's plain float64 torch-autograd
restatement generalised to a list of layers (fresh contexts: zero moments, step count 0)."""
import numpy as np
import pytest
import torch

from fsrl_amd import _lib
from fsrl_amd.engine import Engine, EngineConfig, EngineSacGroup
from test_gpu_bc import ACTOR_SECTIONS, LR, MAXA, N_UPD, ROWS, rel

pytestmark = pytest.mark.gpu

# Bars = 4 x the largest deviation of THIS restatement run in float32 torch on the CPU from its float64 run, over the cases below, per
# quantity and relative to the quantity's scale (max |value| of the float64 result).  Measured float32 deviations: loss 2.1e-7 (the
# ragged nll case), first gradient 5.5e-7 (the clamp case), parameters after 1 and after 3 updates 7.9e-7 (the 1040-wide case),
# elsewhere at most 9.0e-8.  The factor 4 allows for the MFMA summation order and the device's tanhf / expf.
BAR = {"loss": 4 * 2.1e-7, "grad": 4 * 5.5e-7, "p1": 4 * 7.9e-7, "p3": 4 * 7.9e-7}

# head, loss, hidden, (obs_dim, act_dim), batch, unbounded, sigma-head scale, force_layered
CASES = [
    ("onpolicy", "mse", (32, 32, 32), (6, 2), 16, False, 1.0, False),      # the plain path
    ("onpolicy", "nll", (20, 7, 33), (5, 1), 17, True, 1.0, False),        # ragged widths, K & 3 != 0, a one-row second tile
    ("gauss", "nll", (64, 48, 32), (33, 8), 48, False, 40.0, False),       # raw log sigma on both sides of [-20, 2]
    ("ddpg", "mse", (300,), (6, 2), 17, False, 1.0, False),                # one hidden layer, 19 column tiles: waves take a second job
    ("gauss", "mse", (16,) * 8, (6, 2), 33, True, 1.0, False),             # FSRL_MAX_HIDDEN layers, three tiles, uneven wgrad row split
    ("onpolicy", "nll", (1040, 16), (6, 2), 16, False, 1.0, False),        # the DEVWS form
    ("onpolicy", "mse", (64, 64), (6, 2), 16, False, 1.0, True),           # a two-layer net through the new path
]

def make_case(head, hidden, dims, batch, sig_scale, seed=0):
    # actor tensors in the API's flat order ([sigma] W0 b0 ... Wm bm [Ws bs]), the stored rows and the update indices
    rng = np.random.default_rng(seed)
    Do, Da = dims
    w = lambda *s: (rng.standard_normal(s) / np.sqrt(s[-1])).astype(np.float32)
    actor, widths = {}, [Do, *hidden]
    if head == "onpolicy":
        actor["sigma"] = (-0.5 + 0.3 * rng.standard_normal(Da)).astype(np.float32)
    for l, (i, o) in enumerate(zip(widths, widths[1:])):
        actor[f"W{l}"], actor[f"b{l}"] = w(o, i), 0.1 * w(o)
    actor["Wm"], actor["bm"] = w(Da, widths[-1]), 0.1 * w(Da)
    if head == "gauss":
        actor["Ws"] = (sig_scale * w(Da, widths[-1])).astype(np.float32); actor["bs"] = 0.1 * w(Da)
    obs = rng.standard_normal((ROWS, Do)).astype(np.float32)
    act = (0.8 * rng.standard_normal((ROWS, Da))).astype(np.float32)
    return actor, obs, act, rng.integers(0, ROWS, (N_UPD, batch))

def reference(head, loss, unbounded, n_layers, actor, obs, act, idx, dtype):
    # -> losses, first gradient, parameters after 1 and after N_UPD updates (flat, API order)
    p = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in actor.items()}
    opt = torch.optim.Adam(list(p.values()), lr=LR, betas=(0.9, 0.999), eps=1e-8)
    X, A = torch.tensor(obs, dtype=dtype), torch.tensor(act, dtype=dtype)
    flat = lambda f: torch.cat([f(t).detach().reshape(-1) for t in p.values()]).numpy().astype(np.float64)
    losses, out = [], {}
    for u in range(len(idx)):
        h, a = X[idx[u]], A[idx[u]]
        for l in range(n_layers):
            h = torch.relu(h @ p[f"W{l}"].T + p[f"b{l}"])
        m = h @ p["Wm"].T + p["bm"]
        if head == "ddpg" or not unbounded:
            m = MAXA * torch.tanh(m)
        if loss == "mse":
            L = ((m - a) ** 2).sum(1).mean()
        else:
            raw = p["sigma"].expand_as(m) if head == "onpolicy" else h @ p["Ws"].T + p["bs"]
            ls = raw if head == "onpolicy" else torch.clamp(raw, -20.0, 2.0)
            L = ((a - m) ** 2 / (2 * torch.exp(ls) ** 2) + ls).sum(1).mean()
            if u == 0:
                out["raw_log_sigma"] = raw.detach().numpy()
        opt.zero_grad(set_to_none=False)
        (L + 0 * sum(t.sum() for t in p.values())).backward()      # unused tensors (sigma under mse): a zero gradient, not None
        if u == 0:
            out["grad"] = flat(lambda t: t.grad)
        opt.step()
        losses.append(float(L.detach()))
        if u == 0:
            out["p1"] = flat(lambda t: t)
    out["loss"], out["p3"] = np.array(losses), flat(lambda t: t)
    return out

def make_engine(head, hidden, dims, unbounded, actor, obs, act, force=False, seed=1):
    # a context of the head's kind holding the rows in slots 0 .. ROWS - 1 -> (engine, read the actor back)
    (Do, Da), rng = dims, np.random.default_rng(seed)
    cfg = dict(obs_dim=Do, act_dim=Da, hidden_sizes=hidden, force_layered=force, env_num=1, buffer_size=64, max_action=MAXA, lr=LR)
    a_flat = np.concatenate([v.reshape(-1) for v in actor.values()])
    if head == "onpolicy":
        eng = Engine(EngineConfig(unbounded=unbounded, **cfg), device=0)
        eng.set_params(np.concatenate([a_flat, (0.1 * rng.standard_normal(eng.n_params - a_flat.size)).astype(np.float32)]))
        get = lambda: eng.get_params()[:a_flat.size]
    else:
        eng = Engine(EngineConfig(algo=_lib.ALGO_SAC_LAG, **cfg), device=0)
        eng.sac_init(actor_lr=LR, deterministic=head == "ddpg", unbounded=None if head == "ddpg" else unbounded)
        eng.sac_set_params(a_flat, (0.1 * rng.standard_normal(eng.n_sac_critics)).astype(np.float32))
        get = lambda: eng.sac_get_params(0)[0]
    z = np.zeros(1)
    for t in range(ROWS):
        eng.push([0], obs[t:t + 1], act[t:t + 1], z, z, np.zeros(1, bool), np.zeros(1, bool), obs[t:t + 1])
    return eng, get

@pytest.mark.parametrize("head,loss,hidden,dims,batch,unbounded,sig_scale,force", CASES)
def test_bc_update_layered_matches_float64_autograd(head, loss, hidden, dims, batch, unbounded, sig_scale, force):
    actor, obs, act, idx = make_case(head, hidden, dims, batch, sig_scale)
    ref = reference(head, loss, unbounded, len(hidden), actor, obs, act, idx, torch.float64)
    if sig_scale != 1.0:        # the clamp case: both branches occur in the first batch
        assert 0 < ((ref["raw_log_sigma"] >= -20.0) & (ref["raw_log_sigma"] <= 2.0)).sum() < ref["raw_log_sigma"].size
    eng, get = make_engine(head, hidden, dims, unbounded, actor, obs, act, force)
    try:
        l1 = eng.bc_update_layered(batch, 1, loss=loss, indices=idx[:1])
        got = {"p1": get()}
        got["grad"] = eng.get_grads()[:got["p1"].size]
        l2 = eng.bc_update_layered(batch, N_UPD - 1, loss=loss, indices=idx[1:])
        got["p3"], got["loss"] = get(), np.concatenate([l1, l2])
    finally:
        eng.close()
    dev = {k: rel(v, ref[k]) for k, v in got.items()}
    print("bc layered deviations", head, loss, hidden, dims, batch, dev)
    assert all(d <= BAR[k] for k, d in dev.items()), (dev, BAR)

@pytest.mark.parametrize("algo,loss", [("ppol", "nll"), ("cpo", "mse"), ("sacl", "nll"), ("ddpgl", "mse"), ("cvpo", "nll")])
def test_pretrain_routes_layered_and_leaves_everything_else_alone(algo, loss):
    # test_gpu_bc's policy test on layered engines (BasePolicy.pretrain routes on the shape); layered contexts keep the fused contexts'
    # section tags, so its ACTOR_SECTIONS serves as it is
    from fsrl_amd.agent import CPOAgent, CVPOAgent, DDPGLagAgent, PPOLagAgent, SACLagAgent
    from fsrl_amd.data.batch import Batch
    from fsrl_amd.env import SyntheticSafetyVectorEnv
    cls = {"ppol": PPOLagAgent, "cpo": CPOAgent, "sacl": SACLagAgent, "ddpgl": DDPGLagAgent, "cvpo": CVPOAgent}[algo]
    env = SyntheticSafetyVectorEnv(env_num=2, obs_dim=6, act_dim=2, episode_len=20, seed=1)
    agents = [cls(env, None, cost_limit=10, device="cuda:0", seed=3, hidden_sizes=(32, 32, 32), training_num=2) for _ in range(2)]
    (pol, eng), (_, twin) = [(a.policy, a.policy.engine) for a in agents]
    _, obs, act, idx = make_case("ddpg", (32, 32, 32), (6, 2), 17, 1.0)
    z = np.zeros(1)
    for t in range(ROWS):
        eng.push([0], obs[t:t + 1], act[t:t + 1], z, z, np.zeros(1, bool), np.zeros(1, bool), obs[t:t + 1])
    try:
        before, version = eng.train_state_sections(True), eng.store_version()
        params = eng.get_params() if "P" in before else None
        pol.pretrain(None, batch_size=17, n_updates=2, loss=loss, seed=4)
        after = eng.train_state_sections(True)
        assert set(after) == set(before) and eng.store_version() == version
        assert {k for k in after if not np.array_equal(after[k], before[k])} <= ACTOR_SECTIONS
        if "P" in after:        # on-policy: one vector; the critics' parameters through the API, their moments: no moment moves where no parameter did
            n_a, moved = eng.n_actor_params, (after["P"] != before["P"]).reshape(-1, 4).any(1)[:after["M"].size // 4]
            assert np.array_equal(eng.get_params()[n_a:], params[n_a:]) and not np.array_equal(eng.get_params()[:n_a], params[:n_a])
            assert all(not np.any((after[k].view(np.float32) != before[k].view(np.float32)) & ~moved) for k in "MV")
        else:
            assert not np.array_equal(after["PA"], before["PA"])
            assert algo == "sacl" or np.array_equal(after["PAT"], after["PA"])
        pol.eval()
        with torch.no_grad():
            out = pol(Batch(obs=obs[:9], info={}))
        # SACLagAgent builds its policy with deterministic_eval=False (the host SAMPLES in eval mode): its deterministic action is the squashed mean
        host = (torch.tanh(out.logits[0]) if algo == "sacl" else out.act).numpy()
        np.testing.assert_allclose(eng.actor_sample(obs[:9], deterministic=True), host, rtol=0, atol=2e-6)
        twin.load_train_state(eng.train_state(with_store=True))
        la, lb = eng.bc_update_layered(17, 1, loss=loss, indices=idx[2:]), twin.bc_update_layered(17, 1, loss=loss, indices=idx[2:])
        assert np.array_equal(la, lb) and eng.train_state(with_store=False) == twin.train_state(with_store=False)
    finally:
        eng.close(); twin.close()

def test_bc_update_layered_refusals_name_their_reason_and_change_nothing():
    hid, dims = (32, 32, 32), (6, 2)
    actor, obs, act, idx = make_case("ddpg", hid, dims, 16, 1.0)
    eng, _ = make_engine("ddpg", hid, dims, False, actor, obs, act)
    empty = Engine(EngineConfig(obs_dim=6, act_dim=2, hidden_sizes=hid, env_num=1, buffer_size=64), device=0)
    fused = Engine(EngineConfig(obs_dim=6, act_dim=2, hidden_sizes=(64, 64), env_num=1, buffer_size=64), device=0)
    try:
        states = [e.train_state() for e in (eng, empty, fused)]
        for e, kw, reason in ((fused, dict(indices=idx[:1]), "use fsrl_bc_update"), (eng, dict(loss="nll", indices=idx[:1]), "deterministic"),
                              (eng, dict(indices=np.full((1, 16), ROWS)), "outside the stored rows"), (empty, dict(), "store is empty"),
                              (eng, dict(indices=idx[:1]), "member of a live group")):
            group = EngineSacGroup([eng]) if "group" in reason else None
            with pytest.raises(AssertionError, match=reason):
                e.bc_update_layered(16, 1, **kw)
            if group is not None:
                group.close()
        assert [e.train_state() for e in (eng, empty, fused)] == states
    finally:
        eng.close(); empty.close(); fused.close()
