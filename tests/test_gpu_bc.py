"""Behaviour cloning on the device (fsrl_bc_update) against a plain float64 torch-autograd restatement: the same gathered rows, the
same loss, torch.optim.Adam in float64 from the context's parameters (fresh contexts: zero moments, step count 0)."""
import numpy as np
import pytest
import torch

from fsrl_amd import _lib
from fsrl_amd.engine import Engine, EngineConfig, EngineSacGroup

pytestmark = pytest.mark.gpu

LR, MAXA, ROWS, N_UPD = 1e-3, 1.5, 60, 3
# Bars = 4 x the largest deviation of THIS restatement run in float32 torch on the CPU from its float64 run, over the cases below, per
# quantity and relative to the quantity's scale (max |value| of the float64 result).  Measured float32 deviations: loss 2.7e-7,
# first gradient 2.8e-6 (the clamp case), parameters after 1 and after 3 updates 8.5e-6 (on-policy mse at 256 x 256: entries whose
# gradient is near Adam's eps), elsewhere at most 2.2e-7.  The factor 4 allows for the MFMA summation order
# and the device's tanhf / expf / logf differing from libm in the last bits.
BAR = {"loss": 4 * 2.7e-7, "grad": 4 * 2.8e-6, "p1": 4 * 8.5e-6, "p3": 4 * 8.5e-6}

# head, loss, hidden, (obs_dim, act_dim), batch, unbounded, sigma-head scale (gauss nll: raw log sigma inside and outside [-20, 2])
CASES = [
    ("onpolicy", "mse", (64, 64), (6, 2), 16, False, 1.0),
    ("onpolicy", "nll", (256, 256), (33, 8), 17, True, 1.0),
    ("onpolicy", "nll", (48, 48), (5, 1), 48, False, 1.0),
    ("onpolicy", "mse", (256, 256), (6, 2), 48, True, 1.0),
    ("gauss", "mse", (256, 256), (5, 1), 17, True, 1.0),
    ("gauss", "nll", (64, 64), (33, 8), 48, False, 1.0),
    ("gauss", "nll", (64, 64), (6, 2), 48, True, 40.0),
    ("ddpg", "mse", (256, 256), (33, 8), 16, False, 1.0),
    ("ddpg", "mse", (48, 48), (6, 2), 17, False, 1.0),
]

def make_case(head, hidden, dims, batch, sig_scale, seed=0):
    # actor tensors in the API's flat order, the stored rows and the update indices
    rng = np.random.default_rng(seed)
    (h1, h2), (Do, Da) = hidden, dims
    w = lambda *s: (rng.standard_normal(s) / np.sqrt(s[-1])).astype(np.float32)
    actor = {"W1": w(h1, Do), "b1": 0.1 * w(h1), "W2": w(h2, h1), "b2": 0.1 * w(h2), "W3": w(Da, h2), "b3": 0.1 * w(Da)}
    if head == "onpolicy":
        actor = {"sigma": (-0.5 + 0.3 * rng.standard_normal(Da)).astype(np.float32), **actor}
    if head == "gauss":
        actor["Ws"] = (sig_scale * w(Da, h2)).astype(np.float32); actor["bs"] = 0.1 * w(Da)
    obs = rng.standard_normal((ROWS, Do)).astype(np.float32)
    act = (0.8 * rng.standard_normal((ROWS, Da))).astype(np.float32)
    idx = rng.integers(0, ROWS, (N_UPD, batch))
    return actor, obs, act, idx

def reference(head, loss, unbounded, actor, obs, act, idx, dtype):
    # -> losses, first gradient, parameters after 1 and after N_UPD updates (flat, API order)
    p = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in actor.items()}
    opt = torch.optim.Adam(list(p.values()), lr=LR, betas=(0.9, 0.999), eps=1e-8)
    X, A = torch.tensor(obs, dtype=dtype), torch.tensor(act, dtype=dtype)
    flat = lambda f: torch.cat([f(t).detach().reshape(-1) for t in p.values()]).numpy().astype(np.float64)
    losses, out = [], {}
    for u in range(len(idx)):
        x, a = X[idx[u]], A[idx[u]]
        h = torch.relu(torch.relu(x @ p["W1"].T + p["b1"]) @ p["W2"].T + p["b2"])
        m = h @ p["W3"].T + p["b3"]
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

def make_engine(head, hidden, dims, unbounded, actor, obs, act, seed=1):
    # a fused context of the head's kind holding the rows in slots 0 .. ROWS - 1 -> (engine, read the actor back)
    (Do, Da), rng = dims, np.random.default_rng(seed)
    cfg = dict(obs_dim=Do, act_dim=Da, hidden_sizes=hidden, env_num=1, buffer_size=64, max_action=MAXA, lr=LR)
    a_flat = np.concatenate([v.reshape(-1) for v in actor.values()])
    if head == "onpolicy":
        eng = Engine(EngineConfig(unbounded=unbounded, **cfg), device=0)
        critics = (0.1 * rng.standard_normal(eng.n_params - a_flat.size)).astype(np.float32)
        eng.set_params(np.concatenate([a_flat, critics]))
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

def rel(x, ref):
    return float(np.max(np.abs(np.asarray(x, np.float64) - ref)) / np.max(np.abs(ref)))

@pytest.mark.parametrize("head,loss,hidden,dims,batch,unbounded,sig_scale", CASES)
def test_bc_update_matches_float64_autograd(head, loss, hidden, dims, batch, unbounded, sig_scale):
    actor, obs, act, idx = make_case(head, hidden, dims, batch, sig_scale)
    ref = reference(head, loss, unbounded, actor, obs, act, idx, torch.float64)
    if sig_scale != 1.0:        # the clamp case: both branches occur in the first batch
        assert 0 < ((ref["raw_log_sigma"] >= -20.0) & (ref["raw_log_sigma"] <= 2.0)).sum() < ref["raw_log_sigma"].size
    eng, get = make_engine(head, hidden, dims, unbounded, actor, obs, act)
    try:
        l1 = eng.bc_update(batch, 1, loss=loss, indices=idx[:1])
        got = {"p1": get()}
        got["grad"] = eng.get_grads()[:got["p1"].size]
        l2 = eng.bc_update(batch, N_UPD - 1, loss=loss, indices=idx[1:])
        got["p3"], got["loss"] = get(), np.concatenate([l1, l2])
    finally:
        eng.close()
    dev = {k: rel(v, ref[k]) for k, v in got.items()}
    print("bc deviations", head, loss, hidden, dims, batch, dev)
    assert all(d <= BAR[k] for k, d in dev.items()), (dev, BAR)

ACTOR_SECTIONS = {"HOST", "P", "M", "V", "PA", "MA", "VA", "PAT", "SACS", "CVPS"}      # what a BC step may move (checked further below)

@pytest.mark.parametrize("algo,loss", [("ppol", "nll"), ("focops", "mse"), ("cpo", "nll"), ("ddpgl", "mse"), ("cvpo", "nll")])
def test_pretrain_leaves_everything_else_alone(algo, loss):
    # through the policy object: critics (parameters and moments), store, store version and env state bit-identical; actor_old := actor;
    # the device actor acts with the new weights and equals the synced host mirror; a twin restored from the exported training state
    # takes the same next step
    from fsrl_amd.agent import CPOAgent, CVPOAgent, DDPGLagAgent, FOCOPSAgent, PPOLagAgent
    from fsrl_amd.data.batch import Batch
    from fsrl_amd.env import SyntheticSafetyVectorEnv
    cls = {"ppol": PPOLagAgent, "focops": FOCOPSAgent, "cpo": CPOAgent, "ddpgl": DDPGLagAgent, "cvpo": CVPOAgent}[algo]
    env = SyntheticSafetyVectorEnv(env_num=2, obs_dim=6, act_dim=2, episode_len=20, seed=1)
    agents = [cls(env, None, cost_limit=10, device="cuda:0", seed=3, hidden_sizes=(64, 64), training_num=2) for _ in range(2)]
    (pol, eng), (_, twin) = [(a.policy, a.policy.engine) for a in agents]
    _, obs, act, idx = make_case("ddpg", (64, 64), (6, 2), 17, 1.0)
    z = np.zeros(1)
    for t in range(ROWS):
        eng.push([0], obs[t:t + 1], act[t:t + 1], z, z, np.zeros(1, bool), np.zeros(1, bool), obs[t:t + 1])
    henv = eng.devenv_create(_lib.DEVENV_LINEAR, 2, 20, seed=5, A=0.9 * np.eye(6), B=0.1 * np.ones((2, 6)))
    eng.devenv_reset(henv, 2)
    try:
        before, version, envs = eng.train_state_sections(True), eng.store_version(), eng.devenv_get_state(henv, 2, 6)
        params = eng.get_params() if "P" in before else None
        pol.pretrain(None, batch_size=17, n_updates=2, loss=loss, seed=4)
        after = eng.train_state_sections(True)
        assert set(after) == set(before) and eng.store_version() == version
        assert all(np.array_equal(a, b) for a, b in zip(envs, eng.devenv_get_state(henv, 2, 6)))
        assert {k for k in after if not np.array_equal(after[k], before[k])} <= ACTOR_SECTIONS
        if "P" in after:        # on-policy: one vector; the critics' parameters through the API, their moments: no moment moves where no parameter did
            n_a, moved = eng.n_actor_params, (after["P"] != before["P"]).reshape(-1, 4).any(1)[:after["M"].size // 4]     # W2 mirrors behind
            assert np.array_equal(eng.get_params()[n_a:], params[n_a:]) and not np.array_equal(eng.get_params()[:n_a], params[:n_a])
            assert all(not np.any((after[k].view(np.float32) != before[k].view(np.float32)) & ~moved) for k in "MV")
        else:
            assert not np.array_equal(after["PA"], before["PA"]) and np.array_equal(after["PAT"], after["PA"])
        pol.eval()
        with torch.no_grad():
            host = pol(Batch(obs=obs[:9], info={})).act.numpy()
        np.testing.assert_allclose(eng.actor_sample(obs[:9], deterministic=True), host, rtol=0, atol=2e-6)
        twin.load_train_state(eng.train_state(with_store=True))
        la, lb = eng.bc_update(17, 1, loss=loss, indices=idx[2:]), twin.bc_update(17, 1, loss=loss, indices=idx[2:])
        assert np.array_equal(la, lb) and eng.train_state(with_store=False) == twin.train_state(with_store=False)
    finally:
        eng.devenv_destroy(henv); eng.close(); twin.close()

def test_bc_update_refusals_name_their_reason_and_change_nothing():
    actor, obs, act, idx = make_case("ddpg", (64, 64), (6, 2), 16, 1.0)
    eng, get = make_engine("ddpg", (64, 64), (6, 2), False, actor, obs, act)
    empty = Engine(EngineConfig(obs_dim=6, act_dim=2, hidden_sizes=(64, 64), env_num=1, buffer_size=64), device=0)
    layered = Engine(EngineConfig(obs_dim=6, act_dim=2, hidden_sizes=(32, 32, 32), env_num=1, buffer_size=64), device=0)
    try:
        state = eng.train_state()
        for e, kw, reason in ((eng, dict(loss="nll", indices=idx[:1]), "deterministic"),
                              (eng, dict(indices=np.full((1, 16), ROWS)), "outside the stored rows"),
                              (empty, dict(), "store is empty"), (layered, dict(), "layered"),
                              (eng, dict(indices=idx[:1]), "member of a live group")):
            group = EngineSacGroup([eng]) if "group" in reason else None
            with pytest.raises(AssertionError, match=reason):
                e.bc_update(16, 1, **kw)
            if group is not None:
                group.close()
        assert eng.train_state() == state
    finally:
        eng.close(); empty.close(); layered.close()
