"""The clipped PPO-Lagrangian step in two launches (ppo_wgrad_kernel<H, false, true, true>: the weight-gradient launch exchanges its
workgroups' squared-norm partials inside the launch and applies clip + Adam itself) against the three-launch step of the same
library.  Every context gets its mode from fsrl_ppo_set_clip_fuse, so nothing here depends on the automatic rule.  The change moves
the clip and the Adam step into another launch, not their arithmetic (one summation routine, one Adam routine for both), so everything
is compared bit for bit: the logged statistics, the parameters, the Adam state (the training-state blob without the store: step
count, random streams, P with its mirrors, M, V), the last gradient norm and the KL stop.

Shapes: obs 8, act 2, 600 rows in minibatches of 256 (one 256-row minibatch and the merged last one of 344, both on the
one-workgroup-per-tile route), two passes, max_grad_norm 0.5, hidden 64 (28 blocks in the exchange) and 256 (244: all but twelve CUs
of an MI355X).  The mixed case adds a minibatch above 512 rows (split-K weight gradients and their own clip + Adam launch) next to a
512-row one that takes the two-launch step.  The forced fallback sets the wait limit to 0: every workgroup gives up before its first
poll, nothing is applied, and the update is replayed from its snapshot inside fsrl_ppo_end -- no wait runs out, nothing hangs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ENVS, DO, DA = 4, 8, 2


def _data(T, passes):
    rng = np.random.default_rng(11)
    d = dict(obs=rng.standard_normal((T + 1, ENVS, DO)).astype(np.float32),
             act=(0.3 * rng.standard_normal((T, ENVS, DA))).astype(np.float32),
             rew=rng.normal(0.5, 0.5, (T, ENVS)), cost=(rng.random((T, ENVS)) < 0.1).astype(np.float64),
             trunc=np.zeros((T, ENVS), bool), term=np.zeros((T, ENVS), bool))
    d["trunc"][T // 2 - 1::T // 2] = True
    d["perms"] = [rng.permutation(T * ENVS) for _ in range(passes)]
    return d


def _engine(H, mode, limit=-1, target_kl=None, T=150, d=None, **kw):
    from fsrl_amd.engine import Engine, EngineConfig
    eng = Engine(EngineConfig(env_num=ENVS, obs_dim=DO, act_dim=DA, hidden=H, max_grad_norm=0.5, target_kl=target_kl, **kw), device=0)
    eng.ppo_set_clip_fuse(mode, limit)
    eng.set_params((0.1 * np.random.default_rng(3).standard_normal(eng.n_params)).astype(np.float32))
    ids = np.arange(ENVS)
    for t in range(T):
        eng.push(ids, d["obs"][t], d["act"][t], d["rew"][t], d["cost"][t], d["term"][t], d["trunc"][t], d["obs"][t + 1])
    return eng


def _update(eng, d, batch, passes):
    stats, stopped = eng.ppo_update(np.array([0.5]), 1.0 / 1.5, batch, passes, perms=d["perms"][:passes])
    return dict(stats=stats.copy(), stopped=stopped, params=eng.get_params().copy(), state=eng.train_state(with_store=False),
                cf=eng.ppo_clip_fuse_stats())


def _same(a, b):
    assert a["stats"].shape == b["stats"].shape, (a["stats"].shape, b["stats"].shape)
    assert np.isfinite(a["stats"]).all() and np.isfinite(a["params"]).all()
    assert np.array_equal(a["stats"], b["stats"]), int((a["stats"] != b["stats"]).sum())
    assert np.array_equal(a["params"], b["params"]), int((a["params"] != b["params"]).sum())
    assert a["state"] == b["state"]                                     # adam_t, P with mirrors, M, V
    assert a["stopped"] == b["stopped"]
    assert a["cf"]["grad_norm"].tobytes() == b["cf"]["grad_norm"].tobytes(), (a["cf"], b["cf"])
    assert a["cf"]["grad_norm"] > 0


def _pair(H, batch, passes, T=150, target_kl=None, limit=-1):
    d = _data(T, passes)
    out = []
    for mode in (1, 0):
        eng = _engine(H, mode, limit if mode == 1 else -1, target_kl, T, d)
        out.append((eng, _update(eng, d, batch, passes)))
    return d, out


@pytest.mark.parametrize("H", [64, 256])
def test_two_launch_step_bit_identical_to_three_launches(H):
    _, ((e1, on), (e0, off)) = _pair(H, 256, 2)
    try:
        assert on["stats"].shape == (4, 11)
        assert on["cf"] == dict(on["cf"], available=True, fallbacks=0, steps=4, last_update_fused=True), on["cf"]
        assert off["cf"] == dict(off["cf"], available=False, fallbacks=0, steps=0, last_update_fused=False), off["cf"]
        _same(on, off)
        assert not np.array_equal(on["params"], np.zeros_like(on["params"]))
    finally:
        e1.close(); e0.close()


def test_kl_stop_is_the_same_pass_and_step_count():
    """The logged KL is the estimate mean(logp_old - logp): on actions that the policy did not draw it drifts below zero and never
    stops anything (measured on _data's actions: -0.0003, -0.0026, -0.0050, -0.0070, -0.0086 over five passes).  So the actions of
    this case are drawn from the initial policy, and the learning rate is 3e-3 so that ten steps move it visibly.  target_kl comes from
    the KL the three-launch run logs without a stop: the first pass whose mean KL is positive and above every earlier pass's is the
    pass the stop has to fall in, with 1.5 * target_kl half-way between that mean and the largest one before it; one more pass is
    asked for than the stop allows."""
    H, d, kw = 64, _data(150, 6), dict(lr=3e-3)
    probe = _engine(H, 0, d=d, **kw)
    mu, sigma = probe.actor_forward(d["obs"][:150].reshape(-1, DO))
    d["act"] = (mu + sigma * np.random.default_rng(5).standard_normal(mu.shape)).astype(np.float32).reshape(150, ENVS, DA)
    probe.close()
    probe = _engine(H, 0, d=d, **kw)
    kl = _update(probe, d, 256, 5)["stats"][:, 5].astype(np.float64).reshape(5, 2).mean(axis=1)
    probe.close()
    print("mean KL per pass", kl)
    want = next((j for j in range(5) if kl[j] > 0 and kl[j] > 1.05 * max([0.0, *kl[:j]])), None)
    assert want is not None, kl
    target = (max([0.0, *kl[:want]]) + kl[want]) / 2 / 1.5
    res = []
    for mode in (1, 0):
        eng = _engine(H, mode, target_kl=float(target), d=d, **kw)
        res.append(_update(eng, d, 256, want + 2))
        eng.close()
    on, off = res
    assert off["stopped"] == want and off["stats"].shape[0] == 2 * (want + 1), (off["stopped"], off["stats"].shape, kl, target)
    assert on["cf"]["steps"] == 2 * (want + 1) and on["cf"]["fallbacks"] == 0, on["cf"]
    _same(on, off)


def test_mixed_pass_keeps_the_split_k_route_for_the_large_minibatch():
    """1 100 rows in minibatches of 512: a 512-row step (two launches) and the merged 588-row one (split-K weight gradients, their
    sum, the logged row and the clip + Adam launch), two passes"""
    _, ((e1, on), (e0, off)) = _pair(256, 512, 2, T=275)
    try:
        assert on["stats"].shape == (4, 11)
        assert on["cf"]["steps"] == 2 and on["cf"]["fallbacks"] == 0 and on["cf"]["last_update_fused"], on["cf"]
        _same(on, off)
    finally:
        e1.close(); e0.close()


def test_forced_fallback_replays_the_update_and_turns_the_mode_off():
    d, ((e1, on), (e0, off)) = _pair(256, 256, 2, limit=0)
    try:
        assert on["cf"] == dict(on["cf"], available=False, fallbacks=1, last_update_fused=False), on["cf"]
        _same(on, off)
        # a second update on the context that fell back: three launches per step from the start, no further replay
        on2, off2 = _update(e1, d, 256, 2), _update(e0, d, 256, 2)
        assert on2["cf"]["fallbacks"] == 1 and on2["cf"]["steps"] == on["cf"]["steps"] and not on2["cf"]["available"], on2["cf"]
        _same(on2, off2)
        assert not np.array_equal(on2["params"], on["params"])
    finally:
        e1.close(); e0.close()
