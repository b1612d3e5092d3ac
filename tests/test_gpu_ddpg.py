"""GPU parity of the DDPG-Lagrangian update through the C ABI against the golden vectors
recorded from the unmodified reference.  Tolerances as for SAC: stats 5e-5 rel + 5e-6 abs, parameters
99 % within 5e-6 (Adam on noise-level gradients may move single entries by ~lr per step)."""
import numpy as np
import pytest

from test_oracle_ddpg import ddpg_setup

pytestmark = pytest.mark.gpu

KEYS = ["loss/rescaling", "loss/lagrangian", "loss/actor_safety", "loss/alpha_loss", "loss/alpha_value",
        "loss/actor_rew", "loss/actor_total", "loss/q0", "loss/q1", "loss/q_total"]


def _engine(cfg, g):
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig
    eng = Engine(EngineConfig(algo=_lib.ALGO_SAC_LAG, obs_dim=cfg["obs_dim"], act_dim=cfg["act_dim"],
                              hidden_sizes=tuple(cfg["hidden"]), n_critics=2, env_num=cfg["env_num"], buffer_size=cfg["buffer_size"],
                              gamma=cfg["gamma"], max_action=cfg["max_action"], target_kl=None))
    eng.sac_init(actor_lr=cfg["actor_lr"], critic_lr=cfg["critic_lr"], tau=cfg["tau"], n_step=cfg["n_step"],
                 use_lagrangian=cfg["use_lagrangian"], deterministic=True)
    eng.sac_set_params(g["theta_actor0"], g["theta_critics0"], 0.0)
    rows = g["env_rows"]; off = np.concatenate([[0], np.cumsum(rows)])
    for t in range(rows.max()):
        ids = [e for e in range(len(rows)) if t < rows[e]]
        sel = np.array([off[e] + t for e in ids])
        eng.push(ids, g["st_obs"][sel], g["st_act"][sel], g["st_rew"][sel], g["st_cost"][sel], g["st_terminated"][sel],
                 g["st_truncated"][sel], g["st_obs_next"][sel])
    return eng


# wide16: act_dim 16 and obs_dim + act_dim = 128, a compact fixture without target-network snapshots (1 MiB limit)
@pytest.mark.parametrize("name", ["small", "scaled", "nolag", "deep3", "wide16"])
def test_ddpg_updates_vs_golden(name):
    g, cfg, ocfg, store, index = ddpg_setup(name)
    eng = _engine(cfg, g)
    assert np.array_equal(eng.sac_get_params(0)[0], g["theta_actor0"]) and np.array_equal(eng.sac_get_params(3)[0], g["theta_actor0"])
    assert np.array_equal(eng.sac_get_params(1)[0], g["theta_critics0"])
    lag = g["lagrangian"] if cfg["use_lagrangian"] else np.zeros(0)
    resc = 1.0 / (lag.sum() + 1.0)
    ka = [str(k) for k in g["stats_actor_keys"]]; kc = [str(k) for k in g["stats_critic_keys"]]
    B, Da = cfg["batch_size"], cfg["act_dim"]
    zero = np.zeros((B, Da), np.float32)
    for u in range(cfg["n_updates"]):
        st = eng.sac_update(B, lag, resc, indices=g["indices"][u], eps_target=zero, eps_pi=zero)
        want = {**dict(zip(ka, g["stats_actor"][u])), **dict(zip(kc, g["stats_critic"][u]))}
        for j, k in enumerate(KEYS):
            if k in want:
                assert abs(st[j] - want[k]) <= 5e-5 * abs(want[k]) + 5e-6, (u, k, st[j], want[k])
    for which, key in ((0, "theta_actor_final"), (3, "theta_actor_old_final"), (1, "theta_critics_final"),
                       (2, "theta_critics_old_final")):
        if name == "wide16" and "old" in key:
            continue                  # not in the compact fixture: test_ddpg_variants_vs_oracle checks the targets at this shape
        d = np.abs(eng.sac_get_params(which)[0] - g[key])
        assert np.quantile(d, 0.99) <= 5e-6 and d.max() <= 2e-3, (key, np.quantile(d, 0.99), d.max())
    # collector-time action: deterministic = max_action * tanh(actor(s)); exploration adds N(0, 0.1^2)
    obs = g["st_obs"][:5]
    a_det = eng.actor_sample(obs, deterministic=True)
    assert np.abs(a_det).max() <= cfg["max_action"] + 1e-6
    a = np.stack([eng.actor_sample(obs, seed=3 if i == 0 else 0) for i in range(400)])
    assert abs((a - a_det).std() - 0.1) < 0.01
    eng.close()


def _synthetic_engine(Do, Da, hidden, rows, n_step, use_lag, max_action, seed, sub=128):
    """A DDPG-Lag context and the oracle on the same random replay store (fan-in scaled parameters: the heads stay off tanh's tails)."""
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig
    from helpers import fan_in_params as init, replay_problem
    from oracle.ddpg_lag import DDPGConfig, DDPGLagOracle
    rng = np.random.default_rng(seed)
    E = len(rows)
    hs = (hidden, hidden) if isinstance(hidden, int) else tuple(hidden)
    ocfg = DDPGConfig(obs_dim=Do, act_dim=Da, hidden=hs, max_action=max_action, gamma=0.98, n_step=n_step, tau=0.1,
                      actor_lr=1e-3, critic_lr=1e-3, use_lagrangian=use_lag)
    eng = Engine(EngineConfig(algo=_lib.ALGO_SAC_LAG, obs_dim=Do, act_dim=Da, hidden_sizes=hs, n_critics=2, env_num=E,
                              buffer_size=E * sub, gamma=0.98, max_action=max_action, target_kl=None))
    eng.sac_init(actor_lr=1e-3, critic_lr=1e-3, tau=0.1, n_step=n_step, use_lagrangian=use_lag, deterministic=True)
    o = DDPGLagOracle(ocfg)
    tha, thc = init(rng, o.aspec), np.concatenate([init(rng, o.cspec), init(rng, o.cspec)])
    o.set_params(tha, thc); eng.sac_set_params(tha, thc, 0.0)
    store, index, valid = replay_problem(rng, [eng], rows, Do, Da, lambda z: max_action * np.tanh(z), sub)
    return eng, o, store, index, valid, rng


DDPG_VARIANTS = [  # Do, Da, hidden, rows per env, batch, n_step, use_lagrangian, max_action, plan
    (112, 16, 128, [70, 50], 100, 2, True, 2.0, 0),         # Din = 128 with the widest head, batch not a multiple of 16
    (30, 16, 256, [33], 1, 1, False, 1.0, 0),               # a batch of one row at the widest hidden width, no Lagrangian term
    (9, 13, 64, [60, 45], 333, 3, True, 1.0, 0),            # odd action width, batch larger than the store
    (9, 13, 64, [60, 45], 333, 3, True, 1.0, 1),            # the same with split-K weight gradients below 512 rows (plan bit 0)
    (20, 16, 256, [100, 80, 120], 700, 2, True, 1.0, 0),    # above 512 rows: the split-K weight-gradient path
    (120, 8, 64, [64, 64], 64, 2, True, 1.0, 0),            # Din = 128 at H = 64
    (7, 11, (40, 72, 24), [40, 17], 64, 2, True, 1.0, 0),   # a layered context with a wide head
]


@pytest.mark.parametrize("Do,Da,hidden,rows,B,n_step,use_lag,amax,plan", DDPG_VARIANTS)
def test_ddpg_variants_vs_oracle(Do, Da, hidden, rows, B, n_step, use_lag, amax, plan):
    """Shapes outside the golden set (action heads up to 16 wide, critic inputs up to FSRL_MAX_OBS) against the oracle on the same
    random problem; bounds as test_sac_variants_vs_oracle."""
    eng, o, store, index, valid, rng = _synthetic_engine(Do, Da, hidden, rows, n_step, use_lag, amax, seed=Do + 10 * Da)
    eng.sac_set_plan(plan)
    lag = np.array([0.3]) if use_lag else np.zeros(0)
    zero = np.zeros((B, Da), np.float32)
    for u in range(3):
        idx = rng.choice(valid, B)
        sa, sc, _ = o.update(store, index, idx, lag, 1 / 1.3)
        st = eng.sac_update(B, lag, 1 / 1.3, indices=idx, eps_target=zero, eps_pi=zero)
        want = {**sa, **sc}
        for j, kname in enumerate(KEYS):
            if kname in want:
                w = float(want[kname])
                assert abs(st[j] - w) <= 1e-4 * abs(w) + 1e-5, (u, kname, st[j], w)
    for which, ref in ((0, o.actor_flat()), (3, o.actor_flat(old=True)), (1, o.critics_flat()), (2, o.critics_flat(old=True))):
        d = np.abs(eng.sac_get_params(which)[0] - ref)      # Adam: an entry whose gradient is rounding noise moves by +-lr per step
        assert np.quantile(d, 0.99) <= 5e-6 and d.max() <= 3 * 1e-3, (which, np.quantile(d, 0.99), d.max())
    eng.close()


def test_ddpg_on_a_wrapped_store_device_and_host_chains_agree():
    """act_dim 16, sub-buffers overwritten 2.5 times: the device sampler's n-step chains and the caller-RNG mode's (host) give
    bit-identical DDPG-Lag updates from the same indices."""
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig
    rng = np.random.default_rng(3)
    Do, Da, E, sub = 20, 16, 3, 40

    def make():
        eng = Engine(EngineConfig(algo=_lib.ALGO_SAC_LAG, obs_dim=Do, act_dim=Da, hidden_sizes=(128, 128), n_critics=2, env_num=E,
                                  buffer_size=E * sub, gamma=0.97, target_kl=None))
        eng.sac_init(n_step=3, deterministic=True)
        r = np.random.default_rng(0)
        eng.sac_set_params((0.1 * r.standard_normal(eng.n_sac_actor)).astype(np.float32),
                           (0.1 * r.standard_normal(eng.n_sac_critics)).astype(np.float32), 0.0)
        return eng
    dev, twin = make(), make()
    T = 100                                                  # 2.5 x the sub-buffer
    obs = rng.standard_normal((T + 1, E, Do)).astype(np.float32)
    act = np.tanh(rng.standard_normal((T, E, Da))).astype(np.float32)
    rew = rng.normal(0, 1, (T, E)); cost = (rng.random((T, E)) < 0.3).astype(np.float64)
    term = rng.random((T, E)) < 0.05; trunc = np.zeros((T, E), bool); trunc[12::13] = True
    for t in range(T):
        ids = [0, 1, 2] if t % 7 else [0, 2]                 # env 1 lags: different write cursors
        for e_ in (dev, twin):
            e_.push(ids, obs[t, ids], act[t, ids], rew[t, ids], cost[t, ids], term[t, ids], trunc[t, ids], obs[t + 1, ids])
    assert len(dev) == E * sub
    for u in range(6):
        dev.sac_update(64, [0.2], 1 / 1.2, seed=5 if u == 0 else 0, sync=False)
        idx, et, ep = dev.sac_last_sample(64)
        assert (idx >= 0).all() and (idx < E * sub).all()
        st = twin.sac_update(64, [0.2], 1 / 1.2, indices=idx, eps_target=et, eps_pi=ep)
    rows = dev.sac_drain()
    assert np.isfinite(rows).all() and np.array_equal(rows[-1], st)
    for which in (0, 1, 2, 3):
        assert np.array_equal(dev.sac_get_params(which)[0], twin.sac_get_params(which)[0])
    dev.close(); twin.close()


@pytest.mark.parametrize("batch", [256, 1024])
def test_ddpg_launch_plans_are_bit_identical(batch):
    """test_fused_launch_plan_is_bit_identical_to_the_separate_launches (test_gpu_sac.py) on a DDPG-Lag context at act_dim 16: every
    plan there (none sets bit 0, which changes sums) gives bit-identical statistics, parameters and samples over library-RNG updates,
    rows pushed in between, and a caller-index update."""
    Do, Da, rows = 20, 16, [200, 150, 180, 170]
    outs = []
    for plan in (0, 32, 64, 16, 6, 2, 8, 40, 14, 22):
        eng, o, store, index, valid, rng = _synthetic_engine(Do, Da, 128, rows, 2, True, 1.0, seed=11, sub=256)
        eng.sac_set_plan(plan)
        got = [eng.sac_update(batch, [0.5], 1 / 1.5, seed=7 if u == 0 else 0).copy() for u in range(12)]
        k = len(rows)                                       # new rows: the store changed, a prefetched sample must be dropped
        eng.push(np.arange(k), store["obs"][:k], store["act"][:k], np.ones(k), np.zeros(k), np.zeros(k, bool), np.zeros(k, bool),
                 store["obs"][:k])
        got += [eng.sac_update(batch, [0.5], 1 / 1.5, sync=(u % 2 == 0)) for u in range(6)]
        got = [r.copy() for r in got if r is not None]
        idx = np.random.default_rng(1).choice(valid, batch)
        zero = np.zeros((batch, Da), np.float32)
        got.append(eng.sac_update(batch, [0.5], 1 / 1.5, indices=idx, eps_target=zero, eps_pi=zero).copy())
        outs.append((np.stack(got), eng.sac_get_params(0)[0], eng.sac_get_params(1)[0], eng.sac_get_params(2)[0],
                     eng.sac_get_params(3)[0], eng.sac_last_sample(batch)[0].copy()))
        eng.close()
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert np.array_equal(a, b)
    assert np.isfinite(outs[0][0]).all()


def test_ddpg_facade_matches_reference_and_agent_learns(tmp_path):
    import json
    from fsrl_amd.agent import DDPGLagAgent
    from fsrl_amd.data import Batch, HipVectorReplayBuffer
    from fsrl_amd.env import Box, SyntheticSafetyVectorEnv
    from fsrl_amd.policy import DDPGLagrangian, SACLagrangian
    from fsrl_amd.utils import BaseLogger
    from fsrl_amd.utils.net import Actor, Critic, Net
    import torch
    g, cfg, ocfg, store, index = ddpg_setup("small")
    Do, Da, h = cfg["obs_dim"], cfg["act_dim"], tuple(cfg["hidden"])
    actor = Actor(Net((Do, ), hidden_sizes=h), (Da, ), max_action=cfg["max_action"])
    critics = [Critic(Net((Do, ), (Da, ), hidden_sizes=h, concat=True)) for _ in range(2)]
    SACLagrangian._unflat([actor], g["theta_actor0"]); SACLagrangian._unflat(critics, g["theta_critics0"])

    class Cap:
        def __init__(self): self.rows = []
        def store(self, tab=None, **kw): self.rows.append(dict(kw))
        def print(self, *a, **k): pass
    log = Cap()
    pol = DDPGLagrangian(actor, critics, torch.optim.Adam(actor.parameters(), lr=cfg["actor_lr"]),
                         torch.optim.Adam(torch.nn.ModuleList(critics).parameters(), lr=cfg["critic_lr"]), logger=log,
                         tau=cfg["tau"], n_step=cfg["n_step"], cost_limit=cfg["cost_limit"], gamma=cfg["gamma"],
                         observation_space=Box(-np.inf, np.inf, (Do, )), action_space=Box(-1, 1, (Da, )), device=0,
                         env_num=cfg["env_num"], reference_rng=True)
    pol.train()
    buf = HipVectorReplayBuffer(pol.engine, cfg["buffer_size"], cfg["env_num"])
    rows = g["env_rows"]; off = np.concatenate([[0], np.cumsum(rows)])
    for t in range(rows.max()):
        ids = np.array([e for e in range(len(rows)) if t < rows[e]])
        sel = np.array([off[e] + t for e in ids])
        buf.add(Batch(obs=g["st_obs"][sel], act=g["st_act"][sel], rew=g["st_rew"][sel], info={"cost": g["st_cost"][sel]},
                      terminated=g["st_terminated"][sel], truncated=g["st_truncated"][sel], obs_next=g["st_obs_next"][sel]),
                buffer_ids=ids)
    pol.pre_update_fn(stats_train={"cost": cfg["cost_stat"]})
    import random
    seed = cfg["seed"] + 7
    random.seed(seed); np.random.seed(seed); torch.manual_seed(seed)
    ka = [str(k) for k in g["stats_actor_keys"]]; kc = [str(k) for k in g["stats_critic_keys"]]
    for u in range(cfg["n_updates"]):
        pol.update(cfg["batch_size"], buf)
        np.testing.assert_allclose([log.rows[2 * u][k] for k in ka], g["stats_actor"][u], rtol=5e-5, atol=5e-6)
        np.testing.assert_allclose([log.rows[2 * u + 1][k] for k in kc], g["stats_critic"][u], rtol=5e-5, atol=5e-6)
    sd = pol.state_dict()
    assert "actor_old.last.model.0.weight" in sd and "critics_old.1.preprocess.model.model.0.weight" in sd
    d = np.abs(SACLagrangian._flat([pol.actor_old]) - g["theta_actor_old_final"])
    assert np.quantile(d, 0.99) <= 5e-6
    env = SyntheticSafetyVectorEnv(env_num=4, episode_len=30, seed=2)
    agent = DDPGLagAgent(env, BaseLogger(str(tmp_path), name="g"), cost_limit=10, device="cuda:0", seed=1,
                         hidden_sizes=(64, 64), training_num=4, buffer_size=2000)
    ep, stat, info = agent.learn(env, None, epoch=2, episode_per_collect=4, step_per_epoch=240, update_per_step=0.2,
                                 batch_size=32, verbose=False, save_ckpt=False)
    assert ep == 2 and np.isfinite(list(stat.values())).all() and "loss/q_total" in stat
