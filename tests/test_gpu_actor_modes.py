"""The actor-mean option of the stochastic replay agents on the device (fsrl_sac_config.actor_mean / fsrl_cvpo_config.actor_mean):
SAC-Lag with ActorProb(unbounded=False) -- mu = max_action * tanh(head), what the reference's sacl_cfg.py trains with -- and CVPO
with ActorProb(unbounded=True), mu = head (cvpo_cfg.py MujocoBaseCfg).

* golden parity against the UNMODIFIED reference run in the new mode (tests/golden/gen_golden_actor_modes.py), indices and noise
  injected, at the bars of test_sac_updates_vs_golden / test_cvpo_updates_vs_golden: SAC stats 5e-5 rel + 5e-6 abs, SAC parameters
  0.99-quantile <= 5e-6 and max <= 5e-4; CVPO stats 1e-4 rel + 1e-5 abs, duals rtol 1e-4 with atol 1e-6 / 1e-5, CVPO parameters
  0.99-quantile <= 1e-5 and max <= 4e-3.  Every fixture records that the reference in the OTHER mode sits at least 10 bars away
  (tests/test_actor_modes_host.py), so a device that ignored the option fails here;
* the explicit value of today's mode (SAC 1, CVPO 2) against the option left out: bit for bit;
* the collector's actor against the torch mirror (1e-6, the bar of test_gpu_cvpo.py), resident against launched: bit for bit;
* groups in the new mode: a group of one and three layered members against their solo twins, bit for bit; refusals;
* the agents' facade."""
import numpy as np
import pytest

from test_oracle_cvpo import cvpo_setup, final_stride
from test_oracle_sac import sac_setup

pytestmark = pytest.mark.gpu

SAC_KEYS = ["loss/rescaling", "loss/lagrangian", "loss/actor_safety", "loss/alpha_loss", "loss/alpha_value",
            "loss/actor_rew", "loss/actor_total", "loss/q0", "loss/q1", "loss/q_total"]
CVPO_KW = ("actor_lr", "critic_lr", "tau", "n_step", "double_critic", "sample_act_num", "estep_iter_num", "mstep_iter_num",
           "estep_kl", "estep_dual_max", "estep_dual_lr", "mstep_kl_mu", "mstep_kl_std", "mstep_dual_max", "mstep_dual_lr")
MODE = {None: {}, True: {"unbounded": True}, False: {"unbounded": False}}


def _push_store(eng, g):
    rows = g["env_rows"]
    off = np.concatenate([[0], np.cumsum(rows)])
    for t in range(rows.max()):
        ids = [e for e in range(len(rows)) if t < rows[e]]
        sel = np.array([off[e] + t for e in ids])
        ptr, *_ = eng.push(ids, g["st_obs"][sel], g["st_act"][sel], g["st_rew"][sel], g["st_cost"][sel],
                           g["st_terminated"][sel], g["st_truncated"][sel], g["st_obs_next"][sel])
        assert np.array_equal(ptr, g["slots"][sel])


def _sac_engine(cfg, g, unbounded):
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig
    eng = Engine(EngineConfig(algo=_lib.ALGO_SAC_LAG, obs_dim=cfg["obs_dim"], act_dim=cfg["act_dim"], hidden_sizes=tuple(cfg["hidden"]),
                              n_critics=2, env_num=cfg["env_num"], buffer_size=cfg["buffer_size"], gamma=cfg["gamma"],
                              max_action=cfg["max_action"], target_kl=None))
    eng.sac_init(actor_lr=cfg["actor_lr"], critic_lr=cfg["critic_lr"], alpha_lr=cfg["alpha_lr"], tau=cfg["tau"], alpha=cfg["alpha"],
                 n_step=cfg["n_step"], auto_alpha=cfg["auto_alpha"], **MODE[unbounded])
    eng.sac_set_params(g["theta_actor0"], g["theta_critics0"], 0.0)
    _push_store(eng, g)
    return eng


def _cvpo_engine(cfg, g, qc_thres, unbounded):
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig
    eng = Engine(EngineConfig(algo=_lib.ALGO_SAC_LAG, obs_dim=cfg["obs_dim"], act_dim=cfg["act_dim"], hidden_sizes=tuple(cfg["hidden"]),
                              n_critics=2, env_num=cfg["env_num"], buffer_size=cfg["buffer_size"], gamma=cfg["gamma"],
                              max_action=cfg["max_action"], target_kl=None))
    eng.cvpo_init(qc_thres, **{k: cfg[k] for k in CVPO_KW}, **MODE[unbounded])
    eng.sac_set_params(g["theta_actor0"], g["theta_critics0"], 0.0)
    _push_store(eng, g)
    return eng


def _sac_run(eng, g, cfg):
    lag = g["lagrangian"]
    resc = 1.0 / (lag.sum() + 1.0)
    rows = [eng.sac_update(cfg["batch_size"], lag, resc, indices=g["indices"][u], eps_target=g["eps_target"][u],
                           eps_pi=g["eps_pi"][u]).copy() for u in range(cfg["n_updates"])]
    return np.stack(rows), [eng.sac_get_params(w)[0] for w in (0, 1, 2)], eng.sac_get_params(0)[1]


def _cvpo_run(eng, g, cfg):
    rows, duals, olds, u = [], [], [], 0
    for c in range(cfg["cycles"]):
        eng.cvpo_pre_update()
        for _ in range(cfg["updates_per_cycle"]):
            rows.append(eng.cvpo_update(cfg["batch_size"], indices=g["indices"][u], eps_target=g["eps_target"][u],
                                        eps_particles=g["eps_particles"][u]).copy())
            duals.append(eng.cvpo_duals().copy())
            u += 1
        eng.cvpo_post_update()
        olds.append(eng.sac_get_params(3)[0])
    return np.stack(rows), np.stack(duals), olds, [eng.sac_get_params(w)[0] for w in (0, 1, 2)]


# ---------------------------------------------------------------- golden parity
@pytest.mark.parametrize("splitk", [0, 1])      # weight gradients: 0 = one workgroup per output tile, 1 = split-K
@pytest.mark.parametrize("name", ["bounded_small", "bounded_c4", "bounded_deep3"])
def test_sac_bounded_mean_vs_reference(name, splitk):
    g, cfg, ocfg, store, index = sac_setup(name)
    assert cfg["unbounded"] is False
    eng = _sac_engine(cfg, g, False)
    assert eng.actor_unbounded is False
    eng.sac_set_plan(splitk)
    st, th, alpha = _sac_run(eng, g, cfg)
    eng.close()
    ka = [str(k) for k in g["stats_actor_keys"]]; kc = [str(k) for k in g["stats_critic_keys"]]
    for u in range(cfg["n_updates"]):
        want = {**dict(zip(ka, g["stats_actor"][u])), **dict(zip(kc, g["stats_critic"][u]))}
        for j, k in enumerate(SAC_KEYS):
            if k in want:
                print(name, splitk, u, k, st[u, j], want[k])
                assert abs(st[u, j] - want[k]) <= 5e-5 * abs(want[k]) + 5e-6, (u, k, st[u, j], want[k])
    s = int(g.get("theta_final_stride", 1))
    for got, key in ((th[0], "theta_actor_final"), (th[1][::s], "theta_critics_final"), (th[2][::s], "theta_critics_old_final")):
        d = np.abs(got - g[key])
        print(name, splitk, key, np.quantile(d, 0.99), d.max())
        assert np.quantile(d, 0.99) <= 5e-6 and d.max() <= 5e-4, (key, np.quantile(d, 0.99), d.max())
    assert abs(alpha - float(g["alpha_final"])) < 1e-6


@pytest.mark.parametrize("name", ["unbounded_small", "unbounded_double", "unbounded_deep3"])
def test_cvpo_unbounded_mean_vs_reference(name):
    g, cfg, ocfg, store, index = cvpo_setup(name)
    assert cfg["unbounded"] is True
    eng = _cvpo_engine(cfg, g, ocfg.qc_thres, True)
    assert eng.actor_unbounded is True
    st, duals, olds, th = _cvpo_run(eng, g, cfg)
    eng.close()
    keys = [str(k) for k in g["stats_keys"]]
    for u in range(len(st)):
        for j, k in enumerate(keys):
            print(name, u, k, st[u, j], g["stats"][u, j])
            assert abs(st[u, j] - g["stats"][u, j]) <= 1e-4 * abs(g["stats"][u, j]) + 1e-5, (u, k, st[u, j], g["stats"][u, j])
        np.testing.assert_allclose(duals[u, :2], g["estep_dual"][u], rtol=1e-4, atol=1e-6, err_msg=f"u={u}")
        np.testing.assert_allclose(duals[u, 2:], g["mstep_dual"][u], rtol=1e-4, atol=1e-5, err_msg=f"u={u}")
    close = lambda d: np.quantile(d, 0.99) <= 1e-5 and d.max() <= 4e-3          # noqa: E731  (test_gpu_cvpo.py's parameter bars)
    for c, old in enumerate(olds):
        d = np.abs(old - g["theta_actor_old_cycles"][c])
        assert close(d), (c, np.quantile(d, 0.99), d.max())
    for which, key in ((0, "theta_actor_final"), (1, "theta_critics_final"), (2, "theta_critics_old_final")):
        d = np.abs((th[which][::final_stride(g)] if which else th[which]) - g[key])
        print(name, key, np.quantile(d, 0.99), d.max())
        assert close(d), (key, np.quantile(d, 0.99), d.max())


# ---------------------------------------------------------------- the explicit default is today's path
def test_explicit_default_mode_is_bit_identical_to_the_option_left_out():
    g, cfg, ocfg, store, index = sac_setup("small")
    cfg = dict(cfg, max_action=1.0)
    outs = []
    for mode in (None, True):                       # SAC-Lag's mode today: unbounded (actor_mean 1)
        eng = _sac_engine(cfg, g, mode)
        assert eng.actor_unbounded is True
        outs.append(_sac_run(eng, g, cfg))
        eng.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][2] == outs[1][2]
    for a, b in zip(outs[0][1], outs[1][1]):
        assert np.array_equal(a, b)
    g, cfg, ocfg, store, index = cvpo_setup("small")
    outs = []
    for mode in (None, False):                      # CVPO's mode today: max_action * tanh (actor_mean 2)
        eng = _cvpo_engine(cfg, g, ocfg.qc_thres, mode)
        assert eng.actor_unbounded is False
        outs.append(_cvpo_run(eng, g, cfg))
        eng.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    for a, b in zip(outs[0][2] + outs[0][3], outs[1][2] + outs[1][3]):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------- collector
def _plain_engine(kind, hs, Do, Da, unbounded, seed=0, env_num=20, amax=1.5, T=0, key=None, **kw):
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig
    eng = Engine(EngineConfig(algo=_lib.ALGO_SAC_LAG, obs_dim=Do, act_dim=Da, hidden_sizes=tuple(hs), n_critics=2, env_num=env_num,
                              buffer_size=env_num * 400, gamma=0.99, max_action=amax, target_kl=None))
    if kind == "cvpo":
        eng.cvpo_init(0.1, sample_act_num=8, **MODE[unbounded], **kw)
    else:
        eng.sac_init(deterministic=(kind == "ddpgl"), **MODE[unbounded], **kw)
    rng = np.random.default_rng(100 + seed)
    # parameters of 0.1 N(0, 1): head outputs of a few tenths, so fp32 rounding stays two orders below the 1e-6 the mirror is held to
    eng.sac_set_params(0.1 * rng.standard_normal(eng.n_sac_actor).astype(np.float32),
                       0.1 * rng.standard_normal(eng.n_sac_critics).astype(np.float32), float(np.log(0.2)))
    ids = np.arange(env_num)
    for t in range(T):
        term = rng.random(env_num) < 0.03
        eng.push(ids, rng.standard_normal((env_num, Do)).astype(np.float32), np.tanh(rng.standard_normal((env_num, Da))).astype(np.float32),
                 rng.normal(0.5, 0.5, env_num), (rng.random(env_num) < 0.2).astype(np.float64), term,
                 np.full(env_num, (t + 1) % 50 == 0) & ~term, rng.standard_normal((env_num, Do)).astype(np.float32))
    if key is not None:
        eng.actor_sample(np.zeros((1, Do), np.float32), seed=key)      # keys the collector's noise stream
    return eng


def _mirror(eng, hs, Do, Da, unbounded, amax):
    import torch
    from fsrl_amd.policy import SACLagrangian
    from fsrl_amd.utils.net import ActorProb, Net
    actor = ActorProb(Net((Do, ), hidden_sizes=tuple(hs)), (Da, ), max_action=amax, conditioned_sigma=True, unbounded=unbounded)
    SACLagrangian._unflat([actor], eng.sac_get_params(0)[0])

    def fwd(obs):
        with torch.no_grad():
            (mu, sigma), _ = actor(obs)
        return mu.numpy(), sigma.numpy()
    return fwd


@pytest.mark.parametrize("hs", [(128, 128), (48, 64, 40)])       # fused, layered
@pytest.mark.parametrize("kind,unbounded", [("sacl", False), ("cvpo", True)])
def test_collector_actor_matches_the_host_mirror(kind, unbounded, hs):
    Do, Da, amax = 8, 8, 1.5
    eng = _plain_engine(kind, hs, Do, Da, unbounded, amax=amax)
    obs = np.random.default_rng(3).standard_normal((20, Do)).astype(np.float32)          # a full tile and a ragged one
    mu_h, sg_h = _mirror(eng, hs, Do, Da, unbounded, amax)(obs)
    other = _mirror(eng, hs, Do, Da, not unbounded, amax)(obs)[0]
    assert np.abs(mu_h - other).max() > 1e-2                      # the inputs tell the two modes apart
    mu, sigma = eng.sac_actor_forward(obs)
    print(kind, hs, np.abs(mu - mu_h).max(), np.abs(sigma / sg_h - 1).max())
    np.testing.assert_allclose(mu, mu_h, rtol=0, atol=1e-6)
    np.testing.assert_allclose(sigma, sg_h, rtol=0, atol=1e-6)
    det_resident = eng.actor_sample(obs, deterministic=True)
    want = np.tanh(mu_h) if kind == "sacl" else mu_h              # SAC squashes the (deterministic) draw, CVPO does not
    np.testing.assert_allclose(det_resident, want, rtol=0, atol=1e-6)
    eng.actor_release()
    eng.actor_set_resident(False)                                 # the launched actor: the same bits
    assert np.array_equal(eng.actor_sample(obs, deterministic=True), det_resident)
    mu2, sigma2 = eng.sac_actor_forward(obs)
    assert np.array_equal(mu2, mu) and np.array_equal(sigma2, sigma)
    eng.close()


# ---------------------------------------------------------------- groups
class _Log:
    def __init__(self):
        self.rows = []

    def store(self, tab=None, **kw):
        self.rows.append(sorted(kw.items()))

    def store_rows(self, keys, rows):
        self.rows.append((list(keys), np.asarray(rows).tolist()))

    def print(self, *a):
        pass


def _policies(algo, hs, k, T0=90):
    """k agents in the new mode, members differing in seed, data and store length; -> (agents, buffers)"""
    from fsrl_amd.agent import CVPOAgent, SACLagAgent
    from fsrl_amd.data import HipVectorReplayBuffer
    from fsrl_amd.env import SyntheticSafetyVectorEnv
    agents, bufs = [], []
    for s in range(k):
        env = SyntheticSafetyVectorEnv(env_num=4, obs_dim=8, act_dim=2, episode_len=30, seed=10 + s)
        if algo == "sacl":
            ag = SACLagAgent(env, None, cost_limit=10, device="cuda:0", seed=1 + s, hidden_sizes=hs, training_num=4, buffer_size=2000,
                             unbounded=False)
        else:
            ag = CVPOAgent(env, None, cost_limit=10, device="cuda:0", seed=1 + s, hidden_sizes=hs, training_num=4, buffer_size=2000,
                           unbounded=True, sample_act_num=8, mstep_kl_mu=2e-4, mstep_kl_std=2e-6)
        assert ag.policy.engine.actor_unbounded is (algo == "cvpo")
        ag.policy.logger = _Log()
        ag.policy.train()
        eng = ag.policy.engine
        bufs.append(HipVectorReplayBuffer(eng, 2000, 4))
        rng = np.random.default_rng(50 + s)
        ids = np.arange(4)
        for t in range(T0 + 23 * s):
            term = rng.random(4) < 0.03
            eng.push(ids, rng.standard_normal((4, 8)).astype(np.float32), np.tanh(rng.standard_normal((4, 2))).astype(np.float32),
                     rng.normal(0.5, 0.5, 4), (rng.random(4) < 0.2).astype(np.float64), term, np.full(4, (t + 1) % 30 == 0) & ~term,
                     rng.standard_normal((4, 8)).astype(np.float32))
        agents.append(ag)
    return agents, bufs


def _policy_state(ag, algo):
    eng = ag.policy.engine
    ag.policy.post_update_fn(stats_train={"cost": 12.0})           # drains the statistics rows into the logger
    which = (0, 1, 2, 3) if algo == "cvpo" else (0, 1, 2)
    return [eng.sac_get_params(w)[0] for w in which], eng.sac_get_params(0)[1], ag.policy.logger.rows


@pytest.mark.parametrize("algo,hs,k,n", [("sacl", (64, 64), 1, [6]), ("sacl", (48, 64, 40), 3, [5, 3, 4]),
                                         ("cvpo", (64, 64), 1, [5]), ("cvpo", (48, 64, 40), 3, [4, 2, 3])])
def test_policy_groups_in_the_new_mode_are_their_members_own_updates(algo, hs, k, n):
    """SACPolicyGroup / CVPOPolicyGroup with every member in the new mode: a group of one (fused) and three layered members are
    bit-identical to their solo twins -- parameters, targets, alpha and every logged row"""
    from fsrl_amd.policy import CVPOPolicyGroup, SACPolicyGroup
    B = 40                                           # two full tiles and a ragged one
    grouped, gbufs = _policies(algo, hs, k)
    solo, sbufs = _policies(algo, hs, k)
    for ag in grouped + solo:
        ag.policy.pre_update_fn(stats_train={"cost": 12.0})
    grp = (SACPolicyGroup if algo == "sacl" else CVPOPolicyGroup)([a.policy for a in grouped])
    grp.update(gbufs, B, n)
    for ag, buf, ni in zip(solo, sbufs, n):
        for _ in range(ni):
            ag.policy.update(B, buf)
    for i in range(k):
        x, y = _policy_state(grouped[i], algo), _policy_state(solo[i], algo)
        for j, (u, v) in enumerate(zip(x[0], y[0])):
            assert np.array_equal(u, v), (i, j, np.abs(u - v).max())
        assert x[1] == y[1] and x[2] == y[2] and len(x[2]) > 0, i
        assert np.isfinite(x[0][0]).all()
    grp.close()
    for ag in grouped + solo:
        ag.policy.engine.close()


@pytest.mark.parametrize("kind,unbounded,hs,envs", [("sacl", False, (128, 128), (20, )), ("cvpo", True, (128, 128), (20, )),
                                                    ("sacl", False, (48, 64, 40), (3, 20, 1)), ("cvpo", True, (48, 64, 40), (3, 20, 1))])
def test_collect_group_in_the_new_mode_is_every_members_collect_step(kind, unbounded, hs, envs):
    """EngineCollectGroup with every member in the new mode: a group of one (fused: the group's resident kernel) and three layered
    members give each member's own collect_step bit for bit, deterministic and sampled, and the mirror's mean"""
    from fsrl_amd.engine import EngineCollectGroup
    from test_gpu_collect_group import _same_step, _solo_steps
    from test_gpu_group_collect import _close, _random_step, _same_stores, _step_b
    Do, Da, amax = 8, 2, 1.5
    mk = lambda i, e: _plain_engine(kind, hs, Do, Da, unbounded, seed=i, env_num=e, amax=amax, key=1000 + i)     # noqa: E731
    a = [mk(i, e) for i, e in enumerate(envs)]
    b = [mk(i, e) for i, e in enumerate(envs)]
    cg = EngineCollectGroup(b)
    rng = np.random.default_rng(7)
    script = []
    for step in range(8):
        prevs, oas = _random_step(rng, envs, Do, Da, k_act_zero=0.0)
        script.append((prevs, oas, step % 3 == 0, (0, 1, 2)[step % 3], None, None))
    want = _solo_steps(a, script)
    for step, st in enumerate(script):
        got = _step_b(cg, *st)
        _same_step(want[step], got, step)
        if st[2]:                                    # a deterministic step: the policy action is the mirror's mean (SAC: squashed)
            for i, o in enumerate(st[1]):
                mu = _mirror(b[i], hs, Do, Da, unbounded, amax)(o)[0]
                np.testing.assert_allclose(got[i][0], np.tanh(mu) if kind == "sacl" else mu, rtol=0, atol=1e-6)
    cg.actor_release()
    _same_stores(a, b)
    _close(cg, a, b)


def test_members_that_disagree_on_the_option_and_ddpg_with_it_are_refused():
    from fsrl_amd.engine import EngineCollectGroup, EngineCvpoGroup, EngineSacGroup
    from fsrl_amd.policy import CVPOPolicyGroup, SACPolicyGroup
    Do, Da = 8, 2
    for hs in ((64, 64), (48, 64, 40)):
        s_def, s_new = _plain_engine("sacl", hs, Do, Da, None, env_num=4), _plain_engine("sacl", hs, Do, Da, False, env_num=4)
        c_def, c_new = _plain_engine("cvpo", hs, Do, Da, None, env_num=4), _plain_engine("cvpo", hs, Do, Da, True, env_num=4)
        for Group, pair in ((EngineSacGroup, (s_def, s_new)), (EngineSacGroup, (s_new, s_def)), (EngineCvpoGroup, (c_def, c_new)),
                            (EngineCvpoGroup, (c_new, c_def)), (EngineCollectGroup, (s_def, s_new)), (EngineCollectGroup, (c_new, c_def))):
            with pytest.raises(AssertionError, match="actor_mean"):         # FSRL_EINVAL, the option named
                Group(list(pair))
        # the explicit value of the default mode agrees with the option left out
        s_exp, c_exp = _plain_engine("sacl", hs, Do, Da, True, env_num=4), _plain_engine("cvpo", hs, Do, Da, False, env_num=4)
        for Group, pair in ((EngineSacGroup, (s_def, s_exp)), (EngineCvpoGroup, (c_def, c_exp)), (EngineCollectGroup, (s_exp, s_def))):
            Group(list(pair)).close()
        for e in (s_def, s_new, c_def, c_new, s_exp, c_exp):
            e.close()
    # the policy groups build these engine groups: the same refusal
    (p_new, ), _ = _policies("sacl", (64, 64), 1, T0=0)
    from fsrl_amd.agent import SACLagAgent
    from fsrl_amd.env import SyntheticSafetyVectorEnv
    p_def = SACLagAgent(SyntheticSafetyVectorEnv(env_num=4, obs_dim=8, act_dim=2, episode_len=30, seed=3), None, device="cuda:0",
                        hidden_sizes=(64, 64), training_num=4, buffer_size=2000)
    with pytest.raises(AssertionError, match="actor_mean"):
        SACPolicyGroup([p_def.policy, p_new.policy])
    p_def.policy.engine.close(); p_new.policy.engine.close()
    # DDPG-Lag: tianshou's Actor has no such option
    for mode in (True, False):
        with pytest.raises(AssertionError, match="actor_mean"):
            _plain_engine("ddpgl", (64, 64), Do, Da, mode, env_num=4)
    _plain_engine("ddpgl", (64, 64), Do, Da, None, env_num=4).close()


# ---------------------------------------------------------------- facade
def _load(prefix, module, sd):
    module.load_state_dict({k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}, strict=True)


@pytest.mark.parametrize("algo", ["sacl", "cvpo"])
def test_agents_build_act_and_learn_in_the_new_mode(algo, tmp_path):
    import torch
    from fsrl_amd.agent import CVPOAgent, SACLagAgent
    from fsrl_amd.data import Batch
    from fsrl_amd.env import SyntheticSafetyVectorEnv
    from fsrl_amd.utils import BaseLogger
    from fsrl_amd.utils.net import ActorProb, DoubleCritic, Net, SingleCritic
    env = SyntheticSafetyVectorEnv(env_num=4, obs_dim=8, act_dim=2, episode_len=30, seed=2)
    log = BaseLogger(str(tmp_path), name="g")
    if algo == "sacl":      # the values of the reference's sacl_cfg.TrainCfg that reach the agent
        agent = SACLagAgent(env, log, cost_limit=10, device="cuda:0", seed=1, actor_lr=5e-4, critic_lr=1e-3, hidden_sizes=(128, 128),
                            auto_alpha=True, alpha_lr=3e-4, alpha=0.005, tau=0.05, n_step=2, use_lagrangian=True,
                            lagrangian_pid=(0.05, 0.0005, 0.1), rescaling=True, gamma=0.97, conditioned_sigma=True, unbounded=False,
                            last_layer_scale=False, deterministic_eval=True, action_scaling=True, action_bound_method="clip",
                            training_num=4, buffer_size=2000)
        unbounded = False
    else:                   # cvpo_cfg.MujocoBaseCfg's
        agent = CVPOAgent(env, log, cost_limit=25, device="cuda:0", seed=1, estep_iter_num=1, estep_kl=0.02, estep_dual_max=20,
                          estep_dual_lr=0.02, sample_act_num=16, mstep_iter_num=1, mstep_kl_mu=0.005, mstep_kl_std=0.0005,
                          mstep_dual_max=0.5, mstep_dual_lr=0.1, actor_lr=5e-4, critic_lr=1e-3, gamma=0.995, n_step=3, tau=0.05,
                          hidden_sizes=(128, 128), double_critic=False, conditioned_sigma=True, unbounded=True, last_layer_scale=False,
                          deterministic_eval=True, action_scaling=True, action_bound_method="clip", training_num=4, buffer_size=2000)
        unbounded = True
    pol = agent.policy
    assert pol.actor._unbounded is unbounded and pol.engine.actor_unbounded is unbounded
    # host and device actor agree on deterministic actions
    obs = (0.3 * np.random.default_rng(0).standard_normal((20, 8))).astype(np.float32)
    pol.eval()
    with torch.no_grad():
        host = pol(Batch(obs=torch.as_tensor(obs))).act.numpy()
    np.testing.assert_allclose(pol.engine.actor_sample(obs, deterministic=True), host, rtol=0, atol=1e-6)
    pol.engine.actor_release()
    pol.train()
    ep, stat, info = agent.learn(env, None, epoch=1, episode_per_collect=4, step_per_epoch=240, update_per_step=0.2, batch_size=32,
                                 verbose=False, save_ckpt=False, device_actor=True)
    assert ep == 1 and np.isfinite(list(stat.values())).all() and "loss/q_total" in stat
    # the trained state dict is the reference's wire format: strict load into reference-shaped modules, which then act as the device does
    sd = pol.state_dict()
    actor = ActorProb(Net((8, ), hidden_sizes=(128, 128)), (2, ), max_action=float(pol.actor._max), conditioned_sigma=True,
                      unbounded=unbounded)
    qnet = lambda: Net((8, ), (2, ), hidden_sizes=(128, 128), concat=True)      # noqa: E731
    mk = (lambda: DoubleCritic(qnet(), qnet())) if algo == "sacl" else (lambda: SingleCritic(qnet()))
    _load("actor.", actor, sd)
    for i in range(2):
        _load(f"critics.{i}.", mk(), sd)
        _load(f"critics_old.{i}.", mk(), sd)
    if algo == "cvpo":
        _load("actor_old.", ActorProb(Net((8, ), hidden_sizes=(128, 128)), (2, ), conditioned_sigma=True, unbounded=True), sd)
    with torch.no_grad():
        (mu, sigma), _ = actor(obs)
    mu_d, sg_d = pol.engine.sac_actor_forward(obs)
    np.testing.assert_allclose(mu_d, mu.numpy(), rtol=0, atol=1e-6)
    np.testing.assert_allclose(sg_d, sigma.numpy(), rtol=2e-6, atol=0)      # two fp32 exponentials of log sigmas a few 1e-7 apart
    pol.engine.close()


def test_conditioned_sigma_false_is_still_refused_by_name():
    from fsrl_amd.agent import CVPOAgent, SACLagAgent
    from fsrl_amd.env import SyntheticSafetyVectorEnv
    env = SyntheticSafetyVectorEnv(env_num=4, obs_dim=8, act_dim=2, episode_len=30, seed=2)
    for Agent in (SACLagAgent, CVPOAgent):
        with pytest.raises(AssertionError, match="conditioned_sigma"):
            Agent(env, None, device="cuda:0", conditioned_sigma=False, training_num=4, buffer_size=2000)
