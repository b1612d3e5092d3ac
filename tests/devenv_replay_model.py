"""Host model of the replay agents' head arithmetic in a device collect (kernels_devcollect.hpp DC_HEAD_GAUSS / DC_HEAD_DDPG).  TEST
INFRASTRUCTURE ONLY.  numpy; written from include/fsrl_hip.h "fsrl_collect_device" and the host's sac_actor_finish / actor_draw,
not from the kernel.

    SAC-Lag   a = tanh(m + sigma eps)        deterministic: tanh(m)
    CVPO      a = m + sigma eps              deterministic: m
    DDPG-Lag  a = m + sigma eps              deterministic: m          (sigma = exploration_sigma, m = max_action tanh(head))
    Gaussian heads: m = head or max_action tanh(head), sigma = exp(clamp(log-sigma head, -20, 2))

Every formula exists in `dtype=np.float64` (the reference distances are measured to) and `dtype=np.float32` (the device's
arithmetic restated: every operation rounded on its own)."""
import numpy as np

F32, F64 = np.float32, np.float64
AGENTS = ("sacl", "cvpo", "ddpgl")
LOG_SIG_MIN, LOG_SIG_MAX = -20.0, 2.0


def head_mean(raw, max_action, mean_tanh, dtype):
    raw = np.asarray(raw, dtype)
    return (dtype(max_action) * np.tanh(raw).astype(dtype)).astype(dtype) if mean_tanh else raw


def head_sigma(raw_log_sigma, dtype):
    l = np.clip(np.asarray(raw_log_sigma, dtype), dtype(LOG_SIG_MIN), dtype(LOG_SIG_MAX))
    return np.exp(l).astype(dtype)


def action(agent, m, sigma, eps, deterministic, dtype):
    """the stored action of `agent` from the mean, the standard deviation and the N(0, 1) draw"""
    assert agent in AGENTS
    m = np.asarray(m, dtype)
    u = m if deterministic else (m + (np.asarray(sigma, dtype) * np.asarray(eps, dtype)).astype(dtype)).astype(dtype)
    return np.tanh(u).astype(dtype) if agent == "sacl" else u


def action_scale(m, sigma, eps, deterministic):
    """what the action's rounding errors scale with: the magnitudes of the terms of m + sigma eps, at least 1.  It bounds the squashed
    action's errors as well: tanh contracts, and its own rounding is relative to a value of at most 1."""
    m, se = np.abs(np.asarray(m, F64)), np.abs(np.asarray(sigma, F64) * np.asarray(eps, F64))
    return np.maximum(1.0, m if deterministic else m + se)


# ---------------------------------------------------------------------------------------------- what the GPU and the CPU tests share
PC = dict(radius=0.12, x_lim=0.3, dt=0.1)          # resets land in [-0.5, 0.5)^2: r > 0.48 and |x| > 0.3 both happen, neither always
SHAPES = {"pc": (6, 2), "lin8": (8, 2), "lin33": (33, 8), "lin20": (20, 16)}      # lin20: DDPG-Lag's widest head (16 columns)
# the edges of the collect's own staging loop (the sm.xT fill): Da = 1 (div_magic(1) == 0), obs 16 | 17 (the LDS-FMA | MFMA first
# layer), obs 64 (the linear env's widest state: one exact trip of the MFMA layer's k loop, 16 * Do == 1024 threads at 256 wide)
SHAPES.update(lin2=(2, 1), lin16=(16, 2), lin17=(17, 2), lin64=(64, 8), lin64w=(64, 16))
EXPLORATION_SIGMA = 0.1
ENV_SEED = 11
# (agent, env, env_num, n_episode) of the row-by-row test: SAC-Lag's full 16-column head row, two tiles with one row in the second,
# four full tiles, one env, the widest DDPG-Lag head
CASES = [("sacl", "lin33", 5, 12), ("sacl", "pc", 17, 25), ("cvpo", "lin8", 64, 70), ("cvpo", "lin8", 1, 3), ("ddpgl", "lin20", 5, 12)]


def actor_params(n):
    """the fixed random actor of the tests, in the API order of the oracles' specs"""
    return (0.15 * np.random.default_rng(7).standard_normal(n)).astype(F32)


def linear_host(kind, n):
    from fsrl_amd.env import SyntheticSafetyVectorEnv
    from fsrl_amd.env.synthetic import stable_coupling
    Do, Da = SHAPES[kind]
    return SyntheticSafetyVectorEnv(env_num=n, obs_dim=Do, act_dim=Da, episode_len=7, coupling=stable_coupling(Do), cost_threshold=0.7)


def cpu_actor(agent, kind, hidden=(64, 64), max_action=1.0, unbounded=None, exploration_sigma=EXPLORATION_SIGMA):
    """obs [k, Do] -> (m, sigma) in float32 from the oracles' actor networks over actor_params (oracle/sac_lag.py, cvpo.py,
    ddpg_lag.py): SAC-Lag's mean is the head, CVPO's and DDPG-Lag's max_action tanh(head).  unbounded: ActorProb's option for the
    two Gaussian agents -- True: the head, False: max_action tanh(head), None: the agent's default (SAC-Lag True, CVPO False)"""
    import torch
    from oracle import cvpo, ddpg_lag, sac_lag
    Do, Da = SHAPES[kind]
    spec = ddpg_lag.mlp_spec(Do, Da, hidden) if agent == "ddpgl" else sac_lag.actor_spec(Do, Da, hidden)
    n = sum(int(np.prod(s)) for s in spec.values())
    p, _ = sac_lag._leaves(torch.as_tensor(actor_params(n)), spec, 0)

    def forward(obs):
        x = torch.as_tensor(np.asarray(obs, F32))
        with torch.no_grad():
            if agent == "ddpgl":
                m = max_action * torch.tanh(ddpg_lag.mlp(p, x))
                return m.numpy(), np.full(m.shape, exploration_sigma, F32)
            m, sigma = cvpo.CVPOOracle(cvpo.CVPOConfig(Do, Da, hidden, max_action=max_action)).pi(p, x)
            if (agent == "sacl") if unbounded is None else unbounded:
                m = torch.nn.functional.linear(sac_lag._trunk(p, x, len(hidden)), p["Wmu"], p["bmu"])
            return m.numpy(), sigma.numpy()
    return forward, n


def onpolicy_params(n):
    """the fixed random parameters of the on-policy device-collect tests (tests/test_gpu_devcollect.py make), oracle layout"""
    return (0.3 * np.random.default_rng(7).standard_normal(n)).astype(F32)


def cpu_onpolicy_actor(kind, hidden=(64, 64), max_action=1.0, unbounded=False):
    """obs [k, Do] -> (mu, sigma) in float32 from oracle/ppo_lag.py's actor over onpolicy_params"""
    import torch
    from oracle.ppo_lag import PPOLagConfig, PPOLagOracle
    Do, Da = SHAPES[kind]
    o = PPOLagOracle(PPOLagConfig(obs_dim=Do, act_dim=Da, hidden=tuple(hidden), max_action=max_action, unbounded=unbounded))
    o.set_params(onpolicy_params(o.n_params))

    def forward(obs):
        with torch.no_grad():
            dist = o.actor_dist(torch.as_tensor(np.asarray(obs, F32)))
            return dist.mean.numpy(), dist.stddev.numpy()
    return forward, o.n_params


# ---------------------------------------------------------------------------------------------- the wider cases
# (agent or "onpolicy", env kind, env_num, n_episode, hidden, head options) of tests/test_gpu_devcollect_shapes.py, whose CPU
# preconditions tests/test_devcollect_shapes_model.py asserts.  Head options: max_action, unbounded (None: the agent's default),
# exploration_sigma (DDPG-Lag), hidden_sizes (two unrelated widths that the device pads to `hidden`).
SHAPE_CASES = [
    # on-policy: 128 and 256 wide, four full tiles of obs 64 at 256 wide, obs 16 | 17, Da = 1, a padded width, both mean modes
    ("onpolicy", "lin8", 17, 25, 128, {}), ("onpolicy", "lin8", 17, 25, 256, {}), ("onpolicy", "lin64", 64, 70, 256, {}),
    ("onpolicy", "lin16", 17, 25, 128, {}), ("onpolicy", "lin17", 17, 25, 128, {}), ("onpolicy", "lin2", 5, 12, 64, {}),
    ("onpolicy", "lin8", 17, 25, 128, {"hidden_sizes": (100, 72)}),
    ("onpolicy", "lin8", 17, 25, 64, {"max_action": 1.5}), ("onpolicy", "lin8", 17, 25, 64, {"max_action": 1.5, "unbounded": True}),
    # replay heads: every head at 128 and 256 wide, the 16-column DDPG-Lag and Gaussian rows at 256 wide, obs 16 | 17 | 64, Da = 1
    ("ddpgl", "lin64w", 64, 70, 256, {}), ("sacl", "lin64", 17, 25, 256, {}), ("cvpo", "lin16", 17, 25, 128, {}),
    ("sacl", "lin17", 20, 30, 128, {}), ("ddpgl", "lin2", 5, 12, 64, {}), ("cvpo", "lin33", 20, 30, 256, {}),
    ("sacl", "pc", 17, 25, 256, {}), ("cvpo", "pc", 20, 30, 128, {}),
    # head modes
    ("sacl", "lin8", 17, 25, 64, {"max_action": 1.5, "unbounded": False}), ("sacl", "lin8", 17, 25, 256, {"max_action": 1.5, "unbounded": False}),
    ("cvpo", "lin8", 17, 25, 64, {"unbounded": True}), ("cvpo", "lin8", 17, 25, 64, {"max_action": 1.5}),
    # DDPG-Lag with max_action 1.5 is GROUP_DIFF_CASES' ("ddpgl", "lin8", 17, 25, 64, max_action 1.5, exploration_sigma 0.3).  At
    # sigma 0.1 no training action of obs 8 / act 2 passes +-1; obs 20 / act 16 has them, but its deterministic means reach
    # |tanh(head)| >= 0.5, where two float32 evaluations of 1.5 tanh(head) -- the host's in (m, sigma), the device's in the collect --
    # sit up to 2 ulp of m apart while the rule's floor is one ulp at scale max(1, |m|): the float32 restatement of the mean itself
    # misses that floor (tests/test_devcollect_shapes_model.py shows it), so the case was moved
]
# members of one grouped launch that differ where the member table allows it; each is a solo case as well
GROUP_DIFF_CASES = {
    "onpolicy": [("onpolicy", "lin8", 5, 12, 128, {"max_action": 1.0}), ("onpolicy", "lin8", 17, 25, 128, {"max_action": 1.5}),
                 ("onpolicy", "lin8", 3, 8, 128, {"max_action": 0.5})],
    "ddpgl": [("ddpgl", "lin8", 5, 12, 64, {"max_action": 1.0, "exploration_sigma": 0.1}),
              ("ddpgl", "lin8", 17, 25, 64, {"max_action": 1.5, "exploration_sigma": 0.3}),
              ("ddpgl", "lin8", 3, 8, 64, {"max_action": 0.5, "exploration_sigma": 0.05})],
    "cvpo": [("cvpo", "lin8", 5, 12, 64, {"max_action": 1.0}), ("cvpo", "lin8", 17, 25, 64, {"max_action": 1.5}),
             ("cvpo", "lin8", 3, 8, 64, {"max_action": 0.5})],
}
ALL_CASES = SHAPE_CASES + [c for cs in GROUP_DIFF_CASES.values() for c in cs if c not in SHAPE_CASES]


def case_id(case):
    agent, kind, n, n_ep, H, opts = case
    return "-".join([agent, kind, f"n{n}", f"h{H}"] + [f"{k}={v}".replace(" ", "") for k, v in sorted(opts.items())])


def case_hidden(case):
    return tuple(case[5].get("hidden_sizes", (case[4], case[4])))


def case_actor(case, **override):
    """the CPU actor of `case`, with head options replaced by `override` (what a device that read the wrong value would compute)"""
    agent, kind, _, _, _, opts = case
    o = {k: v for k, v in opts.items() if k != "hidden_sizes"}
    o.update(override)
    if agent == "onpolicy":
        return cpu_onpolicy_actor(kind, case_hidden(case), o.get("max_action", 1.0), bool(o.get("unbounded", False)))[0]
    return cpu_actor(agent, kind, case_hidden(case), o.get("max_action", 1.0), o.get("unbounded"),
                     o.get("exploration_sigma", EXPLORATION_SIGMA))[0]


def formula(agent):
    """whose action formula: the on-policy head's is CVPO's, a = m + sigma eps unsquashed"""
    return "cvpo" if agent == "onpolicy" else agent
