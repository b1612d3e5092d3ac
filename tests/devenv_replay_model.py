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


def cpu_actor(agent, kind, hidden=(64, 64)):
    """obs [k, Do] -> (m, sigma) in float32 from the oracles' actor networks over actor_params (oracle/sac_lag.py, cvpo.py,
    ddpg_lag.py): SAC-Lag's mean is the head, CVPO's and DDPG-Lag's max_action tanh(head) with max_action 1"""
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
                m = torch.tanh(ddpg_lag.mlp(p, x))
                return m.numpy(), np.full(m.shape, EXPLORATION_SIGMA, F32)
            m, sigma = cvpo.CVPOOracle(cvpo.CVPOConfig(Do, Da, hidden)).pi(p, x)
            if agent == "sacl":
                m = torch.nn.functional.linear(sac_lag._trunk(p, x, len(hidden)), p["Wmu"], p["bmu"])
            return m.numpy(), sigma.numpy()
    return forward, n
