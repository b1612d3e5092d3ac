"""Host model of the device environments (fsrl_amd/csrc/device_env.hpp) and of the device collect loop.  TEST INFRASTRUCTURE ONLY.
numpy + oracle.sampler's Philox; written from the definitions in DESIGN.md 3.4.1 and include/fsrl_hip.h, not from the kernels.

Random numbers.  One Philox4x32-10 block per
    counter = (env id, reset ordinal, step in the episode, stream << 28 | dim // 4),   key = seed * KEY_MUL + DEFAULT_KEY
streams: 0 reset draws, 1 action noise, 2 env step noise.  Dimension d of a stream is element d & 3 of block d >> 2: a uniform is
(word >> 8) / 2^24, a normal comes from Box-Muller over words (0, 1) (elements 0, 1) or (2, 3) (elements 2, 3).  The reset that
starts an episode has ordinal `ord` = the number of resets of that env before it; the episode's action and step draws use the same
ordinal with t = 0, 1, ...; the reset's own draws use t = 0 on stream 0.

Every env exists twice: `dtype=np.float64` is the reference the GPU tests measure distances to, `dtype=np.float32` restates the
device's arithmetic -- every *, +, -, / and sqrt rounded on its own, sums in ascending index -- and so equals the device bit for bit
wherever no transcendental is involved."""
import numpy as np

from oracle import sampler

F32, F64 = np.float32, np.float64
STREAM_RESET, STREAM_ACT, STREAM_STEP = 0, 1, 2
POINT_CIRCLE, LINEAR = 0, 1
BAND = 1e-5            # a discontinuous output may differ where its decision variable is within BAND * scale of the threshold
BAND_CAP = 0.02        # ... on at most this share of the rows


def key_of(seed):
    return (int(seed) * sampler.KEY_MUL + sampler.DEFAULT_KEY) & sampler.MASK64


def blocks(key, env, ordinal, t, stream, blk):
    """Philox blocks of the broadcast (env, ordinal, t, blk) -> [..., 4] uint64 holding 32-bit words"""
    env, ordinal, t, blk = np.broadcast_arrays(np.asarray(env, np.uint64), np.asarray(ordinal, np.int64).astype(np.uint64),
                                               np.asarray(t, np.uint64), np.asarray(blk, np.uint64))
    ctr = np.stack([env, ordinal & sampler.M32, t, (np.uint64(stream) << np.uint64(28)) | blk], -1)
    return sampler.philox4x32_10(ctr, (key & 0xFFFFFFFF, key >> 32))


def _word_pair(key, env, ordinal, t, stream, d):
    d = np.asarray(d, np.int64)
    r = blocks(key, env, ordinal, t, stream, d >> 2)
    hi = (d & 2) != 0
    return np.where(hi, r[..., 2], r[..., 0]), np.where(hi, r[..., 3], r[..., 1])


def uniform(key, env, ordinal, t, stream, d):
    """U[0, 1) on the 2^-24 grid: exact in float32 and float64 alike"""
    a, b = _word_pair(key, env, ordinal, t, stream, d)
    w = np.where((np.asarray(d) & 1) != 0, b, a)
    return (w >> np.uint64(8)).astype(F64) / 16777216.0


def normal(key, env, ordinal, t, stream, d, dtype=F64):
    """N(0, 1).  float64: oracle.sampler.box_muller.  float32: the same formula with every operation in float32."""
    a, b = _word_pair(key, env, ordinal, t, stream, d)
    odd = (np.asarray(d) & 1) != 0
    if dtype is F64:
        n0, n1, _ = sampler.box_muller(a, b)
        return np.where(odd, n1, n0)
    u1 = ((a >> np.uint64(8)).astype(F32) + F32(1.0)) * F32(1.0 / 16777216.0)
    u2 = (b >> np.uint64(8)).astype(F32) * F32(1.0 / 16777216.0)
    rad = np.sqrt(F32(-2.0) * np.log(u1))
    ang = F32(np.pi) * (F32(2.0) * u2)
    return np.where(odd, rad * np.sin(ang), rad * np.cos(ang)).astype(F32)


def normal_scale(key, env, ordinal, t, stream, d):
    """the magnitude a normal's rounding errors scale with: its radius sqrt(-2 ln u1), at least 1"""
    a, b = _word_pair(key, env, ordinal, t, stream, d)
    return np.maximum(sampler.box_muller(a, b)[2], 1.0)


# ---------------------------------------------------------------------------------------------- map_action
def map_action(act, bound_method, low=None, high=None, dtype=F32):
    a = np.asarray(act, dtype)
    if bound_method == 1:
        a = np.clip(a, dtype(-1.0), dtype(1.0))
    elif bound_method == 2:
        a = np.tanh(a).astype(dtype)
    if low is not None:
        low, high = np.asarray(low, dtype), np.asarray(high, dtype)
        a = low + (high - low) * (a + dtype(1.0)) / dtype(2.0)
    return a.astype(dtype)


# ---------------------------------------------------------------------------------------------- point circle (fsrl_amd/env/toy.py)
def point_obs(state, radius, x_lim, dtype):
    s = np.asarray(state, dtype)
    px, py = s[:, 0], s[:, 1]
    rn = np.sqrt(px * px + py * py)
    return np.stack([px, py, s[:, 2], s[:, 3], rn - dtype(radius), dtype(x_lim) - np.abs(px)], 1).astype(dtype)


def point_reset(key, env, ordinal, radius, x_lim, dtype=F64):
    env = np.asarray(env)
    u = np.stack([uniform(key, env, ordinal, 0, STREAM_RESET, 0), uniform(key, env, ordinal, 0, STREAM_RESET, 1)], 1).astype(dtype)
    state = np.concatenate([u - dtype(0.5), np.zeros((len(env), 2), dtype)], 1)
    return state, point_obs(state, radius, x_lim, dtype)


def point_step(state, act, radius, x_lim, dt, dtype=F64):
    """-> dict(state, obs_next, rew, cost, terminated, margins): margins[name] = (decision variable, threshold, scale)"""
    s = np.asarray(state, dtype)
    a = np.clip(np.asarray(act, dtype), dtype(-1.0), dtype(1.0))
    radius, x_lim, dt = dtype(radius), dtype(x_lim), dtype(dt)
    vx, vy = dtype(0.9) * s[:, 2] + dt * a[:, 0], dtype(0.9) * s[:, 3] + dt * a[:, 1]
    px, py = s[:, 0] + dt * vx, s[:, 1] + dt * vy
    r = np.sqrt(px * px + py * py) + dtype(1e-8)
    rew = ((-py * vx + px * vy) / r / (dtype(1.0) + np.abs(r - radius))).astype(F64)
    ns = np.stack([px, py, vx, vy], 1).astype(dtype)
    four_r = dtype(4.0) * radius
    ob = point_obs(ns, radius, x_lim, dtype)
    return dict(state=ns, obs_next=ob, rew=rew, cost=(np.abs(px) > x_lim).astype(F64),
                terminated=r > four_r, rew_scale=np.ones(len(s)), obs_scale=np.maximum(np.abs(ob.astype(F64)), 1.0),
                margins=dict(cost=(np.abs(px).astype(F64), float(x_lim), np.maximum(float(x_lim), 1.0)),
                             terminated=(r.astype(F64), float(four_r), np.maximum(float(four_r), 1.0))))


# ---------------------------------------------------------------------------------------------- linear (SyntheticSafetyVectorEnv)
def linear_reset(key, env, ordinal, obs_dim, dtype=F64):
    env = np.asarray(env)
    d = np.arange(obs_dim)
    s = normal(key, env[:, None], np.asarray(ordinal)[:, None] if np.ndim(ordinal) else ordinal, 0, STREAM_RESET, d[None, :], dtype)
    return s.astype(dtype), s.astype(dtype)


def linear_step(state, act, A, B, noise, cost_threshold, dtype=F64):
    """s' = s @ A + act @ B + 0.05 noise with both sums in ascending index; rew / cost as SyntheticSafetyVectorEnv.step"""
    s, a = np.asarray(state, dtype), np.asarray(act, dtype)
    A, B, noise = np.asarray(A, dtype), np.asarray(B, dtype), np.asarray(noise, dtype)
    sa, sb = np.zeros_like(s), np.zeros_like(s)
    for i in range(s.shape[1]):
        sa = sa + s[:, i:i + 1] * A[i][None, :]
    for k in range(a.shape[1]):
        sb = sb + a[:, k:k + 1] * B[k][None, :]
    ns = ((sa + sb) + dtype(0.05) * noise).astype(dtype)
    a2 = np.zeros(len(s), dtype)
    for k in range(a.shape[1]):
        a2 = a2 + a[:, k] * a[:, k]
    rew = (ns[:, 0] * a[:, 0] - dtype(0.1) * a2).astype(F64) + 0.5
    obs_scale = np.abs(s).astype(F64) @ np.abs(A).astype(F64) + np.abs(a).astype(F64) @ np.abs(B).astype(F64) + 0.05 * np.abs(noise)
    rew_scale = np.abs(ns[:, 0] * a[:, 0]).astype(F64) + 0.1 * a2.astype(F64) + 0.5
    thr = float(dtype(cost_threshold))
    return dict(state=ns, obs_next=ns, rew=rew, cost=(np.abs(ns[:, 1]) > dtype(cost_threshold)).astype(F64),
                terminated=np.zeros(len(s), bool), obs_scale=np.maximum(obs_scale, 1.0), rew_scale=np.maximum(rew_scale, 1.0),
                margins=dict(cost=(np.abs(ns[:, 1]).astype(F64), thr, np.maximum(obs_scale[:, 1], 1.0))))


def band_share(step32):
    """share of rows whose cost / terminated decision lies within BAND * scale of its threshold, from the float32 restatement alone"""
    near = np.zeros(len(step32["rew"]), bool)
    for var, thr, scale in step32["margins"].values():
        near |= np.abs(var - thr) <= BAND * scale
    return near.mean(), near


# ---------------------------------------------------------------------------------------------- an env with its counters
class ModelEnv:
    """env_num envs of one kind with the device env's bookkeeping: state, steps of the running episode, reset ordinals"""

    def __init__(self, kind, env_num, max_episode_steps, seed, params, obs_dim, act_dim, A=None, B=None, dtype=F64):
        self.kind, self.env_num, self.max_steps, self.key = kind, env_num, max_episode_steps, key_of(seed)
        self.params, self.Do, self.Da, self.A, self.B, self.dtype = params, obs_dim, act_dim, A, B, dtype
        sd = 4 if kind == POINT_CIRCLE else obs_dim
        self.state = np.zeros((env_num, sd), dtype)
        self.obs = np.zeros((env_num, obs_dim), dtype)
        self.t = np.zeros(env_num, np.int64)
        self.ordinal = np.zeros(env_num, np.int64)

    def reset(self, ids=None):
        ids = np.arange(self.env_num) if ids is None else np.asarray(ids)
        if self.kind == POINT_CIRCLE:
            st, ob = point_reset(self.key, ids, self.ordinal[ids], self.params[0], self.params[1], self.dtype)
        else:
            st, ob = linear_reset(self.key, ids, self.ordinal[ids], self.Do, self.dtype)
        self.state[ids], self.obs[ids] = st, ob
        self.t[ids] = 0
        self.ordinal[ids] += 1
        return self.obs[ids].copy()

    def step_noise(self, ids, dtype=None):
        ids = np.asarray(ids)
        return normal(self.key, ids[:, None], (self.ordinal[ids] - 1)[:, None], self.t[ids][:, None], STREAM_STEP,
                      np.arange(self.Do)[None, :], dtype or self.dtype)

    def action_noise(self, ids, dtype=None):
        ids = np.asarray(ids)
        return normal(self.key, ids[:, None], (self.ordinal[ids] - 1)[:, None], self.t[ids][:, None], STREAM_ACT,
                      np.arange(self.Da)[None, :], dtype or self.dtype)

    def step(self, act, ids=None):
        ids = np.arange(self.env_num) if ids is None else np.asarray(ids)
        if self.kind == POINT_CIRCLE:
            r = point_step(self.state[ids], act, *self.params[:3], dtype=self.dtype)
        else:
            r = linear_step(self.state[ids], act, self.A, self.B, self.step_noise(ids), self.params[0], self.dtype)
        self.state[ids], self.obs[ids] = r["state"], r["obs_next"]
        self.t[ids] += 1
        r["truncated"] = self.t[ids] >= self.max_steps
        return r


def collect(env, n_episode, policy):
    """FastCollector.collect(n_episode) (fsrl/data/fast_collector.py:283-368) over a ModelEnv: every finished env is reset at once, then
    surplus = live - (n_episode - episodes) drops the first `surplus` finished envs in position order; all envs are reset at the end.
    policy(obs, ids) -> env actions.  -> (rows [(env, ordinal, t, done)], episodes, vector steps)"""
    ready = np.arange(min(env.env_num, n_episode))
    rows, episodes, steps = [], 0, 0
    while True:
        act = policy(env.obs[ready], ready)
        before = [(int(e), int(env.ordinal[e] - 1), int(env.t[e])) for e in ready]
        r = env.step(act, ready)
        done = r["terminated"] | r["truncated"]
        rows += [b + (bool(d), ) for b, d in zip(before, done)]
        steps += 1
        if done.any():
            local = np.where(done)[0]
            episodes += len(local)
            env.reset(ready[local])
            surplus = len(ready) - (n_episode - episodes)
            if surplus > 0:
                mask = np.ones(len(ready), bool)
                mask[local[:surplus]] = False
                ready = ready[mask]
        if episodes >= n_episode:
            break
    env.reset()
    return rows, episodes, steps


# ---------------------------------------------------------------------------------------------- the inputs of the GPU tests' env-alone cases
def env_alone_cases():
    """name -> dict(kind, obs_dim, act_dim, env_num, params, A, B, state, act, t, ordinal): what tests/test_gpu_devcollect.py injects
    with fsrl_devenv_set_state before ONE fsrl_devenv_step.  States sit at random places AND just inside / outside every threshold
    (|pos x| vs x_lim, r vs 4 radius, |s'[1]| vs cost_threshold: the latter by steering s through a solve of the noiseless step)."""
    from fsrl_amd.env.synthetic import SyntheticSafetyVectorEnv, stable_coupling
    cases = {}
    rng = np.random.default_rng(20261020)
    n, radius, x_lim, dt = 64, 0.25, 0.3, 0.1
    state = np.concatenate([rng.uniform(-1.2, 1.2, (n, 2)), rng.uniform(-0.5, 0.5, (n, 2))], 1).astype(F32)
    act = rng.uniform(-1.5, 1.5, (n, 2)).astype(F32)
    for j, rel in enumerate([1e-3, -1e-3, 1e-2, -1e-2]):                  # |x'| just outside / inside x_lim; r' around 4 radius
        state[j, 2:] = 0.0; act[j] = 0.0
        state[j, 0], state[j, 1] = x_lim * (1 + rel), 0.1
        state[8 + j, 2:] = 0.0; act[8 + j] = 0.0
        state[8 + j, 0], state[8 + j, 1] = 0.6 * 4 * radius * (1 + rel), 0.8 * 4 * radius * (1 + rel)
    cases["point_circle"] = dict(kind=POINT_CIRCLE, obs_dim=6, act_dim=2, env_num=n, params=(radius, x_lim, dt), A=None, B=None,
                                 state=state, act=act, t=rng.integers(0, 7, n).astype(np.int32), ordinal=rng.integers(1, 50, n))
    for Do, Da in ((8, 2), (33, 8)):
        host = SyntheticSafetyVectorEnv(env_num=n, obs_dim=Do, act_dim=Da, episode_len=7, coupling=stable_coupling(Do), cost_threshold=0.7)
        state = rng.standard_normal((n, Do)).astype(F32)
        act = rng.uniform(-1, 1, (n, Da)).astype(F32)
        t, ordinal = rng.integers(0, 7, n).astype(np.int32), rng.integers(1, 50, n)
        for j, rel in enumerate([1e-3, -1e-3, 1e-2, -1e-2]):
            # move s[1] so that s'[1] lands at cost_threshold * (1 + rel), noise included (float64 solve, then rounded to float32)
            key = key_of(5)
            noise = normal(key, np.full((1, 1), j), np.full((1, 1), ordinal[j] - 1), np.full((1, 1), t[j]), STREAM_STEP, np.arange(Do)[None, :])
            cur = linear_step(state[j:j + 1], act[j:j + 1], host.A, host.B, noise, 0.7, F64)["state"][0, 1]
            state[j, 1] += F32((0.7 * (1 + rel) - cur) / float(host.A[1, 1]))
        cases[f"linear_{Do}_{Da}"] = dict(kind=LINEAR, obs_dim=Do, act_dim=Da, env_num=n, params=(0.7, ), A=host.A, B=host.B, state=state,
                                          act=act, t=t, ordinal=ordinal)
    for c in cases.values():
        c["seed"], c["max_episode_steps"] = 5, 7
    return cases


def env_alone_expected(case, dtype):
    """the step of `case` in `dtype` -> the dict of point_step / linear_step, `truncated` added"""
    ids = np.arange(case["env_num"])
    if case["kind"] == POINT_CIRCLE:
        r = point_step(case["state"], case["act"], *case["params"], dtype=dtype)
    else:
        noise = normal(key_of(case["seed"]), ids[:, None], (case["ordinal"] - 1)[:, None], case["t"][:, None], STREAM_STEP,
                       np.arange(case["obs_dim"])[None, :], dtype)
        r = linear_step(case["state"], case["act"], case["A"], case["B"], noise, case["params"][0], dtype)
    r["truncated"] = case["t"] + 1 >= case["max_episode_steps"]
    return r


def yardstick(dev, f64, r32, scale):
    """(device's distance, restatement's distance, bound): max over elements of |x - float64| / scale; the device may sit 3 x as far
    from float64 as the float32 restatement does, and is never held tighter than one float32 ulp at the value's scale"""
    scale = np.broadcast_to(np.asarray(scale, F64), np.shape(f64))
    d_dev = float(np.max(np.abs(np.asarray(dev, F64) - f64) / scale))
    d_r32 = float(np.max(np.abs(np.asarray(r32, F64) - f64) / scale))
    return d_dev, d_r32, max(3.0 * d_r32, float(np.finfo(F32).eps))
