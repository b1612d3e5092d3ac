"""Environments that live on the GPU (include/fsrl_hip.h "Device environments"): the env's dynamics are device functions, its state
never leaves HBM.  `DeviceVectorEnv` gives such an env the calling convention of `SyntheticSafetyVectorEnv` -- `len(env)`,
`reset(ids=None) -> (obs, info)`, `step(act, ids) -> (obs, rew, terminated, truncated, {"cost": cost})` -- one small launch per call
(`fsrl_devenv_reset` / `fsrl_devenv_step`), so every collector of this package works over it unchanged.  What it is for is
`DeviceCollector` (fsrl_amd/data/device_collector.py): a whole `collect(n_episode)` in a handful of launches -- with a buffer the
training collect (fsrl_collect_device), without one the evaluation that stores nothing (fsrl_evaluate_device), which is what the
agents' `learn(train_envs, test_envs)` and `evaluate(test_envs)` run over device test envs of their own engine.  Layered engines
and `render=True` evaluate through `FastCollector` over `step`, call by call."""
from types import SimpleNamespace

import numpy as np

from fsrl_amd import _lib
from fsrl_amd.env.synthetic import Box

KINDS = {"point-circle": _lib.DEVENV_POINT_CIRCLE, "linear": _lib.DEVENV_LINEAR}


def _engine_of(engine_or_policy):
    eng = getattr(engine_or_policy, "engine", engine_or_policy)
    if eng is None or not hasattr(eng, "devenv_create"):
        raise TypeError("DeviceVectorEnv needs an Engine or a policy that has one")
    return eng


class DeviceVectorEnv:
    """`kind`: "point-circle" (params radius, x_lim, dt) or "linear" (params cost_threshold; A [obs, obs], B [act, obs]).  The env is
    bound to the engine it was created on: its shapes are the engine's, and only that engine's DeviceCollector can drive it."""

    def __init__(self, engine_or_policy, kind, env_num, max_episode_steps, seed=0, params=(), A=None, B=None, spec_id="DeviceEnv-v0"):
        self.engine = _engine_of(engine_or_policy)
        self.kind = KINDS[kind] if isinstance(kind, str) else int(kind)
        self.env_num = int(env_num)
        self.obs_dim, self.act_dim = self.engine.cfg.obs_dim, self.engine.cfg.act_dim
        self.state_dim = 4 if self.kind == _lib.DEVENV_POINT_CIRCLE else self.obs_dim
        self.observation_space = Box(-np.inf, np.inf, (self.obs_dim, ))
        self.action_space = Box(-1.0, 1.0, (self.act_dim, ))
        self.spec = SimpleNamespace(id=spec_id, max_episode_steps=int(max_episode_steps))
        self._h = self.engine.devenv_create(self.kind, self.env_num, max_episode_steps, seed, params, A, B)

    def __len__(self):
        return self.env_num

    def seed(self, seed):
        """a new random stream: the reset ordinals start again at zero, the envs stay where they are"""
        self.engine.devenv_seed(self._h, seed)

    def reset(self, ids=None, **kwargs):
        return self.engine.devenv_reset(self._h, self.env_num, ids), {}

    def step(self, act, ids=None):
        obs, rew, cost, term, trunc = self.engine.devenv_step(self._h, self.env_num, act, ids)
        return obs, rew, term, trunc, {"cost": cost}

    def get_state(self):
        """-> (state [env_num, state_dim], steps of the running episodes, reset ordinals)"""
        return self.engine.devenv_get_state(self._h, self.env_num, self.state_dim)

    def set_state(self, state=None, t=None, ordinal=None):
        self.engine.devenv_set_state(self._h, state, t, ordinal)

    def close(self):
        if getattr(self, "_h", None):
            self.engine.devenv_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DevicePointCircle(DeviceVectorEnv):
    """`PointCircleEnv` (fsrl_amd/env/toy.py) in float32 on the device: obs 6, act 2"""

    def __init__(self, engine_or_policy, env_num, max_episode_steps=100, radius=1.5, x_lim=1.0, dt=0.1, seed=0):
        super().__init__(engine_or_policy, "point-circle", env_num, max_episode_steps, seed, (radius, x_lim, dt), spec_id="DevicePointCircle-v0")
        self.radius, self.x_lim, self.dt = float(radius), float(x_lim), float(dt)


class DeviceLinear(DeviceVectorEnv):
    """`SyntheticSafetyVectorEnv`'s dynamics on the device.  `like`: a host env to take A, B, the episode length and the cost
    threshold from (its env_num too, unless one is given)."""

    def __init__(self, engine_or_policy, env_num=None, episode_len=300, cost_threshold=1.0, A=None, B=None, seed=0, like=None):
        if like is not None:
            A, B = like.A, like.B
            episode_len, cost_threshold = like.episode_len, like.cost_threshold
            env_num = like.env_num if env_num is None else env_num
        if A is None or B is None:
            raise ValueError("DeviceLinear needs A and B, or like=SyntheticSafetyVectorEnv(...)")
        self.A, self.B = np.asarray(A, np.float32), np.asarray(B, np.float32)
        self.cost_threshold = float(cost_threshold)
        super().__init__(engine_or_policy, "linear", env_num, episode_len, seed, (cost_threshold, ), self.A, self.B, spec_id="DeviceLinear-v0")
