"""FastCollector.collect(n_episode) for a `DeviceVectorEnv`, as a whole on the GPU (fsrl_collect_device): actor, action noise,
map_action, env step, store write and episode bookkeeping run in one workgroup that loops on the device; the host sees a handful of
launches and one small read-back per collect instead of one doorbell round trip per vector step.  Same result dict, same counters,
same store contents and episode-exact behaviour (surplus envs dropped, every env reset at the end of a collect) as `FastCollector`;
the action noise comes from the env's Philox stream, not from the library's xoshiro stream.  On-policy and replay
policies alike (SAC-Lag, DDPG-Lag, CVPO: the actor's head arithmetic runs on the device too; a prioritised buffer's leaves follow
the rows); layered and grouped engines are refused by the library, with the reason."""
import time
from typing import Any, Dict

import numpy as np


class DeviceCollector:
    def __init__(self, policy, env, buffer, max_steps_per_launch: int = 0, exploration_noise: bool = False):
        """exploration_noise is taken for call compatibility with FastCollector: the device draws the action as the policy's
        training-mode forward does (the replay agents' Gaussian / exploration noise included) unless the policy is in
        deterministic evaluation, whatever this argument says."""
        from fsrl_amd.env.device import DeviceVectorEnv
        if not isinstance(env, DeviceVectorEnv):
            raise TypeError("DeviceCollector collects from a DeviceVectorEnv")
        eng = getattr(policy, "engine", None)
        if eng is None or eng is not env.engine:
            raise ValueError("the device env was created on another engine than the policy's")
        if buffer is None:
            raise ValueError("DeviceCollector writes into the engine's store: pass its HipVectorReplayBuffer")
        assert buffer.buffer_num >= len(env)
        self.policy, self.env, self.buffer = policy, env, buffer
        self.env_num = len(env)
        self.max_steps_per_launch = int(max_steps_per_launch)
        self.device_actor = True
        self.last_launches = 0
        self.reset(False)

    # ------------------------------------------------------------------ resets (FastCollector's)
    def reset(self, reset_buffer: bool = True) -> None:
        self.reset_env()
        if reset_buffer:
            self.reset_buffer()
        self.reset_stat()

    def reset_stat(self) -> None:
        self.collect_step, self.collect_episode, self.collect_time = 0, 0, 0.0

    def reset_buffer(self, keep_statistics: bool = False) -> None:
        self.buffer.reset(keep_statistics=keep_statistics)

    def reset_env(self) -> None:
        self.env.reset()

    # ------------------------------------------------------------------ collect
    def collect(self, n_episode: int = 1, **_ignored) -> Dict[str, Any]:
        if n_episode is None:
            raise TypeError("Please specify n_episode in DeviceCollector.collect().")
        assert n_episode > 0
        pol, eng = self.policy, self.policy.engine
        t0 = time.time()
        if hasattr(pol, "_drain"):
            pol._drain()
        # deterministic, bound method and bounds as FastCollector._collect_fused derives them
        det = bool(pol._deterministic_eval and not pol.training)
        space = pol.action_space
        bound = {"": 0, "clip": 1, "tanh": 2}[pol.action_bound_method] if space is not None else 0
        low = np.asarray(space.low, np.float32) if (space is not None and pol.action_scaling) else None
        high = np.asarray(space.high, np.float32) if low is not None else None
        r = eng.collect_device(self.env._h, n_episode, det, bound, low, high, self.max_steps_per_launch)
        self.last_launches = r["launches"]
        self.buffer.sync_sizes()
        n_ep = len(r["ep_rews"])
        self.collect_step += r["steps"]
        self.collect_episode += n_ep
        self.collect_time += max(time.time() - t0, 1e-9)
        done_count = r["terminated"] + r["truncated"]
        return {"n/ep": n_ep, "n/st": r["steps"], "rew": float(r["ep_rews"].mean()), "len": float(r["ep_lens"].mean()),
                "total_cost": r["total_cost"], "cost": r["total_cost"] / n_ep, "truncated": r["truncated"] / done_count,
                "terminated": r["terminated"] / done_count}
