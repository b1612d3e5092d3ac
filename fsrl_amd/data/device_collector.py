"""FastCollector.collect(n_episode) for a `DeviceVectorEnv`, as a whole on the GPU (fsrl_collect_device): actor, action noise,
map_action, env step, store write and episode bookkeeping run in one workgroup that loops on the device; the host sees a handful of
launches and one small read-back per collect instead of one doorbell round trip per vector step.  Same result dict, same counters,
same store contents and episode-exact behaviour (surplus envs dropped, every env reset at the end of a collect) as `FastCollector`;
the action noise comes from the env's Philox stream, not from the library's xoshiro stream.  On-policy and replay
policies alike (SAC-Lag, DDPG-Lag, CVPO: the actor's head arithmetic runs on the device too; a prioritised buffer's leaves follow
the rows).  Layered engines (hidden_sizes of any depth and width) collect through the layered entry points of the library
(fsrl_collect_device_layered / fsrl_evaluate_device_layered: one kernel for every shape, the weights streamed from L2); the collectors
route on `_layered(engine)`.  A `DeviceCollector` of its own on a grouped fused engine is refused by the library, with the reason.

Grouped seeds (k seeds on one GPU, in an EngineGroup / EngineSacGroup / EngineCvpoGroup / EngineCollectGroup or in none) collect
through `GroupDeviceCollector(collectors)`: ONE launch per `max_steps_per_launch` vector steps carries every member's collect, a
workgroup per member (fsrl_collect_device_group), and each member's rows, env states, statistics and counters are what its own
`DeviceCollector.collect` would have produced, bit for bit.  `GroupCollector` over `DeviceCollector`s delegates to it.

Evaluation: `DeviceCollector(policy, test_envs)` with no buffer is the reference's `FastCollector(policy, test_envs)` (it makes a
`DeviceEvalCollector`, whose collect() is the other library call; a storing collector's collect() only ever sees training envs) -- the
same launches in their store-less form (fsrl_evaluate_device): the same statistics, and nothing of the engine's store, books, sampler or
random streams moves, so a run with test envs trains to the bits of the run without.  It also works where a storing collector is
refused: on a member of a group, with a trajectory archive attached, with more test envs than the store has sub-buffers.
`evaluation_collector(policy, test_envs)` is what the agents' `learn()` and `evaluate()` build; a `GroupDeviceCollector` of store-less
collectors evaluates every seed in one launch (fsrl_evaluate_device_group)."""
import time
from typing import Any, Dict, List, Sequence, Union

import numpy as np


def _collect_args(pol):
    """deterministic, bound method and bounds as FastCollector._collect_fused derives them"""
    det = bool(pol._deterministic_eval and not pol.training)
    space = pol.action_space
    bound = {"": 0, "clip": 1, "tanh": 2}[pol.action_bound_method] if space is not None else 0
    low = np.asarray(space.low, np.float32) if (space is not None and pol.action_scaling) else None
    high = np.asarray(space.high, np.float32) if low is not None else None
    return det, bound, low, high


def _collect_stats(r):
    n_ep = len(r["ep_rews"])
    done_count = r["terminated"] + r["truncated"]
    return {"n/ep": n_ep, "n/st": r["steps"], "rew": float(r["ep_rews"].mean()), "len": float(r["ep_lens"].mean()),
            "total_cost": r["total_cost"], "cost": r["total_cost"] / n_ep, "truncated": r["truncated"] / done_count,
            "terminated": r["terminated"] / done_count}


def _layered(eng) -> bool:
    """whether the engine's context is a layered one (include/fsrl_hip.h fsrl_config.n_hidden): its device collects and
    evaluations are the library's _layered calls"""
    hs = eng.cfg.hidden_sizes
    if hs is None:
        return False
    return not (len(hs) == 2 and max(hs) <= 256 and not eng.cfg.force_layered)


def evaluation_collector(policy, test_envs, render: bool = False):
    """The collector an agent evaluates with (None without test envs): the store-less DeviceCollector when the envs live on the
    GPU of this policy's engine -- a whole evaluation in a handful of launches -- and FastCollector(policy, test_envs), which steps
    any vector env (a device env too: layered engines, rendering), otherwise."""
    if test_envs is None:
        return None
    from fsrl_amd.env.device import DeviceVectorEnv
    eng = getattr(policy, "engine", None)
    if isinstance(test_envs, DeviceVectorEnv) and eng is not None and test_envs.engine is eng and not _layered(eng) and not render:
        return DeviceCollector(policy, test_envs)
    from fsrl_amd.data.fast_collector import FastCollector
    return FastCollector(policy, test_envs)


class DeviceCollector:
    def __new__(cls, policy=None, env=None, buffer=None, *args, **kwargs):
        # DeviceCollector(policy, env) with no buffer IS the store-less collector: its collect() is another library call
        return object.__new__(DeviceEvalCollector if (cls is DeviceCollector and buffer is None) else cls)

    def __init__(self, policy, env, buffer=None, max_steps_per_launch: int = 0, exploration_noise: bool = False):
        """exploration_noise is taken for call compatibility with FastCollector: the device draws the action as the policy's
        training-mode forward does (the replay agents' Gaussian / exploration noise included) unless the policy is in
        deterministic evaluation, whatever this argument says.
        buffer=None: the store-less collector (a DeviceEvalCollector): collect() runs fsrl_evaluate_device and no store is touched."""
        from fsrl_amd.env.device import DeviceVectorEnv
        if not isinstance(env, DeviceVectorEnv):
            raise TypeError("DeviceCollector collects from a DeviceVectorEnv")
        eng = getattr(policy, "engine", None)
        if eng is None or eng is not env.engine:
            raise ValueError("the device env was created on another engine than the policy's")
        assert buffer is None or buffer.buffer_num >= len(env)
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
        if self.buffer is not None:
            self.buffer.reset(keep_statistics=keep_statistics)

    def reset_env(self) -> None:
        self.env.reset()

    # ------------------------------------------------------------------ collect
    def collect(self, n_episode: int = 1, **_ignored) -> Dict[str, Any]:
        eng = self.policy.engine
        return self._collect(n_episode, eng.collect_device_layered if _layered(eng) else eng.collect_device)

    def _collect(self, n_episode, run) -> Dict[str, Any]:
        if n_episode is None:
            raise TypeError("Please specify n_episode in DeviceCollector.collect().")
        assert n_episode > 0
        pol, eng = self.policy, self.policy.engine
        t0 = time.time()
        if hasattr(pol, "_drain"):
            pol._drain()
        det, bound, low, high = _collect_args(pol)
        r = run(self.env._h, n_episode, det, bound, low, high, self.max_steps_per_launch)
        self.last_launches = r["launches"]
        if self.buffer is not None:
            self.buffer.sync_sizes()
        self.collect_step += r["steps"]
        self.collect_episode += len(r["ep_rews"])
        self.collect_time += max(time.time() - t0, 1e-9)
        return _collect_stats(r)


class DeviceEvalCollector(DeviceCollector):
    """The store-less collector, the reference's FastCollector(policy, test_envs): what `DeviceCollector(policy, env)` without a
    buffer makes.  The same resets, result dict and counters; collect() is fsrl_evaluate_device and reset_buffer() has nothing to do."""

    def __init__(self, policy, env, buffer=None, max_steps_per_launch: int = 0, exploration_noise: bool = False):
        assert buffer is None, "a DeviceEvalCollector stores nothing: DeviceCollector(policy, env, buffer) collects into a buffer"
        super().__init__(policy, env, None, max_steps_per_launch, exploration_noise)

    def collect(self, n_episode: int = 1, **_ignored) -> Dict[str, Any]:
        eng = self.policy.engine
        return self._collect(n_episode, eng.evaluate_device_layered if _layered(eng) else eng.evaluate_device)


class GroupDeviceCollector:
    """`DeviceCollector.collect` of every member in one looping launch (fsrl_collect_device_group).  collectors: one `DeviceCollector`
    per seed; the seeds' engines may be members of any kind of group, or of none.  The collectors all store (training) or are all
    store-less (evaluation, fsrl_evaluate_device_group)."""

    def __init__(self, collectors: Sequence[DeviceCollector], max_steps_per_launch: int = 0):
        self.collectors = list(collectors)
        assert self.collectors, "a group collector needs at least one collector"
        assert all(isinstance(c, DeviceCollector) for c in self.collectors), "GroupDeviceCollector: every collector is a DeviceCollector"
        n_eval = sum(c.buffer is None for c in self.collectors)
        assert n_eval in (0, len(self.collectors)), \
            "GroupDeviceCollector: a mix of store-less and storing collectors; a group evaluates or collects with every member"
        self.store = n_eval == 0
        # one launch, one kernel family: the members' engines are all layered or all fused
        self.layered = _layered(self.collectors[0].policy.engine)
        for i, c in enumerate(self.collectors):
            assert _layered(c.policy.engine) == self.layered, \
                f"GroupDeviceCollector: member {i} is a {'layered' if not self.layered else 'fused'} engine and member 0 a " \
                f"{'layered' if self.layered else 'fused'} one; a group is all layered or all fused"
        self.max_steps_per_launch = int(max_steps_per_launch)
        self.last_launches = 0

    def collect(self, n_episode: Union[int, Sequence[int]] = 1, **_ignored) -> List[Dict[str, Any]]:
        """n_episode: one count or one per member -> one stats dict per member, with the keys of DeviceCollector.collect"""
        from fsrl_amd.engine import collect_device_group, collect_device_layered, evaluate_device_group, evaluate_device_layered
        cols = self.collectors
        n = len(cols)
        ns = [int(n_episode)] * n if np.isscalar(n_episode) else [int(x) for x in n_episode]
        assert len(ns) == n and all(x > 0 for x in ns), "n_episode: a positive count, or one per member"
        t0 = time.time()
        args = []
        for col in cols:
            if hasattr(col.policy, "_drain"):
                col.policy._drain()
            args.append(_collect_args(col.policy))
        # one library call carries every member: they must agree on what the call takes once
        assert len({a[0] for a in args}) == 1 and len({a[1] for a in args}) == 1, "members must agree on deterministic / action_bound_method"
        assert len({a[2] is None for a in args}) == 1, "members must agree on action_scaling"
        det, bound = args[0][0], args[0][1]
        lows = None if args[0][2] is None else np.stack([a[2] for a in args])
        highs = None if args[0][2] is None else np.stack([a[3] for a in args])
        run = ((collect_device_layered if self.store else evaluate_device_layered) if self.layered
               else (collect_device_group if self.store else evaluate_device_group))
        res = run([col.policy.engine for col in cols], [col.env._h for col in cols], ns, det, bound, lows, highs, self.max_steps_per_launch)
        dt = max(time.time() - t0, 1e-9)
        stats = []
        for col, r in zip(cols, res):
            col.last_launches = self.last_launches = r["launches"]
            if col.buffer is not None:
                col.buffer.sync_sizes()
            col.collect_step += r["steps"]
            col.collect_episode += len(r["ep_rews"])
            col.collect_time += dt
            stats.append(_collect_stats(r))
        return stats
