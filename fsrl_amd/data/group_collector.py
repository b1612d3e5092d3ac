"""Lock-step collection for the members of a grouped run (multi-seed on one GPU): PPO-Lagrangian or FOCOPS seeds through their
PolicyGroup / EngineGroup, SAC-Lag, DDPG-Lag or CVPO seeds through an EngineCollectGroup (fsrl_collect_group_step: the replay
agents' collect group, independent of their update groups).

`GroupCollector(policy_group, collectors).collect(n_episode)` is `collector.collect(n_episode)` of every member, with the members'
vector envs stepped in lock step and ONE library call per vector step for all of them (`EngineGroup.collect_step` ->
fsrl_group_collect_step: one actor request, served by one resident kernel for the whole group -- or, for a group of layered
PPO-Lagrangian seeds, by one sequence of L + 2 launches carrying every member's rows).  Per member the bookkeeping is
FastCollector._collect_fused's interpreted loop -- episode counts, resets of finished envs, surplus envs dropped, fill levels, the
collector's counters, `reset_env` at the end -- and the library calls a member sees are the ones its own collect would make, so the
stored rows, the actions and the member's noise stream are the same bit for bit.  A member that has its episodes stops contributing
rows while the others go on.

When every member's env is a worker-process env (`native_desc`: ShmemVectorEnv) the whole collect is ONE library call
(`collect_episodes` -> fsrl_group_collect_episodes / fsrl_collect_episodes_group): the same loop in C, with the step and reset
commands of all members posted to their workers before the first is waited for -- the interpreted loop below steps member 0's env,
waits, steps member 1's ... and so pays k env-step times per vector step.  `native_loop=False` keeps the interpreted loop."""
import time
from typing import Any, Dict, List, Sequence, Union

import numpy as np


class GroupCollector:
    def __init__(self, policy_group, collectors: Sequence, native_loop: bool = True):
        # policy_group: a PolicyGroup (its EngineGroup is used), an EngineCollectGroup (replay agents) or anything with
        # EngineGroup's collect_step / actor_release
        self.group = getattr(policy_group, "group", policy_group)
        self.collectors = list(collectors)
        self.native_loop = bool(native_loop)
        engines = getattr(self.group, "engines", None)
        assert self.collectors, "a group collector needs at least one collector"
        # device envs: every member's whole collect in one looping launch (GroupDeviceCollector), no lock step on the host
        from fsrl_amd.data.device_collector import DeviceCollector, GroupDeviceCollector
        n_dev = sum(isinstance(col, DeviceCollector) for col in self.collectors)
        assert n_dev in (0, len(self.collectors)), \
            "GroupCollector: a mix of DeviceCollectors and other collectors; a group collects on the device with every member or with none"
        self.device = GroupDeviceCollector(self.collectors, max(c.max_steps_per_launch for c in self.collectors)) if n_dev else None
        for i, col in enumerate(self.collectors):
            assert col.device_actor, "GroupCollector: collectors with device_actor=True"
            assert col.buffer is not None, "GroupCollector: every collector has its member's buffer"
            eng = col.policy.engine
            assert getattr(col.buffer, "engine", None) is eng, "collector i's buffer must be its policy's HipVectorReplayBuffer"
            if engines is not None:
                assert engines[i] is eng, "collector i must belong to member i of the group"

    def collect(self, n_episode: Union[int, Sequence[int]] = 1) -> List[Dict[str, Any]]:
        """FastCollector.collect(n_episode) of every member (n_episode: one count or one per member) -> one stats dict per member.
        The group's resident actor kernel lives for the length of this call."""
        if self.device is not None:
            return self.device.collect(n_episode)
        try:
            stats = self._collect(n_episode)
            for buf in {id(b): b for b in (c._traj_buffer() for c in self.collectors) if b is not None}.values():
                buf.sync()          # TrajectoryBuffer.attach(collector): its keep / filter decisions, once per collect
            return stats
        finally:
            self.group.actor_release()

    def _collect(self, n_episode):
        cols = self.collectors
        n = len(cols)
        ns = [int(n_episode)] * n if np.isscalar(n_episode) else [int(x) for x in n_episode]
        assert len(ns) == n and all(x > 0 for x in ns), "n_episode: a positive count, or one per member"
        t0 = time.time()
        mem, dets, bounds, lows, highs = [], [], [], [], []
        for col, ne in zip(cols, ns):
            pol = col.policy
            if hasattr(pol, "_drain"):
                pol._drain()
            space = pol.action_space
            dets.append(bool(pol._deterministic_eval and not pol.training))
            bounds.append({"": 0, "clip": 1, "tanh": 2}[pol.action_bound_method] if space is not None else 0)
            low = np.asarray(space.low, np.float32) if (space is not None and pol.action_scaling) else None
            lows.append(low)
            highs.append(np.asarray(space.high, np.float32) if low is not None else None)
            ready = np.arange(min(col.env_num, ne))
            mem.append(dict(col=col, n_episode=ne, ready=ready, obs=np.asarray(col._obs[:len(ready)], np.float32), act=None,
                            env_act=None, steps=0, cost=0.0, episodes=0, term=0, trunc=0, ep_rews=[], ep_lens=[], live=True,
                            pending=None, nxt=None, nready=None))
        # one library call carries every member: they must agree on what the call takes once
        assert len(set(dets)) == 1 and len(set(bounds)) == 1, "members must agree on deterministic / action_bound_method"
        assert len({lo is None for lo in lows}) == 1, "members must agree on action_scaling"
        det, bound = dets[0], bounds[0]
        low = None if lows[0] is None else np.stack(lows)
        high = None if lows[0] is None else np.stack(highs)
        if self.native_loop and hasattr(self.group, "collect_episodes") and all(hasattr(c.env, "native_desc") for c in cols):
            return self._collect_native(mem, ns, t0, det, bound, low, high)
        out = self.group.collect_step([None] * n, [m["obs"] for m in mem], det, bound, low, high)
        for m, o in zip(mem, out):
            m["act"], m["env_act"] = o[0], o[1]
        while any(m["live"] for m in mem):
            prevs, obs_acts = [None] * n, [None] * n
            for i, m in enumerate(mem):
                if not m["live"]:
                    continue
                col, ready = m["col"], m["ready"]
                obs_next, rew, terminated, truncated, info = col.env.step(m["env_act"], ready)
                terminated, truncated = np.asarray(terminated, bool), np.asarray(truncated, bool)
                done = terminated | truncated
                cost = np.asarray(info.get("cost", np.zeros(len(ready))), np.float64) if isinstance(info, dict) \
                    else np.array([x.get("cost", 0.0) for x in info], np.float64)
                m["cost"] += float(cost.sum())
                m["steps"] += len(ready)
                prevs[i] = (ready, m["obs"], m["act"], rew, cost, terminated, truncated, obs_next)
                nxt, nready = obs_next, ready
                m["pending"] = None
                if done.any():
                    local = np.where(done)[0]
                    n_done = len(local)
                    m["term"] += int(terminated.sum()); m["trunc"] += int(truncated.sum())
                    nxt = np.array(obs_next, np.float32)
                    obs_reset, _ = col.env.reset(ready[local])
                    nxt[local] = obs_reset
                    surplus = len(ready) - (m["n_episode"] - m["episodes"] - n_done)
                    if surplus > 0:      # drop finished envs that are no longer needed (unbiased tail)
                        mask = np.ones(len(ready), bool)
                        mask[local[:surplus]] = False
                        nready, nxt = ready[mask], nxt[mask]
                    last = m["episodes"] + n_done >= m["n_episode"]
                    m["pending"] = (local, n_done, last)
                    obs_acts[i] = None if last else nxt
                else:
                    obs_acts[i] = nxt
                m["nxt"], m["nready"] = nxt, nready
            out = self.group.collect_step(prevs, obs_acts, det, bound, low, high)
            for m, o in zip(mem, out):
                if not m["live"]:
                    continue
                m["act"], m["env_act"], ep_rew, ep_len = o
                if m["pending"] is not None:
                    local, n_done, last = m["pending"]
                    m["episodes"] += n_done
                    m["ep_lens"].append(ep_len[local].copy()); m["ep_rews"].append(ep_rew[local].copy())
                    if last:
                        m["live"] = False
                        continue
                m["obs"], m["ready"] = np.asarray(m["nxt"], np.float32), m["nready"]
        dt = max(time.time() - t0, 1e-9)
        stats = []
        for m in mem:
            col = m["col"]
            col.buffer.sync_sizes()
            col.collect_step += m["steps"]
            col.collect_episode += m["episodes"]
            col.collect_time += dt
            col.reset_env()
            rews, lens = np.concatenate(m["ep_rews"]), np.concatenate(m["ep_lens"])
            done_count = m["term"] + m["trunc"]
            stats.append({"n/ep": m["episodes"], "n/st": m["steps"], "rew": float(rews.mean()), "len": float(lens.mean()),
                          "total_cost": m["cost"], "cost": m["cost"] / m["episodes"], "truncated": m["trunc"] / done_count,
                          "terminated": m["term"] / done_count})
        return stats

    def _collect_native(self, mem, ns, t0, det, bound, low, high):
        """worker-process envs: the whole collect of every member in one library call; afterwards, per member, what
        FastCollector._collect_native does.  A failed call may have left a command half-handled on the failing member's env only
        (the library waits for the others'): that env refuses every later command, the others stay usable."""
        cols = self.collectors
        descs = [col.env.native_desc() for col in cols]
        try:
            res = self.group.collect_episodes(descs, [m["ready"] for m in mem], [m["obs"] for m in mem], ns, det, bound, low, high)
        except BaseException as e:
            bad = getattr(e, "failed_member", -1)
            for col in cols:
                col.env.sync_native()
            # an argument error (AssertionError): nothing was posted to any env.  A failed step call names no member: env commands are
            # waited for before a step call, so none is in flight then
            if 0 <= bad < len(cols) and not isinstance(e, AssertionError):
                cols[bad].env.mark_broken("a native group collect failed while env commands were in flight")
            if bad >= 0 and e.args:
                e.args = (f"GroupCollector, member {bad}: {e.args[0]}", ) + tuple(e.args[1:])
            raise
        dt = max(time.time() - t0, 1e-9)
        stats = []
        for col, r in zip(cols, res):
            col.env.sync_native()
            col.buffer.sync_sizes()
            col.collect_step += r["steps"]
            col.collect_episode += len(r["ep_rews"])
            col.collect_time += dt
            col.reset_env()
            done_count = r["terminated"] + r["truncated"]
            stats.append({"n/ep": len(r["ep_rews"]), "n/st": r["steps"], "rew": float(r["ep_rews"].mean()),
                          "len": float(r["ep_lens"].mean()), "total_cost": r["total_cost"],
                          "cost": r["total_cost"] / len(r["ep_rews"]), "truncated": r["truncated"] / done_count,
                          "terminated": r["terminated"] / done_count})
        return stats
