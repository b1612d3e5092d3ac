"""Grouped trust-region seeds: k independent CPO policies, or k TRPOLagrangian policies, of one network shape (multi-seed runs)
on one MI355X.  What is shared is COLLECTION: an `EngineCollectGroup` over the policies' engines answers every seed's actor
request of a vector step with one launch (`GroupCollector(collect_group, collectors)`).  The UPDATES are not grouped launches --
a CPO update is some forty host decisions with read-backs between its launches, and the seeds diverge in dual-solve case and in
backtracks -- they are the members' own `fsrl_tr_begin` / `fsrl_cpo_learn[_mb]` / `fsrl_trpo_learn[_mb]`, each on its own streams,
run beside each other on one host thread per member (ctypes releases the GIL inside the library), so that one member's read-back
gaps are filled by another member's kernels.  Per member, `TrustPolicyGroup.update(buffers, batch_size, repeat)` is
`policy.update(0, buffer, batch_size=..., repeat=...)` bit for bit: same parameters, same logged rows, same draws from numpy's and
torch's global streams (they stay on the calling thread, in member order), same lr_scheduler step.

    cgroup = EngineCollectGroup([agent.policy.engine for agent in agents])
    gcol = GroupCollector(cgroup, collectors)
    group = TrustPolicyGroup([agent.policy for agent in agents], collect_group=cgroup)
    ... gcol.collect(...); every agent's pre_update_fn sees ITS cost ...
    group.update(buffers, batch_size=99999, repeat=4)
"""
from concurrent.futures import ThreadPoolExecutor, wait
from typing import Sequence, Union

from fsrl_amd.policy.cpo import CPO
from fsrl_amd.policy.trpo_lag import TRPOLagrangian

MAX_THREADS = 16            # one worker per member up to here; more members take turns


def _shape(p):
    c = p.engine.cfg
    hs = tuple(c.hidden_sizes) if getattr(c, "hidden_sizes", None) is not None else (c.hidden, c.hidden)
    return (c.obs_dim, c.act_dim, hs)


class TrustPolicyGroup:
    def __init__(self, policies: Sequence[Union[CPO, TRPOLagrangian]], collect_group=None):
        """collect_group: the EngineCollectGroup the policies' engines collect through, if any -- update() ends its kernel first"""
        self.policies = list(policies)
        assert self.policies, "a group needs at least one policy"
        cls = CPO if isinstance(self.policies[0], CPO) else TRPOLagrangian
        assert all(isinstance(p, cls) for p in self.policies), \
            "grouped trust-region updates: all CPO or all TRPOLagrangian policies (one algorithm per group)"
        assert all(_shape(p) == _shape(self.policies[0]) for p in self.policies), \
            "members must have one network shape (obs_dim, act_dim, hidden_sizes)"
        assert len({getattr(p.engine, "device", 0) for p in self.policies}) == 1, "members live on one device"
        assert len({id(p.engine) for p in self.policies}) == len(self.policies), "a policy is listed twice"
        self.collect_group = collect_group
        self._pool = None

    def close(self):
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _device_parts(self, plans):
        """every member's _learn_device on a worker thread; all of them are joined before anything is raised"""
        pols = self.policies
        if len(pols) == 1:
            return [pols[0]._learn_device(plans[0])]
        if self._pool is None:
            self._pool = ThreadPoolExecutor(max_workers=min(len(pols), MAX_THREADS), thread_name_prefix="trust-group")
        futs = [self._pool.submit(p._learn_device, plan) for p, plan in zip(pols, plans)]
        wait(futs)                                               # no member's call stays in flight behind another's error
        for i, f in enumerate(futs):
            err = f.exception()
            if err is not None:
                raise RuntimeError("member %d: %s" % (i, err)) from err
        return [f.result() for f in futs]

    def update(self, buffers, batch_size: int = 99999, repeat: int = 4):
        pols = self.policies
        assert len(buffers) == len(pols), "one buffer per policy"
        for p, b in zip(pols, buffers):
            assert getattr(b, "engine", None) is p.engine, "buffer i must be the HipVectorReplayBuffer of policy i"
        try:
            if self.collect_group is not None:
                self.collect_group.actor_release()               # the collect is over: its kernel ends before any member's update
            batches = [p.process_fn(None, b, None) for p, b in zip(pols, buffers)]
            plans = [p._learn_prepare(batch, batch_size, repeat) for p, batch in zip(pols, batches)]
            done = self._device_parts(plans)
            out = [p._learn_finish(plan, *res) for p, plan, res in zip(pols, plans, done)]
        except BaseException:
            # a failed update may have stepped some parameters already: the host mirrors are stale, nobody is updating
            for p in pols:
                p.updating = False
                p._pending = None
                p._mark_stale()
            raise
        for p in pols:
            p.updating = False
            p._step_lr_scheduler()
        return out
