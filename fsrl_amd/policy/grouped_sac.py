"""Grouped SAC-Lagrangian updates: k independent SACLagrangian policies of one network shape (multi-seed runs) stepped in lock
step on one MI355X -- `fsrl_sac_group_update`, every launch of an update carrying all members.  Per member,
`SACPolicyGroup.update(buffers, batch_size, n_updates)` is what OffpolicyTrainer.policy_update_fn does between pre_update_fn and
post_update_fn: n_i calls of `policy.update(batch_size, buffer)` -- same lambda and rescaling, same Philox stream, same statistics
rows, same lr_scheduler steps.  The policies' buffers may be `HipPrioritizedVectorReplayBuffer`s (all of them, made before the
group; alpha, beta and weight_norm may differ): the grouped update then draws every member's batch from its sum tree, weights its
critics' loss and writes its new priorities back inside the shared launches, as n_i prioritised `policy.update` calls would.

    group = SACPolicyGroup([agent.policy for agent in agents])
    ... every agent collects into ITS buffer (its own resident device actor), steps ITS PID multiplier (pre_update_fn) ...
    group.update(buffers, batch_size=256, n_updates=[n_0, n_1, ...])
    ... post_update_fn per agent (drains the rows into its logger) ...

`ReplayPolicyGroup` holds the loop; `SACPolicyGroup` here and `DDPGPolicyGroup` (grouped_ddpg.py) name their policy class, and
`CVPOPolicyGroup` (grouped_cvpo.py) its engine group and its engine call as well."""
from typing import Sequence, Union

from fsrl_amd.engine import EngineSacGroup
from fsrl_amd.policy.sac_lag import SACLagrangian

_RING_DRAIN = 2048          # the policies' learn() drains their statistics ring after this many pending updates


class ReplayPolicyGroup:
    """k policies of `policy_cls` over an EngineSacGroup (fsrl_sac_group_*); subclasses set `policy_cls` and `algo_name`, and
    override `_make_group` / `_update_args` where their engine group is another"""
    policy_cls: type = None
    algo_name: str = ""

    def __init__(self, policies: Sequence, engine_group=None):
        self.policies = list(policies)
        assert self.policies, "a group needs at least one policy"
        assert all(isinstance(p, self.policy_cls) for p in self.policies), \
            "grouped %s updates: %s policies" % (self.algo_name, self.policy_cls.__name__)
        # reference_rng=True draws the sample and the noise from the host's numpy / torch streams, one update at a time: a grouped
        # update has the device's Philox streams only
        assert not any(getattr(p, "_reference_rng", False) for p in self.policies), "reference_rng policies cannot be grouped"
        # prioritised replay (the policies' HipPrioritizedVectorReplayBuffers, made before the group): on every member or on none
        per = [bool(getattr(p.engine, "per_on", False)) for p in self.policies]
        assert all(per) or not any(per), "grouped updates: every policy's buffer is a HipPrioritizedVectorReplayBuffer, or none is"
        self.group = engine_group if engine_group is not None else self._make_group([p.engine for p in self.policies])

    def _make_group(self, engines):
        return EngineSacGroup(engines)

    def _update_args(self):
        """what `group.update(B, step, ...)` takes after the counts, the same for every chunk of one update"""
        pols = self.policies
        lags, resc = [], []
        for p in pols:
            lg, rs = p.lagrangians_and_rescaling() if p.use_lagrangian else ([], 1.0)
            lags.append([float(x) for x in lg] or [0.0])
            resc.append(float(rs))
        return (lags if pols[0].use_lagrangian else None, resc)

    def close(self):
        self.group.close()

    def update(self, buffers, batch_size: int = 256, n_updates: Union[int, Sequence[int]] = 1):
        pols = self.policies
        k = len(pols)
        n = [int(n_updates)] * k if isinstance(n_updates, (int,)) else [int(x) for x in n_updates]
        assert len(n) == k and all(x >= 0 for x in n), "n_updates: one count >= 0 per policy"
        assert len(buffers) == k, "one buffer per policy"
        for p, b in zip(pols, buffers):
            assert getattr(b, "engine", None) is p.engine, "buffer i must be the HipVectorReplayBuffer of policy i"
        B = int(batch_size)
        for p in pols:
            p.updating = True
        try:
            # a fresh policy's first update keys its Philox stream (learn: seed + 1): that one runs on its own
            for i, (p, b) in enumerate(zip(pols, buffers)):
                if n[i] > 0 and p.gradient_steps == 0:
                    p.update(B, b)
                    p.updating = True
                    n[i] -= 1
            args = self._update_args()
            # an lr scheduler moves the rates between two updates: one update per grouped call then
            per_call = 1 if any(p.lr_scheduler is not None for p in pols) else _RING_DRAIN
            left = list(n)
            while any(left):
                step = [min(x, per_call, _RING_DRAIN - p._pending) for x, p in zip(left, pols)]
                self.group.update(B, step, *args)
                for i, p in enumerate(pols):
                    if not step[i]:
                        continue
                    left[i] -= step[i]
                    p.gradient_steps += step[i]
                    p._pending += step[i]
                    p._dirty = p._rest_dirty = True
                    for _ in range(step[i]):
                        p._step_lr_scheduler()
                    if p._pending >= _RING_DRAIN:
                        p._drain()
        except BaseException:
            # a failed group update may have stepped some parameters already: the host mirrors are stale, nobody is updating
            for p in pols:
                p.updating = False
                p._dirty = p._rest_dirty = True
                p._mark_stale()
            raise
        for p in pols:
            p.updating = False
        return [{} for _ in pols]


class SACPolicyGroup(ReplayPolicyGroup):
    policy_cls = SACLagrangian
    algo_name = "SAC"
