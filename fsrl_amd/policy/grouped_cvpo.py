"""Grouped CVPO updates: k independent CVPO policies of one launch structure (multi-seed runs) stepped in lock step on one MI355X
-- `fsrl_cvpo_group_update`, every launch of an update carrying all members.  Per member,
`CVPOPolicyGroup.update(buffers, batch_size, n_updates)` is what OffpolicyTrainer.policy_update_fn does between pre_update_fn and
post_update_fn: n_i calls of `policy.update(batch_size, buffer)` -- same Philox stream, same statistics rows, same lr_scheduler
steps.

    group = CVPOPolicyGroup([agent.policy for agent in agents])
    ... every agent collects into ITS buffer (its own resident device actor), resets ITS M-step multipliers (pre_update_fn) ...
    group.update(buffers, batch_size=256, n_updates=[n_0, n_1, ...])
    ... post_update_fn per agent (drains the rows into its logger, actor_old <- actor) ..."""
from typing import Sequence, Union

from fsrl_amd.engine import EngineCvpoGroup
from fsrl_amd.policy.cvpo import CVPO

_RING_DRAIN = 2048          # CVPO.learn drains its statistics ring after this many pending updates


class CVPOPolicyGroup:
    def __init__(self, policies: Sequence[CVPO], engine_group=None):
        self.policies = list(policies)
        assert self.policies, "a group needs at least one policy"
        assert all(isinstance(p, CVPO) for p in self.policies), "grouped CVPO updates: CVPO policies"
        # reference_rng=True draws the sample and the noise from the host's numpy / torch streams, one update at a time: a grouped
        # update has the device's Philox streams only
        assert not any(getattr(p, "_reference_rng", False) for p in self.policies), "reference_rng policies cannot be grouped"
        self.group = engine_group if engine_group is not None else EngineCvpoGroup([p.engine for p in self.policies])

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
            # a fresh policy's first update keys its Philox stream (CVPO.learn: seed + 1): that one runs on its own
            for i, (p, b) in enumerate(zip(pols, buffers)):
                if n[i] > 0 and p.gradient_steps == 0:
                    p.update(B, b)
                    p.updating = True
                    n[i] -= 1
            # an lr scheduler moves the rates between two updates: one update per grouped call then
            per_call = 1 if any(p.lr_scheduler is not None for p in pols) else _RING_DRAIN
            left = list(n)
            while any(left):
                step = [min(x, per_call, _RING_DRAIN - p._pending) for x, p in zip(left, pols)]
                self.group.update(B, step)
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
