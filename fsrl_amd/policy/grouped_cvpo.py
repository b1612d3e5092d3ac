"""Grouped CVPO updates: k independent CVPO policies of one launch structure (multi-seed runs) stepped in lock step on one MI355X
-- `fsrl_cvpo_group_update`, every launch of an update carrying all members.  Per member,
`CVPOPolicyGroup.update(buffers, batch_size, n_updates)` is what OffpolicyTrainer.policy_update_fn does between pre_update_fn and
post_update_fn: n_i calls of `policy.update(batch_size, buffer)` -- same Philox stream, same statistics rows, same lr_scheduler
steps.

    group = CVPOPolicyGroup([agent.policy for agent in agents])
    ... every agent collects into ITS buffer (its own resident device actor), resets ITS M-step multipliers (pre_update_fn) ...
    group.update(buffers, batch_size=256, n_updates=[n_0, n_1, ...])
    ... post_update_fn per agent (drains the rows into its logger, actor_old <- actor) ...

The policies' networks are all fused (two hidden layers of at most 256 units) or all layered of one `hidden_sizes`; layered seeds
collect in lock step through `GroupCollector` over an `EngineCollectGroup` of their engines (L + 2 launches per vector step).

The loop is grouped_sac.ReplayPolicyGroup's."""
from fsrl_amd.engine import EngineCvpoGroup
from fsrl_amd.policy.cvpo import CVPO
from fsrl_amd.policy.grouped_sac import ReplayPolicyGroup


class CVPOPolicyGroup(ReplayPolicyGroup):
    policy_cls = CVPO
    algo_name = "CVPO"

    def _make_group(self, engines):
        return EngineCvpoGroup(engines)

    def _update_args(self):
        return ()           # no multiplier from the host: CVPO's duals live on the device
