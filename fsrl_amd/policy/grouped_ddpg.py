"""Grouped DDPG-Lagrangian updates: k independent DDPGLagrangian policies of one network shape (multi-seed runs) stepped in lock
step on one MI355X -- `fsrl_sac_group_update` over deterministic-actor contexts, every launch of an update carrying all members.
Per member, `DDPGPolicyGroup.update(buffers, batch_size, n_updates)` is n_i calls of `policy.update(batch_size, buffer)`: same
lambda and rescaling, same Philox stream, same statistics rows, same lr_scheduler steps, and the same Polyak steps of
`actor_old` and `critics_old`.

    group = DDPGPolicyGroup([agent.policy for agent in agents])
    ... every agent collects into ITS buffer, steps ITS PID multiplier (pre_update_fn) ...
    group.update(buffers, batch_size=256, n_updates=[n_0, n_1, ...])
    ... post_update_fn per agent (drains the rows into its logger) ...

The loop is grouped_sac.ReplayPolicyGroup's."""
from fsrl_amd.policy.ddpg_lag import DDPGLagrangian
from fsrl_amd.policy.grouped_sac import ReplayPolicyGroup


class DDPGPolicyGroup(ReplayPolicyGroup):
    policy_cls = DDPGLagrangian
    algo_name = "DDPG"
