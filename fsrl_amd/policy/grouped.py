"""Grouped on-policy updates: k independent policies of one network shape (multi-seed runs) stepped in lock step on one
MI355X -- `fsrl_group_ppo_update`, every launch of the minibatch step carrying all members ("optional within-GPU
batching of k seeds").  The reference runs seeds as separate jobs; per member this is
- PPOLagrangian.update (fsrl/policy/ppo_lag.py:214-257 after base_policy.py:332-355), or
- FOCOPS.update (fsrl/policy/focops.py:126-251): each member's nu step (FOCOPS.nu_step, the host float32 arithmetic of
  process_fn), then the grouped update,
with the same arguments, the same logger keys and the same lr_scheduler step.  A group is all PPOLagrangian or all FOCOPS.
The members (PPOLagrangian or FOCOPS) may be layered (`hidden_sizes` other than two layers of at most 256 units) when all of them
have the same `hidden_sizes`: the layered minibatch step then carries every member in each of its 2 L + 5 launches, and a
member's grouped update is its own update bit for bit.

    group = PolicyGroup([agent.policy for agent in agents])
    ... every agent collects into ITS buffer, steps ITS PID multiplier / sees ITS cost (trainer.policy_update_fn does
    pre_update_fn) ...
    group.update(buffers, batch_size=256, repeat=4)

A PPOLagrangian group may be a sweep: the members' own eps_clip, dual_clip, vf_coef, max_grad_norm value, target_kl, advantage /
reward normalisation, value clip and optimiser settings are used, each member as in its own update (they must agree on the network
shape, the number of critics, max_action, `unbounded` and on whether max_grad_norm is on), and `batch_size` / `repeat` may be one
int per member.  A FOCOPS group keeps one set of hyper-parameters.

Random streams: the library shuffles (member i seeded from `seed`), so k grouped seeds are k independent runs but not the
reference's numpy permutation stream (PPOLagrangian.learn / FOCOPS.learn draw np.random.permutation per pass); pass `perms`
for that."""
from typing import List, Optional, Sequence, Union

import numpy as np

from fsrl_amd.engine import EngineGroup
from fsrl_amd.policy.focops import FOCOPS
from fsrl_amd.policy.ppo_lag import PPO_STAT_KEYS, PPOLagrangian


class PolicyGroup:
    def __init__(self, policies: Sequence[Union[PPOLagrangian, FOCOPS]], seed: int = 1, engine_group=None):
        """engine_group: the EngineGroup of the policies' engines (default: made here; tests pass a stand-in)"""
        self.policies = list(policies)
        assert self.policies, "a group needs at least one policy"
        cls = PPOLagrangian if isinstance(self.policies[0], PPOLagrangian) else FOCOPS
        assert all(isinstance(p, cls) for p in self.policies), \
            "grouped updates: all PPOLagrangian or all FOCOPS policies (one algorithm per group)"
        self.focops = cls is FOCOPS
        # reference_rng=True burns the torch draws the reference wastes inside update(); a grouped update has no
        # single-policy random stream to follow
        assert not any(getattr(p, "_reference_rng", False) for p in self.policies), "reference_rng policies cannot be grouped"
        self.group = engine_group if engine_group is not None else EngineGroup([p.engine for p in self.policies])
        self._seed, self._calls = int(seed), 0

    def close(self):
        self.group.close()

    def update(self, buffers, batch_size: Union[int, Sequence[int]] = 256, repeat: Union[int, Sequence[int]] = 4,
               perms: Optional[List] = None):
        """batch_size / repeat: an int for every member, or one int per member (a sweep over batch_size / repeat_per_collect of a
        PPOLagrangian group: EngineGroup.ppo_update_each; perms[i] then holds repeat[i] permutations)."""
        pols = self.policies
        each = not (isinstance(batch_size, (int, np.integer)) and isinstance(repeat, (int, np.integer)))
        if each:
            assert not self.focops, "a FOCOPS group takes one batch_size and one repeat (sweeps are PPOLagrangian groups)"
            per = lambda v: [int(v)] * len(pols) if isinstance(v, (int, np.integer)) else [int(x) for x in v]
            batch_size, repeat = per(batch_size), per(repeat)
            assert len(batch_size) == len(pols) and len(repeat) == len(pols), "one batch_size and one repeat per member"
        for p, b in zip(pols, buffers):
            assert getattr(b, "engine", None) is p.engine, "buffer i must be the HipVectorReplayBuffer of policy i"
            p.updating = True
        try:
            self._calls += 1
            seed = 0 if perms is not None else self._seed + 7919 * self._calls
            if self.focops:
                nus = [p.nu_step() for p in pols]
                stats, stopped = self.group.focops_update([x[0] for x in nus], [x[1] for x in nus], batch_size, repeat,
                                                          perms=perms, seed=seed)
            else:
                lr = [p.lagrangians_and_rescaling() if p.use_lagrangian else ([0.0] * (p.critics_num - 1), 1.0) for p in pols]
                lags = np.array([x[0] if len(x[0]) else [0.0] for x in lr], np.float64)
                resc = [x[1] for x in lr]
                update = self.group.ppo_update_each if each else self.group.ppo_update
                stats, stopped = update(lags, resc, batch_size, repeat, perms=perms, seed=seed)
        except BaseException:
            # a failed group update may have stepped some parameters already: the host mirrors are stale, nobody is updating
            for p in pols:
                p.updating = False
                p._mark_stale()
            raise
        out = []
        for p, st, sp in zip(pols, stats, stopped):
            if self.focops:                                  # FOCOPS.learn: the early-stop message, then the rows
                if sp >= 0:
                    p.logger.print("Early stop at step %d due to reaching max kl." % sp)
                out.append(p.log_learn(st, sp))
            else:
                out.append(self._log_ppo(p, st, sp))
            p._step_lr_scheduler()
            p.updating = False
        return out

    @staticmethod
    def _log_ppo(p, st, sp):
        drop = set()
        if not p.use_lagrangian or p.critics_num < 2:
            drop |= {"loss/lagrangian", "loss/actor_safety"}
        if p.critics_num < 2:
            drop.add("loss/vf1")
        cols = [j for j, k in enumerate(PPO_STAT_KEYS) if k not in drop]
        keys = [PPO_STAT_KEYS[j] for j in cols]
        table = getattr(p.logger, "store_rows", None)
        if table is not None:
            table(keys, st[:, cols])
        else:
            for row in st:
                p.logger.store(**{k: float(row[j]) for j, k in zip(cols, keys)})
        if sp >= 0:
            p.logger.print("Early stop at step %d due to reaching max kl." % sp)
        p.gradient_steps += len(st)
        p.logger.store(gradient_steps=p.gradient_steps, tab="update")
        p._mark_stale()
        return {"gradient_steps": len(st), "early_stop_pass": sp}
