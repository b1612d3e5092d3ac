"""TRPOLagrangian over the HIP engine: constructor arguments and logger keys of
fsrl/policy/trpo_lag.py:16-301.  `update()` = process_fn + `repeat` x { natural-gradient step by
CG with Fisher-vector products (damping 0.1), step = sqrt(2 delta / d'Hd), backtracking line
search ; optim_critic_iters critic Adam steps } through `fsrl_tr_begin` / `fsrl_trpo_learn`."""
from typing import Any, List, Optional, Tuple, Union

import numpy as np
import torch
from torch import nn

from fsrl_amd.policy.base_policy import DeviceBatch
from fsrl_amd.policy.lagrangian_base import LagrangianPolicy

TRPO_KEYS = ("loss/rescaling", "loss/lagrangian", "loss/actor_safety", "loss/actor_rew", "loss/actor_total",
             "loss/vf0", "loss/vf1", "loss/vf_total", "loss/kl", "loss/step_size", "loss/entropy")


def _split_sizes(n: int, size: int):
    """row counts of tianshou's Batch.split(size, merge_last=True) over n rows"""
    size = max(1, min(int(size), max(n, 1)))
    out, i, merge = [], 0, (n % size) > 0
    while i < n:
        if merge and i + 2 * size >= n:
            out.append(n - i)
            break
        out.append(min(size, n - i))
        i += size
    return out


class TRPOLagrangian(LagrangianPolicy):
    def __init__(self, actor: nn.Module, critics: Union[nn.Module, List[nn.Module]],
                 optim: torch.optim.Optimizer, dist_fn, logger=None,
                 # TRPO specific arguments
                 target_kl: float = 0.001, backtrack_coeff: float = 0.8, max_backtracks: int = 10,
                 optim_critic_iters: int = 5, gae_lambda: float = 0.95,
                 advantage_normalization: bool = True,
                 # Lagrangian specific arguments
                 use_lagrangian: bool = True, lagrangian_pid: Tuple = (0.05, 0.0005, 0.1),
                 cost_limit: Union[List, float] = np.inf, rescaling: bool = True,
                 # Base policy common arguments
                 gamma: float = 0.99, max_batchsize: int = 99999, reward_normalization: bool = False,
                 deterministic_eval: bool = True, action_scaling: bool = True,
                 action_bound_method: str = "clip", observation_space=None, action_space=None,
                 lr_scheduler=None, device: Union[int, str] = 0, env_num: int = 1,
                 buffer_size: int = 100000, reference_rng: bool = False) -> None:
        super().__init__(actor, critics, dist_fn, logger, use_lagrangian, lagrangian_pid, cost_limit,
                         rescaling, gamma, max_batchsize, reward_normalization, deterministic_eval,
                         action_scaling, action_bound_method, observation_space, action_space, lr_scheduler)
        assert self.critics_num == 2, "the HIP path supports one cost constraint"
        self.optim = optim
        self._reference_rng = reference_rng
        self._lambda, self._norm_adv = gae_lambda, advantage_normalization
        self._max_backtracks, self._delta = max_backtracks, target_kl
        self._backtrack_coeff, self._optim_critic_iters = backtrack_coeff, optim_critic_iters
        self._damping = 0.1
        self._make_engine(device, env_num, buffer_size, optim, gae_lambda=gae_lambda, target_kl=None,
                          use_lagrangian=use_lagrangian)

    def _burn(self, n_rows: int, forwards: int) -> None:
        """The reference's forward() samples an action ([n, Da] normals from torch's stream) every time it is
        called in training mode, also inside update(); reference_rng=True consumes the same amount."""
        if self._reference_rng and (self.training or not self._deterministic_eval):
            da = self.engine.cfg.act_dim
            for _ in range(forwards):
                torch.normal(torch.zeros(n_rows, da), torch.ones(n_rows, da))

    def process_fn(self, batch=None, buffer=None, indices=None, **kwargs: Any):
        """trpo_lag.py:132-146 on the device = `fsrl_tr_begin`: sample(0), V / GAE per critic, advantage normalisation, logp_old.
        -> DeviceBatch; `batch` / `indices` ignored (the on-policy batch is the whole store)."""
        assert getattr(buffer, "engine", None) is self.engine
        self.updating = True
        g = self.optim.param_groups[0]
        n = self.engine.tr_begin(target_kl=self._delta, backtrack_coeff=self._backtrack_coeff, damping=self._damping,
                                 l2_reg=0.0, critic_lr=g["lr"], max_backtracks=self._max_backtracks,
                                 optim_critic_iters=self._optim_critic_iters, cg_iters=10, norm_adv=self._norm_adv)
        self._pending = DeviceBatch(self.engine, n, 0)
        return self._pending

    # learn() in three parts, so that fsrl_amd.policy.TrustPolicyGroup can run the device part of k policies on k threads while
    # everything that touches a host random stream or the logger stays on the calling thread, in member order
    def _learn_prepare(self, batch, batch_size: int, repeat: int) -> dict:
        """host, before the device: takes the pending batch, reads the multiplier, draws learn's permutations from numpy's stream"""
        assert isinstance(batch, DeviceBatch) and batch is getattr(self, "_pending", None), \
            "learn() takes the DeviceBatch the last process_fn() returned (the processed batch lives in HBM)"
        self._pending = None
        n = batch.n
        lags, rescaling = self.lagrangians_and_rescaling() if self.use_lagrangian else ([], 1.0)
        # Batch.split(batch_size, merge_last=True) inside learn (trpo_lag.py:177-178) draws one np.random.permutation per
        # repeat from numpy's global stream -- also when one minibatch covers the batch (then the order only moves sums and
        # the device keeps store order)
        perms = [np.random.permutation(n) for _ in range(repeat)] if n > 0 else None
        sizes = _split_sizes(n, batch_size)
        return dict(n=n, repeat=repeat, batch_size=batch_size, sizes=sizes, perms=perms if len(sizes) > 1 else None,
                    lags=lags, rescaling=rescaling)

    def _learn_device(self, plan: dict):
        """library calls only (ctypes releases the GIL inside them): -> (stats rows, line-search evaluations per row)"""
        if plan["n"] <= 0:
            return np.zeros((0, 11), np.float32), np.zeros(0, np.int32)
        stats = self.engine.trpo_learn(plan["lags"], plan["rescaling"], plan["repeat"], batch_size=plan["batch_size"],
                                       perms=plan["perms"])
        return stats, self.engine.tr_linesearch_evals(cap=len(stats) + 1)

    def _learn_finish(self, plan: dict, stats, evals):
        """host, after the device: the logged rows, the reference's wasted torch draws, the stale mark"""
        for row in stats:
            d = dict(zip(TRPO_KEYS, (float(v) for v in row)))
            kl, step, ent = d.pop("loss/kl"), d.pop("loss/step_size"), d.pop("loss/entropy")
            self.gradient_steps += self._optim_critic_iters
            self.logger.store(**d)
            self.logger.store(kl=kl, step_size=step, entropy=ent, tab="loss")
        self.logger.store(gradient_steps=self.gradient_steps, tab="update")
        if plan["n"] > 0:   # process_fn: one forward over the batch; per minibatch: 2 forward(s) + one per line-search evaluation
            self._burn(plan["n"], 1)
            for rows, ev in zip(plan["sizes"] * plan["repeat"], evals):
                self._burn(rows, 2 + int(ev))
        self._mark_stale()                                       # host mirror refreshed on demand
        return {"gradient_steps": len(stats)}

    def learn(self, batch, batch_size: int = 99999, repeat: int = 4, **kwargs: Any):
        """trpo_lag.py:173-251 on the device = `fsrl_trpo_learn[_mb]`; `batch` is what process_fn returned."""
        plan = self._learn_prepare(batch, batch_size, repeat)
        return self._learn_finish(plan, *self._learn_device(plan))

    def update(self, sample_size: int, buffer, batch_size: int = 99999, repeat: int = 4, **kwargs: Any):
        """base_policy.py:332-355: sample(0) -> process_fn -> learn -> lr scheduler"""
        if buffer is None:
            return {}
        assert sample_size == 0
        try:
            batch = self.process_fn(None, buffer, None)
            result = self.learn(batch, batch_size=batch_size, repeat=repeat)
        finally:
            self.updating = False
        self._step_lr_scheduler()
        return result
