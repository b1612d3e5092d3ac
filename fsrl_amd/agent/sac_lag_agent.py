"""SACLagAgent + the off-policy learn loop: keyword arguments and defaults of
fsrl/agent/sac_lag_agent.py:75-203 and fsrl/agent/base_agent.py:108-209."""
from typing import Optional, Tuple

import numpy as np
import torch

from fsrl_amd.agent._nets import adam, offpolicy_nets
from fsrl_amd.agent.base_agent import BaseAgent
from fsrl_amd.data import FastCollector, HipPrioritizedVectorReplayBuffer, HipVectorReplayBuffer
from fsrl_amd.data.device_collector import evaluation_collector
from fsrl_amd.policy.sac_lag import SACLagrangian
from fsrl_amd.trainer.offpolicy import OffpolicyTrainer
from fsrl_amd.utils.exp_util import seed_all
from fsrl_amd.utils.logger import DummyLogger


class OffpolicyAgent(BaseAgent):
    name = "OffpolicyAgent"

    def __init__(self) -> None:
        pass

    def learn(self, train_envs, test_envs=None, epoch: int = 300, episode_per_collect: int = 5,
              step_per_epoch: int = 3000, update_per_step: float = 0.1, buffer_size: Optional[int] = None,
              testing_num: int = 2, batch_size: int = 256, reward_threshold: float = 450,
              save_interval: int = 4, resume: bool = False, save_ckpt: bool = True, verbose: bool = True,
              show_progress: bool = True, device_actor: bool = False, ckpt_store: bool = True, prefill=None,
              prioritized_replay: Optional[dict] = None):
        """resume=True continues the run whose training state `<log_dir>/checkpoint/train_state.pt` holds (saved with every periodic
        checkpoint while save_ckpt is on): epoch numbering, env steps, the best result, the replay store, optimiser state and
        random streams carry over; without such a file the run starts fresh and says so.  Env state is never saved: a resumed
        run resets its envs.  ckpt_store: whether the replay store goes into train_state.pt (about 320 MB for a million rows of
        33 observations and 8 actions); without it a resumed run starts from an empty store.
        prefill: a TrajectoryBuffer, or the path of a dataset one saved -- its episodes are poured into the replay store
        (HipVectorReplayBuffer.fill_from, actions mapped back with this policy's inverse action map) after the store has been cut
        to this call's geometry and before the first collect; no env step is counted for them.  Skipped, with a printed line, when
        resume=True restored a store.
        prioritized_replay: None, or dict(alpha=..., beta=..., weight_norm=True) -- the replay buffer is then what tianshou's
        PrioritizedVectorReplayBuffer(buffer_size, len(train_envs), alpha, beta, weight_norm) is to the reference: updates draw
        their batch by priority, weight the critics' loss and hand |TD| back as the new priorities, all on the device.  SAC-Lag
        and DDPG-Lag with the library's sampler (not reference_rng, whose indices come from the host's uniform draw)."""
        assert self.policy is not None, "The policy is not initialized"
        self.policy.train()
        eng = self.policy.engine
        from fsrl_amd.env.venv import as_vector_env
        train_envs = as_vector_env(train_envs)                 # a single env: one sub-buffer (base_agent.py:160-163)
        assert eng.cfg.env_num >= len(train_envs)
        # VectorReplayBuffer(buffer_size, len(train_envs)) of the reference (base_agent.py:279): the store is re-cut to
        # that geometry.  None = the size the agent was built with (its `buffer_size`, default 100 000 like the
        # reference's learn()); an explicit size must fit that allocation (AssertionError otherwise).
        if prioritized_replay is not None:
            self._check_prioritized(prioritized_replay)
            buffer = HipPrioritizedVectorReplayBuffer(eng, buffer_size, len(train_envs), **prioritized_replay)
        else:
            buffer = HipVectorReplayBuffer(eng, buffer_size, len(train_envs))
        # device_actor=True: actor + noise on the MI355X (library RNG); over a worker-process env the collector then also
        # overlaps the actor with the env workers when that pays (split_phase="auto")
        from fsrl_amd.env.device import DeviceVectorEnv
        if isinstance(train_envs, DeviceVectorEnv):
            # the envs live on the GPU: a collect is a handful of launches of one looping kernel (fsrl_collect_device), and with a
            # prioritised buffer the rows' leaves are written behind each of them
            from fsrl_amd.data.device_collector import DeviceCollector
            train_collector = DeviceCollector(self.policy, train_envs, buffer, exploration_noise=True)
        else:
            train_collector = FastCollector(self.policy, train_envs, buffer, exploration_noise=True, device_actor=device_actor,
                                            split_phase="auto" if device_actor else False)
        test_collector = evaluation_collector(self.policy, test_envs)       # device test envs: store-less DeviceCollector

        def stop_fn(reward, cost):
            return reward > reward_threshold and cost < self.cost_limit

        if save_ckpt:
            self.logger.setup_checkpoint_fn(lambda: {"model": self.state_dict})
        trainer = OffpolicyTrainer(policy=self.policy, train_collector=train_collector,
                                   test_collector=test_collector, max_epoch=epoch, batch_size=batch_size,
                                   cost_limit=self.cost_limit, step_per_epoch=step_per_epoch,
                                   update_per_step=update_per_step, episode_per_test=testing_num,
                                   episode_per_collect=episode_per_collect, stop_fn=stop_fn,
                                   logger=self.logger, resume_from_log=resume,
                                   save_model_interval=save_interval, verbose=verbose,
                                   show_progress=show_progress)
        if save_ckpt:                            # registered late: the state is the trainer's and the policy's
            self.logger.setup_train_state_fn(lambda: trainer.train_state(with_store=ckpt_store))
        if prefill is not None:
            self._prefill(prefill, buffer, resumed=resume and len(buffer) > 0)
        ep, stat, info = 0, {}, {}
        for ep, stat, info in trainer:
            self.logger.store(tab="train", cost_limit=self.cost_limit)
            if verbose:
                print(f"Epoch: {ep}", info)
        return ep, stat, info

    def _check_prioritized(self, prioritized_replay: dict) -> None:
        unknown = set(prioritized_replay) - {"alpha", "beta", "weight_norm"}
        if unknown or not {"alpha", "beta"} <= set(prioritized_replay):
            raise ValueError(f"prioritized_replay takes alpha, beta and optionally weight_norm, got {sorted(prioritized_replay)}")
        if getattr(self.policy, "_reference_rng", False):
            raise ValueError("prioritized_replay needs the library's sampler: with reference_rng=True the batch indices are drawn "
                             "uniformly on the host")

    def _prefill(self, prefill, buffer, resumed: bool) -> int:
        """learn(prefill=...): a TrajectoryBuffer or a dataset path -> rows poured into `buffer`"""
        if resumed:
            print(f"prefill: skipped, the resumed run restored a replay store of {len(buffer)} rows")
            return 0
        from fsrl_amd.data.traj_buf import TrajectoryBuffer, _read_dataset
        tb, own = prefill, False
        if not isinstance(prefill, TrajectoryBuffer):
            # a file: an archive of its own on this engine's device, sized for the file, attached to nothing (it records nothing)
            # and gone after the fill; every episode of the file is kept (no window, no filter)
            data = _read_dataset(prefill)
            ends = np.flatnonzero(np.asarray(data["terminals"]).astype(bool) | np.asarray(data["timeouts"]).astype(bool)) + 1
            longest = int(np.diff(np.concatenate([[0], ends])).max()) if len(ends) else 1
            tb = TrajectoryBuffer(max_trajectory=max(len(ends), 1), use_grid_filter=False, max_rows=max(len(data["rewards"]), longest, 1),
                                  max_episode_len=longest)
            tb._create(self.policy.engine, self.policy)
            own = True
            tb.load(data)
        try:
            rows = buffer.fill_from(tb, policy=self.policy)
        finally:
            if own:
                tb.close()
        print(f"prefill: {rows} rows poured into the replay store ({len(buffer)} rows held)")
        return rows


class SACLagAgent(OffpolicyAgent):
    name = "SACLagAgent"

    def __init__(self, env, logger=None, cost_limit: float = 10, device: str = "cuda:0", thread: int = 4,
                 seed: int = 10, actor_lr: float = 5e-4, critic_lr: float = 1e-3,
                 hidden_sizes: Tuple[int, ...] = (128, 128), auto_alpha: bool = True, alpha_lr: float = 3e-4,
                 alpha: float = 0.002, tau: float = 0.05, n_step: int = 2, use_lagrangian: bool = True,
                 lagrangian_pid: Tuple[float, ...] = (0.05, 0.0005, 0.1), rescaling: bool = True,
                 gamma: float = 0.99, conditioned_sigma: bool = True, unbounded: bool = True,
                 last_layer_scale: bool = False, deterministic_eval: bool = False, action_scaling: bool = True,
                 action_bound_method: str = "clip", lr_scheduler=None, training_num: int = 10,
                 buffer_size: int = 100000, reference_rng: bool = False) -> None:
        super().__init__()
        self.logger = logger if logger is not None else DummyLogger()
        self.cost_limit = cost_limit
        assert np.isscalar(cost_limit), "the HIP SAC path: one cost"
        assert conditioned_sigma, \
            "conditioned_sigma=False is not supported on the HIP SAC path: a state-independent sigma is another parameter layout"
        seed_all(seed)
        torch.set_num_threads(thread)
        actor, critics = offpolicy_nets(env, hidden_sizes, "double", unbounded=unbounded, last_layer_scale=last_layer_scale)
        actor_optim, critic_optim = adam(actor, actor_lr), adam(critics, critic_lr)
        if auto_alpha:
            target_entropy = -float(np.prod(env.action_space.shape))
            log_alpha = torch.zeros(1, requires_grad=True)
            alpha = (target_entropy, log_alpha, torch.optim.Adam([log_alpha], lr=alpha_lr))
        self.policy = SACLagrangian(actor=actor, critics=critics, actor_optim=actor_optim,
                                    critic_optim=critic_optim, logger=self.logger, alpha=alpha, tau=tau,
                                    gamma=gamma, exploration_noise=None, n_step=n_step,
                                    use_lagrangian=use_lagrangian, lagrangian_pid=lagrangian_pid,
                                    cost_limit=cost_limit, rescaling=rescaling, reward_normalization=False,
                                    deterministic_eval=deterministic_eval, action_scaling=action_scaling,
                                    action_bound_method=action_bound_method,
                                    observation_space=env.observation_space, action_space=env.action_space,
                                    lr_scheduler=lr_scheduler, device=device, env_num=training_num,
                                    buffer_size=buffer_size, reference_rng=reference_rng, seed=seed)
