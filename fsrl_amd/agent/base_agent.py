"""Agent base classes: `evaluate`, `state_dict` and the on-policy `learn` loop with the keyword
arguments of fsrl/agent/base_agent.py:53-93,225-324.  The replay buffer created here is the
HIP-resident store proxy bound to the policy's engine."""
from abc import ABC, abstractmethod
from typing import Optional, Tuple

import numpy as np

from fsrl_amd.data import FastCollector, HipVectorReplayBuffer
from fsrl_amd.data.device_collector import evaluation_collector
from fsrl_amd.trainer import OnpolicyTrainer
from fsrl_amd.utils.logger import BaseLogger, DummyLogger


class BaseAgent(ABC):
    name = "BaseAgent"

    @abstractmethod
    def __init__(self, *args, **kwargs) -> None:
        self.policy = None
        self.logger: BaseLogger = DummyLogger()
        self.cost_limit = 0

    @abstractmethod
    def learn(self, *args, **kwargs):
        raise NotImplementedError

    def evaluate(self, test_envs, state_dict: Optional[dict] = None, eval_episodes: int = 10,
                 render: bool = False, train_mode: bool = False) -> Tuple[float, float, float]:
        if state_dict is not None:
            self.policy.load_state_dict(state_dict)
        self.policy.train() if train_mode else self.policy.eval()
        # device envs of this policy's engine: the whole evaluation on the GPU, nothing stored (fsrl_evaluate_device)
        result = evaluation_collector(self.policy, test_envs, render=render).collect(n_episode=eval_episodes, render=render)
        return result["rew"], result["len"], result["cost"]

    @property
    def state_dict(self):
        return self.policy.state_dict()

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

    def pretrain_from(self, dataset, batch_size: int = 256, n_updates: int = 1000, loss: str = "mse", seed: int = 0) -> np.ndarray:
        """Warm-start the actor by behaviour cloning (policy.pretrain -> fsrl_bc_update / fsrl_bc_update_layered) on a dataset: a TrajectoryBuffer, or the
        path of one saved (examples/collect_dataset.py).  Its episodes are poured into the agent's store, the actor is regressed
        onto their actions for n_updates Adam steps of batch_size rows (loss "mse" | "nll"), and the store is emptied again, so
        that learn() afterwards starts as it does today -- from the pre-trained actor.  Critics are not touched.  Every agent, any
        hidden_sizes: two launches per update whatever the depth.  -> the per-update losses."""
        buffer = HipVectorReplayBuffer(self.policy.engine)
        buffer.reset()
        try:
            self._prefill(dataset, buffer, resumed=False)
            return self.policy.pretrain(buffer, batch_size=batch_size, n_updates=n_updates, loss=loss, seed=seed)
        finally:
            buffer.reset()


def pretrain_group_from(agents, dataset, batch_size=256, n_updates=1000, loss="mse", seeds=None, shared_store=True):
    """BaseAgent.pretrain_from for k agents at once (fsrl_amd.policy.pretrain_group -> fsrl_bc_update_group): the dataset is poured
    ONCE, into agents[0]'s store, every agent's actor is regressed onto its rows in the same two launches per step, and that store
    is emptied again.  Agent i's indices are drawn from seeds[i] (default: i), so the seeds see different minibatches of the one
    dataset; its actor is what its own pretrain_from leaves with that seed.  shared_store=False pours the dataset into every agent's
    own store instead.  Call it before the agents' policies are put into a PolicyGroup.  -> one array of losses per agent."""
    from fsrl_amd.policy import pretrain_group
    agents = list(agents)
    holders = agents[:1] if shared_store else agents
    buffers = [HipVectorReplayBuffer(ag.policy.engine) for ag in holders]
    for b in buffers:
        b.reset()
    try:
        for ag, b in zip(holders, buffers):
            ag._prefill(dataset, b, resumed=False)
        return pretrain_group([ag.policy for ag in agents], buffers[0] if shared_store else None, batch_size=batch_size, n_updates=n_updates,
                              loss=loss, seeds=list(range(len(agents))) if seeds is None else seeds, shared_store=shared_store)
    finally:
        for b in buffers:
            b.reset()


class OnpolicyAgent(BaseAgent):
    name = "OnpolicyAgent"

    def __init__(self) -> None:
        pass

    def learn(self, train_envs, test_envs=None, epoch: int = 300, episode_per_collect: int = 20,
              step_per_epoch: int = 10000, repeat_per_collect: int = 4, buffer_size: Optional[int] = None,
              testing_num: int = 2, batch_size: int = 512, reward_threshold: float = 450,
              save_interval: int = 4, resume: bool = False, save_ckpt: bool = True,
              verbose: bool = True, show_progress: bool = True, device_actor: bool = False, ckpt_store: bool = True):
        """resume=True continues the run whose training state `<log_dir>/checkpoint/train_state.pt` holds (saved with every periodic
        checkpoint while save_ckpt is on): epoch numbering, env steps, the best result, optimiser state and random streams carry
        over; without such a file the run starts fresh and says so.  Env state is never saved: a resumed run resets its envs.
        ckpt_store: whether the transition store goes into train_state.pt."""
        assert self.policy is not None, "The policy is not initialized"
        self.policy.train()
        eng = self.policy.engine
        from fsrl_amd.env.venv import as_vector_env
        train_envs = as_vector_env(train_envs)                 # a single env: one sub-buffer (base_agent.py:160-163)
        assert eng.cfg.env_num >= len(train_envs), \
            f"agent built for {eng.cfg.env_num} env sub-buffers, got {len(train_envs)} envs (pass training_num)"
        # VectorReplayBuffer(buffer_size, len(train_envs)) of the reference (base_agent.py:279): the store is re-cut to
        # that geometry.  None = the size the agent was built with (its `buffer_size`, default 100 000 like the
        # reference's learn()); an explicit size must fit that allocation (AssertionError otherwise).
        buffer = HipVectorReplayBuffer(eng, buffer_size, len(train_envs))
        # device_actor=True: actor + noise on the MI355X (library RNG); over a worker-process env the collector then also
        # overlaps the actor with the env workers when that pays (split_phase="auto")
        from fsrl_amd.env.device import DeviceVectorEnv
        if isinstance(train_envs, DeviceVectorEnv):
            # the envs live on the GPU: a collect is a handful of launches of one looping kernel (fsrl_collect_device)
            from fsrl_amd.data.device_collector import DeviceCollector
            train_collector = DeviceCollector(self.policy, train_envs, buffer)
        else:
            train_collector = FastCollector(self.policy, train_envs, buffer, exploration_noise=True, device_actor=device_actor,
                                            split_phase="auto" if device_actor else False)
        test_collector = evaluation_collector(self.policy, test_envs)       # device test envs: store-less DeviceCollector

        def stop_fn(reward, cost):
            return reward > reward_threshold and cost < self.cost_limit

        if save_ckpt:
            self.logger.setup_checkpoint_fn(lambda: {"model": self.state_dict})
        trainer = OnpolicyTrainer(policy=self.policy, train_collector=train_collector,
                                  test_collector=test_collector, max_epoch=epoch, batch_size=batch_size,
                                  cost_limit=self.cost_limit, step_per_epoch=step_per_epoch,
                                  repeat_per_collect=repeat_per_collect, episode_per_test=testing_num,
                                  episode_per_collect=episode_per_collect, stop_fn=stop_fn,
                                  logger=self.logger, resume_from_log=resume,
                                  save_model_interval=save_interval, verbose=verbose,
                                  show_progress=show_progress)
        if save_ckpt:                            # registered late: the state is the trainer's and the policy's
            self.logger.setup_train_state_fn(lambda: trainer.train_state(with_store=ckpt_store))
        ep, stat, info = 0, {}, {}
        for ep, stat, info in trainer:
            self.logger.store(tab="train", cost_limit=self.cost_limit)
            if verbose:
                print(f"Epoch: {ep}", info)
        return ep, stat, info
