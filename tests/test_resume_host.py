"""learn(resume=True) above the engine, without a GPU: the trainer's counters, the policy's training-state dict, the logger's
train_state.pt and progress.txt -- over a fake engine whose whole "training state" is a counter and a blob of bytes."""
import os
import random

import numpy as np
import pytest
import torch
from torch import nn

from fsrl_amd.policy.base_policy import BasePolicy
from fsrl_amd.trainer import OnpolicyTrainer
from fsrl_amd.utils.logger import BaseLogger, DummyLogger


class FakeEngine:
    def __init__(self):
        self.updates, self.lrs, self.loaded = 0, {}, None

    def train_state(self, with_store=True):
        return b"STATE" + bytes([self.updates % 256, int(with_store)]) + self.flat.tobytes()

    def load_train_state(self, blob):
        blob = bytes(np.asarray(blob, np.uint8).tobytes())
        assert blob[:5] == b"STATE"
        self.updates, self.loaded, self.flat = blob[5], blob, np.frombuffer(blob[7:], np.float32).copy()

    def get_params(self):
        return self.flat.copy()

    def set_lr(self, group, lr):
        self.lrs[group] = lr


class FakePolicy(BasePolicy):
    def __init__(self, logger=None, seed=0):
        torch.manual_seed(seed)
        actor, critic = nn.Linear(2, 2), nn.Linear(2, 1)
        self_optim = torch.optim.Adam(actor.parameters(), lr=1e-2)
        sched = torch.optim.lr_scheduler.StepLR(self_optim, step_size=1, gamma=0.5)
        super().__init__(actor, critic, logger=logger, lr_scheduler=sched)
        self.optim = self_optim
        self.engine = FakeEngine()
        self.engine.flat = self._flat_params(fresh=False)
        self.lag = 0.0

    def get_extra_state(self):
        return [{"lag": self.lag}]

    def set_extra_state(self, state):
        self.lag = state[0]["lag"]

    def learn(self, batch, **kwargs):
        return {}

    def update(self, sample_size, buffer, **kwargs):
        self.engine.updates += 1
        self.gradient_steps += 3
        self.lag += 0.25
        self.optim.step()
        self._step_lr_scheduler()
        self.logger.store(**{"loss/total": 1.0 / self.engine.updates})
        return {}


class FakeCollector:
    buffer = None

    def __init__(self, policy):              # the reward follows the policy's progress, which a resumed run continues
        self.collect_step, self.collect_time, self.policy = 0, 0.0, policy

    def reset_stat(self):
        self.collect_step, self.collect_time = 0, 0.0

    def reset_buffer(self, keep_statistics=False):
        pass

    def collect(self, n_episode):
        self.collect_step += 10
        self.collect_time += 1e-3
        return {"n/ep": n_episode, "n/st": 10, "rew": float(self.policy.engine.updates + 1), "len": 5.0, "total_cost": 2.0, "cost": 2.0 / n_episode}


class Logger(BaseLogger):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.printed = []

    def print(self, msg, color="green"):
        self.printed.append(msg)


def _run(log_dir, epochs, resume, seed=0, save_interval=1):
    logger = Logger(str(log_dir), name="run")
    policy = FakePolicy(logger, seed=seed)
    logger.setup_checkpoint_fn(lambda: {"model": policy.state_dict()})
    trainer = OnpolicyTrainer(policy, FakeCollector(policy), max_epoch=epochs, step_per_epoch=20, repeat_per_collect=1,
                              episode_per_collect=2, logger=logger, resume_from_log=resume, save_model_interval=save_interval,
                              verbose=False)
    logger.setup_train_state_fn(trainer.train_state)
    out = [(ep, dict(info)) for ep, _, info in trainer]
    return trainer, policy, logger, out


def test_trainer_state_round_trips(tmp_path):
    trainer, policy, _, out = _run(tmp_path, 2, False)
    sd = trainer.state_dict()
    assert sd["epoch"] == 2 and sd["env_step"] == 40 and sd["cum_episode"] == 8 and sd["cum_cost"] == 8.0
    assert sd["best_reward"] == trainer.best_perf_rew and np.isfinite(sd["best_reward"])
    pol = FakePolicy()
    other = OnpolicyTrainer(pol, FakeCollector(pol), max_epoch=5, step_per_epoch=20, repeat_per_collect=1, verbose=False)
    other.load_state_dict(sd)
    assert other.state_dict() == sd
    other.reset()                                                        # reset() keeps the loaded counters
    assert (other.epoch, other.env_step, other.cum_episode) == (2, 40, 8)


def test_policy_train_state_dict_round_trips():
    a = FakePolicy(seed=1)
    for _ in range(3):
        a.update(0, None)
    np.random.seed(5); random.seed(6); torch.manual_seed(7)
    d = a.train_state_dict(with_store=False)
    assert d["engine"].dtype == torch.uint8 and bytes(d["engine"].numpy().tobytes()) == a.engine.train_state(False)
    assert d["gradient_steps"] == 9 and d["extra_state"] == [{"lag": 0.75}] and "lr_scheduler" in d
    want = (np.random.rand(), random.random(), float(torch.rand(1)))
    b = FakePolicy(seed=2)
    b.load_train_state_dict(d)
    assert (np.random.rand(), random.random(), float(torch.rand(1))) == want          # the generators continue where they were saved
    assert b.gradient_steps == 9 and b.lag == 0.75 and b.engine.updates == 3 and b._stale
    assert b.engine.lrs == {0: pytest.approx(1e-2 * 0.5 ** 3)}                        # the schedule's rate went to the engine
    assert b.lr_scheduler.state_dict() == a.lr_scheduler.state_dict()


def test_resume_without_a_file_starts_fresh_with_a_notice(tmp_path):
    trainer, _, logger, out = _run(tmp_path, 2, True)
    assert [ep for ep, _ in out] == [1, 2]
    assert any("no saved training state" in m for m in logger.printed), logger.printed
    assert trainer.env_step == 40
    pol = FakePolicy()
    quiet = OnpolicyTrainer(pol, FakeCollector(pol), max_epoch=1, step_per_epoch=20, repeat_per_collect=1,
                            logger=DummyLogger(), resume_from_log=True, verbose=False)
    assert [ep for ep, _, _ in quiet] == [1]                              # the dummy logger has nothing to resume from


def test_resume_continues_epochs_steps_best_and_progress_table(tmp_path):
    first, pol1, _, out1 = _run(tmp_path, 2, False)
    assert [ep for ep, _ in out1] == [1, 2]
    path = os.path.join(str(tmp_path), "run", "checkpoint", "train_state.pt")
    assert os.path.exists(path) and not os.path.exists(path + ".tmp")
    second, pol2, logger, out2 = _run(tmp_path, 4, True, seed=9)
    assert [ep for ep, _ in out2] == [3, 4]
    assert any("continuing after epoch 2" in m for m in logger.printed), logger.printed
    assert second.env_step == 80 and second.cum_episode == 16 and second.cum_cost == 16.0
    assert pol2.engine.loaded == pol1.engine.train_state(True)             # the engine got the saved blob, byte for byte
    for k, v in pol1.state_dict().items():                                 # the host mirror follows the loaded parameters (seed 9 built others)
        assert not torch.is_tensor(v) or torch.equal(pol2.state_dict()[k], v), k
    assert pol2.engine.updates == 8 and pol2.gradient_steps == 24 and pol2.lag == 2.0
    assert out2[0][1]["best_reward"] >= first.best_perf_rew
    lines = open(os.path.join(str(tmp_path), "run", "progress.txt")).read().splitlines()
    assert sum(ln.startswith("Steps\t") for ln in lines) == 1 and lines[0].startswith("Steps\t")
    steps = [int(ln.split("\t")[0]) for ln in lines[1:]]
    assert steps == [20, 40, 60, 80]
    # an uninterrupted run of four epochs writes the same counters
    whole, pol3, _, out3 = _run(tmp_path / "whole", 4, False)
    assert whole.state_dict() == second.state_dict() and pol3.engine.updates == pol2.engine.updates
    assert pol3.lr_scheduler.state_dict() == pol2.lr_scheduler.state_dict()


def test_train_state_follows_the_checkpoint_cadence(tmp_path):
    _run(tmp_path, 3, False, save_interval=2)
    state = torch.load(os.path.join(str(tmp_path), "run", "checkpoint", "train_state.pt"), weights_only=False)
    assert state["trainer"]["epoch"] == 2                                 # saved with model.pt at epoch 2, not for `best` at epoch 3
    assert not os.path.exists(os.path.join(str(tmp_path), "run", "checkpoint", "train_state_best.pt"))


def test_state_file_is_replaced_atomically(tmp_path):
    logger = Logger(str(tmp_path), name="run")
    logger.setup_train_state_fn(lambda: {"n": 1})
    logger.save_train_state()
    path = logger.train_state_path
    before = open(path, "rb").read()

    class Unpicklable:
        def __reduce__(self):
            raise RuntimeError("cannot be written")

    logger.setup_train_state_fn(lambda: {"n": 2, "bad": Unpicklable()})    # fails INSIDE torch.save, after the file was opened
    with pytest.raises(RuntimeError):
        logger.save_train_state()
    assert open(path, "rb").read() == before and os.listdir(os.path.dirname(path)) == ["train_state.pt"]
    assert logger.load_train_state() == {"n": 1}

    def boom():
        raise ValueError("no state")
    logger.setup_train_state_fn(boom)
    with pytest.raises(ValueError):
        logger.save_train_state()
    assert open(path, "rb").read() == before


def test_model_checkpoint_holds_what_it_held(tmp_path):
    _, policy, _, _ = _run(tmp_path, 1, False)
    ckpt = torch.load(os.path.join(str(tmp_path), "run", "checkpoint", "model.pt"), weights_only=False)
    assert list(ckpt) == ["model"]
    want = policy.state_dict()
    assert list(ckpt["model"]) == list(want)
    for k, v in want.items():
        assert torch.equal(ckpt["model"][k], v) if torch.is_tensor(v) else ckpt["model"][k] == v
