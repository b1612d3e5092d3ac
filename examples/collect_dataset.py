#!/usr/bin/env python
"""Collect an offline safe-RL dataset while training (the job of the reference's examples/customized/collect_dataset.py): train
PPO-Lagrangian on the synthetic SafetyCarCircle-shaped vector env over a few cost limits with a TrajectoryBuffer attached, keep the
finished episodes whose returns lie inside a window, thin dense regions of the (reward return, cost return) plane with the grid
filter, and save the rest in the DSRL column layout.

The buffer taps the engine's store ingest: the rows of every episode stay in HBM from the collector's push until save().

    python examples/collect_dataset.py --cost-limits 5,20,40 --epoch 2 --out /tmp/dataset
    python examples/collect_dataset.py --grouped --seeds 4 --epoch 2          # k grouped seeds feed ONE buffer (one cost limit each)
"""
import argparse
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fsrl_amd.agent import PPOLagAgent  # noqa: E402
from fsrl_amd.data import FastCollector, GroupCollector, HipVectorReplayBuffer, TrajectoryBuffer  # noqa: E402
from fsrl_amd.env import SyntheticSafetyVectorEnv  # noqa: E402
from fsrl_amd.utils import BaseLogger  # noqa: E402

EP_LEN = 300


def make(a, seed, cost_limit):
    env = SyntheticSafetyVectorEnv(env_num=a.envs, obs_dim=8, act_dim=2, episode_len=EP_LEN, seed=seed)
    logger = BaseLogger(tempfile.mkdtemp(prefix=f"fsrl_amd_ds{seed}_"), name=f"ppol-c{cost_limit:g}")
    agent = PPOLagAgent(env, logger, cost_limit=cost_limit, device=a.device, seed=seed, hidden_sizes=(a.hidden, a.hidden), training_num=a.envs)
    agent.policy.train()
    buf = HipVectorReplayBuffer(agent.policy.engine, None, a.envs)
    return agent, buf, FastCollector(agent.policy, env, buf, exploration_noise=True, device_actor=True)


def report(tag, tb):
    m = tb.metrics
    span = f"reward {m[:, 0].min():.1f} .. {m[:, 0].max():.1f}, cost {m[:, 1].min():.1f} .. {m[:, 1].max():.1f}" if len(m) else "empty"
    print(f"{tag}: {tb.num_trajectories} trajectories, {len(tb)} transitions ({span})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cost-limits", default="5,20,40", help="one training run per cost limit (--grouped: one seed per cost limit, cycled)")
    ap.add_argument("--epoch", type=int, default=2)
    ap.add_argument("--step-per-epoch", type=int, default=6000)
    ap.add_argument("--envs", type=int, default=20)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--grouped", action="store_true", help="the seeds train as one group and feed one buffer")
    ap.add_argument("--seeds", type=int, default=3, help="--grouped: members of the group")
    ap.add_argument("--max-trajectory", type=int, default=200)
    ap.add_argument("--no-grid-filter", action="store_true", help="at capacity replace a random stored trajectory instead")
    ap.add_argument("--rmin", type=float, default=-np.inf)
    ap.add_argument("--rmax", type=float, default=np.inf)
    ap.add_argument("--cmin", type=float, default=-np.inf)
    ap.add_argument("--cmax", type=float, default=np.inf)
    ap.add_argument("--out", default="", help="directory of dataset.npz (and dataset.hdf5 where h5py is installed)")
    a = ap.parse_args()
    limits = [float(x) for x in a.cost_limits.split(",")]
    tb = TrajectoryBuffer(max_trajectory=a.max_trajectory, use_grid_filter=not a.no_grid_filter, rmin=a.rmin, rmax=a.rmax, cmin=a.cmin,
                          cmax=a.cmax, max_episode_len=EP_LEN)
    if a.grouped:
        from fsrl_amd.policy import PolicyGroup
        runs = [make(a, s, limits[s % len(limits)]) for s in range(a.seeds)]
        agents, bufs, cols = [r[0] for r in runs], [r[1] for r in runs], [r[2] for r in runs]
        for col in cols:
            tb.attach(col)
        group = PolicyGroup([ag.policy for ag in agents])
        gcol = GroupCollector(group, cols)
        for ep in range(a.epoch):
            budget = a.step_per_epoch
            while budget > 0:
                for ag, st in zip(agents, gcol.collect(n_episode=a.envs)):
                    ag.policy.pre_update_fn(stats_train=st)
                budget -= st["n/st"]
                group.update(bufs, batch_size=256, repeat=4)
                for col in cols:
                    col.reset_buffer(keep_statistics=True)
            report(f"epoch {ep + 1}, {a.seeds} grouped seeds", tb)
        print("trajectories per seed:", np.bincount(tb.sources, minlength=a.seeds).tolist())
        group.close()
        engines = [ag.policy.engine for ag in agents]
    else:
        engines = []
        for seed, cl in enumerate(limits):
            agent, buf, col = make(a, seed, cl)
            tb.attach(col)
            for ep in range(a.epoch):
                budget = a.step_per_epoch
                while budget > 0:
                    st = col.collect(n_episode=a.envs)
                    budget -= st["n/st"]
                    agent.policy.pre_update_fn(stats_train=st)
                    agent.policy.update(0, buf, batch_size=256, repeat=4)
                    agent.policy.post_update_fn(stats_train=st)
                    col.reset_buffer(keep_statistics=True)
                report(f"cost limit {cl:g}, epoch {ep + 1}", tb)
            tb.detach(col)
            engines.append(agent.policy.engine)
    print("archive:", tb.counters())
    out = a.out or tempfile.mkdtemp(prefix="fsrl_amd_dataset_")
    path = tb.save(out, "dataset.hdf5")
    back = np.load(path)
    print(f"saved {path}: " + ", ".join(f"{k} {back[k].shape}" for k in back.files))
    print(f"train a replay agent from it: python examples/train_agent.py --algo sacl --prefill {path}")
    tb.close()
    for eng in engines:
        eng.close()


if __name__ == "__main__":
    main()
