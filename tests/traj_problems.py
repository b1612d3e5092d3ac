"""Shared by tests/test_traj_host.py and tests/test_gpu_traj.py: the recorded TrajectoryBuffer.store streams of
tests/golden/traj_store_cases.npz as transitions, and a pure-Python stand-in for the fsrl_traj_* calls (the methods of
fsrl_amd.engine.TrajArchive) that keeps its rows in numpy arrays."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
COLUMNS = ("observations", "next_observations", "actions", "rewards", "costs", "terminals", "timeouts")


def load_store_cases():
    z = np.load(os.path.join(GOLDEN, "traj_store_cases.npz"))
    cases = {}
    for name in z["names"]:
        c = {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")}
        c["kwargs"] = {k[3:]: (float(v) if k[3:] in ("rmin", "rmax", "cmin", "cmax", "filter_interval") else int(v))
                       for k, v in c.items() if k.startswith("kw_")}
        if "use_grid_filter" in c["kwargs"]:
            c["kwargs"]["use_grid_filter"] = bool(c["kwargs"]["use_grid_filter"])
        cases[str(name)] = c
    return cases


def episodes_of(case, obs_dim=5, act_dim=3):
    """The case's stream as a list of episodes: dict of the pushed columns, [rows, ...] each.  observations[:, 0] is the episode
    number, [:, 1] the step; the rest, and the (policy) actions, come from the case's seed."""
    rng = np.random.default_rng(int(case["seed"]) + 77)
    out, at = [], 0
    for ep, n in enumerate(case["lens"]):
        n = int(n)
        obs = rng.standard_normal((n + 1, obs_dim)).astype(np.float32)
        obs[:, 0] = ep; obs[:, 1] = np.arange(n + 1)
        term, trunc = np.zeros(n, bool), np.zeros(n, bool)
        term[-1], trunc[-1] = ep % 2 == 0, ep % 2 == 1
        out.append(dict(obs=obs[:-1], obs_next=obs[1:], act=(1.5 * rng.standard_normal((n, act_dim))).astype(np.float32),
                        rew=case["rews"][at:at + n].astype(np.float64), cost=case["costs"][at:at + n].astype(np.float64),
                        terminated=term, truncated=trunc))
        at += n
    return out


class FakeArchive:
    """fsrl_amd.engine.TrajArchive without a device: same methods, same id / table-order rules (include/fsrl_hip.h)."""

    def __init__(self):
        self.window = (-np.inf, np.inf, -np.inf, np.inf)
        self.table = []             # dicts: id, rows, rew, cost, source, data
        self.next_id = 0
        self.n = dict(committed=0, rejected_window=0, keeps=0)

    def set_window(self, rmin, rmax, cmin, cmax):
        self.window = (rmin, rmax, cmin, cmax)

    def push_episode(self, ep, source=0):
        rew = cost = 0.0
        for r, c in zip(ep["rew"], ep["cost"]):
            rew += float(r); cost += float(c)
        rmin, rmax, cmin, cmax = self.window
        if rew > rmax or rew < rmin or cost > cmax or cost < cmin:
            self.n["rejected_window"] += 1
            return
        data = dict(observations=ep["obs"], next_observations=ep["obs_next"], actions=np.clip(ep["act"], -1.0, 1.0),
                    rewards=ep["rew"], costs=ep["cost"], terminals=ep["terminated"], timeouts=ep["truncated"])
        self.table.append(dict(id=self.next_id, rows=len(ep["rew"]), rew=rew, cost=cost, source=source, data=data))
        self.next_id += 1
        self.n["committed"] += 1

    def flush(self):
        pass

    def episodes(self):
        t = self.table
        return (np.array([e["id"] for e in t], np.int32), np.array([e["rows"] for e in t], np.int32),
                np.array([e["rew"] for e in t], np.float64), np.array([e["cost"] for e in t], np.float64),
                np.array([e["source"] for e in t], np.int32))

    def keep(self, ids):
        by_id = {e["id"]: e for e in self.table}
        assert len(set(int(i) for i in ids)) == len(ids)
        self.table = [by_id[int(i)] for i in ids]
        self.n["keeps"] += 1

    def export(self):
        if not self.table:
            return {k: np.zeros(0) for k in COLUMNS}
        return {k: np.concatenate([e["data"][k] for e in self.table]) for k in COLUMNS}

    def clear(self):
        self.table = []

    def counters(self):
        return dict(self.n, episodes=len(self.table), rows=sum(e["rows"] for e in self.table))
