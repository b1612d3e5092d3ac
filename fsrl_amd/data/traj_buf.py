"""TrajectoryBuffer: keep the finished episodes of a training run and export them as an offline dataset (DSRL column layout).

Behaviour of fsrl/data/traj_buf.py, restated: an episode is stored when its reward and cost returns lie inside the window; below
`max_trajectory` every such episode stays; at capacity either the grid filter thins the (reward return, cost return) plane whenever
`int(filter_interval * max_trajectory)` episodes have gathered, or a uniformly drawn stored episode is replaced.

What differs is where the rows are.  The reference's collector hands the buffer one transition at a time on the host.  Here the
buffer is a TAP on the engine's store ingest (fsrl_traj_*, include/fsrl_hip.h): every row any collector pushes -- solo, grouped,
over worker-process envs, inside the native collect loops -- also reaches an archive in HBM, and comes back to the host only in
get_all() / save().  load() reads a saved dataset back into the archive, and HipVectorReplayBuffer.fill_from pours archived episodes
into a replay store on the device.  Python is not in the push loop, so the keep / filter / replace decisions are made when the
buffer is next looked at (len(), metrics, get_all(), ...): the episodes committed since the last look are run through the reference's decision sequence in commit
order, which gives the reference's result because that sequence depends on nothing but the order of the accepted episodes and the
random streams (`random` for the grid filter, `np.random` for the replacement).  The archive therefore has to hold what gathers
between two looks: `max_rows` / `max_episode_len`; FastCollector-driven training looks after every collect when the buffer was
attached to the collector.

`actions` holds the action the env received, as basic_collector.py:239-247 stores `action_remap`: the library's map_action of the
pushed policy action under this buffer's `action_bound_method` and `action_space`.  With the actor on the device that is bit for
bit the env_act the collect calls hand out.  Collectors that map actions in numpy (the host-actor path) record the library's mapping
of the stored action, not numpy's.

The archive is not part of Engine.train_state(): a resumed run starts with an empty buffer (save() before stopping, load() after)."""
import numbers
import os
import random
from collections import defaultdict
from typing import Optional

import numpy as np

COLUMNS = ("observations", "next_observations", "actions", "rewards", "costs", "terminals", "timeouts")


def filter_points(points, target_size: int) -> list:
    """Indices of `target_size` of the 2-D `points`, spread over a ceil(sqrt(target_size))^2 grid: one point from every occupied
    cell (the last one that fell into it), then points drawn from cells that still have some (traj_buf.py:119-161, same cell
    arithmetic -- a point on the maximum lands in an extra cell -- and the same calls of `random` in the same order, so under one
    random.seed the indices are the reference's).  ValueError where the reference divides by zero or runs out of points."""
    points = np.array(points, dtype=np.float64).reshape(-1, 2)
    target_size = int(target_size)
    if target_size < 1:
        raise ValueError(f"filter_points: target_size must be positive, got {target_size}")
    if len(points) < target_size:
        raise ValueError(f"filter_points: {len(points)} points cannot be thinned to target_size = {target_size}")
    grid_size = int(np.ceil(np.sqrt(target_size)))
    lo, hi = points.min(axis=0), points.max(axis=0)
    for i, name in enumerate(("reward", "cost")):
        if not hi[i] > lo[i]:
            raise ValueError(f"filter_points: the {name} returns have zero spread (all {lo[i]!r}): the grid has no cell size")
    cell_size = [(hi[i] - lo[i]) / grid_size for i in range(2)]
    grid = defaultdict(list)
    for n, point in enumerate(points):
        cell = tuple(int((point[i] - lo[i]) // cell_size[i]) for i in range(2))
        grid[cell].append(n)
    kept = [idxs.pop() for idxs in grid.values()]
    non_empty = [cell for cell, idxs in grid.items() if len(idxs) > 0]
    while len(kept) < target_size:
        cell = random.choice(non_empty)
        kept.append(grid[cell].pop())
        if len(grid[cell]) == 0:
            non_empty.remove(cell)
    return kept[:target_size]


BOUND_CODES = {None: 0, "": 0, "clip": 1, "tanh": 2}
TANH_CLAMP = np.float32(1.0 - 2.0 ** -24)


def inverse_action(act, bound_method=0, low=None, high=None) -> np.ndarray:
    """BasePolicy.map_action_inverse in float32 numpy, as fsrl_store_fill applies it on the device: the recorded env action back to
    the raw policy action a replay store holds.  low / high None: no rescale.  bound_method 0 none, 1 clip, 2 tanh (or the names).
    One departure from the reference, the library's: under tanh the value is clamped to +-(1 - 2**-24) before the inverse, where
    the reference returns +-inf at +-1."""
    code = BOUND_CODES.get(bound_method, bound_method)
    a = np.asarray(act, np.float32)
    if low is not None:
        low = np.asarray(low, np.float32)
        scale = np.asarray(high, np.float32) - low
        eps = np.finfo(np.float32).eps.item()
        scale = np.where(scale < eps, scale + np.float32(eps), scale).astype(np.float32)
        a = (a - low) * np.float32(2.0) / scale - np.float32(1.0)
    if code == 2:
        a = np.clip(a, -TANH_CLAMP, TANH_CLAMP)
        a = (np.log(np.float32(1.0) + a) - np.log(np.float32(1.0) - a)) / np.float32(2.0)
    return a.astype(np.float32)


def policy_action_map(policy):
    """(bound code, low, high) of a policy's map_action: what fill_from and the archive's `actions` column are mapped with"""
    if policy is None:
        return 0, None, None
    space = getattr(policy, "action_space", None)
    if space is None:
        return 0, None, None
    scale = bool(getattr(policy, "action_scaling", False)) and hasattr(space, "low")
    return (BOUND_CODES[getattr(policy, "action_bound_method", "")], space.low if scale else None, space.high if scale else None)


def _read_dataset(x) -> dict:
    """the seven DSRL columns from a dict, an .npz, or an HDF5 file (h5py permitting)"""
    if isinstance(x, dict):
        data = x
    else:
        path = os.fspath(x)
        stem, ext = os.path.splitext(path)
        if ext.lower() != ".npz":
            try:
                import h5py
            except ImportError:
                h5py = None
            if h5py is not None and hasattr(h5py, "File"):
                with h5py.File(path, "r") as f:
                    data = {k: np.asarray(f[k]) for k in COLUMNS}
            elif os.path.exists(stem + ".npz"):
                path, data = stem + ".npz", None
            else:
                raise ImportError(f"{path}: reading HDF5 needs h5py, and there is no {stem}.npz beside it")
        else:
            data = None
        if data is None:
            with np.load(path) as f:
                data = {k: f[k] for k in COLUMNS}
    missing = [k for k in COLUMNS if k not in data]
    if missing:
        raise KeyError(f"dataset without the column(s) {missing}")
    return data


def _engine_of(x):
    """an Engine, a policy (`.engine`) or a collector (`.policy`) -> (engine, policy or None)"""
    pol = None
    if hasattr(x, "policy") and not hasattr(x, "push"):
        x = x.policy
    if hasattr(x, "engine") and not hasattr(x, "push"):
        pol, x = x, x.engine
    if x is None or not hasattr(x, "push") or not hasattr(x, "_ctx"):
        raise TypeError("TrajectoryBuffer taps an Engine's store ingest: attach an Engine, a policy that owns one, or a collector of "
                        "such a policy")
    return x, pol


class TrajectoryBuffer:
    """TrajectoryBuffer(engine_or_policy, max_trajectory=99999, ...) creates the archive at once and attaches `engine_or_policy`;
    TrajectoryBuffer(max_trajectory) -- the reference's call -- creates it at the first attach().

    max_rows / max_episode_len size the archive in HBM (defaults: 1000 rows per episode, room for the episodes the decision logic can
    hold plus what gathers between two looks, capped at 2**20 rows); an episode longer than max_episode_len is dropped and counted.
    action_space / action_bound_method: what `actions` is mapped with; default: the attached policy's own."""

    filter_points = staticmethod(filter_points)

    def __init__(self, engine_or_policy=None, max_trajectory: int = 99999, use_grid_filter: bool = True, rmin: float = -np.inf,
                 rmax: float = np.inf, cmin: float = -np.inf, cmax: float = np.inf, filter_interval: float = 2,
                 max_rows: Optional[int] = None, max_episode_len: Optional[int] = None, action_space=None,
                 action_bound_method: Optional[str] = "clip", archive=None):
        if isinstance(engine_or_policy, numbers.Integral):          # the reference's TrajectoryBuffer(max_trajectory)
            engine_or_policy, max_trajectory = None, int(engine_or_policy)
        self.max_trajectory = int(max_trajectory)
        self.rmin, self.rmax, self.cmin, self.cmax = rmin, rmax, cmin, cmax
        self.use_grid_filter = bool(use_grid_filter)
        if self.use_grid_filter:
            assert filter_interval > 1, "the filter interval should be greater than 1"
            self.filtering_thres = int(filter_interval * self.max_trajectory)
        self._max_rows, self._max_episode_len = max_rows, max_episode_len
        self._action_space, self._bound_method = action_space, action_bound_method
        self._archive = archive                 # tests: any object with the TrajArchive methods
        self._sources = {}                      # id(engine) -> (engine, source number)
        self._ids, self._rows, self._met, self._src = [], [], [], []       # the stored episodes, in the reference's list order
        self._version, self._cache = 0, None
        if self._archive is not None:
            self._archive.set_window(rmin, rmax, cmin, cmax)
        if engine_or_policy is not None:
            self.attach(engine_or_policy)

    # ------------------------------------------------------------------ the tap
    def _create(self, engine, policy):
        from fsrl_amd.engine import TrajArchive
        cap = self.filtering_thres if self.use_grid_filter else self.max_trajectory + 1
        ep_len = int(self._max_episode_len or 1000)
        max_episodes = cap + max(1024, 4 * engine.cfg.env_num)
        max_rows = int(self._max_rows or min(max_episodes * ep_len, 1 << 20))
        space = self._action_space if self._action_space is not None else getattr(policy, "action_space", None)
        method = self._bound_method
        if self._action_space is None and policy is not None:
            method = getattr(policy, "action_bound_method", method)
        scale = space is not None and getattr(policy, "action_scaling", True) and hasattr(space, "low")
        self._archive = TrajArchive(engine, max_rows, max_episodes, ep_len, {None: 0, "": 0, "clip": 1, "tanh": 2}[method],
                                    low=space.low if scale else None, high=space.high if scale else None)
        self._archive.set_window(self.rmin, self.rmax, self.cmin, self.cmax)

    def attach(self, x) -> int:
        """Tap the engine of `x` (an Engine, a policy, a collector).  -> the source number its episodes carry.  A policy or a
        collector also gets the buffer as `traj_buffer`: FastCollector (every collector over that policy that stores rows, the
        ones agent.learn() builds included) then has the decisions made after every collect and the open episodes of envs it
        resets in mid-episode discarded.  An Engine is tapped and nothing else."""
        engine, policy = _engine_of(x)
        if id(engine) in self._sources:
            return self._sources[id(engine)][1]
        if self._archive is None:
            self._create(engine, policy)
        src = self._archive.attach(engine)
        self._sources[id(engine)] = (engine, src)
        if not hasattr(x, "_ctx"):
            x.traj_buffer = self
        return src

    def detach(self, x) -> None:
        engine, _ = _engine_of(x)
        if self._sources.pop(id(engine), None) is not None and engine._ctx:
            self._archive.detach(engine)
        if getattr(x, "traj_buffer", None) is self:
            x.traj_buffer = None

    def abandon(self, x) -> None:
        """The envs behind `x` were reset in mid-episode (a collector's reset_env): their open episodes are no trajectories."""
        engine, _ = _engine_of(x)
        if id(engine) in self._sources and engine._ctx:
            self._archive.abandon(engine)

    def close(self) -> None:
        if self._archive is not None and hasattr(self._archive, "close"):
            self._archive.close()
        self._sources = {}

    # ------------------------------------------------------------------ decisions (traj_buf.py:60-95, per committed episode)
    def sync(self) -> None:
        """Run the episodes committed since the last look through the reference's store() decisions, in commit order."""
        a = self._archive
        if a is None:
            return
        a.flush()
        ids, rows, rew, cost, src = a.episodes()
        known = len(self._ids)
        assert list(ids[:known]) == self._ids, "the archive's table changed behind the buffer"
        if len(ids) == known:
            return
        changed = False
        for j in range(known, len(ids)):
            item = (int(ids[j]), int(rows[j]), np.array([rew[j], cost[j]]), int(src[j]))
            if len(self._ids) < self.max_trajectory:
                self._append(item)
            elif self.use_grid_filter:
                self._append(item)
                if len(self._ids) >= self.filtering_thres:
                    kept = set(filter_points(self._met, self.max_trajectory))
                    order = [i for i in range(len(self._ids)) if i in kept]         # apply_grid_filter: survivors keep their order
                    for name in ("_ids", "_rows", "_met", "_src"):
                        setattr(self, name, [getattr(self, name)[i] for i in order])
                    changed = True
            else:
                i = int(np.random.randint(0, len(self._ids)))
                self._ids[i], self._rows[i], self._met[i], self._src[i] = item
                changed = True
        if changed:
            a.keep(self._ids)
        self._version += 1

    def _append(self, item):
        for lst, v in zip((self._ids, self._rows, self._met, self._src), item):
            lst.append(v)

    # ------------------------------------------------------------------ the reference's surface
    @property
    def metrics(self) -> np.ndarray:
        """(episodes, 2) float64: reward return, cost return of every stored episode"""
        self.sync()
        return np.array(self._met, np.float64).reshape(-1, 2)

    @property
    def num_trajectories(self) -> int:
        self.sync()
        return len(self._ids)

    @property
    def lengths(self) -> np.ndarray:
        self.sync()
        return np.array(self._rows, np.int64)

    @property
    def sources(self) -> np.ndarray:
        """which attached engine (attach()'s return value) every stored episode came from"""
        self.sync()
        return np.array(self._src, np.int64)

    def __len__(self) -> int:
        """stored transitions, as the reference counts"""
        self.sync()
        return int(sum(self._rows))

    def get_all(self) -> dict:
        """The seven DSRL columns of every stored episode, episodes in stored order, rows chronological inside an episode."""
        self.sync()
        if self._cache is None or self._cache[0] != self._version:
            if self._archive is None:
                data = dict(observations=np.zeros((0, 0), np.float32), next_observations=np.zeros((0, 0), np.float32),
                            actions=np.zeros((0, 0), np.float32), rewards=np.zeros(0), costs=np.zeros(0),
                            terminals=np.zeros(0, bool), timeouts=np.zeros(0, bool))
            else:
                data = self._archive.export()
            self._cache = (self._version, data)
        return dict(self._cache[1])

    def sample(self, batch_size: int) -> dict:
        """batch_size transitions: a uniform stored trajectory, then a uniform transition of it (np.random, on the host, in the
        reference's call order); the rows come through the export path."""
        data = self.get_all()
        n = len(self._ids)
        if n == 0:
            raise ValueError("sample() from an empty TrajectoryBuffer")
        starts = np.concatenate([[0], np.cumsum(self._rows)[:-1]])
        traj = np.random.randint(0, n, size=batch_size)
        at = np.array([starts[t] + np.random.randint(0, self._rows[t]) for t in traj], np.int64)
        return {k: v[at] for k, v in data.items()}

    def save(self, log_dir: str, dataset_name: str = "dataset.hdf5") -> str:
        """Writes <log_dir>/<stem of dataset_name>.npz always, and <log_dir>/<dataset_name> as HDF5 with the reference's keys
        (one gzip-compressed dataset per column) when h5py imports.  h5py is not among this project's test dependencies: the HDF5
        branch is untested.  -> the path of the .npz"""
        os.makedirs(log_dir, exist_ok=True)
        data = self.get_all()
        npz = os.path.join(log_dir, os.path.splitext(dataset_name)[0] + ".npz")
        np.savez_compressed(npz, **data)
        try:
            import h5py
        except ImportError:
            h5py = None
        if h5py is not None and hasattr(h5py, "File"):
            h5 = dataset_name if os.path.splitext(dataset_name)[1] else dataset_name + ".hdf5"
            with h5py.File(os.path.join(log_dir, h5), "w") as f:
                for k, v in data.items():
                    f.create_dataset(k, data=v, compression="gzip")
        return npz

    def load(self, path_or_dict, source: Optional[int] = None) -> int:
        """Read a dataset back into the archive: a `.npz` written by save(), the dict get_all() returns, or an HDF5 file with the
        reference's keys where h5py imports (h5py is not among this project's test dependencies: the HDF5 branch is untested; a
        `.hdf5` path without h5py falls back to the `.npz` of the same stem, which save() always writes).  -> the number of
        episodes the archive accepted.

        An episode ends at every row where terminals | timeouts is set; a trailing run without an end flag is an open episode and
        is dropped.  Every episode is committed as a collected one is -- float64 returns summed in row order, this buffer's reward /
        cost window, max_episode_len -- and then passes through the same decisions in file order (capacity, grid filter, random
        replacement): loading is the reference's store() applied episode by episode.  `source`: the number the loaded episodes
        carry in `sources` (default -1: no attached engine).  The archive lives on an engine's device, so one must be attached
        first.  The file goes in pieces of whole episodes with a look between them, so that a dataset larger than what the archive
        holds between two looks still loads when the decisions thin it."""
        if self._archive is None:
            raise RuntimeError("TrajectoryBuffer.load: attach an engine first (attach(engine_or_policy), or pass one to the "
                               "constructor): the archive lives on its device")
        data = _read_dataset(path_or_dict)
        src = -1 if source is None else int(source)
        self.sync()
        ends = np.flatnonzero(np.asarray(data["terminals"]).astype(bool) | np.asarray(data["timeouts"]).astype(bool)) + 1
        n = len(data["rewards"])
        accepted, at = 0, 0
        budget = max(1, int(getattr(self._archive, "max_rows", 1 << 16)) // 4)
        while at < n:
            # as many whole episodes as fit the budget, at least one; the open tail goes with the last piece
            k = int(np.searchsorted(ends, at + budget, side="right"))       # episode ends inside the budget
            if k == 0 or ends[k - 1] <= at:
                k = int(np.searchsorted(ends, at, side="right")) + 1        # none: the next episode alone
            stop = n if k >= len(ends) else int(ends[k - 1])
            piece = {c: np.asarray(data[c])[at:stop] for c in COLUMNS}
            try:
                accepted += self._archive.import_rows(piece, src)[0]
            except MemoryError:
                accepted += getattr(self._archive, "last_import", (0, 0))[0]
                self.sync()
                raise
            self.sync()
            at = stop
        return accepted

    def clear(self) -> None:
        if self._archive is not None:
            self._archive.clear()
        self._ids, self._rows, self._met, self._src = [], [], [], []
        self._version += 1

    def counters(self) -> dict:
        """the archive's counters (committed, rejected_window, dropped_long, compactions, rows, refused_full, episodes, launches,
        h2d_bytes, abandoned) as of now"""
        self.sync()
        return self._archive.counters() if self._archive is not None else {}
