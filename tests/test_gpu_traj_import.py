"""fsrl_traj_import on the device (fsrl_amd/csrc/host_traj.inc, the bookkeeping in traj_plan.hpp): host columns in the export layout
are committed as tapped episodes are -- import then export is the accepted episodes bit for bit, with the float64 returns, ids and
sources of the episode table; episodes outside the window or longer than max_episode_len are counted and absent; an archive without
room reports it and keeps what it had; imported and tapped episodes share one archive in commit order; TrajectoryBuffer.load on top.

Episodes of 1 .. 300 rows at (obs, act) = (5, 1), (8, 2), (33, 8)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
COLUMNS = ("observations", "next_observations", "actions", "rewards", "costs", "terminals", "timeouts")
LENS = [1, 300, 17, 128, 129, 2, 1, 64, 255]


def engine(Do, Da, env_num=2):
    from fsrl_amd.engine import Engine, EngineConfig
    eng = Engine(EngineConfig(obs_dim=Do, act_dim=Da, hidden_sizes=(64, 64), env_num=env_num, buffer_size=env_num * 64, target_kl=None,
                              max_grad_norm=0.5))
    eng.set_params((0.1 * np.random.default_rng(0).standard_normal(eng.n_params)).astype(F32))
    return eng


def dataset(Do, Da, lens, seed, open_tail=0):
    """episodes of the given lengths (odd ones end in a timeout, every sixth in both flags), then `open_tail` rows without an end"""
    rng = np.random.default_rng(seed)
    n = int(sum(lens)) + open_tail
    term, tout = np.zeros(n, bool), np.zeros(n, bool)
    for j, e in enumerate(np.cumsum(lens) - 1):
        term[e], tout[e] = j % 2 == 0, j % 2 == 1 or j % 6 == 0
    return dict(observations=rng.standard_normal((n, Do)).astype(F32), next_observations=rng.standard_normal((n, Do)).astype(F32),
                actions=rng.uniform(-3, 3, (n, Da)).astype(F32), rewards=rng.normal(0.5, 1.0, n), costs=(rng.random(n) < 0.3).astype(F64),
                terminals=term, timeouts=tout)


def slices(lens):
    at = np.concatenate([[0], np.cumsum(lens)])
    return [slice(int(a), int(b)) for a, b in zip(at[:-1], at[1:])]


def returns(data, sl):
    """float64 sums in row order, as `current_rew += rew.item()` makes them"""
    rew = cost = 0.0
    for r, c in zip(data["rewards"][sl], data["costs"][sl]):
        rew += float(r); cost += float(c)
    return rew, cost


def assert_holds(arch, data, kept, ids=None, sources=None):
    """the archive holds exactly the episodes `kept` (slices of `data`), in that order, bit for bit"""
    got_ids, rows, rew, cost, src = arch.episodes()
    assert rows.tolist() == [s.stop - s.start for s in kept]
    want = [returns(data, s) for s in kept]
    assert np.array_equal(rew, np.array([w[0] for w in want], F64)) and np.array_equal(cost, np.array([w[1] for w in want], F64))
    if ids is not None:
        assert got_ids.tolist() == list(ids)
    if sources is not None:
        assert src.tolist() == list(sources)
    out = arch.export()
    for k in COLUMNS:
        w = np.concatenate([data[k][s] for s in kept]) if kept else data[k][:0]
        assert out[k].dtype == w.dtype and out[k].shape == w.shape, k
        assert np.array_equal(np.ascontiguousarray(out[k]).view(np.uint8), np.ascontiguousarray(w).view(np.uint8)), k


@pytest.mark.parametrize("Do,Da", [(5, 1), (8, 2), (33, 8)])
def test_import_then_export_is_the_dataset_bit_for_bit(Do, Da):
    from fsrl_amd.engine import TrajArchive
    eng = engine(Do, Da)
    data = dataset(Do, Da, LENS, seed=Do, open_tail=9)
    arch = TrajArchive(eng, 2048, 64, 300)
    assert arch.import_rows(data, source=3) == (len(LENS), sum(LENS))       # the nine open rows are dropped, and counted
    c = arch.counters()
    assert c["import_open"] == 1 and c["committed"] == len(LENS) and c["rows"] == sum(LENS) and c["launches"] == 0
    assert_holds(arch, data, slices(LENS), ids=range(len(LENS)), sources=[3] * len(LENS))
    # a second import appends: ids go on, the first one's rows are untouched
    more = dataset(Do, Da, [5, 40], seed=77)
    assert arch.import_rows(more, source=4) == (2, 45)
    both = {k: np.concatenate([data[k][:sum(LENS)], more[k]]) for k in COLUMNS}
    assert_holds(arch, both, slices(LENS + [5, 40]), ids=range(len(LENS) + 2), sources=[3] * len(LENS) + [4, 4])
    arch.close(); eng.close()


def test_episodes_outside_the_window_or_too_long_are_counted_and_absent():
    from fsrl_amd.engine import TrajArchive
    eng = engine(8, 2)
    lens = [10, 301, 20, 30, 300, 15, 25]
    data = dataset(8, 2, lens, seed=5)
    sl = slices(lens)
    ret = [returns(data, s) for s in sl]
    rmin = sorted(r for r, _ in ret)[2]                     # the two lowest reward returns fall out of the window
    arch = TrajArchive(eng, 2048, 64, 300)
    arch.set_window(rmin, np.inf, -np.inf, np.inf)
    long = [i for i, n in enumerate(lens) if n > 300]
    out = [i for i in range(len(lens)) if i not in long and ret[i][0] < rmin]
    kept = [i for i in range(len(lens)) if i not in long and i not in out]
    assert long == [1] and len(out) >= 1
    assert arch.import_rows(data) == (len(kept), sum(lens[i] for i in kept))
    c = arch.counters()
    assert (c["dropped_long"], c["rejected_window"], c["committed"]) == (1, len(out), len(kept))
    assert_holds(arch, data, [sl[i] for i in kept], ids=range(len(kept)))
    arch.close(); eng.close()


def test_an_archive_that_is_too_small_says_so_and_keeps_what_it_has():
    from fsrl_amd.engine import TrajArchive
    eng = engine(8, 2)
    lens = [40, 30, 50, 20, 8]
    data = dataset(8, 2, lens, seed=6)
    sl = slices(lens)
    arch = TrajArchive(eng, 100, 64, 64)
    with pytest.raises(MemoryError, match="max_rows = 100"):
        arch.import_rows(data)
    # 40 + 30 fit, 50 does not (dropped, counted), 20 fits, 8 fits: 98 rows
    assert arch.last_import == (4, 98)
    c = arch.counters()
    assert (c["refused_full"], c["committed"], c["rows"]) == (1, 4, 98)
    assert_holds(arch, data, [sl[0], sl[1], sl[3], sl[4]], ids=[0, 1, 2, 3])
    # dead rows (replace() leaves them where they are) are reclaimed by a compaction in the MIDDLE of the next import: the 2-row
    # episode still fits behind the tail and is sent first, the 30-row one needs the compaction
    arch.replace(0)                                         # the newest episode (id 3) takes the place of id 0
    more = dataset(8, 2, [2, 30], seed=8)
    c0 = arch.counters()["compactions"]
    assert arch.import_rows(more) == (2, 32)
    assert arch.counters()["compactions"] == c0 + 1
    both = {k: np.concatenate([data[k], more[k]]) for k in COLUMNS}
    at = sum(lens)
    assert_holds(arch, both, [sl[4], sl[1], sl[3], slice(at, at + 2), slice(at + 2, at + 32)], ids=[3, 1, 2, 4, 5])
    arch.close(); eng.close()


def test_imported_and_tapped_episodes_interleave_in_one_archive():
    from fsrl_amd.engine import TrajArchive
    Do, Da = 8, 2
    eng = engine(Do, Da)
    arch = TrajArchive(eng, 1024, 64, 64, 0)                # bound none: the archive's action is the pushed one
    assert arch.attach(eng) == 0
    rng = np.random.default_rng(1)
    pushed = {k: [] for k in COLUMNS}

    def tapped_episode(env, n):
        for t in range(n):
            row = dict(observations=rng.standard_normal(Do).astype(F32), next_observations=rng.standard_normal(Do).astype(F32),
                       actions=rng.standard_normal(Da).astype(F32), rewards=float(rng.normal()), costs=float(rng.random() < 0.3),
                       terminals=t == n - 1, timeouts=False)
            eng.push([env], row["observations"], row["actions"], [row["rewards"]], [row["costs"]], [row["terminals"]], [False],
                     row["next_observations"])
            for k in COLUMNS:
                pushed[k].append(row[k])

    first, second = dataset(Do, Da, [7, 33], seed=2), dataset(Do, Da, [12], seed=3)
    tapped_episode(0, 9)
    arch.flush()
    assert arch.import_rows(first, source=8) == (2, 40)
    tapped_episode(1, 21)
    arch.flush()
    assert arch.import_rows(second, source=9) == (1, 12)
    tap = {k: np.array(v, dtype=first[k].dtype) for k, v in pushed.items()}
    everything = {k: np.concatenate([tap[k][:9], first[k], tap[k][9:], second[k]]) for k in COLUMNS}
    assert_holds(arch, everything, slices([9, 7, 33, 21, 12]), ids=range(5), sources=[0, 8, 8, 0, 9])
    arch.close(); eng.close()


def test_trajectory_buffer_load_of_save_on_the_device(tmp_path):
    """TrajectoryBuffer.load over the real archive: what save() wrote comes back as get_all(), metrics included, and a buffer at
    capacity thins a loaded file by its own decisions"""
    import random
    from fsrl_amd.data import TrajectoryBuffer
    eng = engine(8, 2)
    data = dataset(8, 2, LENS, seed=12, open_tail=4)
    a = TrajectoryBuffer(eng, max_trajectory=64, max_rows=2048, max_episode_len=300)
    assert a.load(data, source=2) == len(LENS)
    path = a.save(str(tmp_path), "d.hdf5")
    want, met = a.get_all(), a.metrics
    assert np.array_equal(met, np.array([returns(data, s) for s in slices(LENS)]))
    b = TrajectoryBuffer(max_trajectory=64, max_rows=2048, max_episode_len=300)
    with pytest.raises(RuntimeError, match="attach an engine first"):
        b.load(path)
    a.detach(eng)                                           # a context has one tap at a time
    b = TrajectoryBuffer(eng, max_trajectory=64, max_rows=2048, max_episode_len=300)
    assert b.load(path) == len(LENS)
    got = b.get_all()
    for k in COLUMNS:
        assert got[k].dtype == want[k].dtype and np.array_equal(np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8)), k
    assert np.array_equal(b.metrics, met) and b.lengths.tolist() == LENS
    # at capacity without the grid filter: every further episode replaces a uniformly drawn one (np.random), as store() does
    random.seed(0); np.random.seed(0)
    small = TrajectoryBuffer(max_trajectory=4, use_grid_filter=False, max_rows=2048, max_episode_len=300, archive=None)
    b.detach(eng)
    small.attach(eng)
    assert small.load(path) == len(LENS) and small.num_trajectories == 4 and len(small.get_all()["rewards"]) == len(small)
    np.random.seed(0)
    held = list(range(4))
    for j in range(4, len(LENS)):
        held[int(np.random.randint(0, 4))] = j
    assert small.lengths.tolist() == [LENS[j] for j in held]
    a.close(); b.close(); small.close(); eng.close()
