"""TrajectoryBuffer's host side (fsrl_amd/data/traj_buf.py) against fixtures recorded from the unmodified reference
(tests/golden/gen_golden_traj.py): filter_points index for index, its ValueError cases, the store() decision sequence over a
pure-Python stand-in for the fsrl_traj calls, save() / np.load, and the data package's exports.  No GPU."""
import os
import random

import numpy as np
import pytest

from traj_problems import COLUMNS, GOLDEN, FakeArchive, episodes_of, load_store_cases

FILTER = np.load(os.path.join(GOLDEN, "traj_filter_cases.npz"))
STORE = load_store_cases()


def test_data_package_exports_the_reference_surface():
    from fsrl_amd.data import BasicCollector, FastCollector, TrajectoryBuffer
    import fsrl_amd.data as data
    assert {"BasicCollector", "FastCollector", "TrajectoryBuffer"} <= set(data.__all__)
    assert issubclass(BasicCollector, FastCollector)
    tb = TrajectoryBuffer(100)                      # the reference's call: no engine yet, the archive comes with attach()
    assert tb.max_trajectory == 100 and tb.filtering_thres == 200 and len(tb) == 0 and tb.num_trajectories == 0
    assert tb.metrics.shape == (0, 2)


@pytest.mark.parametrize("name", [str(n) for n in FILTER["names"]])
def test_filter_points_equals_the_reference_index_for_index(name):
    from fsrl_amd.data.traj_buf import TrajectoryBuffer, filter_points
    pts, target, seed = FILTER[name + "/points"], int(FILTER[name + "/target"]), int(FILTER[name + "/seed"])
    random.seed(seed)
    kept = filter_points(pts, target)
    assert kept == FILTER[name + "/kept"].tolist()
    random.seed(seed)
    assert TrajectoryBuffer.filter_points(list(pts), target) == kept        # the reference's call form: a list of arrays


def test_filter_points_names_what_the_reference_would_crash_on():
    from fsrl_amd.data.traj_buf import filter_points
    pts = np.random.default_rng(0).standard_normal((20, 2))
    with pytest.raises(ValueError, match="target_size = 21"):
        filter_points(pts, 21)                      # the reference: random.choice on an empty list
    flat = pts.copy(); flat[:, 1] = 3.0
    with pytest.raises(ValueError, match="cost returns have zero spread"):
        filter_points(flat, 5)                      # the reference: division by a zero cell size
    flat = pts.copy(); flat[:, 0] = -1.0
    with pytest.raises(ValueError, match="reward returns have zero spread"):
        filter_points(flat, 5)
    with pytest.raises(ValueError, match="positive"):
        filter_points(pts, 0)
    assert sorted(filter_points(pts, 20)) == list(range(20))


def _replay(case, look_every):
    from fsrl_amd.data.traj_buf import TrajectoryBuffer
    fake = FakeArchive()
    random.seed(int(case["seed"])); np.random.seed(int(case["seed"]))
    tb = TrajectoryBuffer(archive=fake, **case["kwargs"])
    eps = episodes_of(case)
    for i, ep in enumerate(eps):
        fake.push_episode(ep)
        if look_every and (i + 1) % look_every == 0:
            tb.sync()
    return tb, fake, eps


@pytest.mark.parametrize("look_every", [1, 4, 0], ids=["every_episode", "every_4", "at_the_end"])
@pytest.mark.parametrize("name", sorted(STORE))
def test_decisions_reproduce_the_reference_store(name, look_every):
    """whether the buffer looks after every episode (the reference's store()), every few, or once at the end: the same episodes
    survive in the same order with the same metrics, because the decisions are replayed in commit order"""
    case = STORE[name]
    tb, fake, eps = _replay(case, look_every)
    surv = case["survivors"]
    assert tb.num_trajectories == len(surv) and len(tb) == int(case["transitions"])
    assert np.array_equal(tb.metrics, case["metrics"])                      # float64 sums in push order: bit for bit
    data = tb.get_all()
    assert set(data) == set(COLUMNS)
    assert np.array_equal(data["observations"][:, 0], np.concatenate([np.full(int(case["lens"][e]), e) for e in surv]))
    assert np.array_equal(data["rewards"], np.concatenate([eps[e]["rew"] for e in surv]))
    assert np.array_equal(tb.lengths, case["lens"][surv])
    if name == "grid_twice":
        assert fake.n["keeps"] >= 1
    if name == "window":
        assert fake.n["rejected_window"] == len(case["lens"]) - len(surv) > 0


def test_sample_draws_a_trajectory_then_a_transition():
    tb, fake, eps = _replay(STORE["under_capacity"], 0)
    np.random.seed(5)
    s = tb.sample(64)
    np.random.seed(5)
    traj = np.random.randint(0, tb.num_trajectories, size=64)
    rows = [int(np.random.randint(0, len(eps[t]["rew"]))) for t in traj]
    assert np.array_equal(s["observations"][:, 0], traj) and np.array_equal(s["observations"][:, 1], rows)
    assert s["actions"].shape == (64, 3) and s["terminals"].dtype == bool
    assert len(set(traj)) == tb.num_trajectories            # 64 draws over 6 trajectories: every one is hit


def test_save_round_trips_the_seven_columns(tmp_path):
    tb, _, _ = _replay(STORE["replace"], 1)
    path = tb.save(str(tmp_path / "ds"), "unit.hdf5")
    assert path == str(tmp_path / "ds" / "unit.npz") and os.path.exists(path)
    back, data = np.load(path), tb.get_all()
    assert sorted(back.files) == sorted(COLUMNS)
    for k in COLUMNS:
        assert back[k].dtype == data[k].dtype and np.array_equal(back[k], data[k]), k
    assert back["observations"].dtype == np.float32 and back["rewards"].dtype == np.float64 and back["timeouts"].dtype == bool
