"""TrajectoryBuffer.load on the host (fsrl_amd/data/traj_buf.py) over a pure-Python stand-in for the archive: what save() wrote comes
back bit for bit, an open tail is dropped, loading past max_trajectory makes the decisions the reference's store() makes on the same
episode stream (tests/golden/traj_store_cases.npz), and the numpy inverse action map the GPU tests take as their expected value is
BasePolicy.map_action_inverse.  No GPU."""
import random

import numpy as np
import pytest

from traj_problems import COLUMNS, FakeArchive, episodes_of, load_store_cases

STORE = load_store_cases()
F32 = np.float32


class ImportingFake(FakeArchive):
    """FakeArchive + TrajArchive.import_rows as include/fsrl_hip.h words fsrl_traj_import: episodes end where a flag is set, an open
    tail is dropped and counted, float64 returns in row order, the window, ids in commit order."""

    max_rows = 1 << 12

    def __init__(self):
        super().__init__()
        self.n["import_open"] = 0
        self.calls = []

    def import_rows(self, data, source=0):
        done = np.asarray(data["terminals"]).astype(bool) | np.asarray(data["timeouts"]).astype(bool)
        first, eps, rows = 0, 0, 0
        self.calls.append(len(done))
        for i in np.flatnonzero(done):
            sl = slice(first, int(i) + 1)
            before = self.n["committed"]
            ep = dict(obs=data["observations"][sl], obs_next=data["next_observations"][sl], act=data["actions"][sl],
                      rew=data["rewards"][sl], cost=data["costs"][sl], terminated=data["terminals"][sl], truncated=data["timeouts"][sl])
            self.push_episode(ep, source)
            if self.n["committed"] > before:
                self.table[-1]["data"]["actions"] = ep["act"]       # imported as recorded: the env's action, not mapped again
                eps += 1; rows += len(ep["rew"])
            first = int(i) + 1
        if first < len(done):
            self.n["import_open"] += 1
        return eps, rows


def _stream(case):
    """the case's episodes as one dataset in the export layout"""
    eps = episodes_of(case)
    cat = lambda k: np.concatenate([e[k] for e in eps])
    return eps, dict(observations=cat("obs"), next_observations=cat("obs_next"), actions=np.clip(cat("act"), -1.0, 1.0),
                     rewards=cat("rew"), costs=cat("cost"), terminals=cat("terminated"), timeouts=cat("truncated"))


def _buffer(case):
    from fsrl_amd.data.traj_buf import TrajectoryBuffer
    fake = ImportingFake()
    random.seed(int(case["seed"])); np.random.seed(int(case["seed"]))
    return TrajectoryBuffer(archive=fake, **case["kwargs"]), fake


def test_load_needs_an_archive_and_says_so():
    from fsrl_amd.data.traj_buf import TrajectoryBuffer
    with pytest.raises(RuntimeError, match="attach an engine first"):
        TrajectoryBuffer(100).load({k: np.zeros(0) for k in COLUMNS})


@pytest.mark.parametrize("how", ["npz", "dict", "hdf5_name"])
def test_load_of_save_is_get_all_bit_for_bit(tmp_path, how):
    case = STORE["under_capacity"]
    _, data = _stream(case)
    a, _ = _buffer(case)
    assert a.load(data) == len(case["lens"])
    want, met = a.get_all(), a.metrics
    path = a.save(str(tmp_path), "unit.hdf5")
    b, fake = _buffer(case)
    src = {"npz": path, "dict": want, "hdf5_name": str(tmp_path / "unit.hdf5")}[how]
    assert b.load(src, source=4) == a.num_trajectories
    got = b.get_all()
    for k in COLUMNS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), k
    assert np.array_equal(b.metrics, met) and np.array_equal(b.lengths, a.lengths)
    assert b.sources.tolist() == [4] * a.num_trajectories and a.sources.tolist() == [-1] * a.num_trajectories


def test_a_trailing_open_run_is_dropped():
    case = STORE["under_capacity"]
    eps, data = _stream(case)
    cut = {k: v[:-1] for k, v in data.items()}              # the last episode loses its end flag
    tb, fake = _buffer(case)
    assert tb.load(cut) == len(eps) - 1
    assert fake.n["import_open"] == 1
    assert len(tb) == len(data["rewards"]) - len(eps[-1]["rew"])
    assert np.array_equal(tb.get_all()["rewards"], data["rewards"][:len(tb)])


@pytest.mark.parametrize("name", sorted(STORE))
def test_loading_makes_the_decisions_of_the_reference_store(name):
    """the recorded stream as ONE dataset: the same episodes survive in the same order with the same metrics as when the reference's
    store() saw them one by one"""
    case = STORE[name]
    eps, data = _stream(case)
    tb, fake = _buffer(case)
    accepted = tb.load(data)
    surv = case["survivors"]
    assert accepted == fake.n["committed"]
    assert tb.num_trajectories == len(surv) and len(tb) == int(case["transitions"])
    assert np.array_equal(tb.metrics, case["metrics"])
    got = tb.get_all()
    assert np.array_equal(got["observations"][:, 0], np.concatenate([np.full(int(case["lens"][e]), e) for e in surv]))
    assert np.array_equal(got["rewards"], np.concatenate([eps[e]["rew"] for e in surv]))
    assert np.array_equal(tb.lengths, case["lens"][surv])
    if name == "window":
        assert fake.n["rejected_window"] == len(case["lens"]) - len(surv) > 0


def test_a_large_file_goes_in_pieces_of_whole_episodes():
    case = STORE["under_capacity"]
    eps, data = _stream(case)
    tb, fake = _buffer(case)
    fake.max_rows = 4 * max(len(e["rew"]) for e in eps)     # a quarter of it is the budget of one piece: one episode at least
    assert tb.load(data) == len(eps)
    assert len(fake.calls) > 1 and sum(fake.calls) == len(data["rewards"])
    assert np.array_equal(tb.get_all()["rewards"], data["rewards"])


class _Space:
    def __init__(self, low, high):
        self.low, self.high = np.asarray(low, F32), np.asarray(high, F32)
        self.shape = self.low.shape


@pytest.mark.parametrize("method", ["", "clip", "tanh"])
@pytest.mark.parametrize("scaling", [False, True])
def test_inverse_action_is_base_policy_map_action_inverse(method, scaling):
    from fsrl_amd.data.traj_buf import inverse_action, policy_action_map
    from fsrl_amd.policy.base_policy import BasePolicy

    class P:                                                # the attributes map_action_inverse reads, without a device
        _BOUND = BasePolicy._BOUND
        _act_range = BasePolicy._act_range
        map_action_inverse = BasePolicy.map_action_inverse
        action_space = _Space([-2.0, 0.5, 1.0, -1.0], [0.7, 3.5, 1.0, 1.0])        # a dimension with high == low
        action_scaling = scaling
        action_bound_method = method

    rng = np.random.default_rng(3)
    sp = P.action_space
    unit = rng.uniform(-0.999, 0.999, (257, 4)).astype(F32)
    act = (sp.low + (sp.high - sp.low) * (unit + F32(1.0)) / F32(2.0)).astype(F32) if scaling else unit
    code, low, high = policy_action_map(P())
    assert code == {"": 0, "clip": 1, "tanh": 2}[method] and (low is not None) == scaling
    want = np.asarray(P().map_action_inverse(act))
    got = inverse_action(act, code, low, high)
    assert got.dtype == F32 and want.dtype == F32
    if method == "tanh" and scaling:                        # the degenerate dimension rescales to -1: see the departure below
        assert np.all(np.isinf(want[:, 2])) and np.all(np.isfinite(got[:, 2]))
        got, want = np.delete(got, 2, axis=1), np.delete(want, 2, axis=1)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if method == "tanh" and not scaling:                    # the one departure: +-1 is clamped where the reference returns +-inf
        edge = inverse_action(np.array([1.0, -1.0], F32), 2)
        assert np.all(np.isfinite(edge)) and np.array_equal(edge, inverse_action(np.array([1.0, -1.0], F32) * F32(1 - 2.0 ** -24), 2))
        with np.errstate(divide="ignore"):
            assert np.all(np.isinf(P().map_action_inverse(np.array([1.0, -1.0], F32))))
