"""fsrl_store_fill on the device (fsrl_amd/csrc/host_traj.inc, store_fill_plan.hpp, store_fill_kernel): pouring archived episodes into
a context's store is, bit for bit, the loop of fsrl_store_push calls the header defines it by -- store columns, sizes, sample order
and the books (shown by one further push per sub-buffer) -- over wrapped, part-filled and unflushed stores; the tanh inverse stays
within 4x the float32 reference formula's own error and is finite at +-1; a replay agent trained on a filled store and on a pushed one
cannot tell them apart; every refusal names its field and leaves the store as it was; the Python surface on top.

Shapes: episodes of 1 .. 300 rows at (obs, act) = (5, 1), (8, 2), (33, 8); stores of 1 .. 4 sub-buffers of 64 .. 512 rows."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(5, 1), (8, 2), (33, 8)]
LENS = [1, 128, 37, 129, 300, 2, 64]            # 1, exactly one job, one job + 1, several jobs


# ---------------------------------------------------------------- data
def box(Da):
    """an action box that is not [-1, 1]; its last dimension has high == low when there is more than one"""
    low = np.linspace(-2.0, 0.5, Da).astype(F32)
    high = (low + np.linspace(0.7, 3.0, Da)).astype(F32)
    if Da > 1:
        high[-1] = low[-1]
    return low, high


def dataset(Do, Da, lens, seed, low=None, high=None):
    """episodes in the export layout; `actions` is what an env with the box [low, high] received (exact +-1 units among them)"""
    rng = np.random.default_rng(seed)
    n = int(sum(lens))
    unit = rng.uniform(-1.0, 1.0, (n, Da)).astype(F32)
    unit[rng.random((n, Da)) < 0.05] = 1.0
    unit[rng.random((n, Da)) < 0.05] = -1.0
    act = unit if low is None else (low + (high - low) * (unit + F32(1.0)) / F32(2.0)).astype(F32)
    ends = np.cumsum(lens) - 1
    term, tout = np.zeros(n, bool), np.zeros(n, bool)
    for j, e in enumerate(ends):
        term[e], tout[e] = j % 3 != 1, j % 3 != 0              # terminal, timeout, both
    return dict(observations=rng.standard_normal((n, Do)).astype(F32), next_observations=rng.standard_normal((n, Do)).astype(F32),
                actions=act, rewards=rng.normal(0.5, 1.0, n), costs=(rng.random(n) < 0.3).astype(F64), terminals=term, timeouts=tout)


def episode_slices(data):
    done = np.flatnonzero(data["terminals"] | data["timeouts"])
    first = np.concatenate([[0], done[:-1] + 1])
    return [slice(int(a), int(b) + 1) for a, b in zip(first, done)]


def ppo_engine(Do, Da, env_num, sub, seed=0):
    from fsrl_amd.engine import Engine, EngineConfig
    eng = Engine(EngineConfig(obs_dim=Do, act_dim=Da, hidden_sizes=(64, 64), env_num=env_num, buffer_size=env_num * sub,
                              target_kl=None, max_grad_norm=0.5))
    eng.set_params((0.1 * np.random.default_rng(seed).standard_normal(eng.n_params)).astype(F32))
    return eng


def archive_of(eng, data, max_episode_len=512):
    from fsrl_amd.engine import TrajArchive
    arch = TrajArchive(eng, max(len(data["rewards"]), max_episode_len), 256, max_episode_len)
    n_eps = len(episode_slices(data))
    assert arch.import_rows(data) == (n_eps, len(data["rewards"]))
    return arch


def push_loop(eng, data, order, first_env, buffer_num, code, low, high):
    """the model of fsrl_store_fill: every row of episode order[j] through Engine.push into sub-buffer (first_env + j) % buffer_num"""
    from fsrl_amd.data.traj_buf import inverse_action
    act = inverse_action(data["actions"], code, low, high)
    sl = episode_slices(data)
    for j, ep in enumerate(order):
        e = (first_env + j) % buffer_num
        for r in range(sl[ep].start, sl[ep].stop):
            eng.push([e], data["observations"][r], act[r], data["rewards"][r:r + 1], data["costs"][r:r + 1],
                     data["terminals"][r:r + 1], data["timeouts"][r:r + 1], data["next_observations"][r])


def snapshot(eng):
    idx = eng.sample0()
    rows = eng.store_read(idx)
    return dict(sample0=idx, sizes=eng.store_sizes(), **rows)


def assert_same_store(a, b):
    x, y = snapshot(a), snapshot(b)
    for k in x:
        assert x[k].dtype == y[k].dtype and x[k].shape == y[k].shape, k
        assert np.array_equal(np.ascontiguousarray(x[k]).view(np.uint8), np.ascontiguousarray(y[k]).view(np.uint8)), k


def assert_same_books(a, b, buffer_num, seed=99):
    """ONE further push per sub-buffer: what it returns (ptr, ep_rew, ep_len, ep_idx) shows index, ep_rew, ep_len and ep_idx; an
    episode-ending one follows, whose returns show the sums"""
    rng = np.random.default_rng(seed)
    Do, Da = a.cfg.obs_dim, a.cfg.act_dim
    for done in (False, True):
        ids = np.arange(buffer_num)
        row = (ids, rng.standard_normal((buffer_num, Do)).astype(F32), rng.standard_normal((buffer_num, Da)).astype(F32),
               rng.normal(0.5, 1.0, buffer_num), np.zeros(buffer_num), np.full(buffer_num, done), np.zeros(buffer_num, bool),
               rng.standard_normal((buffer_num, Do)).astype(F32))
        for u, v in zip(a.push(*row), b.push(*row)):
            assert np.array_equal(u, v), (done, u, v)
    assert_same_store(a, b)


def fill_and_push(Do, Da, env_num, sub, lens, code, scaled, order=None, first_env=0, before=None, seed=3):
    """twin contexts: A is filled, B is pushed -> (A, B, archive, rows the fill reported)"""
    low, high = box(Da) if scaled else (None, None)
    data = dataset(Do, Da, lens, seed, low, high)
    a, b = ppo_engine(Do, Da, env_num, sub), ppo_engine(Do, Da, env_num, sub)
    if before is not None:
        before(a); before(b)
    arch = archive_of(a, data)
    ids, rows, _, _, _ = arch.episodes()
    c0 = arch.counters()
    n = a.store_fill(arch, None if order is None else ids[order], first_env, code, low, high)
    c1 = arch.counters()
    # one host-to-device copy of a job table and one launch, whatever the fill holds
    assert (c1["fill_launches"] - c0["fill_launches"], c1["fill_copies"] - c0["fill_copies"]) == (1, 1)
    order = list(range(len(lens))) if order is None else list(order)
    assert n == int(sum(lens[i] for i in order)) and rows.tolist() == list(lens)
    push_loop(b, data, order, first_env, env_num, code, low, high)
    return a, b, arch, n


# ---------------------------------------------------------------- 1. fill equals push
@pytest.mark.parametrize("code,scaled", [(0, False), (0, True), (1, False), (1, True)], ids=["none", "none_box", "clip", "clip_box"])
@pytest.mark.parametrize("Do,Da", SHAPES)
def test_fill_equals_push_bit_for_bit(Do, Da, code, scaled):
    """three sub-buffers of 512 rows, nothing wraps: the three shapes (rows of 20, 32 and 132 bytes) under bound none and clip, with
    and without a box (one dimension of it with high == low)"""
    a, b, arch, n = fill_and_push(Do, Da, 3, 512, LENS, code, scaled)
    assert len(a) == n == sum(LENS)
    assert_same_store(a, b)
    assert_same_books(a, b, 3)
    arch.close(); a.close(); b.close()


@pytest.mark.parametrize("buffer_num", [1, 3, 4])
def test_fill_wraps_and_drops_what_it_overwrites(buffer_num):
    """sub_size 64 under episodes of up to 300 rows: sub-buffers wrap, rows a later row of the same fill overwrites are never written"""
    a, b, arch, n = fill_and_push(8, 2, buffer_num, 64, LENS, 1, True)
    assert n == sum(LENS) and len(a) <= 64 * buffer_num < n
    assert_same_store(a, b)
    assert_same_books(a, b, buffer_num)
    arch.close(); a.close(); b.close()


def _complete_episodes(eng, rows_per_env, seed):
    """complete episodes through Engine.push, lock step: `rows_per_env` rows per sub-buffer, an episode ends every 23 rows and at the end"""
    rng = np.random.default_rng(seed)
    k, Do, Da = eng.cfg.env_num, eng.cfg.obs_dim, eng.cfg.act_dim
    for t in range(rows_per_env):
        done = t % 23 == 22 or t == rows_per_env - 1
        eng.push(np.arange(k), rng.standard_normal((k, Do)).astype(F32), rng.standard_normal((k, Da)).astype(F32), rng.normal(0, 1, k),
                 np.zeros(k), np.full(k, done), np.zeros(k, bool), rng.standard_normal((k, Do)).astype(F32))


@pytest.mark.parametrize("held", [40, 100, 150], ids=["part_filled", "wrapped", "wrapped_twice"])
def test_fill_onto_a_store_that_already_holds_episodes(held):
    """the store holds complete episodes -- 40 rows per sub-buffer of 64, or 100 / 150 (wrapped) -- still in the staging window when
    the fill comes: they land first"""
    a, b, arch, n = fill_and_push(8, 2, 3, 64, [30, 1, 17, 45], 1, True, before=lambda e: _complete_episodes(e, held, seed=held))
    assert_same_store(a, b)
    assert_same_books(a, b, 3)
    arch.close(); a.close(); b.close()


def test_fill_a_subset_in_shuffled_order_from_first_env_2():
    order = [4, 0, 6, 2, 1]
    a, b, arch, n = fill_and_push(33, 8, 4, 512, LENS, 0, True, order=order, first_env=2)
    assert n == sum(LENS[i] for i in order)
    assert a.store_sizes().tolist() == [LENS[6], LENS[2], LENS[4] + LENS[1], LENS[0]]
    assert_same_store(a, b)
    assert_same_books(a, b, 4)
    # an empty list is a list: nothing is poured; None is every episode
    assert a.store_fill(arch, []) == 0 and arch.counters()["fill_launches"] == 1
    arch.close(); a.close(); b.close()


def test_fill_from_the_archive_the_context_feeds_adds_nothing_to_it():
    """the filled rows are not tapped; rows the context pushed before the fill are archived as ever"""
    from fsrl_amd.engine import TrajArchive
    data = dataset(8, 2, [9, 20, 5], 11)
    a, b = ppo_engine(8, 2, 2, 128), ppo_engine(8, 2, 2, 128)
    arch = TrajArchive(a, 1024, 64, 64, 0)
    assert arch.attach(a) == 0
    arch.import_rows(data, source=5)
    _complete_episodes(a, 7, seed=1); _complete_episodes(b, 7, seed=1)      # two tapped episodes, unflushed
    assert a.store_fill(arch) == 34 + 14                                     # the flush archived them: they are poured as well
    assert arch.counters()["committed"] == 5 and arch.episodes()[4].tolist() == [5, 5, 5, 0, 0]
    push_loop(b, data, [0, 1, 2], 0, 2, 0, None, None)
    tapped = {k: v[34:] for k, v in arch.export().items()}                 # the two tapped episodes: 3 and 4 of the fill
    push_loop(b, tapped, [0, 1], 3, 2, 0, None, None)
    assert_same_store(a, b)
    _complete_episodes(a, 3, seed=2)
    arch.flush()
    assert arch.counters()["committed"] == 7                                # 5 + the two just pushed: the fill's 48 rows added none
    arch.close(); a.close(); b.close()


# ---------------------------------------------------------------- 2. tanh
def test_tanh_inverse_is_within_4x_the_reference_formulas_own_error_and_finite():
    """inputs in (-0.999, 0.999), 0, +-1e-6, +-(1 - 2^-24), +-1 against float64 arctanh of the float32 input (+-1 clamped to
    +-(1 - 2^-24), the library's stated departure).  The bar is 4x the worst absolute error of the reference formula in numpy float32
    on the same inputs; the figures measured on an MI355X are in DESIGN.md 2.2."""
    from fsrl_amd.data.traj_buf import inverse_action
    Do, Da, n = 5, 8, 256
    rng = np.random.default_rng(0)
    lim = F32(1.0 - 2.0 ** -24)
    x = rng.uniform(-0.999, 0.999, n * Da).astype(F32)
    x[:9] = [0.0, 1e-6, -1e-6, lim, -lim, 1.0, -1.0, 0.999, -0.999]
    data = dataset(Do, Da, [n], 2)
    data["actions"] = x.reshape(n, Da)
    eng = ppo_engine(Do, Da, 1, n)
    arch = archive_of(eng, data)
    assert eng.store_fill(arch, None, 0, 2) == n
    got = eng.store_read(np.arange(n))["act"].reshape(-1)
    want = np.arctanh(np.clip(x, -lim, lim).astype(F64))
    ref_err = np.abs(inverse_action(x, 2).astype(F64) - want).max()
    dev_err = np.abs(got.astype(F64) - want).max()
    print(f"tanh inverse: reference formula (numpy float32) max abs error {ref_err:.3e}, device {dev_err:.3e}, bar {4 * ref_err:.3e}")
    assert np.all(np.isfinite(got))
    assert got[0] == 0.0 and got[5] == got[3] and got[6] == got[4]
    assert dev_err <= 4 * ref_err, (dev_err, ref_err)
    arch.close(); eng.close()


# ---------------------------------------------------------------- 3. a replay agent cannot tell the difference
def replay_engine(kind, seed, env_num=4, sub=128):
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig
    eng = Engine(EngineConfig(algo=_lib.ALGO_SAC_LAG, obs_dim=8, act_dim=2, hidden_sizes=(64, 64), n_critics=2, env_num=env_num,
                              buffer_size=env_num * sub, target_kl=None))
    if kind == "cvpo":
        eng.cvpo_init(qc_thres=0.4, sample_act_num=8)
    else:
        eng.sac_init(auto_alpha=True, n_step=2)
    rng = np.random.default_rng(seed)
    eng.sac_set_params((0.2 * rng.standard_normal(eng.n_sac_actor)).astype(F32), (0.2 * rng.standard_normal(eng.n_sac_critics)).astype(F32), 0.1)
    return eng


def replay_state(eng, kind):
    which = (0, 1, 2) if kind == "sac" else (0, 1, 2, 3)
    return [x for w in which for x in (eng.sac_get_params(w)[0], np.array([eng.sac_get_params(w)[1]]))]


def filled_and_pushed(kind, seed, lens):
    low, high = box(2)
    data = dataset(8, 2, lens, seed, low, high)
    a, b = replay_engine(kind, seed), replay_engine(kind, seed)
    arch = archive_of(a, data)
    assert a.store_fill(arch, None, 0, 1, low, high) == sum(lens)
    push_loop(b, data, range(len(lens)), 0, 4, 1, low, high)
    return a, b, arch


@pytest.mark.parametrize("kind", ["sac", "cvpo"])
def test_three_updates_on_a_filled_and_on_a_pushed_store_are_bit_identical(kind):
    """SAC-Lag (obs 8, act 2, hidden 64, batch 64, n_step 2) and CVPO at its smallest shape (8 particles, batch 32): library sampling
    under one seed, so the flag mirror, the device books and the sampler all see the fill as they see pushes; one sub-buffer wraps"""
    a, b, arch = filled_and_pushed(kind, 5, [60, 90, 33, 70, 150, 12])
    for i in range(3):
        rows = []
        for eng in (a, b):
            seed = 7 if i == 0 else 0
            if kind == "cvpo":
                eng.cvpo_pre_update()
                row = eng.cvpo_update(32, seed=seed)
                eng.cvpo_post_update()
                rows.append([row, eng.cvpo_duals(), *eng.sac_last_sample(32), eng.cvpo_last_particles(32)])
            else:
                rows.append([eng.sac_update(64, [0.3], 0.8, seed=seed), *eng.sac_last_sample(64)])
        for u, v in zip(*rows):
            assert np.array_equal(u, v), i
        assert np.all(np.isfinite(rows[0][0]))
    for u, v in zip(replay_state(a, kind), replay_state(b, kind)):
        assert np.array_equal(u, v)
    arch.close(); a.close(); b.close()


def test_a_group_of_two_sac_members_filled_and_pushed_is_bit_identical():
    from fsrl_amd.engine import EngineSacGroup
    twins = [filled_and_pushed("sac", 20 + i, [50 + 10 * i, 90, 140, 33]) for i in range(2)]
    for i, (a, b, _) in enumerate(twins):                  # key each member's Philox stream: one own update on both twins
        for e in (a, b):
            e.sac_update(64, [0.3 + 0.2 * i], 0.8, seed=11 + i, sync=False)
    ga, gb = EngineSacGroup([t[0] for t in twins]), EngineSacGroup([t[1] for t in twins])
    for g in (ga, gb):
        g.update(64, [3, 3], [[0.3], [0.5]], [0.8, 0.7])
    for a, b, _ in twins:
        ra, rb = a.sac_drain(), b.sac_drain()
        assert ra.shape == rb.shape == (4, ra.shape[1]) and np.array_equal(ra, rb) and np.all(np.isfinite(ra))
        for u, v in zip(replay_state(a, "sac"), replay_state(b, "sac")):
            assert np.array_equal(u, v)
    ga.close(); gb.close()
    for a, b, arch in twins:
        arch.close(); a.close(); b.close()


# ---------------------------------------------------------------- 4. refusals
@pytest.fixture
def refusal_case():
    data = dataset(8, 2, [10, 20, 5], 4)
    eng = ppo_engine(8, 2, 2, 128)
    _complete_episodes(eng, 30, seed=8)
    arch = archive_of(eng, data)
    state = dict(before=snapshot(eng))
    yield eng, arch, state
    before, after = state["before"], snapshot(eng)          # refused before the first write: the store is what it was
    for k in before:
        assert np.array_equal(np.ascontiguousarray(before[k]).view(np.uint8), np.ascontiguousarray(after[k]).view(np.uint8)), k
    assert arch.counters()["fill_launches"] == 0 and arch.counters()["fill_copies"] == 0
    arch.close(); eng.close()


def _estate(exc):
    from fsrl_amd import _lib
    return f"[{_lib.FSRL_ESTATE}]" in str(exc.value)


@pytest.mark.parametrize("Do,Da,field", [(9, 2, "obs_dim"), (8, 3, "act_dim")])
def test_refuses_another_shape(refusal_case, Do, Da, field):
    eng, arch, _ = refusal_case
    other = ppo_engine(Do, Da, 2, 128)
    with pytest.raises(AssertionError, match=field):
        other.store_fill(arch)
    assert len(other) == 0
    other.close()


def test_refuses_another_device(refusal_case):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("a context on a second device needs a second device")
    from fsrl_amd.engine import Engine, EngineConfig
    eng, arch, _ = refusal_case
    other = Engine(EngineConfig(obs_dim=8, act_dim=2, hidden_sizes=(64, 64), env_num=2, buffer_size=256, target_kl=None), device=1)
    with pytest.raises(AssertionError, match="device"):
        other.store_fill(arch)
    other.close()


def test_refuses_inside_an_update(refusal_case):
    from fsrl_amd._lib import FsrlHipError
    eng, arch, _ = refusal_case
    eng.ppo_begin([0.3], 0.8, 32)
    with pytest.raises(FsrlHipError, match="update") as exc:
        eng.store_fill(arch)
    assert _estate(exc)
    eng.ppo_abort()


def test_refuses_a_sub_buffer_with_an_episode_in_progress(refusal_case):
    from fsrl_amd._lib import FsrlHipError
    eng, arch, state = refusal_case
    ids = arch.episodes()[0]
    eng.push([1], np.zeros((1, 8), F32), np.zeros((1, 2), F32), [0.5], [0.0], [False], [False], np.zeros((1, 8), F32))
    state["before"] = snapshot(eng)
    with pytest.raises(FsrlHipError, match=r"sub-buffer 1 .*ep_len 1.*between collects") as exc:
        eng.store_fill(arch)
    assert _estate(exc)
    with pytest.raises(FsrlHipError, match="ep_len"):
        eng.store_fill(arch, ids[:1], first_env=1)


@pytest.mark.parametrize("ids,msg", [([0, 7], r"episode_ids\[1\] = 7"), ([1, 2, 1], r"episode_ids\[2\] = 1 is listed twice"),
                                     ([0], r"episode_ids\[0\] = 0 is not alive")], ids=["unknown", "twice", "dead"])
def test_refuses_an_episode_id_that_is_unknown_dead_or_listed_twice(refusal_case, ids, msg):
    eng, arch, _ = refusal_case
    if msg.endswith("not alive"):
        arch.keep([1, 2])                                   # episode 0 is dead now
    with pytest.raises(AssertionError, match=msg):
        eng.store_fill(arch, ids)


@pytest.mark.parametrize("first_env", [-1, 2])
def test_refuses_first_env_outside_the_sub_buffers(refusal_case, first_env):
    eng, arch, _ = refusal_case
    with pytest.raises(AssertionError, match="first_env"):
        eng.store_fill(arch, None, first_env)


@pytest.mark.parametrize("bound", [-1, 3])
def test_refuses_an_unknown_bound_method(refusal_case, bound):
    eng, arch, _ = refusal_case
    with pytest.raises(AssertionError, match="bound_method"):
        eng.store_fill(arch, None, 0, bound)


# ---------------------------------------------------------------- 5. the Python surface
class _Box:
    def __init__(self, low, high):
        self.low, self.high, self.shape = low, high, low.shape


class _Policy:
    """what fill_from reads off a policy"""

    def __init__(self, method, low, high, scaling=True):
        self.action_bound_method, self.action_scaling, self.action_space = method, scaling, _Box(low, high)


def test_buffer_fill_from_a_trajectory_buffer_under_a_policys_action_box():
    from fsrl_amd.data import HipVectorReplayBuffer, TrajectoryBuffer
    low, high = box(2)
    lens = [12, 40, 7, 90]
    data = dataset(8, 2, lens, 6, low, high)
    rec = ppo_engine(8, 2, 2, 64)
    a, b = ppo_engine(8, 2, 3, 64), ppo_engine(8, 2, 3, 64)
    tb = TrajectoryBuffer(rec, max_trajectory=16, max_rows=1024, max_episode_len=128)
    assert tb.load(data) == 4 and len(tb) == sum(lens) and tb.sources.tolist() == [-1] * 4
    buf = HipVectorReplayBuffer(a)
    pol = _Policy("clip", low, high)
    assert buf.fill_from(tb, episodes=[3, 0, 2], policy=pol, first_env=1) == 90 + 12 + 7
    assert len(buf) == 64 + 12 + 7 and buf._sizes[:3].tolist() == [7, 64, 12]          # sync_sizes ran
    push_loop(b, data, [3, 0, 2], 1, 3, 1, low, high)
    assert_same_store(a, b)
    assert buf.fill_from(tb, policy=pol) == sum(lens)       # None: every stored episode
    push_loop(b, data, [0, 1, 2, 3], 0, 3, 1, low, high)
    assert_same_store(a, b)
    tb.close(); rec.close(); a.close(); b.close()


def test_sac_agent_learns_from_a_prefilled_store(tmp_path, capsys):
    """learn(prefill=path): the store holds the dataset's rows before the first collect, and no env step is counted for them"""
    from fsrl_amd.agent import SACLagAgent
    from fsrl_amd.data import FastCollector
    from fsrl_amd.env import SyntheticSafetyVectorEnv
    from fsrl_amd.utils import BaseLogger
    lens = [40, 25, 40, 13, 31]
    data = dataset(8, 2, lens, 9)
    path = str(tmp_path / "ds.npz")
    np.savez_compressed(path, **data)
    train = SyntheticSafetyVectorEnv(env_num=4, episode_len=40, seed=1)
    agent = SACLagAgent(train, BaseLogger(str(tmp_path), name="s"), cost_limit=10, device="cuda:0", seed=3, hidden_sizes=(64, 64),
                        training_num=4, buffer_size=4000)
    seen = []
    collect = FastCollector.collect

    def spy(self, *args, **kw):
        if self.buffer is not None and not seen:
            seen.append((len(self.buffer), int(self.collect_step), self))
        return collect(self, *args, **kw)

    FastCollector.collect = spy
    try:
        ep, stat, info = agent.learn(train, None, epoch=1, episode_per_collect=4, step_per_epoch=160, update_per_step=0.2, batch_size=64,
                                     verbose=False, save_ckpt=False, prefill=path)
    finally:
        FastCollector.collect = collect
    rows_before, steps_before, collector = seen[0]
    assert (rows_before, steps_before) == (sum(lens), 0)    # before the first collect: the dataset's rows, and no env step
    assert "prefill: 149 rows" in capsys.readouterr().out
    assert ep == 1 and np.isfinite(list(stat.values())).all()
    # every env step the run counted is a collected row on top of the dataset: the fill counted none
    assert collector.collect_step >= 160 and len(agent.policy.engine) == sum(lens) + collector.collect_step
    # a resumed run that restored a store keeps it: the fill is skipped, and says so
    held = len(agent.policy.engine)
    assert agent._prefill(path, collector.buffer, resumed=True) == 0 and len(agent.policy.engine) == held
    assert "prefill: skipped" in capsys.readouterr().out


def test_train_agent_example_refuses_prefill_for_an_on_policy_algorithm():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_agent.py"), "--algo", "ppol", "--prefill", "x"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--prefill fills a replay store" in out.stderr and "ppol" in out.stderr
