"""The trajectory archive on the device (fsrl_traj_*, fsrl_amd/csrc/host_traj.inc + kernels_traj.hpp) and TrajectoryBuffer on top.
Rows are pushed through Engine.push / collect_step with scripted data, so the expected export is known exactly: every comparison
below is bit for bit."""
import random

import numpy as np
import pytest

from traj_problems import COLUMNS, episodes_of, load_store_cases

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


# ---------------------------------------------------------------- scripted streams
class Script:
    """Random rows for the envs asked for, and the episodes they form, in completion order (vector step, then position in the push)."""

    def __init__(self, Do, Da, seed, source=0):
        self.rng, self.Do, self.Da, self.source = np.random.default_rng(seed), Do, Da, source
        self.open, self.done = {}, []

    def rows(self, ids, term, trunc):
        k, r = len(ids), self.rng
        return dict(ids=np.asarray(ids, np.int32), obs=r.standard_normal((k, self.Do)).astype(F32), rew=r.normal(0.5, 1.0, k),
                    cost=(r.random(k) < 0.3).astype(F64), term=np.asarray(term, bool), trunc=np.asarray(trunc, bool),
                    nxt=r.standard_normal((k, self.Do)).astype(F32))

    def policy_act(self, k):
        return (1.5 * self.rng.standard_normal((k, self.Da))).astype(F32)

    def record(self, rows, env_act):
        for j, e in enumerate(rows["ids"]):
            ep = self.open.setdefault(int(e), dict(rows=[], rew=0.0, cost=0.0, source=self.source))
            ep["rows"].append((rows["obs"][j], rows["nxt"][j], np.array(env_act[j], F32), rows["rew"][j], rows["cost"][j],
                               bool(rows["term"][j]), bool(rows["trunc"][j])))
            ep["rew"] += float(rows["rew"][j]); ep["cost"] += float(rows["cost"][j])       # float64, push order
            if rows["term"][j] or rows["trunc"][j]:
                self.done.append(self.open.pop(int(e)))

    def push(self, eng, ids, term, trunc, cost=None):
        """through Engine.push; the archive's action is the library's clip of the pushed one"""
        rows, act = self.rows(ids, term, trunc), self.policy_act(len(ids))
        if cost is not None:
            rows["cost"] = np.asarray(cost, F64)
        eng.push(rows["ids"], rows["obs"], act, rows["rew"], rows["cost"], rows["term"], rows["trunc"], rows["nxt"])
        self.record(rows, np.clip(act, -1.0, 1.0))


class Lengths:
    """per env a cycle of episode lengths -> the done flags of every vector step (odd episodes end truncated, even terminated)"""

    def __init__(self, per_env):
        self.per_env = [list(x) for x in per_env]
        self.k = [0] * len(per_env)
        self.left = [x[0] for x in self.per_env]

    def step(self, ids):
        term, trunc = np.zeros(len(ids), bool), np.zeros(len(ids), bool)
        for j, e in enumerate(ids):
            self.left[e] -= 1
            if self.left[e] == 0:
                (trunc if self.k[e] % 2 else term)[j] = True
                self.k[e] += 1
                self.left[e] = self.per_env[e][self.k[e] % len(self.per_env[e])]
        return term, trunc


def expected(episodes, Do, Da):
    if not episodes:
        return dict(observations=np.zeros((0, Do), F32), next_observations=np.zeros((0, Do), F32), actions=np.zeros((0, Da), F32),
                    rewards=np.zeros(0), costs=np.zeros(0), terminals=np.zeros(0, bool), timeouts=np.zeros(0, bool))
    cols = list(zip(*[r for ep in episodes for r in ep["rows"]]))
    return dict(observations=np.stack(cols[0]), next_observations=np.stack(cols[1]), actions=np.stack(cols[2]),
                rewards=np.array(cols[3], F64), costs=np.array(cols[4], F64), terminals=np.array(cols[5], bool),
                timeouts=np.array(cols[6], bool))


def assert_export(arch, episodes, Do, Da):
    arch.flush()
    ids, rows, rew, cost, src = arch.episodes()
    assert rows.tolist() == [len(ep["rows"]) for ep in episodes]
    assert np.array_equal(rew, np.array([ep["rew"] for ep in episodes], F64))           # the float64 running sums, bit for bit
    assert np.array_equal(cost, np.array([ep["cost"] for ep in episodes], F64))
    assert src.tolist() == [ep["source"] for ep in episodes]
    got, want = arch.export(), expected(episodes, Do, Da)
    for k in COLUMNS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), k         # bit for bit (NaN-proof)
    return ids


def make_engine(kind, Do, Da, env_num=3, buffer_size=None, seed=0):
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig
    hs = (64, 64) if "fused" in kind else (48, 64, 40)
    rng = np.random.default_rng(seed)
    if kind.startswith("sac"):
        eng = Engine(EngineConfig(algo=_lib.ALGO_SAC_LAG, obs_dim=Do, act_dim=Da, hidden_sizes=hs, n_critics=2, env_num=env_num,
                                  buffer_size=buffer_size or env_num * 64, target_kl=None))
        # the stochastic SAC-Lag actor head has 2 x act_dim <= 16 outputs: at act_dim 16 a replay context is a DDPG-Lag one
        eng.sac_init(deterministic=Da > 8)
        eng.sac_set_params(0.1 * rng.standard_normal(eng.n_sac_actor).astype(F32),
                           0.1 * rng.standard_normal(eng.n_sac_critics).astype(F32), float(np.log(0.2)))
    else:
        eng = Engine(EngineConfig(obs_dim=Do, act_dim=Da, hidden_sizes=hs, env_num=env_num, buffer_size=buffer_size or env_num * 64,
                                  target_kl=None, max_grad_norm=0.5))
        eng.set_params((0.1 * rng.standard_normal(eng.n_params)).astype(F32))
    return eng


def archive(eng, max_rows=4096, max_episodes=512, max_episode_len=64, bound=1, low=None, high=None):
    from fsrl_amd.engine import TrajArchive
    arch = TrajArchive(eng, max_rows, max_episodes, max_episode_len, bound, low, high)
    assert arch.attach(eng) == 0
    return arch


# ---------------------------------------------------------------- 1. exactness
@pytest.mark.parametrize("kind", ["ppo_fused", "ppo_layered", "sac_fused", "sac_layered"])
@pytest.mark.parametrize("Do,Da", [(5, 3), (8, 2), (128, 16)])
def test_export_is_the_pushed_stream_bit_for_bit(kind, Do, Da):
    """three envs, episode lengths from 1 .. 40 with a 1 among them, rows through collect_step: get_all() is the pushed rows in
    episode-completion order, metrics the float64 running sums, actions the env_act collect_step returned for those rows -- under
    clip, and under tanh with a non-trivial [low, high].  A replay context holds obs_dim + act_dim <= 128 and a stochastic head of
    act_dim <= 8 (fsrl_sac_init): at the widest shape the sac_* cases are the widest replay context there is, DDPG-Lag at (112, 16)."""
    if kind.startswith("sac") and Do + Da > 128:
        Do = 128 - Da
    eng = make_engine(kind, Do, Da)
    lrng = np.random.default_rng(Do * 100 + Da)
    low = np.linspace(-2.0, 0.5, Da).astype(F32); high = (low + np.linspace(0.7, 3.0, Da)).astype(F32)
    for bound, lo, hi in ((1, None, None), (2, low, high)):
        arch = archive(eng, bound=bound, low=lo, high=hi)
        per_env = [lrng.integers(1, 41, 4).tolist() for _ in range(3)]
        per_env[1][1] = 1
        sc, ln = Script(Do, Da, seed=7 + bound), Lengths(per_env)
        ids = np.arange(3)
        obs = sc.rng.standard_normal((3, Do)).astype(F32)
        act, env_act, _, _ = eng.collect_step(None, obs, False, bound, lo, hi)
        for t in range(130):
            term, trunc = ln.step(ids)
            rows = sc.rows(ids, term, trunc)
            rows["obs"] = obs
            sc.record(rows, env_act)
            prev = (ids, obs, act, rows["rew"], rows["cost"], term, trunc, rows["nxt"])
            obs = rows["nxt"]
            act, env_act, _, _ = eng.collect_step(prev, obs, False, bound, lo, hi)
        assert len(sc.done) >= 6 and 1 in [len(ep["rows"]) for ep in sc.done] and sc.open       # open episodes are never exported
        assert_export(arch, sc.done, Do, Da)
        got = arch.export()["actions"]
        if bound == 2:
            assert (got >= low).all() and (got <= high).all() and got.std() > 0.1
        c = arch.counters()
        assert c["committed"] == len(sc.done) and c["rows"] == len(got) and c["rejected_window"] == c["dropped_long"] == 0
        arch.close()
    eng.close()


# ---------------------------------------------------------------- 2. independence from the store
def test_archive_does_not_depend_on_the_stores_geometry():
    Do, Da = 5, 3
    eng = make_engine("ppo_fused", Do, Da, buffer_size=24)            # sub-buffers of 8 rows
    assert eng.store_geometry() == (8, 3)
    arch = archive(eng, max_rows=8192, max_episode_len=32)
    sc, ln = Script(Do, Da, seed=3), Lengths([[20], [20, 7], [13, 20]])
    ids = np.arange(3)
    for t in range(90):                                               # 20-row episodes through 8-row sub-buffers that wrap
        sc.push(eng, ids, *ln.step(ids))
        if t == 30:
            eng.reset_store(keep_statistics=True)                     # in the middle of every env's episode
        if t == 55:
            eng.store_configure(12, 3)                                # ... and a re-cut store (it empties it)
    assert eng.store_geometry() == (4, 3)
    assert len(sc.done) == 4 + 6 + 5                                  # 90 steps of 20 | 20, 7 | 13, 20
    assert_export(arch, sc.done, Do, Da)
    arch.close(); eng.close()


def test_full_staging_windows_and_several_episodes_of_one_env_in_a_window():
    Do, Da = 5, 3
    eng = make_engine("ppo_fused", Do, Da, buffer_size=3 * 2000)     # nothing wraps: only a full window flushes
    arch = archive(eng, max_rows=8192, max_episode_len=1200)
    sc, ln = Script(Do, Da, seed=4), Lengths([[1000], [1200], [700]])
    ids = np.arange(3)
    for t in range(1500):                                             # 4 500 records: more than a staging window (4 096)
        sc.push(eng, ids, *ln.step(ids))
    # nothing but the full window flushed -- an episode that ends and the next one of its env share a window (two slots per env),
    # no env ended two episodes inside one: one stage launch and one commit launch (episodes of 700 .. 1 200 rows: 6 .. 10 jobs each)
    assert arch.counters()["launches"] == 2
    n = len(sc.done)
    assert [len(e["rows"]) for e in sc.done] == [700, 1000, 1200, 700] and len(sc.open) == 3
    # the envs are reset in mid-episode: the three open episodes are no trajectories
    arch.abandon(eng); sc.open.clear()
    # several episodes of ONE env ending inside one window: lengths 2, 3, 1, 1, 5 of env 1, nothing in between
    ln = Lengths([[1], [2, 3, 1, 1, 5], [1]])
    one = np.array([1])
    for t in range(12):
        sc.push(eng, one, *ln.step(one))
    assert [len(e["rows"]) for e in sc.done[n:]] == [2, 3, 1, 1, 5]
    assert_export(arch, sc.done, Do, Da)
    assert arch.counters()["abandoned"] == 3
    arch.close(); eng.close()


# ---------------------------------------------------------------- 3. limits
def test_limits_window_overlong_compaction_and_a_full_archive():
    Do, Da = 8, 2
    eng = make_engine("ppo_fused", Do, Da)
    arch = archive(eng, max_rows=25, max_episodes=16, max_episode_len=10)
    sc = Script(Do, Da, seed=11)
    zero, two = np.array([0]), np.array([2])

    def episode(ids, n, costs=None):
        for t in range(n):
            sc.push(eng, ids, [t == n - 1], [False], cost=None if costs is None else [costs[t]])

    episode(zero, 10)                                   # exactly max_episode_len: kept
    episode(zero, 11)                                   # one row longer: dropped and counted ...
    long_one = sc.done.pop()
    assert len(long_one["rows"]) == 11
    episode(zero, 4)                                    # ... and the next episode of that env is intact
    ids = assert_export(arch, sc.done, Do, Da)
    assert arch.counters()["dropped_long"] == 1 and [len(e["rows"]) for e in sc.done] == [10, 4]
    # the window drops and counts (traj_buf.py:71-73: strictly outside)
    arch.set_window(-1e9, 1e9, -1.0, 0.5)
    before = len(sc.done)
    for costs in ([0.0, 0.0], [1.0, 0.0], [0.0, 0.0], [1.0, 1.0], [0.0, 0.5], [0.25, 0.5]):      # 0.5 is ON the bound: inside
        episode(two, 2, costs)
    kept = sc.done[:before] + [e for e in sc.done[before:] if e["cost"] <= 0.5]
    rejected = len(sc.done) - len(kept)
    assert rejected == 3
    sc.done = kept
    arch.set_window(-np.inf, np.inf, -np.inf, np.inf)
    ids = assert_export(arch, sc.done, Do, Da)
    assert arch.counters()["rejected_window"] == rejected
    # room for a little over two episodes of ten rows: dead rows are compacted away and the archive keeps going
    arch.keep(ids[:1]); sc.done = sc.done[:1]           # 10 rows alive
    c0 = arch.counters()["compactions"]
    episode(zero, 10)                                   # 20
    ids = assert_export(arch, sc.done, Do, Da)
    arch.replace(int(ids[0])); sc.done = sc.done[1:]    # the newest takes the first one's place: 10 alive, 10 dead, tail at 20
    episode(zero, 10)                                   # 20 + 10 > 25: compacts, then fits
    ids = assert_export(arch, sc.done, Do, Da)
    c = arch.counters()
    assert c["compactions"] == c0 + 1 and c["rows"] == 20 and c["refused_full"] == 0
    # no room even after a compaction: the error names max_rows, nothing is overwritten
    with pytest.raises(MemoryError, match="max_rows = 25"):
        episode(zero, 6)
        arch.flush()
    sc.done.pop()
    assert arch.counters()["refused_full"] == 1
    episode(zero, 5)                                    # 25 rows: exactly full is fine
    assert_export(arch, sc.done, Do, Da)
    arch.close(); eng.close()


# ---------------------------------------------------------------- 4. keep / replace
@pytest.mark.parametrize("name", sorted(load_store_cases()))
def test_reference_store_cases_through_a_tapped_engine(name):
    """tests/golden/traj_store_cases.npz (recorded from the reference's TrajectoryBuffer.store) replayed through Engine.push under a
    TrajectoryBuffer: the surviving episodes, their order, metrics and rows are the fixture's"""
    from fsrl_amd.data import TrajectoryBuffer
    case = load_store_cases()[name]
    Do, Da = 5, 3
    eng = make_engine("ppo_fused", Do, Da)
    random.seed(int(case["seed"])); np.random.seed(int(case["seed"]))
    tb = TrajectoryBuffer(eng, max_episode_len=16, max_rows=512, action_bound_method="clip", **case["kwargs"])
    eps = episodes_of(case, Do, Da)
    for i, ep in enumerate(eps):
        e = np.array([i % 3])
        for t in range(len(ep["rew"])):
            eng.push(e, ep["obs"][t:t + 1], ep["act"][t:t + 1], ep["rew"][t:t + 1], ep["cost"][t:t + 1], ep["terminated"][t:t + 1],
                     ep["truncated"][t:t + 1], ep["obs_next"][t:t + 1])
        if i % 5 == 4:
            tb.sync()
    surv = case["survivors"]
    assert tb.num_trajectories == len(surv) and len(tb) == int(case["transitions"])
    assert np.array_equal(tb.metrics, case["metrics"])
    data = tb.get_all()
    want = dict(observations="obs", next_observations="obs_next", rewards="rew", costs="cost", terminals="terminated",
                timeouts="truncated")
    for k, src in want.items():
        assert np.array_equal(data[k], np.concatenate([eps[e][src] for e in surv])), k
    assert np.array_equal(data["actions"], np.concatenate([np.clip(eps[e]["act"], -1.0, 1.0) for e in surv]))
    c = tb.counters()
    assert c["episodes"] == len(surv) and c["refused_full"] == 0
    if name == "grid_twice":
        assert c["compactions"] >= 2
    tb.close(); eng.close()


@pytest.mark.parametrize("Do,Da", [(5, 3), (8, 2), (128, 16)])
def test_compaction_that_moves_every_episode_by_one_row(Do, Da):
    """drop a first episode of ONE row: every other episode moves down by one row -- 20 bytes of observations at obs_dim 5 (source
    and destination not congruent mod 16: dwords), 32 at obs_dim 8 (16-byte accesses), 8 and 1 for the float64 and byte columns --
    among them an episode of 200 rows (two jobs) and short ones (ragged heads and tails)"""
    eng = make_engine("ppo_fused", Do, Da, env_num=2)
    arch = archive(eng, max_rows=600, max_episode_len=256)
    sc = Script(Do, Da, seed=5)
    zero = np.array([0])
    for n in (1, 7, 9, 200, 3, 1, 33):
        for t in range(n):
            sc.push(eng, zero, [False], [t == n - 1])
    ids = assert_export(arch, sc.done, Do, Da)
    arch.keep(ids[1:]); sc.done = sc.done[1:]
    assert_export(arch, sc.done, Do, Da)
    order = [3, 0, 5, 1, 4, 2]                           # and a permutation: table order is the order given
    arch.keep(ids[1:][order]); sc.done = [sc.done[i] for i in order]
    assert_export(arch, sc.done, Do, Da)
    assert arch.counters()["compactions"] >= 2
    arch.close(); eng.close()


# ---------------------------------------------------------------- 5. plumbing
def _store_episodes(eng, source):
    """the finished episodes in a (not wrapped) store, as Script episodes, in completion order: the envs step in lock step from
    their first row, so an episode's end time is its last row's position in its sub-buffer"""
    idx = eng.sample0()
    rows = eng.store_read(idx)
    sub, _ = eng.store_geometry()
    out, cur = [], {}
    for j, slot in enumerate(idx):
        e, pos = int(slot) // sub, int(slot) % sub
        ep = cur.setdefault(e, dict(rows=[], rew=0.0, cost=0.0, source=source))
        ep["rows"].append((rows["obs"][j], rows["obs_next"][j], rows["act"][j], rows["rew"][j], rows["cost"][j],
                           bool(rows["terminated"][j]), bool(rows["truncated"][j])))
        ep["rew"] += float(rows["rew"][j]); ep["cost"] += float(rows["cost"][j])
        if rows["terminated"][j] or rows["truncated"][j]:
            out.append((pos, e, cur.pop(e)))
    return [ep for _, _, ep in sorted(out, key=lambda x: (x[0], x[1]))]


def test_native_collect_feeds_the_tap():
    """FastCollector's native collect (one library call per collect over the worker-process synthetic env, actor on the device):
    the export equals store_read of the same episodes for every column but `actions` (the store keeps the raw policy action)"""
    from fsrl_amd.agent import PPOLagAgent
    from fsrl_amd.data import FastCollector, HipVectorReplayBuffer, TrajectoryBuffer
    from fsrl_amd.env import ShmemVectorEnv
    env = ShmemVectorEnv(env_num=6, workers=2, obs_dim=8, act_dim=2, episode_len=19, seed=4)
    try:
        agent = PPOLagAgent(env, None, cost_limit=10, device="cuda:0", seed=2, hidden_sizes=(64, 64), training_num=6)
        agent.policy.train()
        eng = agent.policy.engine
        buf = HipVectorReplayBuffer(eng, 6 * 300, 6)
        col = FastCollector(agent.policy, env, buf, exploration_noise=True, device_actor=True, native_loop=True)
        tb = TrajectoryBuffer(col, max_trajectory=100, max_episode_len=32)
        assert col.traj_buffer is tb
        stats = col.collect(n_episode=10)               # 6 episodes end at step 19, two envs are dropped, 4 more end at step 38
        assert stats["n/ep"] == 10 and tb.num_trajectories == 10 and len(tb) == 190
        want_eps = _store_episodes(eng, 0)
        want, got = expected(want_eps, 8, 2), tb.get_all()
        for k in COLUMNS:
            if k != "actions":
                assert np.array_equal(got[k], want[k]), k
        space = agent.policy.action_space
        lo, hi = np.asarray(space.low, F32), np.asarray(space.high, F32)
        clipped = np.clip(want["actions"], -1.0, 1.0)
        assert np.array_equal(got["actions"], lo + (hi - lo) * (clipped + 1.0) / 2.0)       # map_env_action's float32 expression
        assert np.array_equal(tb.metrics[:, 0], [ep["rew"] for ep in want_eps])
        assert tb.counters()["abandoned"] == 0
        tb.close(); eng.close()
    finally:
        env.close()


def test_group_collector_feeds_one_buffer_from_three_seeds(tmp_path):
    """three grouped PPO-Lag seeds (fsrl_group_collect_step pushes per member) into ONE buffer: every episode is whole and carries
    its source"""
    from fsrl_amd.agent import PPOLagAgent
    from fsrl_amd.data import FastCollector, GroupCollector, HipVectorReplayBuffer, TrajectoryBuffer
    from fsrl_amd.env import SyntheticSafetyVectorEnv
    from fsrl_amd.policy import PolicyGroup
    from fsrl_amd.utils import BaseLogger
    envs, ep_len = (5, 12, 3), (30, 17, 41)
    agents, cols = [], []
    for s, (e, L) in enumerate(zip(envs, ep_len)):
        env = SyntheticSafetyVectorEnv(env_num=e, obs_dim=8, act_dim=2, episode_len=L, seed=s)
        ag = PPOLagAgent(env, BaseLogger(str(tmp_path / f"g{s}"), name=f"g{s}"), cost_limit=10.0, device="cuda:0", seed=s,
                         hidden_sizes=(128, 128), training_num=e)
        ag.policy.train()
        agents.append(ag); cols.append(FastCollector(ag.policy, env, HipVectorReplayBuffer(ag.policy.engine, None, e), device_actor=True))
    tb = TrajectoryBuffer(max_trajectory=1000, max_episode_len=64)
    assert [tb.attach(c) for c in cols] == [0, 1, 2]
    group = PolicyGroup([ag.policy for ag in agents])
    stats = GroupCollector(group, cols).collect(n_episode=7)
    assert [s["n/ep"] for s in stats] == [7, 7, 7] and tb.num_trajectories == 21
    data, lengths, sources = tb.get_all(), tb.lengths, tb.sources
    assert sorted(sources.tolist()) == [0] * 7 + [1] * 7 + [2] * 7
    assert lengths.tolist() == [ep_len[s] for s in sources]
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    for s in range(3):
        want = _store_episodes(agents[s].policy.engine, s)
        mine = [i for i in range(21) if sources[i] == s]
        assert len(want) == len(mine) == 7
        for i, ep in zip(mine, want):                   # per source the order is the completion order
            sl = slice(starts[i], starts[i] + lengths[i])
            w = expected([ep], 8, 2)
            for k in ("observations", "next_observations", "rewards", "costs", "terminals", "timeouts"):
                assert np.array_equal(data[k][sl], w[k]), (s, k)
            assert not (data["terminals"][sl] | data["timeouts"][sl])[:-1].any()
            assert tb.metrics[i, 0] == ep["rew"] and tb.metrics[i, 1] == ep["cost"]
    group.close(); tb.close()
    for ag in agents:
        ag.policy.engine.close()


def test_attach_refusals_and_destruction_in_either_order():
    from fsrl_amd.engine import TrajArchive
    a, b = make_engine("ppo_fused", 5, 3), make_engine("ppo_fused", 5, 3, seed=1)
    other = make_engine("ppo_fused", 8, 3)
    arch = archive(a)
    with pytest.raises(AssertionError, match="at most one"):
        arch.attach(a)
    with pytest.raises(AssertionError, match="obs_dim"):
        arch.attach(other)
    other.close()
    assert arch.attach(b) == 1                          # a second context of the same shape feeds the same archive
    sa, sb = Script(5, 3, seed=1, source=0), Script(5, 3, seed=2, source=1)
    ids = np.arange(3)
    la, lb = Lengths([[4], [6], [9]]), Lengths([[5], [5], [3]])
    for t in range(10):
        sa.push(a, ids, *la.step(ids))
        sb.push(b, ids, *lb.step(ids))
    # a context destroyed before the archive detaches itself: what it had finished is archived, the archive lives on
    a.close()
    for t in range(10):
        sb.push(b, ids, *lb.step(ids))
    arch.flush()
    order, src = arch.episodes()[0], arch.episodes()[4]
    assert sorted(src.tolist()) == [0] * len(sa.done) + [1] * len(sb.done)
    got = arch.export()
    rows_b = expected(sb.done, 5, 3)
    mask = np.repeat(src == 1, arch.episodes()[1])
    for k in COLUMNS:
        assert np.array_equal(got[k][mask], rows_b[k]), k
    # the archive destroyed first leaves the context untapped: pushes go on, a new archive can be attached
    arch.close()
    for t in range(5):
        sb.push(b, ids, *lb.step(ids))
    arch2 = TrajArchive(b, 256, 32, 16)
    assert arch2.attach(b) == 0
    arch2.detach(b)
    with pytest.raises(AssertionError, match="does not feed"):
        arch2.detach(b)
    arch2.close(); b.close()


def test_a_tap_changes_nothing_in_the_context_it_is_on():
    """the same pushes and the same update on three twins -- never tapped; tapped for the first half, then detached; tapped
    throughout: identical train_state() bytes before the update (the archive is no part of it), identical parameters and stats
    after it"""
    Do, Da, E, T = 8, 2, 4, 60
    rng = np.random.default_rng(0)
    obs = rng.standard_normal((T + 1, E, Do)).astype(F32); act = (0.3 * rng.standard_normal((T, E, Da))).astype(F32)
    rew = rng.normal(0.5, 0.5, (T, E)); cost = (rng.random((T, E)) < 0.1).astype(F64)
    trunc = np.zeros((T, E), bool); trunc[19::20] = True
    term = np.zeros((T, E), bool)
    perms = [rng.permutation(T * E) for _ in range(2)]
    ids = np.arange(E)
    results = []
    for mode in ("never", "detached", "tapped"):
        eng = make_engine("ppo_fused", Do, Da, env_num=E, buffer_size=E * T, seed=9)
        arch = archive(eng, max_episode_len=32) if mode != "never" else None
        for t in range(T):
            if t == T // 2 and mode == "detached":
                arch.detach(eng)
            eng.push(ids, obs[t], act[t], rew[t], cost[t], term[t], trunc[t], obs[t + 1])
        blob = eng.train_state()
        stats, _ = eng.ppo_update(np.array([0.5]), 1.0 / 1.5, 64, 2, perms=perms)
        results.append((blob, eng.get_params(), np.array(stats)))
        if mode == "tapped":
            arch.flush()
            assert arch.counters()["committed"] == 3 * E
        if arch is not None:
            arch.close()
        eng.close()
    for blob, params, stats in results[1:]:
        assert blob == results[0][0]
        assert np.array_equal(params, results[0][1]) and np.array_equal(stats, results[0][2])
