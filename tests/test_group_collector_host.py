"""GroupCollector's bookkeeping on the host (no GPU): stub engines stand in for the library.  Per member the lock-step loop must make
the calls FastCollector._collect_fused makes -- the same rows stored in the same order, the same observations acted on, the same
episode accounting -- while members with different episode lengths finish at different vector steps."""
import numpy as np
import pytest

from fsrl_amd.data import FastCollector, GroupCollector
from fsrl_amd.env import SyntheticSafetyVectorEnv


class _Box:
    def __init__(self, low, high):
        self.low, self.high = np.asarray(low, np.float32), np.asarray(high, np.float32)


class _StubEngine:
    """Engine.collect_step's interface: actions are a fixed function of the observations; every call is recorded"""

    def __init__(self, env_num, Da):
        self.env_num, self.Da = env_num, Da
        self.calls = []
        self._rew, self._len = np.zeros(env_num), np.zeros(env_num, np.int32)
        self._sizes = np.zeros(env_num, np.int64)

    def collect_step(self, prev, obs_act, deterministic=False, bound_method=1, low=None, high=None):
        k, er, el = 0, np.zeros(0), np.zeros(0, np.int32)
        if prev is not None:
            ids, obs, act, rew, cost, term, trunc, nxt = prev
            k = len(ids)
            er, el = np.zeros(k), np.zeros(k, np.int32)
            for j, e in enumerate(ids):
                self._rew[e] += rew[j]; self._len[e] += 1; self._sizes[e] += 1
                if term[j] or trunc[j]:
                    er[j], el[j] = self._rew[e], self._len[e]
                    self._rew[e], self._len[e] = 0.0, 0
        oa = np.zeros((0, 0), np.float32) if obs_act is None else np.asarray(obs_act, np.float32)
        act = np.tanh(oa[:, :self.Da] * 0.7 + 0.1) if len(oa) else np.zeros((0, self.Da), np.float32)
        env_act = np.clip(act, -1, 1) if bound_method == 1 else act
        if low is not None and len(oa):
            env_act = low + (high - low) * (env_act + 1) / 2
        self.calls.append((None if prev is None else tuple(np.array(x, copy=True) for x in prev), oa.copy(), bool(deterministic),
                           int(bound_method)))
        return act.astype(np.float32), env_act.astype(np.float32), er, el

    def store_sizes(self):
        return self._sizes.copy()

    def actor_release(self):
        pass


class _StubGroup:
    def __init__(self, engines):
        self.engines = engines
        self.n_calls = self.n_release = 0

    def collect_step(self, prevs, obs_acts, deterministic=False, bound_method=1, low=None, high=None):
        self.n_calls += 1
        out = []
        for i, (e, p, o) in enumerate(zip(self.engines, prevs, obs_acts)):
            if p is None and o is None:            # a member with no rows: the library does nothing for it
                out.append((np.zeros((0, Da), np.float32), np.zeros((0, Da), np.float32), np.zeros(0), np.zeros(0, np.int32)))
            else:
                out.append(e.collect_step(p, o, deterministic, bound_method, None if low is None else low[i],
                                          None if high is None else high[i]))
        return out

    def actor_release(self):
        self.n_release += 1


class _StubBuffer:
    def __init__(self, engine):
        self.engine, self.buffer_num = engine, engine.env_num
        self._sizes = np.zeros(engine.env_num, np.int64)

    def sync_sizes(self):
        self._sizes[:] = self.engine.store_sizes()


class _StubPolicy:
    def __init__(self, engine, Da):
        self.engine = engine
        self._deterministic_eval, self.training = True, True
        self.action_space = _Box(-2.0 * np.ones(Da), 3.0 * np.ones(Da))
        self.action_bound_method, self.action_scaling = "clip", True


ENVS, EP_LEN, Do, Da = (5, 12, 3), (9, 14, 23), 4, 2


def _collectors():
    cols = []
    for s, (e, L) in enumerate(zip(ENVS, EP_LEN)):
        eng = _StubEngine(e, Da)
        env = SyntheticSafetyVectorEnv(env_num=e, obs_dim=Do, act_dim=Da, episode_len=L, seed=s)
        cols.append(FastCollector(_StubPolicy(eng, Da), env, _StubBuffer(eng), device_actor=True))
    return cols


def _same_calls(x, y):
    assert len(x) == len(y)
    for cx, cy in zip(x, y):
        assert (cx[0] is None) == (cy[0] is None)
        if cx[0] is not None:
            for u, v in zip(cx[0], cy[0]):
                assert np.array_equal(u, v)
        assert np.array_equal(cx[1], cy[1]) and cx[2:] == cy[2:]


@pytest.mark.parametrize("n_episode", [1, 7, (4, 13, 2)])
def test_group_collector_makes_each_members_fused_collector_calls(n_episode):
    solo, grp = _collectors(), _collectors()
    group = _StubGroup([c.policy.engine for c in grp])
    gc = GroupCollector(group, grp)
    ns = [n_episode] * 3 if np.isscalar(n_episode) else list(n_episode)
    for rnd in range(2):                                       # the second collect starts from the envs the first one left behind
        got = gc.collect(n_episode)
        want = [c.collect(n) for c, n in zip(solo, ns)]
        assert got == want, rnd
        for x, y in zip(solo, grp):
            _same_calls(x.policy.engine.calls, y.policy.engine.calls)
            assert (x.collect_step, x.collect_episode) == (y.collect_step, y.collect_episode)
            assert np.array_equal(x.buffer._sizes, y.buffer._sizes) and np.array_equal(x._obs, y._obs)
    # lock step: one group call per vector step of the longest member (+ the first actor call), the kernel released per collect
    longest = max(len(c.policy.engine.calls) for c in grp)
    assert group.n_calls == longest and group.n_release == 2
    # members finished at different vector steps: the shorter ones sat out the tail with no rows
    assert len({len(c.policy.engine.calls) for c in grp}) > 1


def test_group_collector_checks_its_members():
    cols = _collectors()
    with pytest.raises(AssertionError):
        GroupCollector(_StubGroup([c.policy.engine for c in cols[::-1]]), cols)
