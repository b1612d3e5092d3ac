"""The replay agents' collect group on the host (no GPU): the seven fsrl_collect_group_* symbols in the header, the cross-compiled
library and the ctypes table; the RAW instantiations of actor_group_resident_kernel in the gfx950 code object (no spills, no
scratch); and GroupCollector over a stub with EngineCollectGroup's interface and replay-style collectors (exploration_noise=True):
per member the calls FastCollector._collect_fused makes."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

from fsrl_amd.data import FastCollector, GroupCollector
from fsrl_amd.env import SyntheticSafetyVectorEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "fsrl_amd", "libfsrl_hip.so")
SYMBOLS = ("fsrl_collect_group_create", "fsrl_collect_group_destroy", "fsrl_collect_group_step",
           "fsrl_collect_group_actor_set_resident", "fsrl_collect_group_actor_resident_stats", "fsrl_collect_group_actor_release")


def test_header_library_and_ctypes_table_agree_on_the_collect_group():
    from fsrl_amd import _lib
    src = open(os.path.join(ROOT, "include", "fsrl_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(fsrl_collect_group[a-z0-9_]*)\s*\(", src))
    assert declared == set(SYMBOLS)
    assert re.search(r"typedef struct fsrl_collect_group fsrl_collect_group;", src)       # the seventh name: the handle's type
    lib = _lib.load()
    for s in SYMBOLS:
        assert hasattr(lib, s), f"{s} is not exported"
        assert s in _lib.SIGNATURES, f"{s} has no ctypes signature"
    # the step takes what fsrl_group_collect_step takes, argument for argument
    assert _lib.SIGNATURES["fsrl_collect_group_step"] == _lib.SIGNATURES["fsrl_group_collect_step"]
    for a, b in (("create", "create"), ("destroy", "destroy"), ("actor_set_resident", "actor_set_resident"),
                 ("actor_resident_stats", "actor_resident_stats"), ("actor_release", "actor_release")):
        assert _lib.SIGNATURES["fsrl_collect_group_" + a] == _lib.SIGNATURES["fsrl_group_" + b]


def test_raw_group_kernel_is_in_the_code_object_without_spills():
    if not os.path.exists(LIB):
        pytest.fail("libfsrl_hip.so is not built (fsrl_amd/csrc/build.sh cross-compiles it without a GPU)")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import sonotes
    notes = sonotes.kernel_notes(LIB)
    fam = {n: k for n, k in notes.items() if "actor_group_resident_kernel" in n}
    # template <int H, bool RAW>: ...ILi<H>ELb<RAW>E...
    for H in (64, 128, 256):
        raw = [k for n, k in fam.items() if f"ILi{H}ELb1E" in n]
        onp = [k for n, k in fam.items() if f"ILi{H}ELb0E" in n]
        assert len(raw) == 1, (H, sorted(fam))
        assert len(onp) == 1, (H, sorted(fam))
        assert raw[0]["vgpr_spill_count"] == 0 and raw[0]["private_segment_fixed_size"] == 0, (H, raw[0])
        assert onp[0]["vgpr_spill_count"] == 0 and onp[0]["private_segment_fixed_size"] == 0, (H, onp[0])
        assert raw[0]["max_flat_workgroup_size"] == 4 * H


def test_engine_collect_group_has_engine_groups_collect_interface():
    from fsrl_amd.engine import EngineCollectGroup, EngineGroup
    for name in ("collect_step", "collect_step_outputs", "actor_set_resident", "actor_release", "actor_resident_stats", "close"):
        assert inspect.signature(getattr(EngineCollectGroup, name)) == inspect.signature(getattr(EngineGroup, name)), name
    # one staging implementation, not two
    assert EngineCollectGroup.collect_step is EngineGroup.collect_step


# ---------------------------------------------------------------------------------------------------- GroupCollector over a stub
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


class _StubCollectGroup:
    """EngineCollectGroup's interface over stub engines: no `group` attribute (GroupCollector takes the object itself)"""

    def __init__(self, engines):
        self.engines = engines
        self.n_calls = self.n_release = 0
        self._last = None

    def collect_step(self, prevs, obs_acts, deterministic=False, bound_method=1, low=None, high=None):
        self.n_calls += 1
        Da = self.engines[0].Da
        out = []
        for i, (e, p, o) in enumerate(zip(self.engines, prevs, obs_acts)):
            if p is None and o is None:            # a member with no rows: the library does nothing for it
                out.append((np.zeros((0, Da), np.float32), np.zeros((0, Da), np.float32), np.zeros(0), np.zeros(0, np.int32)))
            else:
                out.append(e.collect_step(p, o, deterministic, bound_method, None if low is None else low[i],
                                          None if high is None else high[i]))
        return out

    def collect_step_outputs(self):
        raise AssertionError("GroupCollector does not read ptr / ep_idx")

    def actor_set_resident(self, on=True, idle_timeout_us=0.0):
        pass

    def actor_resident_stats(self):
        return dict(launches=0, requests=self.n_calls, live=False)

    def actor_release(self):
        self.n_release += 1

    def close(self):
        pass


class _StubBuffer:
    def __init__(self, engine):
        self.engine, self.buffer_num = engine, engine.env_num
        self._sizes = np.zeros(engine.env_num, np.int64)

    def sync_sizes(self):
        self._sizes[:] = self.engine.store_sizes()


class _StubReplayPolicy:
    """a replay agent's policy as the collector sees it: training mode, tanh-squashed actions scaled into the env's box"""

    def __init__(self, engine, Da):
        self.engine = engine
        self._deterministic_eval, self.training = True, True
        self.action_space = _Box(-2.0 * np.ones(Da), 3.0 * np.ones(Da))
        self.action_bound_method, self.action_scaling = "clip", True
        self.n_drain = 0

    def _drain(self):                              # the replay policies' statistics ring: emptied before a collect
        self.n_drain += 1

    def exploration_noise(self, act, batch):
        raise AssertionError("the device actor draws the noise: the host path must not run")


ENVS, EP_LEN, Do, Da = (5, 12, 3), (9, 14, 23), 4, 2


def _collectors():
    cols = []
    for s, (e, L) in enumerate(zip(ENVS, EP_LEN)):
        eng = _StubEngine(e, Da)
        env = SyntheticSafetyVectorEnv(env_num=e, obs_dim=Do, act_dim=Da, episode_len=L, seed=s)
        cols.append(FastCollector(_StubReplayPolicy(eng, Da), env, _StubBuffer(eng), exploration_noise=True, device_actor=True))
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
def test_group_collector_over_a_collect_group_makes_each_members_fused_collector_calls(n_episode):
    from fsrl_amd.engine import EngineCollectGroup
    for name in ("collect_step", "collect_step_outputs", "actor_set_resident", "actor_release", "actor_resident_stats", "close"):
        assert callable(getattr(EngineCollectGroup, name)) and callable(getattr(_StubCollectGroup, name))    # the stub stands for it
    solo, grp = _collectors(), _collectors()
    group = _StubCollectGroup([c.policy.engine for c in grp])
    gc = GroupCollector(group, grp)
    assert gc.group is group
    ns = [n_episode] * 3 if np.isscalar(n_episode) else list(n_episode)
    for rnd in range(2):                                       # the second collect starts from the envs the first one left behind
        got = gc.collect(n_episode)
        want = [c.collect(n) for c, n in zip(solo, ns)]
        assert got == want, rnd
        for x, y in zip(solo, grp):
            _same_calls(x.policy.engine.calls, y.policy.engine.calls)
            assert (x.collect_step, x.collect_episode) == (y.collect_step, y.collect_episode)
            assert np.array_equal(x.buffer._sizes, y.buffer._sizes) and np.array_equal(x._obs, y._obs)
            assert x.policy.n_drain == y.policy.n_drain == rnd + 1
    longest = max(len(c.policy.engine.calls) for c in grp)
    assert group.n_calls == longest and group.n_release == 2
    assert len({len(c.policy.engine.calls) for c in grp}) > 1
