"""A whole lock-step collect of a group over worker-process envs in one library call (fsrl_group_collect_episodes /
fsrl_collect_episodes_group, fsrl_amd/csrc/host_group_episodes.inc; GroupCollector(native_loop=True) over ShmemVectorEnv members).
Every comparison is against a twin set of agents with the same seeds, collected by GroupCollector(native_loop=False) -- the
interpreted loop -- over identical envs, and the bar is bit-equality: both runs make the same library calls per member in the same
order, and the workers of a member's env see the same commands.  Env counts 17 / 3 / 4 (17 rows cross a 16-row tile of the group's
actor kernel), episode lengths 5 / 7 / 4, n_episode 20 / 6 / 2 (more episodes than envs, surplus envs dropped, fewer episodes than envs),
member 1's env with a single worker (one lane).  A set has at most 5 worker processes and the twin sets of a test live one after the
other; the workers never open the GPU."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ENVS, LENS, WORKERS = (17, 3, 4), (5, 7, 4), (2, 1, 2)
N_EP = ((20, 6, 2), (3, 5, 4))                  # two collects: the second one shows where every member's noise stream stands


class _NoNative:
    """a worker-process env that does not offer the native loop"""

    def __init__(self, env):
        self._env = env

    def __len__(self):
        return len(self._env)

    def __getattr__(self, name):
        if name == "native_desc":
            raise AttributeError(name)
        return getattr(self._env, name)


class _Set:
    """k members of one kind over ShmemVectorEnv: agents, envs, collectors, the group and its GroupCollector"""

    def __init__(self, kind, native, k=3, det=False, hide_native=None):
        from fsrl_amd.agent import CPOAgent, DDPGLagAgent, PPOLagAgent, SACLagAgent
        from fsrl_amd.data import FastCollector, GroupCollector, HipVectorReplayBuffer
        from fsrl_amd.engine import EngineCollectGroup
        from fsrl_amd.env import ShmemVectorEnv
        from fsrl_amd.policy import PolicyGroup
        Agent = {"ppol": PPOLagAgent, "ppol_layered": PPOLagAgent, "sacl": SACLagAgent, "ddpgl": DDPGLagAgent, "cpo": CPOAgent}[kind]
        hs = (32, 24, 16) if kind == "ppol_layered" else (64, 64)
        self.envs, self.agents, self.cols = [], [], []
        self.group = self.cgroup = None
        try:
            for s in range(k):
                env = ShmemVectorEnv(env_num=ENVS[s], workers=WORKERS[s], obs_dim=8, act_dim=2, episode_len=LENS[s], seed=20 + s)
                self.envs.append(env)
                assert env.n_lanes == (2 if WORKERS[s] == 2 else 1)
                ag = Agent(env, None, cost_limit=10, device="cuda:0", seed=1 + s, hidden_sizes=hs, training_num=ENVS[s])
                self.agents.append(ag)
                if det:
                    ag.policy.eval()
                else:
                    ag.policy.train()
                buf = HipVectorReplayBuffer(ag.policy.engine, None, ENVS[s])
                cenv = _NoNative(env) if hide_native == s else env
                self.cols.append(FastCollector(ag.policy, cenv, buf, exploration_noise=True, device_actor=True))
            self.engines = [a.policy.engine for a in self.agents]
            if kind in ("ppol", "ppol_layered"):
                self.group = PolicyGroup([a.policy for a in self.agents])
                self.lock = self.group.group
            else:
                self.cgroup = self.lock = EngineCollectGroup(self.engines)
            self.lock.actor_set_resident(True, idle_timeout_us=2.0e5)     # the launch counts below do not depend on a slow env step
            self.py_steps, inner = 0, self.lock.collect_step              # step calls made from Python: none under the native loop

            def counted(*a, **kw):
                self.py_steps += 1
                return inner(*a, **kw)
            self.lock.collect_step = counted
            self.gcol = GroupCollector(self.group if self.group is not None else self.cgroup, self.cols, native_loop=native)
        except BaseException:
            self.close()
            raise

    def snapshot(self):
        out = []
        for c in self.cols:
            eng = c.policy.engine
            idx = eng.sample0()
            out.append(dict(idx=idx, rows=eng.store_read(idx), counters=(c.collect_step, c.collect_episode),
                            sizes=np.array(c.buffer._sizes), obs=np.array(c._obs)))
        return out

    def run(self, n_eps=N_EP):
        """the collects, and after each: the stats dicts, every member's store / counters / next observations, the actor's counters"""
        k = len(self.cols)
        out = []
        for ne in n_eps:
            stats = self.gcol.collect([x for x in ne[:k]])
            out.append(dict(stats=stats, members=self.snapshot(), actor=self.lock.actor_resident_stats(), py_steps=self.py_steps))
        return out

    def close(self):
        for g in (self.group, self.cgroup):
            if g is not None:
                g.close()
        for a in self.agents:
            a.policy.engine.close()
        for e in self.envs:
            e.close()


def _collects(kind, native, **kw):
    s = _Set(kind, native, **kw)
    try:
        return s.run()
    finally:
        s.close()


_RUNS = {}


def _cached(kind, native, **kw):
    key = (kind, native, tuple(sorted(kw.items())))
    if key not in _RUNS:
        _RUNS[key] = _collects(kind, native, **kw)
    return _RUNS[key]


def _twin(kind, **kw):
    """the interpreted loop's collects of a kind: computed once, shared, never changed"""
    return _cached(kind, False, **kw)


def _native(kind, **kw):
    return _cached(kind, True, **kw)


def _assert_same(got, want):
    assert len(got) == len(want)
    for rnd, (g, w) in enumerate(zip(got, want)):
        assert g["stats"] == w["stats"], rnd
        for i, (a, b) in enumerate(zip(g["members"], w["members"])):
            assert a["counters"] == b["counters"], (rnd, i)
            assert np.array_equal(a["sizes"], b["sizes"]) and np.array_equal(a["obs"], b["obs"]), (rnd, i)
            assert np.array_equal(a["idx"], b["idx"]), (rnd, i)
            assert len(a["idx"]) > 0
            for key in b["rows"]:
                assert np.array_equal(a["rows"][key], b["rows"][key]), (rnd, i, key)     # the second round: the actions after the first


def test_native_group_collect_is_the_interpreted_group_collect_bit_for_bit():
    want, got = _twin("ppol"), _native("ppol")
    assert [s["n/ep"] for s in got[0]["stats"]] == list(N_EP[0]) and [s["n/ep"] for s in got[1]["stats"]] == list(N_EP[1])
    # member 0: 17 envs finish at step 5, 3 of them go on to step 10; member 1: 3 envs x 2 episodes of 7; member 2: 2 of 4 envs start
    assert [s["n/st"] for s in got[0]["stats"]] == [17 * 5 + 3 * 5, 3 * 14, 2 * 4]
    _assert_same(got, want)
    # the native collect is one library call: no step call came from Python; the interpreted twin made 1 + 14 per first collect
    assert [g["py_steps"] for g in got] == [0, 0] and want[0]["py_steps"] == 15


@pytest.mark.parametrize("kind,k,det", [("ppol_layered", 2, False), ("sacl", 2, False), ("ddpgl", 2, False), ("cpo", 2, False),
                                        ("ppol", 3, True)])
def test_native_group_collect_of_every_kind_of_group(kind, k, det):
    """a layered PPO-Lag group (L + 2 launches per request), collect groups of SAC-Lag seeds with exploration noise, of DDPG-Lag
    seeds and of CPO seeds (the collect group TrustPolicyGroup runs beside), and eval mode (deterministic actions)"""
    got = _collects(kind, True, k=k, det=det)
    _assert_same(got, _twin(kind, k=k, det=det))
    assert got[-1]["py_steps"] == 0


def test_one_kernel_launch_serves_the_whole_native_collect():
    """fused group: the resident actor kernel is launched once per collect and ends with it.  Requests: the first actions, then one
    per vector step that leaves somebody rows to act on -- every one of the 14 vector steps (member 1's 2 x 7) but the last, after
    which nobody acts: 14, as under the interpreted loop."""
    want, got = _twin("ppol"), _native("ppol")
    a = got[0]["actor"]
    print("first collect:", a, "interpreted:", want[0]["actor"])
    assert a["launches"] == 1 and a["requests"] == 14 and a["live"] is False
    assert [g["actor"] for g in got] == [w["actor"] for w in want]
    assert got[1]["actor"]["launches"] == 2


def test_refusals_name_the_member_and_leave_the_envs_usable():
    from fsrl_amd.env import ShmemVectorEnv
    s = _Set("ppol", True)
    narrow = None
    try:
        narrow = ShmemVectorEnv(env_num=3, workers=1, obs_dim=6, act_dim=2, episode_len=7, seed=1)
        descs = [e.native_desc() for e in s.envs]
        readys = [np.arange(min(e, n)) for e, n in zip(ENVS, N_EP[0])]
        obs = [np.asarray(c._obs[:len(r)], np.float32) for c, r in zip(s.cols, readys)]
        for bad_descs, n_eps, what in (([descs[0], narrow.native_desc(), descs[2]], N_EP[0], "env shape"),
                                       (descs, (20, 0, 2), "n_episode"),
                                       ([descs[0], descs[0], descs[2]], N_EP[0], "listed twice")):
            with pytest.raises(AssertionError, match="member 1.*" + what) as ei:
                s.lock.collect_episodes(bad_descs, readys, obs, n_eps, False, 1, None, None)
            assert ei.value.failed_member == 1
        assert s.lock.actor_resident_stats()["launches"] == 0        # nothing was launched, nothing posted: the envs are as they were
        _assert_same(s.run(), _twin("ppol"))
    finally:
        s.close()
        if narrow is not None:
            narrow.close()


def test_a_member_without_a_native_env_takes_the_interpreted_loop():
    got = _collects("ppol", True, hide_native=1)
    _assert_same(got, _twin("ppol"))
    assert got[0]["py_steps"] == 15


def test_a_dead_worker_fails_the_call_with_its_member_and_spares_the_other_envs():
    """member 1's only worker is killed between two collects (a host process; nothing on the GPU fails): the next native collect
    raises and names member 1, the library has ended the group's resident actor itself, member 1's env refuses every later command,
    and the envs of members 0 and 2 -- whose commands were waited for -- complete a native collect of their own."""
    from fsrl_amd._lib import FsrlHipError
    s = _Set("ppol", True)
    try:
        s.gcol.collect(list(N_EP[0]))
        s.envs[1]._procs[0].terminate(); s.envs[1]._procs[0].join(5)
        # GroupCollector.collect releases the actor in a `finally`, which would hide who ended it: look just before that release
        live_at_release, release = [], s.lock.actor_release
        s.lock.actor_release = lambda: (live_at_release.append(s.lock.actor_resident_stats()["live"]), release())
        t0 = time.time()
        with pytest.raises(FsrlHipError, match="member 1.*worker") as ei:
            s.gcol.collect(list(N_EP[0]))
        assert ei.value.failed_member == 1
        assert time.time() - t0 < 10.0
        assert live_at_release == [False] and s.lock.actor_resident_stats()["live"] is False
        assert getattr(s.envs[1], "_broken", None) and not getattr(s.envs[0], "_broken", None) and not getattr(s.envs[2], "_broken", None)
        with pytest.raises(RuntimeError, match="unusable"):
            s.envs[1].reset()
        for i in (0, 2):
            s.cols[i].reset_env()
            st = s.cols[i].collect(n_episode=3)                      # FastCollector's native loop over the same env
            assert st["n/ep"] == 3 and st["n/st"] == 3 * LENS[i]
    finally:
        s.close()
