"""k seeds' whole collects in one looping launch (fsrl_collect_device_group, GroupDeviceCollector) against the solo call.

The oracle is fsrl_collect_device on an ungrouped TWIN context: same parameters, same store geometry, same env seed.  A member's
grouped collect runs the same device code with the same Philox counters, so everything is compared bit for bit, in training mode
too: the store's rows in sample(0) order, the sub-buffers' sizes and books (what one more push reports), the env's state, steps and
reset ordinals, the statistics and the store's version.  Shapes are the helpers' small ones (tests/test_gpu_devcollect.py,
tests/test_gpu_devcollect_replay.py): hidden 64 unless stated, episodes cut at 7 steps, sub-buffers of 6 - 12 rows that wrap."""
import numpy as np
import pytest

import test_gpu_devcollect as on
import test_gpu_devcollect_replay as rp

pytestmark = pytest.mark.gpu
F32 = np.float32
STAT_KEYS = ("steps", "total_cost", "terminated", "truncated", "ep_rews", "ep_lens")


def snapshot(eng, env):
    idx, rows = on.store_rows(eng) if len(eng) else (np.zeros(0, np.int64), None)
    return dict(idx=idx, rows=rows, sizes=eng.store_sizes().copy(), n=len(eng), state=env.get_state(), version=eng.store_version())


def assert_same_snapshot(a, b, what):
    assert np.array_equal(a["idx"], b["idx"]) and (a["rows"] is None or on.same_rows(a["rows"], b["rows"])), what + ": store rows"
    assert np.array_equal(a["sizes"], b["sizes"]) and a["n"] == b["n"], what + ": sub-buffer sizes"
    assert all(np.array_equal(x, y) for x, y in zip(a["state"], b["state"])), what + ": env state, steps, ordinals"
    assert a["version"] == b["version"], (what + ": store_version", a["version"], b["version"])


def assert_same_stats(a, b, what):
    for k in STAT_KEYS:
        assert np.array_equal(a[k], b[k]), (what, k, a[k], b[k])


def books(eng):
    """the books of sub-buffer 0 as one more push reports them: slot, running episode return / length / start"""
    Do, Da = eng.cfg.obs_dim, eng.cfg.act_dim
    return eng.push(np.array([0]), np.zeros((1, Do), F32), np.zeros((1, Da), F32), np.array([0.25]), np.array([1.0]), np.array([True]),
                    np.array([False]), np.ones((1, Do), F32))


def close(*xs):
    for x in xs:
        x.close()


def group_collect(engs, envs, n_eps, **kw):
    from fsrl_amd.engine import collect_device_group
    return collect_device_group(engs, [v._h for v in envs], n_eps, **kw)


# ------------------------------------------------------------------------------------------------ 1. on-policy members of an EngineGroup
def test_onpolicy_members_of_an_update_group_equal_their_twins():
    """env_num 1 / 17 / 64, n_episode 3 / 25 / 70, 8 vector steps per launch: the members finish in different launches and the
    finished workgroups are launched again idle; then new parameters on everyone and a second collect"""
    onpolicy_members_equal_their_twins(64)


def onpolicy_members_equal_their_twins(H):
    from fsrl_amd.engine import EngineGroup
    ns, n_eps = (1, 17, 64), (3, 25, 70)
    lows = np.array([[-2.0, -0.5], [-1.0, -1.5], [-0.25, -3.0]], F32)
    highs = np.array([[0.5, 1.0], [2.0, 0.75], [1.5, 0.5]], F32)
    mem = [on.make("lin8", n, H=H, rows_per_env=6, seed=3 + i) for i, n in enumerate(ns)]
    twin = [on.make("lin8", n, H=H, rows_per_env=6, seed=3 + i) for i, n in enumerate(ns)]
    group = EngineGroup([e for e, _ in mem])
    for _, v in mem + twin:
        v.reset()
    for rnd in range(2):
        if rnd == 1:        # stale weights, or a launch that is not behind the members' streams, would show here
            for i in range(3):
                theta = (0.3 * np.random.default_rng(20 + i).standard_normal(mem[i][0].n_params)).astype(F32)
                mem[i][0].set_params(theta); twin[i][0].set_params(theta)
        res = group_collect([e for e, _ in mem], [v for _, v in mem], n_eps, deterministic=False, bound_method=1, lows=lows, highs=highs,
                            max_steps_per_launch=8)
        launches = []
        for i, (e, v) in enumerate(twin):
            solo = e.collect_device(v._h, n_eps[i], deterministic=False, bound_method=1, low=lows[i], high=highs[i], max_steps_per_launch=8)
            launches.append(solo["launches"])
            assert_same_stats(res[i], solo, f"round {rnd} member {i}")
            assert len(res[i]["ep_rews"]) == n_eps[i]
            assert_same_snapshot(snapshot(*mem[i]), snapshot(*twin[i]), f"round {rnd} member {i}")
        # the members finish in different launches; the call goes on until the last one is finished
        assert min(launches) < max(launches) == res[0]["launches"], (launches, res[0]["launches"])
    for i in range(3):
        assert all(np.array_equal(x, y) for x, y in zip(books(mem[i][0]), books(twin[i][0]))), f"member {i}: books"
        assert mem[i][0].store_sizes().max() == 6           # the sub-buffers wrapped
    for i in range(3):          # the members' own solo call stays refused
        with pytest.raises(AssertionError, match="grouped contexts"):
            mem[i][0].collect_device(mem[i][1]._h, 1)
    close(*[v for _, v in mem + twin]); group.close(); close(*[e for e, _ in mem + twin])


# ------------------------------------------------------------------------------------------------ 2. replay heads
@pytest.mark.parametrize("agent,kind", [("sacl", "lin33"), ("ddpgl", "lin20"), ("cvpo", "lin8")])
def test_replay_members_equal_their_twins(agent, kind):
    """SAC-Lag members of an EngineSacGroup with prioritised replay on (leaves, max_prio, min_prio and the root too), DDPG-Lag
    members of an EngineCollectGroup, CVPO members of an EngineCvpoGroup; k = 2, unequal env_num and n_episode, 9-row sub-buffers"""
    replay_members_equal_their_twins(agent, kind, 64)


def replay_members_equal_their_twins(agent, kind, H):
    from fsrl_amd.engine import EngineCollectGroup, EngineCvpoGroup, EngineSacGroup
    ns, n_eps = (5, 17), (12, 20)
    per = (0.6, 0.4) if agent == "sacl" else None
    mem = [rp.make(agent, kind, n, H=H, rows_per_env=9, seed=5 + i, per=per) for i, n in enumerate(ns)]
    twin = [rp.make(agent, kind, n, H=H, rows_per_env=9, seed=5 + i, per=per) for i, n in enumerate(ns)]
    Group = {"sacl": EngineSacGroup, "ddpgl": EngineCollectGroup, "cvpo": EngineCvpoGroup}[agent]
    group = Group([e for e, _ in mem])
    for _, v in mem + twin:
        v.reset()
    for rnd, cut in enumerate((5, 0)):
        res = group_collect([e for e, _ in mem], [v for _, v in mem], n_eps, deterministic=False, bound_method=1, max_steps_per_launch=cut)
        for i, (e, v) in enumerate(twin):
            solo = e.collect_device(v._h, n_eps[i], deterministic=False, bound_method=1, max_steps_per_launch=cut)
            assert_same_stats(res[i], solo, f"{agent} round {rnd} member {i}")
            assert_same_snapshot(snapshot(*mem[i]), snapshot(*twin[i]), f"{agent} round {rnd} member {i}")
            if per:
                (lm, mxm, mnm, totm), (lt, mxt, mnt, tott) = mem[i][0].per_state(), e.per_state()
                assert np.array_equal(lm, lt) and (mxm, mnm, totm) == (mxt, mnt, tott), f"round {rnd} member {i}: the sum tree"
                assert np.count_nonzero(lm) == len(mem[i][0]) > 0
        if rnd == 0:
            assert res[0]["launches"] > 1
    for i in range(2):
        assert mem[i][0].store_sizes().max() == 9           # the sub-buffers wrapped
        assert all(np.array_equal(x, y) for x, y in zip(books(mem[i][0]), books(twin[i][0]))), f"member {i}: books"
    with pytest.raises(AssertionError, match="grouped contexts"):
        mem[0][0].collect_device(mem[0][1]._h, 1)
    close(*[v for _, v in mem + twin]); group.close(); close(*[e for e, _ in mem + twin])


# ------------------------------------------------------------------------------------------------ 3. the register-tight instantiation
def test_launch_cuts_change_nothing_at_256_wide():
    ns, n_eps = (17, 5), (20, 9)
    out = []
    for grouped, cut in ((True, 4), (True, 64), (False, 4), (False, 64)):
        pair = [on.make("pc", n, H=256, rows_per_env=12, seed=7 + i) for i, n in enumerate(ns)]
        for _, v in pair:
            v.reset()
        if grouped:
            res = group_collect([e for e, _ in pair], [v for _, v in pair], n_eps, deterministic=False, bound_method=1, max_steps_per_launch=cut)
        else:
            res = [e.collect_device(v._h, n_eps[i], deterministic=False, bound_method=1, max_steps_per_launch=cut) for i, (e, v) in enumerate(pair)]
        out.append((res, [snapshot(e, v) for e, v in pair]))
        close(*[v for _, v in pair]); close(*[e for e, _ in pair])
    assert out[0][0][0]["launches"] > 1 and out[1][0][0]["launches"] == 1
    for j in (1, 2, 3):
        for i in range(2):
            assert_same_stats(out[0][0][i], out[j][0][i], f"run {j} member {i}")
            assert_same_snapshot(out[0][1][i], out[j][1][i], f"run {j} member {i}")
    assert out[0][1][0]["rows"]["terminated"].sum() > 0 and out[0][1][0]["rows"]["cost"].sum() > 0


# ------------------------------------------------------------------------------------------------ 4. ordering against grouped updates
def test_collect_update_collect_equals_the_lock_step_path():
    """deterministic mode, where a device collect is the existing path bit for bit: group A collects with the grouped device call,
    group B with GroupCollector over FastCollector(device_actor=True) over DeviceVectorEnv.step; one grouped ppo_update in between"""
    from fsrl_amd.data import DeviceCollector, FastCollector, GroupCollector, GroupDeviceCollector, HipVectorReplayBuffer
    from fsrl_amd.engine import EngineGroup
    ns, n_eps = (5, 17), (6, 20)
    out = []
    for device in (True, False):
        pair = [on.make("lin8", n, rows_per_env=30, seed=3 + i) for i, n in enumerate(ns)]
        group = EngineGroup([e for e, _ in pair])
        cols = []
        for (e, v), n in zip(pair, ns):
            pol, buf = on.Pol(e, "clip", None), HipVectorReplayBuffer(e, n * 30, n)
            cols.append(DeviceCollector(pol, v, buf) if device else FastCollector(pol, v, buf, device_actor=True))
        gcol = GroupDeviceCollector(cols) if device else GroupCollector(group, cols)
        st1 = gcol.collect(n_eps)
        s1 = [on.store_rows(e) for e, _ in pair]
        upd, _ = group.ppo_update([[0.3], [0.2]], [1 / 1.3, 1 / 1.2], 32, 2, seed=5)
        st2 = gcol.collect(n_eps)
        s2 = [on.store_rows(e) for e, _ in pair]
        out.append((st1, st2, s1, s2, [np.asarray(u) for u in upd], [e.get_params() for e, _ in pair], [v.get_state() for _, v in pair]))
        close(*[v for _, v in pair]); group.close(); close(*[e for e, _ in pair])
    a, b = out
    theta0 = (0.3 * np.random.default_rng(7).standard_normal(a[5][0].size)).astype(F32)      # what on.make set
    assert a[0] == b[0] and a[1] == b[1]
    for i in range(2):
        for sa, sb in ((a[2][i], b[2][i]), (a[3][i], b[3][i])):
            assert np.array_equal(sa[0], sb[0]) and on.same_rows(sa[1], sb[1]), f"member {i}: store"
        assert np.array_equal(a[4][i], b[4][i]) and np.array_equal(a[5][i], b[5][i]), f"member {i}: update statistics / parameters"
        assert all(np.array_equal(x, y) for x, y in zip(a[6][i], b[6][i]))
        assert np.abs(a[5][i] - theta0).max() > 1e-5            # the second collect ran an updated actor


# ------------------------------------------------------------------------------------------------ 5. the collectors
def test_group_device_collector_and_the_delegating_group_collector():
    from fsrl_amd.data import DeviceCollector, FastCollector, GroupCollector, GroupDeviceCollector, HipVectorReplayBuffer
    from fsrl_amd.engine import EngineGroup
    ns, n_eps = (5, 17), (7, 20)

    def collectors(training):
        pair = [on.make("lin8", n, rows_per_env=40, seed=3 + i) for i, n in enumerate(ns)]
        cols = [DeviceCollector(on.Pol(e, "clip", (-1.5, 1.0), training=training), v, HipVectorReplayBuffer(e, n * 40, n), max_steps_per_launch=5)
                for (e, v), n in zip(pair, ns)]
        return pair, cols

    mem, mcols = collectors(True)
    twin, tcols = collectors(True)
    group = EngineGroup([e for e, _ in mem])
    gcol = GroupCollector(group, mcols)                          # every collector a DeviceCollector: delegates
    assert isinstance(gcol.device, GroupDeviceCollector) and gcol.device.max_steps_per_launch == 5
    stats = gcol.collect(n_eps)
    stats += GroupDeviceCollector(mcols, 5).collect(3)           # one count for every member
    want = [c.collect(n_episode=n) for c, n in zip(tcols, n_eps)] + [c.collect(n_episode=3) for c in tcols]
    assert stats == want
    assert set(stats[0]) == {"n/ep", "n/st", "rew", "len", "total_cost", "cost", "truncated", "terminated"}
    for i, (cm, ct) in enumerate(zip(mcols, tcols)):
        assert (cm.collect_step, cm.collect_episode) == (ct.collect_step, ct.collect_episode) and cm.collect_time > 0
        assert np.array_equal(cm.buffer._sizes, ct.buffer._sizes) and len(cm.buffer) == len(ct.buffer)
        assert_same_snapshot(snapshot(*mem[i]), snapshot(*twin[i]), f"member {i}")
    # a mix of device collectors and others
    fast = FastCollector(on.Pol(twin[1][0], "clip", (-1.5, 1.0)), twin[1][1], tcols[1].buffer, device_actor=True)
    with pytest.raises(AssertionError, match="mix of DeviceCollectors and other collectors"):
        GroupCollector(group, [mcols[0], fast])
    # members that disagree on deterministic
    mcols[1].policy.training = False
    with pytest.raises(AssertionError, match="agree on deterministic"):
        gcol.collect(2)
    close(*[v for _, v in mem + twin]); group.close(); close(*[e for e, _ in mem + twin])


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_name_the_member_and_the_reason_and_change_nothing():
    from fsrl_amd import _lib
    from fsrl_amd._lib import FsrlHipError
    from fsrl_amd.engine import TrajArchive
    a, b, c = on.make("lin8", 5, seed=3), on.make("lin8", 4, seed=4), on.make("lin8", 3, seed=5)
    for _, v in (a, b, c):
        v.reset()
    group_collect([a[0], b[0], c[0]], [a[1], b[1], c[1]], 4, bound_method=1)         # rows in every store
    everyone = [a, b, c]

    def refused(members, match, exc=AssertionError, n_eps=3, also=(), **kw):
        watch = everyone + list(also)
        before = [snapshot(e, v) for e, v in watch]
        with pytest.raises(exc, match=match):
            group_collect([e for e, _ in members], [v for _, v in members], n_eps, **kw)
        for (e, v), s in zip(watch, before):
            assert_same_snapshot(snapshot(e, v), s, match)

    refused([], "k 0: .* 1..16 members", n_eps=[])
    refused([a, b, a], "member 2: its context is listed twice")
    refused([a, (b[0], a[1])], "member 1: its device env is listed twice")
    refused([a, (b[0], c[1])], "member 1: the device env was created on another context")
    refused([a, b, c], "member 0: bound_method", bound_method=7)
    refused([a, b, c], "member 2: n_episode", n_eps=[3, 3, 0])
    wide = on.make("lin8", 4, H=128)
    refused([a, b, wide], "member 2: members must have one network shape .*hidden", also=[wide])
    close(wide[1], wide[0])
    circle = on.make("pc", 4)
    lin6 = on.make("pc", 4)          # a linear env on a context of the point-circle shape: obs 6 / act 2
    from fsrl_amd.env import DeviceLinear, SyntheticSafetyVectorEnv
    from fsrl_amd.env.synthetic import stable_coupling
    lin_env = DeviceLinear(lin6[0], like=SyntheticSafetyVectorEnv(env_num=4, obs_dim=6, act_dim=2, episode_len=7, coupling=stable_coupling(6),
                                                                  cost_threshold=0.7), seed=1)
    refused([circle, (lin6[0], lin_env)], "member 1: its device env is of kind 1, member 0's of kind 0", also=[circle])
    close(lin_env, lin6[1], lin6[0], circle[1], circle[0])
    replay = rp.make("cvpo", "lin8", 4)
    refused([a, replay], "member 1 is a Gaussian replay .* context and member 0 an on-policy one", also=[replay])
    close(replay[1], replay[0])
    layered = on.make("lin8", 4, hidden_sizes=(32, 32, 32))
    refused([a, b, layered], "member 2: .*layered", also=[layered])
    close(layered[1], layered[0])
    arch = TrajArchive(b[0], 1000, 100, 50)
    arch.attach(b[0])
    refused([a, b, c], "member 1: .*trajectory tap")
    arch.detach(b[0]); arch.close()
    c[0].ppo_begin([0.3], 1 / 1.3, 16)
    refused([a, b, c], "member 2: .*inside an update", exc=FsrlHipError)
    c[0].ppo_abort()
    res = group_collect([a[0], b[0], c[0]], [a[1], b[1], c[1]], [2, 3, 4], bound_method=1)       # ... and the call still works
    assert [len(r["ep_rews"]) for r in res] == [2, 3, 4]
    close(*[v for _, v in everyone]); close(*[e for e, _ in everyone])


# ------------------------------------------------------------------------------------------------ 7. an env changes roles
@pytest.mark.parametrize("agent", ["onpolicy", "sacl_per"])
def test_envs_change_roles_between_solo_grouped_and_evaluating_calls(agent):
    """An env's member table and events are made by whichever call first needs them, and an env may be the only member, member 0 or a
    later member, collecting or evaluating: solo(A), solo(B), group([B, A]), solo(A), evaluate(B), group([A, B]) on two ungrouped
    engines against twins that make the same calls one member at a time.  3 envs, episodes of 7 steps, 4 episodes, 4 vector steps per
    launch: every call takes several launches and the surplus rule drops envs.  Then the one-member grouped call against the solo call"""
    kw = dict(deterministic=False, bound_method=1, max_steps_per_launch=4)
    per = agent == "sacl_per"

    def pair():
        if per:
            return [rp.make("sacl", "lin8", 3, rows_per_env=9, seed=3 + i, per=(0.6, 0.4)) for i in range(2)]
        return [on.make("lin8", 3, rows_per_env=9, seed=3 + i) for i in range(2)]
    mem, twin = pair(), pair()
    for _, v in mem + twin:
        v.reset()
    A, B = 0, 1
    solo = lambda p, i: p[i][0].collect_device(p[i][1]._h, 4, **kw)
    evaluate = lambda p, i: p[i][0].evaluate_device(p[i][1]._h, 4, **kw)

    def same(i, got, want, what, launches=True):
        assert_same_stats(got, want, what)
        assert not launches or got["launches"] == want["launches"] > 1, (what, got["launches"], want["launches"])
        assert_same_snapshot(snapshot(*mem[i]), snapshot(*twin[i]), what)
        if per:
            (lm, mxm, mnm, totm), (lt, mxt, mnt, tott) = mem[i][0].per_state(), twin[i][0].per_state()
            assert np.array_equal(lm, lt) and (mxm, mnm, totm) == (mxt, mnt, tott), what + ": the sum tree"

    steps = [("solo", [A]), ("solo", [B]), ("group", [B, A]), ("solo", [A]), ("evaluate", [B]), ("group", [A, B])]
    for n, (call, who) in enumerate(steps):
        what = f"{agent} call {n} {call}{who}"
        if call == "group":
            res = group_collect([mem[i][0] for i in who], [mem[i][1] for i in who], [4] * len(who), **kw)
            assert res[0]["launches"] > 1
        else:
            res = [(solo if call == "solo" else evaluate)(mem, who[0])]
        for i, r in zip(who, res):
            want = (evaluate if call == "evaluate" else solo)(twin, i)
            assert len(r["ep_rews"]) == 4
            same(i, r, want, what, launches=call != "group")
    assert all(e.store_sizes().max() == 9 for e, _ in mem)           # the sub-buffers wrapped
    # k = 1 through the grouped entry point == the solo call
    same(A, group_collect([mem[A][0]], [mem[A][1]], [4], **kw)[0], solo(twin, A), f"{agent} k = 1")
    close(*[v for _, v in mem + twin]); close(*[e for e, _ in mem + twin])
