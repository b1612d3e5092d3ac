"""Device evaluations (fsrl_evaluate_device, fsrl_evaluate_device_group, the store-less DeviceCollector) against the training collect.

The oracle is fsrl_collect_device on a TWIN: a context with the same parameters and a device env with the same seed.  An evaluation
runs the same device code on the same Philox counters, so every comparison here is exact (np.array_equal / ==), in training mode
and under the tanh bound too: statistics, episode returns and lengths in order, launches, and the env's state, steps and reset
ordinals.  What an evaluation must NOT move is compared before / after on the evaluated context itself and against a twin that never
evaluated: store rows, sizes, books (what one more push reports), the exported training state, the sum tree, the next update's bits.
Shapes are the smallest of tests/test_gpu_devcollect.py: hidden (64, 64) unless stated, episodes cut at 7 steps, point-circle with
radius 0.12 / x_lim 0.3, the linear env at obs 8 / act 2 and obs 33 / act 8."""
import numpy as np
import pytest

import test_gpu_devcollect as on
import test_gpu_devcollect_replay as rp

pytestmark = pytest.mark.gpu
F32 = np.float32
STAT_KEYS = ("steps", "total_cost", "terminated", "truncated", "ep_rews", "ep_lens", "launches")
BOUNDS = (("clip", 1, None), ("none with bounds", 0, (-0.5, 1.5)), ("tanh", 2, (-1.5, 1.0)))
LAG, RESC = [0.5], 1 / 1.5


def bounds_of(eng, low_high):
    if low_high is None:
        return None, None
    Da = eng.cfg.act_dim
    return np.full(Da, low_high[0], F32), np.full(Da, low_high[1], F32)


def same_stats(a, b, what, keys=STAT_KEYS):
    for k in keys:
        assert np.array_equal(a[k], b[k]), (what, k, a[k], b[k])


def same_state(ea, eb):
    return all(np.array_equal(x, y) for x, y in zip(ea.get_state(), eb.get_state()))


def close(*xs):
    for x in xs:
        x.close()


def twins_agree(ev, co, episodes, what, totals, **kw):
    """ev = (engine, env) evaluates, co = (engine, env) collects; two consecutive calls each"""
    for n_ep in episodes:
        a = ev[0].evaluate_device(ev[1]._h, n_ep, **kw)
        b = co[0].collect_device(co[1]._h, n_ep, **kw)
        same_stats(a, b, f"{what} n_ep={n_ep}")
        assert len(a["ep_rews"]) == n_ep and a["steps"] == int(a["ep_lens"].sum()) > 0
        assert same_state(ev[1], co[1]), f"{what} n_ep={n_ep}: env state, steps, ordinals"
        totals["terminated"] += a["terminated"]; totals["truncated"] += a["truncated"]; totals["cost"] += a["total_cost"]
        totals["steps"].append((n_ep, a["steps"]))


# ------------------------------------------------------------------------------------------------ 1. evaluation == collect on twins
CASES = [("pc", 5, (3, 12)), ("lin8", 17, (20, 9)), ("lin33", 16, (16, 30)), ("pc", 64, (70, 64)), ("lin8", 1, (2, 1))]


def test_cases_reach_the_surplus_rule_both_ways():
    assert any(min(eps) < n for _, n, eps in CASES) and any(max(eps) > n for _, n, eps in CASES)
    assert any(n_ep % n for _, n, eps in CASES for n_ep in eps if n_ep > n)       # a tail in which envs must leave the live set


@pytest.mark.parametrize("kind,n,episodes", CASES)
def test_evaluation_equals_a_collect_on_twins(kind, n, episodes):
    ev, co = on.make(kind, n), on.make(kind, n)
    ev[1].reset(); co[1].reset()
    theta0, version0 = ev[0].get_params(), ev[0].store_version()
    totals = dict(terminated=0, truncated=0, cost=0.0, steps=[])
    for deterministic in (True, False):
        for name, bound, low_high in BOUNDS:
            low, high = bounds_of(ev[0], low_high)
            twins_agree(ev, co, episodes, f"{kind} n={n} {name} det={deterministic}", totals, deterministic=deterministic, bound_method=bound,
                        low=low, high=high)
    # the evaluated context: nothing stored, nothing versioned, the parameters untouched
    assert len(ev[0]) == 0 and ev[0].store_version() == version0 and np.array_equal(ev[0].get_params(), theta0)
    assert len(co[0]) > 0 and co[0].store_version() > version0
    # the cases bite
    assert totals["truncated"] > 0
    if kind == "pc":
        assert totals["terminated"] > 0 and totals["cost"] > 0
    else:       # no termination: every episode is 7 steps, so n_ep episodes are 7 n_ep rows only if surplus envs left the live set
        assert totals["terminated"] == 0 and all(steps == 7 * n_ep for n_ep, steps in totals["steps"])
    close(ev[1], co[1], ev[0], co[0])


# ------------------------------------------------------------------------------------------------ 2. the replay heads
@pytest.mark.parametrize("agent,kind,kw", [("sacl", "pc", dict(unbounded=True)), ("sacl", "lin8", dict(unbounded=False)), ("ddpgl", "lin20", {}),
                                           ("cvpo", "lin8", {}), ("sacl", "pc", dict(per=(0.6, 0.4)))],
                         ids=["sacl-unbounded", "sacl-bounded", "ddpgl-act16", "cvpo", "sacl-prioritised"])
def test_replay_heads_evaluation_equals_a_collect_on_twins(agent, kind, kw):
    for n in (5, 17):
        ev, co = rp.make(agent, kind, n, **kw), rp.make(agent, kind, n, **kw)
        if agent == "ddpgl":
            assert ev[0].cfg.act_dim == 16
        ev[1].reset(); co[1].reset()
        version0 = ev[0].store_version()
        totals = dict(terminated=0, truncated=0, cost=0.0, steps=[])
        for deterministic in (True, False):
            twins_agree(ev, co, (3, n + 3), f"{agent} {kind} n={n} det={deterministic}", totals, deterministic=deterministic, bound_method=1)
        assert len(ev[0]) == 0 and ev[0].store_version() == version0 and len(co[0]) > 0
        if "per" in kw:
            leaves, mx, mn, total = ev[0].per_state()
            assert np.count_nonzero(leaves) == 0 and total == 0 and np.count_nonzero(co[0].per_state()[0]) == len(co[0])
        close(ev[1], co[1], ev[0], co[0])


# ------------------------------------------------------------------------------------------------ 3. nothing else moves
ONE = (np.array([1]), np.zeros((1, 6), F32), np.zeros((1, 2), F32), np.array([0.25]), np.array([1.0]), np.array([False]), np.array([False]),
       np.ones((1, 6), F32))


def everything(eng, train_env):
    idx, rows = on.store_rows(eng)
    return dict(idx=idx, rows=rows, sizes=eng.store_sizes().copy(), n=len(eng), version=eng.store_version(), env=train_env.get_state(),
                blob=eng.train_state())


def assert_nothing_moved(before, after, blob=True):
    assert np.array_equal(before["idx"], after["idx"]) and on.same_rows(before["rows"], after["rows"]), "store rows"
    assert np.array_equal(before["sizes"], after["sizes"]) and before["n"] == after["n"], "sub-buffer sizes"
    assert before["version"] == after["version"], "store_version"
    assert all(np.array_equal(x, y) for x, y in zip(before["env"], after["env"])), "the training env"
    # the exported training state: parameters, optimiser state, random streams, running statistics, books and store.  No field of it
    # is known to move under an evaluation, so the whole export is compared.
    assert not blob or before["blob"] == after["blob"], "the exported training state"


def test_an_evaluation_moves_nothing_but_its_env_onpolicy():
    from fsrl_amd.env import DevicePointCircle
    eng, env = on.make("pc", 5, rows_per_env=9)
    twin, env_t = on.make("pc", 5, rows_per_env=9)
    for e, v in ((eng, env), (twin, env_t)):
        v.reset()
        e.collect_device(v._h, 12, deterministic=False, bound_method=1)
        e.push(*ONE)                                                # an episode open in the books of sub-buffer 1
    assert eng.store_sizes().max() == 9                             # a sub-buffer wrapped
    test = DevicePointCircle(eng, 3, max_episode_steps=7, seed=9, **on.PC)
    test.reset()
    before = everything(eng, env)
    state0 = test.get_state()
    res = [eng.evaluate_device(test._h, n_ep, deterministic=det, bound_method=1) for n_ep, det in ((7, False), (2, True))]
    assert [len(r["ep_rews"]) for r in res] == [7, 2] and not same_state_tuple(state0, test.get_state())
    assert_nothing_moved(before, everything(eng, env))
    assert_nothing_moved(before, everything(twin, env_t), blob=False)       # ... and it is the twin's, which never evaluated
    # the books: one more push reports the twin's slot and running episode
    fin = ONE[:5] + (np.array([True]), ) + ONE[6:]
    pe, pt = eng.push(*fin), twin.push(*fin)
    assert all(np.array_equal(x, y) for x, y in zip(pe, pt)) and pe[2][0] == 2
    ue, ut = eng.ppo_update([0.3], 1 / 1.3, 32, 2, seed=5), twin.ppo_update([0.3], 1 / 1.3, 32, 2, seed=5)
    assert np.array_equal(np.asarray(ue[0]), np.asarray(ut[0])) and np.array_equal(eng.get_params(), twin.get_params())
    close(test, env, env_t, eng, twin)


def same_state_tuple(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_an_evaluation_moves_nothing_but_its_env_prioritised_sac():
    from fsrl_amd.env import DevicePointCircle
    eng, env = rp.make("sacl", "pc", 5, rows_per_env=9, per=(0.6, 0.4))
    twin, env_t = rp.make("sacl", "pc", 5, rows_per_env=9, per=(0.6, 0.4))
    for e, v in ((eng, env), (twin, env_t)):
        v.reset()
        e.collect_device(v._h, 12, deterministic=False, bound_method=1)
        for _ in range(3):                                          # the priorities move, the sampler's counter moves
            e.sac_update(16, LAG, RESC)
        e.push(*ONE)
    assert eng.store_sizes().max() == 9
    test = DevicePointCircle(eng, 3, max_episode_steps=7, seed=9, **on.PC)
    test.reset()
    before, tree0 = everything(eng, env), eng.per_state()
    res = eng.evaluate_device(test._h, 7, deterministic=False, bound_method=1)
    assert len(res["ep_rews"]) == 7
    assert_nothing_moved(before, everything(eng, env))
    for tree in (eng.per_state(), twin.per_state()):
        assert np.array_equal(tree0[0], tree[0]) and tree0[1:] == tree[1:], "the sum tree, max_prio, min_prio, the root"
    se, st = eng.sac_update(16, LAG, RESC), twin.sac_update(16, LAG, RESC)
    assert np.isfinite(se).all() and np.array_equal(se, st)
    assert np.array_equal(eng.sac_last_sample(16)[0], twin.sac_last_sample(16)[0])
    for which in (0, 1):
        assert np.array_equal(eng.sac_get_params(which)[0], twin.sac_get_params(which)[0])
    assert np.array_equal(eng.per_state()[0], twin.per_state()[0])
    close(test, env, env_t, eng, twin)


# ------------------------------------------------------------------------------------------------ 4. accepted where a collect refuses
def test_accepted_with_a_trajectory_tap_more_envs_than_sub_buffers_and_on_a_group_member():
    from fsrl_amd.engine import EngineGroup, TrajArchive
    # a trajectory tap: nothing is stored, nothing reaches the archive
    ev, co = on.make("pc", 5), on.make("pc", 5)
    ev[1].reset(); co[1].reset()
    arch = TrajArchive(ev[0], 1000, 100, 50)
    arch.attach(ev[0])
    c0 = arch.counters()
    a, b = ev[0].evaluate_device(ev[1]._h, 8, deterministic=False, bound_method=1), co[0].collect_device(co[1]._h, 8, deterministic=False, bound_method=1)
    same_stats(a, b, "tap")
    c1 = arch.counters()
    assert c1 == c0 and c1["committed"] == c1["rows"] == c1["episodes"] == 0
    with pytest.raises(AssertionError, match="trajectory tap"):
        ev[0].collect_device(ev[1]._h, 1)
    arch.detach(ev[0]); arch.close()
    close(ev[1], co[1], ev[0], co[0])
    # 64 envs on a store of 4 sub-buffers
    ev, co = on.make("pc", 64, sub_buffers=4), on.make("pc", 64)
    assert ev[0].store_geometry()[1] == 4
    ev[1].reset(); co[1].reset()
    a, b = ev[0].evaluate_device(ev[1]._h, 70, deterministic=False, bound_method=1), co[0].collect_device(co[1]._h, 70, deterministic=False, bound_method=1)
    same_stats(a, b, "64 envs, 4 sub-buffers")
    assert same_state(ev[1], co[1]) and len(ev[0]) == 0
    with pytest.raises(AssertionError, match="sub-buffers"):
        ev[0].collect_device(ev[1]._h, 1)
    close(ev[1], co[1], ev[0], co[0])
    # the solo call on a member of an update group
    ev, other, co = on.make("lin8", 5), on.make("lin8", 4, seed=4), on.make("lin8", 5)
    group = EngineGroup([ev[0], other[0]])
    ev[1].reset(); co[1].reset()
    a, b = ev[0].evaluate_device(ev[1]._h, 8, deterministic=False, bound_method=1), co[0].collect_device(co[1]._h, 8, deterministic=False, bound_method=1)
    same_stats(a, b, "group member")
    assert same_state(ev[1], co[1])
    with pytest.raises(AssertionError, match="grouped contexts"):
        ev[0].collect_device(ev[1]._h, 1)
    close(ev[1], other[1], co[1]); group.close(); close(ev[0], other[0], co[0])


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_name_their_reason_and_change_nothing():
    from fsrl_amd import _lib
    from fsrl_amd._lib import FsrlHipError

    def refused(eng, env, match, exc=AssertionError, **kw):
        before, n_before, v_before = env.get_state(), len(eng), eng.store_version()
        with pytest.raises(exc, match=match):
            eng.evaluate_device(env._h, 3, **kw)
        assert same_state_tuple(before, env.get_state()) and len(eng) == n_before and eng.store_version() == v_before

    eng, env = on.make("pc", 5)
    env.reset()
    other, env_o = on.make("pc", 5)
    refused(other, env, "another context")
    refused(eng, env, "bound_method", bound_method=7)
    refused(eng, env, "max_steps_per_launch", max_steps_per_launch=5000)
    with pytest.raises(AssertionError, match="n_episode"):
        eng.evaluate_device(env._h, 0)
    eng.collect_device(env._h, 5, bound_method=1)
    eng.ppo_begin([0.3], 1 / 1.3, 16)
    refused(eng, env, "fsrl_evaluate_device inside an update", exc=FsrlHipError)
    eng.ppo_abort()
    assert len(eng.evaluate_device(env._h, 3, bound_method=1)["ep_rews"]) == 3           # ... and the call still works
    close(env, env_o, eng, other)
    eng, env = on.make("lin8", 4, hidden_sizes=(32, 32, 32))
    refused(eng, env, "layered")
    close(env, eng)
    eng, env = rp.make("sacl", "lin8", 4, init=False)
    env.reset()
    refused(eng, env, "fsrl_sac_init")
    close(env, eng)


# ------------------------------------------------------------------------------------------------ 6. launch cuts
def test_launch_cuts_change_nothing_at_256_wide():
    out = []
    for cut in (3, 0):
        eng, env = on.make("lin8", 17, H=256, rows_per_env=12)
        env.reset()
        res = [eng.evaluate_device(env._h, n_ep, deterministic=False, bound_method=1, max_steps_per_launch=cut) for n_ep in (20, 5)]
        out.append((res, env.get_state(), len(eng)))
        close(env, eng)
    (ra, sta, na), (rb, stb, nb) = out
    assert ra[0]["launches"] > 1 and ra[1]["launches"] > 1 and rb[0]["launches"] == rb[1]["launches"] == 1
    for x, y in zip(ra, rb):
        same_stats(x, y, "cut", [k for k in STAT_KEYS if k != "launches"])
    assert same_state_tuple(sta, stb) and na == nb == 0


# ------------------------------------------------------------------------------------------------ 7. grouped evaluation
def group_evaluate(members, n_eps, **kw):
    from fsrl_amd.engine import evaluate_device_group
    return evaluate_device_group([e for e, _ in members], [v._h for _, v in members], n_eps, **kw)


def grouped_equals_solo(make_member, ns, n_eps, Group):
    for grouped in (False, True):
        mem = [make_member(n, 3 + i) for i, n in enumerate(ns)]
        twin = [make_member(n, 3 + i) for i, n in enumerate(ns)]
        group = Group([e for e, _ in mem]) if grouped else None
        for _, v in mem + twin:
            v.reset()
        versions = [e.store_version() for e, _ in mem]
        for rnd, cut in enumerate((4, 0)):
            res = group_evaluate(mem, n_eps, deterministic=False, bound_method=1, max_steps_per_launch=cut)
            solo = [e.evaluate_device(v._h, n_eps[i], deterministic=False, bound_method=1, max_steps_per_launch=cut) for i, (e, v) in enumerate(twin)]
            for i in range(len(ns)):
                same_stats(res[i], solo[i], f"grouped={grouped} round {rnd} member {i}", [k for k in STAT_KEYS if k != "launches"])
                assert len(res[i]["ep_rews"]) == n_eps[i]
                assert same_state(mem[i][1], twin[i][1]), f"grouped={grouped} round {rnd} member {i}: env state"
                assert len(mem[i][0]) == 0 and mem[i][0].store_version() == versions[i]
            # one count for the call: the launches of the member that finished last
            assert len({r["launches"] for r in res}) == 1 and res[0]["launches"] == max(s["launches"] for s in solo)
            if rnd == 0:
                assert min(s["launches"] for s in solo) < res[0]["launches"]
        close(*[v for _, v in mem + twin])
        if group is not None:
            group.close()
        close(*[e for e, _ in mem + twin])


def test_grouped_evaluation_of_onpolicy_members_equals_their_solo_evaluations():
    from fsrl_amd.engine import EngineGroup
    grouped_equals_solo(lambda n, seed: on.make("lin8", n, seed=seed), (5, 17, 4), (3, 12, 5), EngineGroup)


def test_grouped_evaluation_of_sac_members_equals_their_solo_evaluations():
    from fsrl_amd.engine import EngineSacGroup
    grouped_equals_solo(lambda n, seed: rp.make("sacl", "lin8", n, seed=seed), (5, 17), (12, 3), EngineSacGroup)


def test_grouped_evaluation_refuses_disagreeing_members_and_mixed_collectors():
    from fsrl_amd.data import DeviceCollector, GroupDeviceCollector, HipVectorReplayBuffer
    a, b = on.make("lin8", 5, seed=3), on.make("lin8", 4, seed=4)
    for _, v in (a, b):
        v.reset()

    def refused(members, match, n_eps=3, **kw):
        before = [v.get_state() for _, v in members]
        with pytest.raises(AssertionError, match=match):
            group_evaluate(members, n_eps, **kw)
        assert all(same_state_tuple(s, v.get_state()) for s, (_, v) in zip(before, members))

    wide = on.make("lin8", 4, H=128)
    refused([a, b, wide], "member 2: members must have one network shape .*hidden")
    replay = rp.make("cvpo", "lin8", 4)
    refused([a, replay], "member 1 is a Gaussian replay .* context and member 0 an on-policy one")
    refused([a, b], "member 1: n_episode", n_eps=[3, 0])
    refused([a, b, a], "member 2: its context is listed twice")
    res = group_evaluate([a, b], [2, 3], bound_method=1)
    assert [len(r["ep_rews"]) for r in res] == [2, 3]
    # collectors: all store-less or all storing
    ev = DeviceCollector(on.Pol(a[0]), a[1])
    st = DeviceCollector(on.Pol(b[0]), b[1], HipVectorReplayBuffer(b[0], 4 * 50, 4))
    assert ev.buffer is None
    with pytest.raises(AssertionError, match="mix of store-less and storing"):
        GroupDeviceCollector([ev, st])
    ev_b = DeviceCollector(on.Pol(b[0]), b[1])
    stats = GroupDeviceCollector([ev, ev_b]).collect([2, 3])
    assert [s["n/ep"] for s in stats] == [2, 3] and (ev.collect_episode, ev_b.collect_episode) == (2, 3) and len(a[0]) == len(b[0]) == 0
    close(a[1], b[1], wide[1], replay[1], a[0], b[0], wide[0], replay[0])


# ------------------------------------------------------------------------------------------------ 8. / 9. facade
class StepSpy:
    """counts DeviceVectorEnv.step calls; records what the agents' helper returns"""

    def __enter__(self):
        from fsrl_amd.agent import base_agent, sac_lag_agent
        from fsrl_amd.env.device import DeviceVectorEnv
        self.steps, self.made = 0, []
        self.cls, self.orig_step = DeviceVectorEnv, DeviceVectorEnv.step
        self.mods, self.orig_helper = (base_agent, sac_lag_agent), base_agent.evaluation_collector
        spy = self

        def step(env, *a, **k):
            spy.steps += 1
            return spy.orig_step(env, *a, **k)

        def helper(*a, **k):
            col = spy.orig_helper(*a, **k)
            spy.made.append(col)
            return col
        DeviceVectorEnv.step = step
        for m in self.mods:
            m.evaluation_collector = helper
        return self

    def __exit__(self, *exc):
        self.cls.step = self.orig_step
        for m in self.mods:
            m.evaluation_collector = self.orig_helper


def test_ppo_lag_agent_evaluates_on_the_device_and_trains_to_the_same_bits(tmp_path):
    from fsrl_amd.agent import PPOLagAgent
    from fsrl_amd.data import DeviceCollector, FastCollector
    from fsrl_amd.env import DevicePointCircle, PointCircleEnv
    from fsrl_amd.utils import BaseLogger
    finals = []
    for with_test in (True, False):
        agent = PPOLagAgent(PointCircleEnv(), BaseLogger(str(tmp_path / str(with_test)), name="d"), cost_limit=10, device="cuda:0", seed=3,
                            hidden_sizes=(64, 64), training_num=4)
        train = DevicePointCircle(agent.policy, 4, max_episode_steps=20, seed=1)
        test = DevicePointCircle(agent.policy, 2, max_episode_steps=20, seed=2) if with_test else None
        with StepSpy() as spy:
            ep, stat, info = agent.learn(train, test, epoch=2, episode_per_collect=4, step_per_epoch=160, repeat_per_collect=2, batch_size=32,
                                         testing_num=2, verbose=False, save_ckpt=False, show_progress=False)
            if with_test:
                rew, length, cost = agent.evaluate(test, eval_episodes=2)
                assert 1 <= length <= 20 and np.isfinite(rew) and cost >= 0
                agent.policy.train()
                rew_t, _, _ = agent.evaluate(test, eval_episodes=2, train_mode=True)         # stochastic: the env's action stream
                assert np.isfinite(rew_t)
        assert ep == 2 and spy.steps == 0
        if with_test:
            assert len(spy.made) == 3 and all(isinstance(c, DeviceCollector) and c.buffer is None and c.env is test for c in spy.made)
            assert np.isfinite(stat["test/reward"]) and np.isfinite(stat["test/cost"])
        else:
            assert spy.made == [None] and "test/reward" not in stat
        finals.append(agent.policy.engine.get_params())
        train.close()
        if test is not None:
            test.close()
    assert np.array_equal(finals[0], finals[1])
    # a layered agent still evaluates over a device env of its engine: stepped from the host
    agent = PPOLagAgent(PointCircleEnv(), BaseLogger(str(tmp_path / "lay"), name="d"), cost_limit=10, device="cuda:0", seed=3,
                        hidden_sizes=(32, 32, 32), training_num=4)
    test = DevicePointCircle(agent.policy, 2, max_episode_steps=20, seed=2)
    with StepSpy() as spy:
        rew, length, cost = agent.evaluate(test, eval_episodes=2)
    assert len(spy.made) == 1 and isinstance(spy.made[0], FastCollector) and spy.steps > 0
    assert 1 <= length <= 20 and np.isfinite(rew) and cost >= 0
    test.close()


def test_sac_lag_agent_trains_to_the_same_bits_with_and_without_test_envs(tmp_path):
    from fsrl_amd.agent import SACLagAgent
    from fsrl_amd.data import DeviceCollector
    from fsrl_amd.env import DevicePointCircle, PointCircleEnv
    from fsrl_amd.utils import BaseLogger
    finals = []
    for with_test in (True, False):
        agent = SACLagAgent(PointCircleEnv(), BaseLogger(str(tmp_path / str(with_test)), name="d"), cost_limit=10, device="cuda:0", seed=3,
                            hidden_sizes=(64, 64), training_num=4)
        train = DevicePointCircle(agent.policy, 4, max_episode_steps=20, seed=1)
        test = DevicePointCircle(agent.policy, 2, max_episode_steps=20, seed=2) if with_test else None
        with StepSpy() as spy:
            # 80 rows per collect, 0.1 updates per row: 8 updates between two collects, 16 between two evaluations
            ep, stat, info = agent.learn(train, test, epoch=2, episode_per_collect=4, step_per_epoch=160, update_per_step=0.1, batch_size=32,
                                         testing_num=2, verbose=False, save_ckpt=False, show_progress=False)
        assert ep == 2 and spy.steps == 0
        if with_test:
            assert all(isinstance(c, DeviceCollector) and c.buffer is None for c in spy.made) and "test/cost" in stat
        eng = agent.policy.engine
        finals.append([eng.sac_get_params(w)[0] for w in (0, 1, 2)] + [np.asarray(len(eng))])
        train.close()
        if test is not None:
            test.close()
    assert finals[0][3] > 0 and all(np.array_equal(x, y) for x, y in zip(*finals))
