"""Wide device evaluations (fsrl_evaluate_device_wide / _wide_layered) against their oracles on TWINS (same parameters, same env seed):
up to 64 envs the narrow evaluation, beyond 64 the storing wide collect.  Both run the same device arithmetic on the same Philox
counters and sum returns in step order in double, and costs are 0.0 / 1.0, so every comparison is exact.  Episodes are cut at 7
steps, hidden 64 unless stated, 4 step launches per batch, so that batches end on steps with finished episodes."""
import numpy as np
import pytest

import devenv_replay_model as rm
import test_gpu_devcollect as on
import test_gpu_devcollect_replay as rp
import test_gpu_devcollect_wide as gw
import test_gpu_devcollect_wide_layered as wl
import test_gpu_deveval as ev

pytestmark = pytest.mark.gpu
KEYS = [k for k in ev.STAT_KEYS if k != "launches"]
LAYERED = (64, 48, 32)


def make(agent, kind, n, shape, wide=True, **kw):
    return wl.make(agent, kind, n, shape, wide=wide, **kw) if isinstance(shape, tuple) else gw.make(agent, kind, n, H=shape, wide=wide, **kw)


def runs(eng, shape):
    """-> (narrow evaluation, wide evaluation, storing wide collect) of the engine's kind"""
    if isinstance(shape, tuple):
        return eng.evaluate_device_layered, eng.evaluate_device_wide_layered, eng.collect_device_wide_layered
    return eng.evaluate_device, eng.evaluate_device_wide, eng.collect_device_wide


@pytest.mark.parametrize("deterministic", [False, True], ids=["training", "deterministic"])
@pytest.mark.parametrize("n", [17, 64])
@pytest.mark.parametrize("agent,kind,shape", [("onpolicy", "pc", 64), ("sacl", "lin33", 64), ("onpolicy", "lin8", LAYERED)])
def test_wide_evaluation_equals_the_narrow_evaluation_on_twins(agent, kind, shape, n, deterministic):
    out = []
    for wide in (False, True):
        eng, env = make(agent, kind, n, shape, wide=wide)
        env.reset()
        res = [runs(eng, shape)[wide](env._h, n_ep, deterministic=deterministic, bound_method=1, max_steps_per_launch=4) for n_ep in (5, n, n + 8)]
        out.append((res, env.get_state(), len(eng)))
        ev.close(env, eng)
    (ra, sa, na), (rb, sb, nb) = out
    for n_ep, a, b in zip((5, n, n + 8), ra, rb):
        ev.same_stats(a, b, f"{agent} {kind} n={n} n_ep={n_ep}", KEYS)
        assert len(b["ep_rews"]) == n_ep and b["steps"] == int(b["ep_lens"].sum()) > 0
    assert rb[2]["launches"] >= 2 * 5 and ev.same_state_tuple(sa, sb) and na == nb == 0


# (agent, env, env_num, n_episode - env_num, shape, episode_len); 1030 envs: two trips of the 256-thread settle; episode_len 1: every
# env ends in every launch, so the park's two sides alternate
BEYOND = [("onpolicy", "lin8", 65, 3, 64, 7), ("sacl", "lin8", 100, 40, 64, 7), ("onpolicy", "pc", 100, 40, 64, 7), ("onpolicy", "lin8", 257, 40, 64, 7),
          ("ddpgl", "lin64w", 65, 3, 256, 7), ("onpolicy", "lin8", 1030, 3, 64, 7), ("onpolicy", "lin8", 100, 40, LAYERED, 7),
          ("onpolicy", "lin8", 70, 130, 64, 1)]


@pytest.mark.parametrize("case", BEYOND, ids=wl.ids)
def test_beyond_64_envs_wide_evaluation_equals_the_storing_wide_collect_on_twins(case):
    agent, kind, n, extra, shape, ep_len = case
    from fsrl_amd.env import DeviceLinear
    out = []
    for which in (1, 2):
        eng, env = make(agent, kind, n, shape, rows_per_env=24)
        if ep_len != 7:
            host = rm.linear_host(kind, n)
            env.close()
            env = DeviceLinear(eng, n, episode_len=ep_len, cost_threshold=host.cost_threshold, A=host.A, B=host.B, seed=3)
        env.reset()
        if ep_len == 7:
            env.set_state(t=gw.t_injected(n))
        res = runs(eng, shape)[which](env._h, n + extra, deterministic=False, bound_method=1, max_steps_per_launch=4)
        out.append((res, env.get_state(), len(eng)))
        ev.close(env, eng)
    (a, sa, na), (b, sb, nb) = out
    ev.same_stats(a, b, wl.ids(case))           # launches too
    assert len(a["ep_rews"]) == n + extra and a["steps"] == int(a["ep_lens"].sum()) == nb and na == 0
    assert ev.same_state_tuple(sa, sb), "env state, steps, ordinals"
    assert len(set(a["ep_lens"].tolist())) > 1 or ep_len == 1           # episodes ended in different steps
    if kind == "pc":
        assert a["terminated"] > 0 and a["total_cost"] > 0


@pytest.mark.parametrize("setting,refusal", [("group", "grouped"), ("tap", "trajectory tap"), ("sub_buffers", "sub-buffers"), ("per", "prioritised")])
def test_a_wide_evaluation_moves_nothing_where_the_storing_call_is_refused(setting, refusal):
    """a context with collected rows, a wrapped sub-buffer and an open episode; 70 test envs on its 5 sub-buffers"""
    from fsrl_amd.engine import EngineGroup, TrajArchive
    from fsrl_amd.env import DevicePointCircle
    eng, env = rp.make("sacl", "pc", 5, rows_per_env=9, per=(0.6, 0.4)) if setting == "per" else on.make("pc", 5, rows_per_env=9)
    env.reset()
    eng.collect_device(env._h, 12, deterministic=False, bound_method=1)
    eng.push(*ev.ONE)
    other = on.make("pc", 4, seed=4) if setting == "group" else None
    group = EngineGroup([eng, other[0]]) if other else None
    arch = TrajArchive(eng, 1000, 100, 50) if setting == "tap" else None
    if arch:
        arch.attach(eng)
    test = DevicePointCircle(eng, 70, max_episode_steps=7, seed=9, **on.PC)
    test.reset()
    before, state0 = ev.everything(eng, env), test.get_state()
    tree0, taps0 = eng.per_state() if setting == "per" else None, arch.counters() if arch else None
    res = eng.evaluate_device_wide(test._h, 75, deterministic=False, bound_method=1, max_steps_per_launch=4)
    assert len(res["ep_rews"]) == 75 and not ev.same_state_tuple(state0, test.get_state())
    ev.assert_nothing_moved(before, ev.everything(eng, env))
    if tree0:
        tree = eng.per_state()
        assert np.array_equal(tree0[0], tree[0]) and tree0[1:] == tree[1:], "the sum tree, max_prio, min_prio, the root"
    with pytest.raises(AssertionError, match=refusal):
        eng.collect_device_wide(test._h, 3)
    ev.assert_nothing_moved(before, ev.everything(eng, env))
    if arch:
        assert arch.counters() == taps0
        arch.detach(eng); arch.close()
    ev.close(test, env)
    if group:
        other[1].close(); group.close(); other[0].close()
    eng.close()


def test_the_collectors_and_an_agent_route_wide_test_envs_to_the_wide_evaluation(tmp_path):
    from fsrl_amd.agent import PPOLagAgent
    from fsrl_amd.data import WideDeviceEvalCollector, evaluation_collector
    from fsrl_amd.data.device_collector import _collect_stats
    from fsrl_amd.env import DevicePointCircle, PointCircleEnv
    from fsrl_amd.utils import BaseLogger
    (eng, env), (twin, env_t) = gw.make("onpolicy", "pc", 70), gw.make("onpolicy", "pc", 70)
    env_t.reset()
    col = evaluation_collector(on.Pol(eng), env)
    assert type(col) is WideDeviceEvalCollector and col.buffer is None and col.env is env
    want = _collect_stats(twin.evaluate_device_wide(env_t._h, 75, deterministic=True, bound_method=1))
    assert col.collect(n_episode=75) == want and (col.collect_episode, col.collect_step) == (75, want["n/st"]) and col.last_launches > 0
    ev.close(env, env_t, eng, twin)
    agent = PPOLagAgent(PointCircleEnv(), BaseLogger(str(tmp_path), name="d"), cost_limit=10, device="cuda:0", seed=3, hidden_sizes=(64, 64), training_num=4)
    test = DevicePointCircle(agent.policy, 70, max_episode_steps=20, seed=2)
    with ev.StepSpy() as spy:
        rew, length, cost = agent.evaluate(test, eval_episodes=75)
    assert len(spy.made) == 1 and type(spy.made[0]) is WideDeviceEvalCollector and spy.steps == 0
    assert 1 <= length <= 20 and np.isfinite(rew) and cost >= 0
    test.close()
