"""Grouped wide device evaluations (fsrl_evaluate_device_wide_group: k members' 16-row tiles in one launch per vector step, the
episodes accumulated and ordered on the GPU) against each member's own solo wide evaluation on a TWIN context and env -- same seed,
weights and env state -- bit for bit: the solo call is pinned to the narrow evaluation and the storing wide collect by
tests/test_gpu_deveval_wide.py.  Members of 17 / 65 / 100 envs, episodes cut at 5 steps (one case: at 1), 3 step launches a batch."""
import numpy as np
import pytest

import devenv_replay_model as rm
import test_gpu_devcollect as on
import test_gpu_devcollect_group as gr
import test_gpu_deveval as ev
import test_gpu_deveval_wide as ew

pytestmark = pytest.mark.gpu
F32 = np.float32
NS = (17, 65, 100)          # less than two tiles | just over four | a ragged last tile
# 5-step episodes: member 0 runs its 17 envs to the time limit together and shrinks to the 3 episodes left (a surplus; step 10 at the
# latest), member 1 ends with its first round (step 5), member 2 ends about 20 episodes a step and drops a surplus across tiles
# beyond step 15: three different last batches.  1-step episodes: 2, 5 and 10 steps
N_EPS = {5: (20, 65, 330), 1: (20, 300, 1000)}
KW = dict(deterministic=False, bound_method=1, max_steps_per_launch=3)


def wide_group(engs, envs, n_eps, **kw):
    from fsrl_amd.engine import evaluate_device_wide_group
    return evaluate_device_wide_group(engs, [v._h for v in envs], n_eps, **kw)


def solo(eng, env, n_ep, **kw):
    from fsrl_amd.data.device_collector import _layered
    return (eng.evaluate_device_wide_layered if _layered(eng) else eng.evaluate_device_wide)(env._h, n_ep, **kw)


def member(agent, kind, shape, i, ep_len=5, n=None, **kw):
    """member i or its twin: env seed 3 + i, the helpers' parameters scaled by 1 + i / 8, a wide env of its own episode length"""
    from fsrl_amd.env import DeviceLinear, DevicePointCircle
    n = n or NS[i]
    eng, env = ew.make(agent, kind, n, shape, rows_per_env=4, **kw)
    env.close()
    if agent == "onpolicy":
        eng.set_params((eng.get_params() * (1 + i / 8)).astype(F32))
    else:
        eng.sac_put_params(0, (eng.sac_get_params(0)[0] * (1 + i / 8)).astype(F32))
    if kind == "pc":
        env = DevicePointCircle(eng, n, max_episode_steps=ep_len, seed=3 + i, wide=True, **on.PC)
    else:
        host = rm.linear_host(kind, n)
        env = DeviceLinear(eng, n, episode_len=ep_len, cost_threshold=host.cost_threshold, A=host.A, B=host.B, seed=3 + i, wide=True)
    env.reset()
    if i and ep_len > 1:           # episodes that end in different steps
        env.set_state(t=np.random.default_rng(n).integers(0, ep_len, n).astype(np.int32))
    return eng, env


def assert_member_is_its_twin(res, mem, twin, want, what):
    ev.same_stats(res, want, what, ew.KEYS)
    assert res["steps"] == int(res["ep_lens"].sum()) > 0, what
    assert ev.same_state(mem[1], twin[1]), what + ": env state, steps, ordinals"
    assert len(mem[0]) == len(twin[0]) == 0 and mem[0].store_version() == twin[0].store_version(), what + ": the store"


CASES = [("onpolicy", "pc", 64, 5), ("sacl", "lin33", 256, 5), ("ddpgl", "lin64w", 256, 5), ("onpolicy", "lin8", ew.LAYERED, 5), ("sacl", "lin8", 64, 1)]


@pytest.mark.parametrize("agent,kind,shape,ep_len", CASES, ids=lambda x: "x".join(map(str, x)) if isinstance(x, tuple) else str(x))
def test_grouped_wide_evaluation_is_each_members_solo_wide_evaluation(agent, kind, shape, ep_len):
    """Member 1 and its twin first run a solo evaluation of one 8 + 1 launch batch, so that the members enter the grouped call with
    different launch-ordinal parities.  Behind the grouped call one more solo evaluation on members and twins alike: the random
    streams and the reset ordinals moved alike."""
    mem, twin = ([member(agent, kind, shape, i, ep_len) for i in range(3)] for _ in range(2))
    for e, v in (mem[1], twin[1]):
        assert solo(e, v, 3, deterministic=False, bound_method=1, max_steps_per_launch=8)["launches"] == 9
    n_eps = N_EPS[ep_len]
    res = wide_group([e for e, _ in mem], [v for _, v in mem], n_eps, **KW)
    want = [solo(e, v, n_ep, **KW) for (e, v), n_ep in zip(twin, n_eps)]
    for i in range(3):
        assert_member_is_its_twin(res[i], mem[i], twin[i], want[i], f"member {i}")
        assert len(res[i]["ep_rews"]) == n_eps[i]
        ev.same_stats(solo(*mem[i], 7 + NS[i], **KW), solo(*twin[i], 7 + NS[i], **KW), f"member {i}, the evaluation behind")
        assert ev.same_state(mem[i][1], twin[i][1])
    # batches x (S + 1) whatever k is: the call's launches are those of the member that finishes last
    assert res[0]["launches"] == max(w["launches"] for w in want) and res[0]["launches"] % 4 == 0
    assert len({w["launches"] for w in want}) == (2 if kind == "pc" else 3), [w["launches"] for w in want]      # point-circle episodes may end early
    if kind == "pc":
        assert res[2]["terminated"] > 0 and res[2]["total_cost"] > 0
    gr.close(*[v for _, v in mem + twin], *[e for e, _ in mem + twin])


@pytest.mark.parametrize("shape", [64, ew.LAYERED], ids=["fused", "layered"])
def test_a_one_member_group_is_the_solo_call(shape):
    (eng, env), (twin, env_t) = (member("onpolicy", "lin8", shape, 2) for _ in range(2))
    res, want = wide_group([eng], [env], [130], **KW)[0], solo(twin, env_t, 130, **KW)
    ev.same_stats(res, want, "k = 1")           # launches too
    assert_member_is_its_twin(res, (eng, env), (twin, env_t), want, "k = 1")
    gr.close(env, env_t, eng, twin)


def test_members_of_a_group_of_none_and_a_prioritised_one_evaluate_and_move_no_store():
    from fsrl_amd.engine import EngineSacGroup
    per = dict(per=(0.6, 0.4))
    mem, twin = ([member("sacl", "pc", 64, i, n=70, **(per if i == 2 else {})) for i in range(3)] for _ in range(2))
    other = member("sacl", "pc", 64, 0, n=70)
    group = EngineSacGroup([mem[0][0], other[0]])
    for e, _ in mem:
        e.push(*ev.ONE)
    before = [(gr.snapshot(e, v), e.per_state() if i == 2 else None) for i, (e, v) in enumerate(mem)]
    res = wide_group([e for e, _ in mem], [v for _, v in mem], (75, 20, 140), **KW)
    for i, n_ep in enumerate((75, 20, 140)):
        ev.same_stats(res[i], solo(*twin[i], n_ep, **KW), f"member {i}", ew.KEYS)
        assert ev.same_state(mem[i][1], twin[i][1]), f"member {i}: env state, steps, ordinals"
        snap, tree = before[i]
        now = gr.snapshot(*mem[i])
        assert now["version"] == snap["version"] and now["n"] == snap["n"] == 1 and np.array_equal(now["sizes"], snap["sizes"]), f"member {i}: the store"
        assert np.array_equal(now["idx"], snap["idx"]) and on.same_rows(now["rows"], snap["rows"]), f"member {i}: store rows"
        if tree:
            after = mem[i][0].per_state()
            assert np.array_equal(tree[0], after[0]) and tree[1:] == after[1:], "the sum tree, max_prio, min_prio, the root"
    group.close()
    gr.close(*[v for _, v in mem + twin + [other]], *[e for e, _ in mem + twin + [other]])


def test_refusals_name_the_member_and_change_nothing():
    made = [member("onpolicy", "pc", 64, 0, n=70), member("onpolicy", "pc", 64, 0, n=70), member("onpolicy", "pc", 64, 1, n=66),
            member("onpolicy", "pc", ew.LAYERED, 1, n=70)]
    a, twin, b, lay = made
    made.append(on.make("pc", 5))           # a narrow env
    made[-1][1].reset()

    def refused(members, match, engs=None):
        before = [v.get_state() for _, v in members]
        with pytest.raises(AssertionError, match=match):
            wide_group(engs or [e for e, _ in members], [v for _, v in members], 3)
        assert all(ev.same_state_tuple(s, v.get_state()) for s, (_, v) in zip(before, members))

    refused([a, lay], "member 1 is a layered context and member 0 a fused one")
    refused([a, b], "member 1: its context is listed twice", engs=[a[0], a[0]])
    refused([a, b, made[-1]], "member 2: .*wide device env")
    ev.same_stats(solo(*a, 75, **KW), solo(*twin, 75, **KW), "after the refusals")
    assert ev.same_state(a[1], twin[1])
    gr.close(*[v for _, v in made], *[e for e, _ in made])


def test_group_device_collector_routes_wide_store_less_groups():
    from fsrl_amd.data import GroupDeviceCollector, WideDeviceEvalCollector
    mem, twin = ([member("onpolicy", "lin8", 64, i) for i in range(2)] for _ in range(2))
    cols, solos = ([WideDeviceEvalCollector(on.Pol(e), v, 3) for e, v in ms] for ms in (mem, twin))
    group = GroupDeviceCollector(cols, 3)
    assert group.collect([20, 70]) == [c.collect(n_episode=n) for c, n in zip(solos, (20, 70))]
    assert group.last_launches == max(c.last_launches for c in solos) and [c.collect_episode for c in cols] == [20, 70]
    gr.close(*[v for _, v in mem + twin], *[e for e, _ in mem + twin])
