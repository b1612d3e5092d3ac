"""Grouped wide device collects (fsrl_collect_device_wide_group: k members' 16-row tiles in one launch per vector step) against each
member's own solo wide collect on a twin context, bit for bit; a member beyond 64 envs row by row against the float64 model by the
rule and bars of tests/devcollect_rows.py, through GroupDeviceCollector; and the refusals.  Episodes are cut at 7 steps."""
import numpy as np
import pytest

import devenv_model as dm
import devenv_replay_model as rm
import test_gpu_devcollect as on
import test_gpu_devcollect_group as gr
import test_gpu_devcollect_wide as gw
from devcollect_rows import action_draws, check_action, check_continuous, check_discontinuous

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
NS, N_EPS = (17, 65, 100), (5, 65, 108)        # less than two tiles | just over four | a ragged last tile; 108: a surplus across tiles


def wide_group(engs, envs, n_eps, **kw):
    from fsrl_amd.engine import collect_device_wide_group
    return collect_device_wide_group(engs, [v._h for v in envs], n_eps, **kw)


def member(agent, kind, hidden, i):
    """member i and its twin: env seed 3 + i, the helpers' parameters scaled by 1 + i / 8"""
    shape = dict(hidden_sizes=hidden) if isinstance(hidden, tuple) else dict(H=hidden)
    eng, env = gw.make(agent, kind, NS[i], seed=3 + i, rows_per_env=12, **shape)
    if agent == "onpolicy":
        eng.set_params((rm.onpolicy_params(eng.n_params) * (1 + i / 8)).astype(F32))
    else:
        eng.sac_put_params(0, (rm.actor_params(eng.n_sac_actor) * (1 + i / 8)).astype(F32))
    env.reset()
    return eng, env


def solo(eng, env, n_ep, **kw):
    from fsrl_amd.data.device_collector import _layered
    return (eng.collect_device_wide_layered if _layered(eng) else eng.collect_device_wide)(env._h, n_ep, **kw)


@pytest.mark.parametrize("agent,kind,hidden", [("onpolicy", "pc", 64), ("sacl", "lin33", 64), ("ddpgl", "lin64w", 256), ("onpolicy", "lin8", (32, 32, 32))],
                         ids=lambda x: "x".join(map(str, x)) if isinstance(x, tuple) else str(x))
def test_grouped_wide_collect_is_each_members_solo_wide_collect(agent, kind, hidden):
    """two grouped collects in a row, 4 step launches a batch (7 is no multiple of 4): the members finish in different batches and
    member 2 drops a surplus across tiles.  Member 1 and its twin first run a solo collect of one 8 + 1 launch batch, so that the
    members enter the grouped calls with different launch-ordinal parities."""
    kw = dict(deterministic=False, bound_method=1, max_steps_per_launch=4)
    mem, twin = ([member(agent, kind, hidden, i) for i in range(3)] for _ in range(2))
    for e, v in (mem[1], twin[1]):
        assert solo(e, v, 3, deterministic=False, bound_method=1, max_steps_per_launch=8)["launches"] % 2 == 1
    for rnd in range(2):
        res = wide_group([e for e, _ in mem], [v for _, v in mem], N_EPS, **kw)
        for i, (e, v) in enumerate(twin):
            gr.assert_same_stats(res[i], solo(e, v, N_EPS[i], **kw), f"round {rnd} member {i}")
            assert len(res[i]["ep_rews"]) == N_EPS[i]
            gr.assert_same_snapshot(gr.snapshot(*mem[i]), gr.snapshot(*twin[i]), f"round {rnd} member {i}")
        assert res[0]["launches"] >= 2 * 5
    for i in range(3):
        assert all(np.array_equal(x, y) for x, y in zip(gr.books(mem[i][0]), gr.books(twin[i][0]))), f"member {i}: books"
        assert mem[i][0].store_sizes().max() == 12          # a sub-buffer wrapped
    gr.close(*[v for _, v in mem + twin], *[e for e, _ in mem + twin])


@pytest.mark.parametrize("deterministic", [False, True], ids=["training", "deterministic"])
def test_a_grouped_member_beyond_64_envs_row_by_row_against_the_model(deterministic):
    """ROW_CASES[0] of tests/test_gpu_devcollect_wide.py as member 1 of GroupDeviceCollector over (20 wide, 65) envs: the checks of
    test_beyond_64_envs_row_by_row_against_the_model on its rows, with its bars"""
    from fsrl_amd.data import DeviceCollector, GroupDeviceCollector, HipVectorReplayBuffer
    case = gw.ROW_CASES[0]
    agent, kind, n, extra, H = case
    what = "grouped " + "-".join(map(str, case)) + (" deterministic" if deterministic else " training")
    pair = [gw.make(agent, kind, 20, H=H, seed=5), gw.make(agent, kind, n, H=H, seed=rm.ENV_SEED)]
    cols = [DeviceCollector(on.Pol(e, "clip", None, training=not deterministic), v, HipVectorReplayBuffer(e, len(v) * 200, len(v))) for e, v in pair]
    eng, env = pair[1]
    env.set_state(t=gw.t_injected(n))
    stats = GroupDeviceCollector(cols, 4).collect([25, n + extra])
    idx = eng.sample0()
    rows = eng.store_read(idx)
    done = rows["terminated"] | rows["truncated"]
    want = sorted(gw.model_rows(case, deterministic)[0], key=lambda r: r[0])
    e, ordinal, t, wdone = (np.array([r[j] for r in want]) for j in range(4))
    assert np.array_equal(idx // eng.store_geometry()[0], e) and np.array_equal(done, wdone) and np.array_equal(rows["truncated"], t == 6)
    assert done.sum() == n + extra == stats[1]["n/ep"] and stats[1]["n/st"] == len(idx) and stats[1]["total_cost"] == rows["cost"].sum() > 0
    assert stats[0]["n/ep"] == 25 and len(pair[0][0]) == stats[0]["n/st"]
    key = dm.key_of(rm.ENV_SEED)
    mu, sigma = eng.actor_forward(rows["obs"])
    draws = action_draws(rows, e, ordinal, t, key, eng.cfg.act_dim)
    check_action(agent, rows["act"], mu, sigma, *draws[:2], deterministic, draws[2], what + " act")
    dd = np.arange(eng.cfg.obs_dim)[None, :]
    r64, r32 = (dm.linear_step(rows["obs"], dm.map_action(rows["act"], 1), env.A, env.B,
                               dm.normal(key, e[:, None], ordinal[:, None], t[:, None], dm.STREAM_STEP, dd, dt), env.cost_threshold, dt) for dt in (F64, F32))
    check_continuous(rows["obs_next"], r64["obs_next"], r32["obs_next"], r32["obs_scale"], what + " obs_next")
    check_continuous(rows["rew"], r64["rew"], r32["rew"], r32["rew_scale"], what + " rew")
    check_discontinuous(rows["cost"], rows["terminated"], r32, what)
    chained = (e[1:] == e[:-1]) & ~done[:-1]
    assert np.array_equal(rows["obs_next"][:-1][chained], rows["obs"][1:][chained]) and chained.sum() > 0
    fresh = t == 0          # an episode that began inside the collect starts at the model's reset draw
    check_continuous(rows["obs"][fresh], *(dm.normal(key, e[fresh, None], ordinal[fresh, None], 0, dm.STREAM_RESET, dd, dt) for dt in (F64, F32)),
                     dm.normal_scale(key, e[fresh, None], ordinal[fresh, None], 0, dm.STREAM_RESET, dd), what + " first obs")
    _, t1, ord1 = env.get_state()
    assert np.all(t1 == 0) and np.all(ord1 >= 2)            # every env was reset at the end
    gr.close(*[v for _, v in pair], *[e for e, _ in pair])


def test_refusals_name_the_member_and_change_nothing():
    from fsrl_amd.env import DevicePointCircle
    made = []

    def make(*a, **kw):
        made.append(gw.make(*a, **kw))
        made[-1][1].reset()
        return made[-1]

    def refused(members, match, envs=None):
        envs = envs or [v for _, v in members]
        before = [(v.get_state(), len(e)) for e, v in members]
        with pytest.raises(AssertionError, match=match):
            wide_group([e for e, _ in members], envs, 3)
        for (e, v), (state, rows) in zip(members, before):
            assert all(np.array_equal(x, y) for x, y in zip(state, v.get_state())) and len(e) == rows

    a, twin, b = make("onpolicy", "pc", 70), make("onpolicy", "pc", 70), make("onpolicy", "pc", 66, seed=4)
    narrow = make("onpolicy", "pc", 5, wide=False)
    refused([a, narrow], "member 1: .*wide device env")
    refused([a, b], "member 1: its device env is listed twice", envs=[a[1], a[1]])
    refused([a, make("onpolicy", "pc", 70, hidden_sizes=(32, 32, 32))], "member 1 is a layered context and member 0 a fused one")
    long_env = DevicePointCircle(b[0], 66, max_episode_steps=9, seed=4, **on.PC)
    refused([a, (b[0], long_env)], "member 1: .*max_episode_steps")
    long_env.close()
    refused([make("sacl", "lin8", 70), make("sacl", "lin8", 70, per=(0.6, 0.4))], "member 1: .*prioritised")
    res = [e.collect_device_wide(v._h, 75, deterministic=False, bound_method=1, max_steps_per_launch=4) for e, v in (a, twin)]
    gr.assert_same_stats(*res, "after the refusals")
    gr.assert_same_snapshot(gr.snapshot(*a), gr.snapshot(*twin), "after the refusals")
    gr.close(*[v for _, v in made], *[e for e, _ in made])
