"""Wide device collects for LAYERED contexts (fsrl_collect_device_wide_layered, kernels_devcollect_wide_layered.hpp) against the
looping layered collect bit for bit up to 64 envs, beyond 64 row by row against the float64 model by the rule and bars of
tests/devcollect_rows.py, and its refusals.  Episodes are cut at 7 steps.  The rows of ROW_CASES stay out of the
discontinuity band and their surplus drops spread over tiles (tests/test_devcollect_wide_layered_host.py, on the CPU)."""
import numpy as np
import pytest

import devenv_model as dm
import devenv_replay_model as rm
import test_gpu_devcollect as on
import test_gpu_devcollect_group as gr
import test_gpu_devcollect_layered as gl
import test_gpu_devcollect_replay as rp
import test_gpu_devcollect_wide as gw
from devcollect_rows import action_draws, check_action, check_continuous, check_discontinuous
from fsrl_amd._lib import DCWL_LDS_WIDTH as W

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
# (agent, hidden_sizes, force_layered, env kind, env_num): the smallest shapes at which the tile actor can go wrong
TWINS = [("onpolicy", (32, 32, 32), False, "pc", 17), ("sacl", (50, 30, 18), False, "lin33", 64), ("onpolicy", (16, ) * 8, False, "lin8", 16),
         ("ddpgl", (64, ), False, "lin20", 5), ("onpolicy", (64, 64), True, "pc", 17), ("onpolicy", (W, ), False, "lin8", 17),
         ("onpolicy", (W + 16, ), False, "lin8", 17)]
# (agent, env, env_num, n_episode - env_num, hidden_sizes): a last tile of one row; unaligned weight rows; 17 workspace slices
ROW_CASES = [("onpolicy", "lin8", 65, 3, (32, 32, 32)), ("sacl", "lin33", 100, 40, (50, 30, 18)), ("onpolicy", "lin8", 257, 40, (W + 16, ))]
ids = lambda c: "-".join(str(x).replace(" ", "") for x in c)


def make(agent, kind, n, hs, wide=True, seed=3, **kw):
    """-> (layered engine with the CPU tests' actor, device env; wide: made again as a wide one where it is none)"""
    eng, env = gl.make_onpolicy(kind, n, hs, seed=seed, **kw) if agent == "onpolicy" else gl.make_replay(agent, kind, n, hs, seed=seed, **kw)
    if wide and not env.wide:
        from fsrl_amd.env import DeviceLinear, DevicePointCircle
        env.close()
        env = DevicePointCircle(eng, n, max_episode_steps=7, seed=seed, wide=True, **on.PC) if kind == "pc" else DeviceLinear(eng, like=rm.linear_host(kind, n), seed=seed, wide=True)
    return eng, env


def model_rows(case, deterministic):
    """gw.model_rows with the case's layered actor -> (rows (env, ordinal, t, done) in the collect's order, band flags per row)"""
    agent, kind, n, extra, hs = case
    Do, Da = rm.SHAPES[kind]
    host = rm.linear_host(kind, n)
    env = dm.ModelEnv(dm.LINEAR, n, 7, rm.ENV_SEED, (0.7, ), Do, Da, host.A, host.B, dtype=F32)
    actor, near = rm.case_actor((agent, kind, n, n + extra, 0, {"hidden_sizes": hs})), []
    step = env.step
    env.step = lambda act, ids=None: near.append(dm.band_share(r := step(act, ids))[1]) or r

    def policy(obs, ids):
        m, sigma = actor(obs)
        eps = env.action_noise(ids, F32)
        act = (m + sigma * eps).astype(F32) if agent == "onpolicy" and not deterministic else rm.action(rm.formula(agent), m, sigma, eps, deterministic, F32)
        return dm.map_action(act, 1)
    env.reset()
    env.t[:] = gw.t_injected(n)
    return dm.collect(env, n + extra, policy)[0], np.concatenate(near)


@pytest.mark.parametrize("agent,hs,forced,kind,n", TWINS, ids=[ids(c) for c in TWINS])
def test_wide_layered_collect_is_the_looping_layered_collect_bit_for_bit(agent, hs, forced, kind, n):
    """training-mode collects of n_episode below, equal to and above env_num, 4 launches per batch, sub-buffers that wrap"""
    out = []
    for wide in (False, True):
        eng, env = make(agent, kind, n, hs, wide=wide, rows_per_env=12, **({"force_layered": True} if forced else {}))
        env.reset()
        run = eng.collect_device_wide_layered if wide else eng.collect_device_layered
        res = [run(env._h, n_ep, deterministic=False, bound_method=1, max_steps_per_launch=4) for n_ep in (5, n, n + 8)]
        Do, Da = eng.cfg.obs_dim, eng.cfg.act_dim
        snap = gr.snapshot(eng, env)
        books = eng.push(np.arange(n), np.zeros((n, Do), F32), np.zeros((n, Da), F32), np.full(n, 0.25), np.ones(n), np.ones(n, bool), np.zeros(n, bool),
                         np.ones((n, Do), F32))
        out.append((res, snap, books))
        gr.close(env, eng)
    (ra, sa, ba), (rb, sb, bb) = out
    for x, y in zip(ra, rb):
        gr.assert_same_stats(x, y, ids((agent, hs, kind, n)))
    assert rb[2]["launches"] >= 2 * 5 and sa["sizes"].max() == 12           # at least two batches of 4 + 1 launches; a sub-buffer wrapped
    gr.assert_same_snapshot(sa, sb, ids((agent, hs, kind, n)))
    assert all(np.array_equal(x, y) for x, y in zip(ba, bb)), "books"


@pytest.mark.parametrize("deterministic", [False, True], ids=["training", "deterministic"])
@pytest.mark.parametrize("case", ROW_CASES, ids=[ids(c) for c in ROW_CASES])
def test_beyond_64_envs_row_by_row_against_the_model(case, deterministic):
    agent, kind, n, extra, hs = case
    what = ids(case) + (" deterministic" if deterministic else " training")
    eng, env = make(agent, kind, n, hs, seed=rm.ENV_SEED)
    env.reset()
    env.set_state(t=gw.t_injected(n))
    res = eng.collect_device_wide_layered(env._h, n + extra, deterministic=deterministic, bound_method=1, max_steps_per_launch=4)
    idx = eng.sample0()
    rows = eng.store_read(idx)
    done = rows["terminated"] | rows["truncated"]
    # ---- who stepped when: the model's rows, env-major (the surplus rule, tile by tile, decides which envs went on)
    e, ordinal, t, wdone = (np.array([r[j] for r in sorted(model_rows(case, deterministic)[0], key=lambda r: r[0])]) for j in range(4))
    assert np.array_equal(idx // eng.store_geometry()[0], e) and np.array_equal(done, wdone) and np.array_equal(rows["truncated"], t == 6)
    assert done.sum() == n + extra == len(res["ep_rews"]) and res["steps"] == len(idx) and res["total_cost"] == rows["cost"].sum() > 0
    # ---- the action, the transition
    key = dm.key_of(rm.ENV_SEED)
    if agent == "onpolicy":
        mu, sigma = eng.actor_forward(rows["obs"])
        eps64, eps32, nscale = action_draws(rows, e, ordinal, t, key, eng.cfg.act_dim)
        check_action(agent, rows["act"], mu, sigma, eps64, eps32, deterministic, nscale, what + " act")
    else:
        rp.replay_action_check(eng, agent, deterministic, what, rows, e, ordinal, t, key)
    dd = np.arange(eng.cfg.obs_dim)[None, :]
    r64, r32 = (dm.linear_step(rows["obs"], dm.map_action(rows["act"], 1), env.A, env.B,
                               dm.normal(key, e[:, None], ordinal[:, None], t[:, None], dm.STREAM_STEP, dd, dt), env.cost_threshold, dt) for dt in (F64, F32))
    check_continuous(rows["obs_next"], r64["obs_next"], r32["obs_next"], r32["obs_scale"], what + " obs_next")
    check_continuous(rows["rew"], r64["rew"], r32["rew"], r32["rew_scale"], what + " rew")
    check_discontinuous(rows["cost"], rows["terminated"], r32, what)
    chained = (e[1:] == e[:-1]) & ~done[:-1]
    assert np.array_equal(rows["obs_next"][:-1][chained], rows["obs"][1:][chained]) and chained.sum() > 0
    assert np.all(env.get_state()[1] == 0)          # every env was reset at the end
    gr.close(env, eng)


def test_refusals_name_their_reason_and_change_nothing():
    from fsrl_amd.engine import Engine, EngineConfig, EngineGroup
    from fsrl_amd.env import DevicePointCircle

    def refused(eng, env, match):
        before, n_before = env.get_state(), len(eng)
        with pytest.raises(AssertionError, match=match):
            eng.collect_device_wide_layered(env._h, 3)
        assert all(np.array_equal(x, y) for x, y in zip(before, env.get_state())) and len(eng) == n_before
        gr.close(env, eng)
    refused(*gw.make("onpolicy", "pc", 70), "fsrl_collect_device_wide")                        # a fused context
    refused(*make("onpolicy", "pc", 5, (32, 32, 32), wide=False), "fsrl_devenv_create_wide")    # an env that is not wide
    refused(*make("sacl", "lin8", 70, (32, 32, 32), per=(0.6, 0.4)), "prioritised")
    engs = [Engine(EngineConfig(obs_dim=6, act_dim=2, hidden=64, hidden_sizes=(32, 32, 32), env_num=70, buffer_size=7000), device=0) for _ in range(2)]
    group = EngineGroup(engs)
    env = DevicePointCircle(engs[0], 70, max_episode_steps=7)
    before = env.get_state()
    with pytest.raises(AssertionError, match="grouped"):
        engs[0].collect_device_wide_layered(env._h, 3)
    assert all(np.array_equal(x, y) for x, y in zip(before, env.get_state())) and len(engs[0]) == 0
    env.close(); group.close()
    gr.close(*engs)
