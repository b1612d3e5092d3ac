"""Wide device collects (fsrl_collect_device_wide: one launch per vector step, a workgroup per 16-row tile) against the looping
kernel bit for bit up to 64 envs, beyond 64 row by row against the float64 model by the rule and bars of tests/devcollect_rows.py
(DESIGN.md 6), as a store (store_push twin, one ppo_update), and its refusals.  Episodes are cut at 7 steps; hidden 64 unless said.
ROW_CASES start from injected step counts, so that episodes end in different vector steps and tiles and one surplus drop takes
positions out of several tiles; their rows stay out of the discontinuity band (tests/test_devcollect_wide_host.py, on the CPU)."""
import numpy as np
import pytest

import devenv_model as dm
import devenv_replay_model as rm
import test_gpu_devcollect as on
import test_gpu_devcollect_group as gr
import test_gpu_devcollect_replay as rp
from devcollect_rows import action_draws, check_action, check_continuous, check_discontinuous

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
# (agent, env, env_num, n_episode - env_num, hidden): the last one is the register-tight instantiation and the widest head row
ROW_CASES = [("onpolicy", "lin8", 65, 3, 64), ("sacl", "lin8", 100, 40, 64), ("cvpo", "lin33", 100, 3, 64), ("onpolicy", "lin8", 257, 40, 64),
             ("ddpgl", "lin64w", 65, 3, 256)]


def t_injected(n):
    return np.random.default_rng(n).integers(0, 7, n).astype(np.int32)


def model_rows(case, deterministic):
    """the case as a closed loop of the float32 model with the oracles' CPU actor -> (rows (env, ordinal, t, done) in the collect's
    order, band flags per row).  The linear env ends episodes by the time limit alone, so the row list is exact."""
    agent, kind, n, extra, H = case
    Do, Da = rm.SHAPES[kind]
    host = rm.linear_host(kind, n)
    env = dm.ModelEnv(dm.LINEAR, n, 7, rm.ENV_SEED, (0.7, ), Do, Da, host.A, host.B, dtype=F32)
    actor, near = rm.case_actor((agent, kind, n, n + extra, H, {})), []
    step = env.step
    env.step = lambda act, ids=None: near.append(dm.band_share(r := step(act, ids))[1]) or r

    def policy(obs, ids):
        m, sigma = actor(obs)
        eps = env.action_noise(ids, F32)
        act = (m + sigma * eps).astype(F32) if agent == "onpolicy" and not deterministic else rm.action(rm.formula(agent), m, sigma, eps, deterministic, F32)
        return dm.map_action(act, 1)
    env.reset()
    env.t[:] = t_injected(n)
    return dm.collect(env, n + extra, policy)[0], np.concatenate(near)


def make(agent, kind, n, H=64, wide=True, **kw):
    """-> (engine, device env) of the helpers' make(); wide: the env made again as a wide one (above 64 envs it is one already)"""
    eng, env = on.make(kind, n, H=H, oracle_params=True, **kw) if agent == "onpolicy" else rp.make(agent, kind, n, H=H, **kw)
    if wide and not env.wide:
        from fsrl_amd.env import DeviceLinear, DevicePointCircle
        env.close()
        seed = kw.get("seed", 3)
        env = DevicePointCircle(eng, n, max_episode_steps=7, seed=seed, wide=True, **on.PC) if kind == "pc" else DeviceLinear(eng, like=rm.linear_host(kind, n), seed=seed, wide=True)
    return eng, env


@pytest.mark.parametrize("n", [17, 64])
@pytest.mark.parametrize("agent,kind", [("onpolicy", "pc"), ("sacl", "lin33")])
def test_wide_collect_is_the_looping_collect_bit_for_bit(agent, kind, n):
    """training-mode collects of n_episode below, equal to and above env_num, 4 launches per batch: batches end on steps with finished
    episodes (every 7th step ends all episodes of the linear env; 7 is no multiple of 4)"""
    out = []
    for wide in (False, True):
        eng, env = make(agent, kind, n, wide=wide, rows_per_env=12)
        env.reset()
        run = eng.collect_device_wide if wide else eng.collect_device
        res = [run(env._h, n_ep, deterministic=False, bound_method=1, max_steps_per_launch=4) for n_ep in (5, n, n + 8)]
        Do, Da = eng.cfg.obs_dim, eng.cfg.act_dim
        snap = gr.snapshot(eng, env)
        books = eng.push(np.arange(n), np.zeros((n, Do), F32), np.zeros((n, Da), F32), np.full(n, 0.25), np.ones(n), np.ones(n, bool), np.zeros(n, bool),
                         np.ones((n, Do), F32))
        out.append((res, snap, books))
        gr.close(env, eng)
    (ra, sa, ba), (rb, sb, bb) = out
    for x, y in zip(ra, rb):
        gr.assert_same_stats(x, y, f"{agent} {kind} n={n}")
    assert rb[2]["launches"] >= 2 * 5 and sa["sizes"].max() == 12           # at least two batches of 4 + 1 launches; a sub-buffer wrapped
    gr.assert_same_snapshot(sa, sb, f"{agent} {kind} n={n}")
    assert all(np.array_equal(x, y) for x, y in zip(ba, bb)), "books"


@pytest.mark.parametrize("deterministic", [False, True], ids=["training", "deterministic"])
@pytest.mark.parametrize("case", ROW_CASES, ids=lambda c: "-".join(map(str, c)))
def test_beyond_64_envs_row_by_row_against_the_model(case, deterministic):
    agent, kind, n, extra, H = case
    what = "-".join(map(str, case)) + (" deterministic" if deterministic else " training")
    eng, env = make(agent, kind, n, H=H, seed=rm.ENV_SEED)
    env.reset()
    env.set_state(t=t_injected(n))
    res = eng.collect_device_wide(env._h, n + extra, deterministic=deterministic, bound_method=1, max_steps_per_launch=4)
    idx = eng.sample0()
    rows = eng.store_read(idx)
    done = rows["terminated"] | rows["truncated"]
    # ---- who stepped when: the model's rows, env-major (the surplus rule, tile by tile, decides which envs went on)
    want = sorted(model_rows(case, deterministic)[0], key=lambda r: r[0])
    e, ordinal, t, wdone = (np.array([r[j] for r in want]) for j in range(4))
    assert np.array_equal(idx // eng.store_geometry()[0], e) and np.array_equal(done, wdone) and np.array_equal(rows["truncated"], t == 6)
    assert done.sum() == n + extra == len(res["ep_rews"]) and res["steps"] == len(idx) and res["total_cost"] == rows["cost"].sum() > 0
    assert sorted(res["ep_lens"].tolist()) == sorted((t[done] + 1 - np.where(ordinal[done] == 0, t_injected(n)[e[done]], 0)).tolist())
    # ---- the action, the transition
    key = dm.key_of(rm.ENV_SEED)
    if agent == "onpolicy":
        mu, sigma = eng.actor_forward(rows["obs"])
        check_action(agent, rows["act"], mu, sigma, *action_draws(rows, e, ordinal, t, key, eng.cfg.act_dim)[:2], deterministic,
                     action_draws(rows, e, ordinal, t, key, eng.cfg.act_dim)[2], what + " act")
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
    fresh = t == 0          # an episode that began inside the collect starts at the model's reset draw
    check_continuous(rows["obs"][fresh], *(dm.normal(key, e[fresh, None], ordinal[fresh, None], 0, dm.STREAM_RESET, dd, dt) for dt in (F64, F32)),
                     dm.normal_scale(key, e[fresh, None], ordinal[fresh, None], 0, dm.STREAM_RESET, dd), what + " first obs")
    _, t1, ord1 = env.get_state()
    assert np.all(t1 == 0) and np.all(ord1 >= 2)            # every env was reset at the end
    gr.close(env, eng)


def test_the_store_is_a_store():
    """the rows of a wide collect at 100 envs pushed into a twin context one vector step at a time: the same store, and one
    ppo_update on each gives the same parameters bit for bit (the method of tests/test_gpu_devcollect.py)"""
    n, n_eps = 100, (130, 40)
    eng_a, env_a = make("onpolicy", "lin8", n, rows_per_env=400)
    eng_b, env_b = make("onpolicy", "lin8", n, rows_per_env=9)
    eng_c, env_c = make("onpolicy", "lin8", n, rows_per_env=9)
    for eng, env in ((eng_a, env_a), (eng_b, env_b)):
        env.reset()
        res = [eng.collect_device_wide(env._h, n_ep, deterministic=False, bound_method=1) for n_ep in n_eps]
    idx_a, rows_a = on.store_rows(eng_a)
    queues = {e: list(np.flatnonzero(idx_a // eng_a.store_geometry()[0] == e)) for e in range(n)}
    got = rp.push_collects(eng_c, rows_a, queues, n, n_eps)
    assert all(len(q) == 0 for q in queues.values())
    assert all(r["ep_rews"].tolist() == g[0] and r["ep_lens"].tolist() == g[1] for r, g in zip(res, got))
    gr.assert_same_snapshot(dict(gr.snapshot(eng_b, env_b), state=()), dict(gr.snapshot(eng_c, env_c), state=()), "store")
    assert eng_b.store_sizes().max() == 9
    ub, uc = (np.asarray(eng.ppo_update([0.3], 1 / 1.3, 64, 2, seed=5)[0]) for eng in (eng_b, eng_c))
    assert np.array_equal(ub, uc) and np.array_equal(eng_b.get_params(), eng_c.get_params())
    gr.close(env_a, env_b, env_c, eng_a, eng_b, eng_c)


def test_refusals_name_their_reason_and_change_nothing():
    import ctypes as C
    from fsrl_amd import _lib
    from fsrl_amd.data import DeviceCollector
    from fsrl_amd.engine import TrajArchive, collect_device_group

    def refused(eng, env, match, run=None, **kw):
        before, n_before = env.get_state(), len(eng)
        with pytest.raises(AssertionError, match=match):
            (run or eng.collect_device_wide)(env._h, 3, **kw)
        assert all(np.array_equal(x, y) for x, y in zip(before, env.get_state())) and len(eng) == n_before

    eng, env = make("onpolicy", "pc", 70)
    env.reset()
    for run in (eng.collect_device, eng.evaluate_device, eng.collect_device_layered, lambda h, k: collect_device_group([eng], [h], k)):
        refused(eng, env, "fsrl_collect_device_wide", run=run)
    with pytest.raises(ValueError, match="collect_device_wide"):
        DeviceCollector(on.Pol(eng), env)
    arch = TrajArchive(eng, 1000, 100, 50)
    arch.attach(eng)
    refused(eng, env, "trajectory tap")
    arch.detach(eng); arch.close()
    cfg, h = _lib.DevEnvConfig(), C.c_void_p()
    cfg.kind, cfg.env_num, cfg.obs_dim, cfg.act_dim, cfg.max_episode_steps = 0, 65, 6, 2, 7
    with pytest.raises(AssertionError, match="env_num 65"):
        _lib.check(eng.lib.fsrl_devenv_create(eng._ctx, C.byref(cfg), C.byref(h)))
    cfg.env_num = 4097
    with pytest.raises(AssertionError, match="env_num 4097"):
        _lib.check(eng.lib.fsrl_devenv_create_wide(eng._ctx, C.byref(cfg), C.byref(h)))
    narrow, env_n = on.make("pc", 5)
    refused(narrow, env_n, "fsrl_devenv_create_wide")
    gr.close(env, env_n, eng, narrow)
    eng, env = make("onpolicy", "lin8", 70, hidden_sizes=(32, 32, 32))
    refused(eng, env, "layered")
    gr.close(env, eng)
    eng, env = make("sacl", "lin8", 70, per=(0.6, 0.4))
    refused(eng, env, "prioritised")
    gr.close(env, eng)
    from fsrl_amd.engine import Engine, EngineConfig, EngineGroup
    engs = [Engine(EngineConfig(obs_dim=6, act_dim=2, hidden=64, env_num=70, buffer_size=7000), device=0) for _ in range(2)]
    group = EngineGroup(engs)
    from fsrl_amd.env import DevicePointCircle
    env = DevicePointCircle(engs[0], 70, max_episode_steps=7)
    refused(engs[0], env, "grouped")
    env.close(); group.close()
    gr.close(*engs)
