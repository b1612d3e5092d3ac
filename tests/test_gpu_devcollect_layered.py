"""Whole collects and evaluations on the GPU for LAYERED contexts (fsrl_collect_device_layered, fsrl_evaluate_device_layered;
fsrl_amd/csrc/kernels_devcollect_layered.hpp) against the lock-step path, the host model of tests/devenv_model.py and their own
solo / storing twins.  The cases are tests/devcollect_layered_cases.py's; their CPU preconditions (rows out of the discontinuity
band, costs and terminations both occurring, the caps on envs and episodes) are asserted in tests/test_devcollect_layered_model.py.
Episodes are cut at 7 steps.

The bars are those of tests/test_gpu_devcollect.py, no new tolerance: deterministic on-policy collects equal
FastCollector(device_actor=True) over the stepped env bit for bit (every layer's output element is accumulated by the MFMA sequence
of the layered forward launches); training-mode rows are held row by row to the float64-yardstick rule of DESIGN.md 6 for
continuous outputs, equality outside the band for discontinuous ones, at most 2 % of the rows inside it, asserted from the float32
restatement alone (devcollect_rows.check_discontinuous)."""
import numpy as np
import pytest

import devcollect_layered_cases as lc
import devenv_replay_model as rm
import test_gpu_devcollect as on
import test_gpu_devcollect_replay as rp
from devcollect_rows import action_draws, check_action, check_collect_rows

pytestmark = pytest.mark.gpu
F32 = np.float32


def close(*xs):
    for x in xs:
        x.close()


def make_onpolicy(kind, n, hidden_sizes, seed=3, params_seed=None, **kw):
    eng, env = on.make(kind, n, seed=seed, hidden_sizes=hidden_sizes, oracle_params=True, **kw)
    if params_seed is not None:
        eng.set_params((0.3 * np.random.default_rng(params_seed).standard_normal(eng.n_params)).astype(F32))
    return eng, env


def make_replay(agent, kind, n, hidden_sizes, seed=rm.ENV_SEED, params_seed=None, **kw):
    """a layered replay engine whose actor is the CPU tests' (rm.actor_params), not the initialisation's"""
    eng, env = rp.make(agent, kind, n, seed=seed, hidden_sizes=hidden_sizes, **kw)
    p = rm.actor_params(eng.n_sac_actor)
    if params_seed is not None:
        p = (0.15 * np.random.default_rng(params_seed).standard_normal(eng.n_sac_actor)).astype(F32)
    eng.sac_put_params(0, p)
    return eng, env


def same_result(a, b, launches=True):
    return all(np.array_equal(a[k], b[k]) for k in a if launches or k != "launches")


# ------------------------------------------------------------------------------------------------ 1. deterministic twins
TWINS = [(f"{sid}-{bid}", hs, forced, kind, n, eps, bound, lh, {})
         for sid, hs, forced, kind, n, eps in lc.TWIN_SHAPES for bid, bound, lh in lc.TWIN_BOUNDS]
TWINS += [(f"{lc.TWIN_HEAD_SHAPE[0]}-{hid}", ) + lc.TWIN_HEAD_SHAPE[1:] + ("clip", None, opts) for hid, opts in lc.TWIN_HEADS]


@pytest.mark.parametrize("hs,forced,kind,n,episodes,bound,low_high,opts", [t[1:] for t in TWINS], ids=[t[0] for t in TWINS])
def test_deterministic_collect_is_the_lockstep_path_bit_for_bit(hs, forced, kind, n, episodes, bound, low_high, opts):
    """DeviceCollector (which routes a layered engine to fsrl_collect_device_layered) against FastCollector(device_actor=True) over
    DeviceVectorEnv.step: rows, slots, sub-buffer sizes, env state, statistics, counters and the next update, bit for bit"""
    kw = dict(hidden_sizes=hs, oracle_params=True, **opts)
    if forced:
        kw["force_layered"] = True
    on.deterministic_collect_twins(kind, n, episodes, bound, low_high, **kw)


# ------------------------------------------------------------------------------------------------ 2. training mode, row by row
@pytest.mark.parametrize("case", lc.ROW_CASES, ids=[lc.case_id(c) for c in lc.ROW_CASES])
def test_training_collect_row_by_row_against_the_model(case):
    """The test prints the figures (device | float32 restatement, both from the float64 model, in units of the value's scale)."""
    agent, kind, n, n_ep, _, opts = case
    hs = opts["hidden_sizes"]
    eng, env = (make_onpolicy(kind, n, hs, seed=rm.ENV_SEED) if agent == "onpolicy" else make_replay(agent, kind, n, hs))
    if agent != "onpolicy":
        assert eng.n_sac_actor == rm.cpu_actor(agent, kind, hs)[1]
    env.reset()
    _, t0, ord0 = env.get_state()
    assert np.all(t0 == 0) and np.all(ord0 == 1)
    res = eng.collect_device_layered(env._h, n_ep, deterministic=False, bound_method=1)
    what = lc.case_id(case) + " training"
    check_collect_rows(eng, env, ord0, res, n_ep, kind, rm.ENV_SEED, what, action_checker(eng, agent, what))
    close(env, eng)


def action_checker(eng, agent, what):
    if agent != "onpolicy":
        return lambda rows, e, ordinal, t, key: rp.replay_action_check(eng, agent, False, what, rows, e, ordinal, t, key)

    def action(rows, e, ordinal, t, key):
        # the action noise: (act - mu) / sigma is the model's normal of (env, ordinal, t, dim); (mu, sigma) from the layered batch forward
        mu, sigma = eng.actor_forward(rows["obs"])
        eps64, eps32, nscale = action_draws(rows, e, ordinal, t, key, eng.cfg.act_dim)
        return check_action("onpolicy", rows["act"], mu, sigma, eps64, eps32, False, nscale, what + " action noise")
    return action


def test_prioritised_collect_rows_and_the_stepped_twins_tree_leaves():
    """D collects on the device; C, its twin, gets the same rows by pushes, one vector step at a time: the same store and the same
    sum-tree leaves, bit for bit.  D's rows are held to the model like every other case's."""
    agent, kind, n, n_ep, _, opts = lc.PER_CASE
    hs = opts["hidden_sizes"]
    eng_d, env_d = make_replay(agent, kind, n, hs, rows_per_env=60, per=(0.6, 0.4))
    eng_c, env_c = make_replay(agent, kind, n, hs, rows_per_env=60, per=(0.6, 0.4))
    env_d.reset()
    _, _, ord0 = env_d.get_state()
    res = eng_d.collect_device_layered(env_d._h, n_ep, deterministic=False, bound_method=1)
    what = lc.case_id(lc.PER_CASE) + " prioritised"
    check_collect_rows(eng_d, env_d, ord0, res, n_ep, kind, rm.ENV_SEED, what, action_checker(eng_d, agent, what))
    idx, rows = rp.store_rows(eng_d)
    sub, num = eng_d.store_geometry()
    queues = {e: list(np.flatnonzero(idx // sub == e)) for e in range(n)}
    pushed = rp.push_collects(eng_c, rows, queues, n, (n_ep, ))
    assert all(len(q) == 0 for q in queues.values()) and (res["ep_rews"].tolist(), res["ep_lens"].tolist()) == pushed[0]
    (idd, rd), (ic, rc) = rp.store_rows(eng_d), rp.store_rows(eng_c)
    assert np.array_equal(idd, ic) and rp.same_rows(rd, rc)
    (ld, mxd, mnd, totd), (lcv, mxc, mnc, totc) = eng_d.per_state(), eng_c.per_state()
    assert np.array_equal(ld, lcv) and (mxd, mnd, totd) == (mxc, mnc, totc)
    sizes = eng_d.store_sizes()
    written = np.concatenate([e * sub + np.arange(sizes[e]) for e in range(num)])
    assert np.all(ld[written] > 0) and np.count_nonzero(ld) == len(written) == res["steps"]
    sd, sc = eng_d.sac_update(16, rp.LAG, rp.RESC), eng_c.sac_update(16, rp.LAG, rp.RESC)       # the next update samples the same tree
    assert np.isfinite(sd).all() and np.array_equal(sd, sc)
    close(env_d, env_c, eng_d, eng_c)


# ------------------------------------------------------------------------------------------------ 3. launch cuts
@pytest.mark.parametrize("agent", ["onpolicy", "sacl"])
def test_launch_cuts_change_nothing(agent):
    out = []
    for cut in (3, 0):
        eng, env = (make_onpolicy("lin8", 17, (50, 30, 18), rows_per_env=12) if agent == "onpolicy"
                    else make_replay(agent, "lin8", 17, (50, 30, 18), rows_per_env=12))
        env.reset()
        res = [eng.collect_device_layered(env._h, n_ep, deterministic=False, bound_method=1, max_steps_per_launch=cut) for n_ep in (20, 5)]
        out.append((res, on.store_rows(eng), eng.store_sizes().copy(), env.get_state()))
        close(env, eng)
    (ra, (ia, rows_a), sza, sta), (rb, (ib, rows_b), szb, stb) = out
    assert ra[0]["launches"] > 1 and rb[0]["launches"] == 1
    for x, y in zip(ra, rb):
        assert same_result(x, y, launches=False)
    assert np.array_equal(ia, ib) and on.same_rows(rows_a, rows_b) and np.array_equal(sza, szb)
    assert all(np.array_equal(x, y) for x, y in zip(sta, stb))


# ------------------------------------------------------------------------------------------------ 4. groups
@pytest.mark.parametrize("agent", ["onpolicy", "sacl"])
def test_group_members_equal_their_own_solo_collects(agent):
    """three members with their own env_num, n_episode, env seed and parameters in one launch; each against its twin's solo call"""
    from fsrl_amd.engine import collect_device_layered

    def members():
        out = []
        for j, (n, _, seed) in enumerate(lc.GROUP_MEMBERS):
            out.append(make_onpolicy("lin8", n, lc.GROUP_HIDDEN, seed=seed, params_seed=20 + j, rows_per_env=12) if agent == "onpolicy"
                       else make_replay(agent, "lin8", n, lc.GROUP_HIDDEN, seed=seed, params_seed=20 + j, rows_per_env=12))
        return out
    grp, solo = members(), members()
    n_eps = [ep for _, ep, _ in lc.GROUP_MEMBERS]
    for _, v in grp + solo:
        v.reset()
    for cut in (4, 0):
        res = collect_device_layered([e for e, _ in grp], [v._h for _, v in grp], n_eps, deterministic=False, bound_method=1, max_steps_per_launch=cut)
        ref = [e.collect_device_layered(v._h, ep, deterministic=False, bound_method=1, max_steps_per_launch=cut) for (e, v), ep in zip(solo, n_eps)]
        for i, ((eg, vg), (es, vs)) in enumerate(zip(grp, solo)):
            assert same_result(res[i], ref[i], launches=False) and len(res[i]["ep_rews"]) == n_eps[i], i
            (ig, rg), (is_, rs) = on.store_rows(eg), on.store_rows(es)
            assert np.array_equal(ig, is_) and on.same_rows(rg, rs), f"member {i}: store rows"
            assert np.array_equal(eg.store_sizes(), es.store_sizes()) and eg.store_version() == es.store_version()
            assert on.same_state(vg, vs), f"member {i}: env state"
        assert len({r["launches"] for r in res}) == 1 and res[0]["launches"] == max(r["launches"] for r in ref)
    # the members did not all store the same rows: three parameter vectors, three env seeds
    assert not np.array_equal(on.store_rows(grp[0][0])[1]["act"][:3], on.store_rows(grp[2][0])[1]["act"][:3])
    close(*[x for pair in grp + solo for x in pair[::-1]])


# ------------------------------------------------------------------------------------------------ 5. evaluation
@pytest.mark.parametrize("agent", ["onpolicy", "sacl"])
def test_evaluation_is_the_storing_twins_collect_and_moves_nothing_else(agent):
    from fsrl_amd.env import DevicePointCircle

    def twin():
        eng, env = (make_onpolicy("pc", 5, (32, 32, 32), rows_per_env=9) if agent == "onpolicy"
                    else make_replay(agent, "pc", 5, (32, 32, 32), rows_per_env=9, per=(0.6, 0.4)))
        env.reset()
        eng.collect_device_layered(env._h, 12, deterministic=False, bound_method=1)      # a store with rows in it, wrapped
        test = DevicePointCircle(eng, 3, max_episode_steps=7, seed=9, **on.PC)
        test.reset()
        return eng, env, test
    (ev, env_e, test_e), (co, env_c, test_c) = twin(), twin()
    assert ev.store_sizes().max() == 9

    def everything(eng, env):
        idx, rows = on.store_rows(eng)
        return dict(idx=idx, rows=rows, sizes=eng.store_sizes().copy(), n=len(eng), version=eng.store_version(), env=env.get_state(),
                    blob=eng.train_state(), per=eng.per_state() if agent != "onpolicy" else None)
    before = everything(ev, env_e)
    for n_ep, det in ((7, False), (2, True)):
        r_e = ev.evaluate_device_layered(test_e._h, n_ep, deterministic=det, bound_method=1)
        r_c = co.collect_device_layered(test_c._h, n_ep, deterministic=det, bound_method=1)
        assert same_result(r_e, r_c) and len(r_e["ep_rews"]) == n_ep
        assert on.same_state(test_e, test_c)
    after = everything(ev, env_e)
    assert np.array_equal(before["idx"], after["idx"]) and on.same_rows(before["rows"], after["rows"]), "store rows"
    assert np.array_equal(before["sizes"], after["sizes"]) and before["n"] == after["n"] and before["version"] == after["version"]
    assert all(np.array_equal(x, y) for x, y in zip(before["env"], after["env"])), "the training env"
    assert before["blob"] == after["blob"], "the exported training state: parameters, optimiser state, random streams, books, store"
    if agent != "onpolicy":
        assert np.array_equal(before["per"][0], after["per"][0]) and before["per"][1:] == after["per"][1:]
    assert co.store_version() > before["version"]
    close(test_e, test_c, env_e, env_c, ev, co)


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_name_their_reason_and_change_nothing():
    from fsrl_amd._lib import FsrlHipError
    from fsrl_amd.engine import collect_device_layered, evaluate_device_layered

    def refused(engs, envs, match, exc=AssertionError, fn=collect_device_layered, **kw):
        before = [(v.get_state(), len(e), e.store_version()) for e, v in zip(engs, envs)]
        with pytest.raises(exc, match=match):
            fn(engs, [v._h for v in envs], 3, **kw)
        for (st, n, ver), e, v in zip(before, engs, envs):
            assert all(np.array_equal(x, y) for x, y in zip(st, v.get_state())) and len(e) == n and e.store_version() == ver

    lay, env_l = make_onpolicy("pc", 5, (32, 32, 32))
    lay_b, env_lb = make_onpolicy("pc", 5, (32, 32, 32))
    narrow, env_n = make_onpolicy("pc", 5, (32, 32, 16))
    fused, env_f = on.make("pc", 5)
    for v in (env_l, env_lb, env_n, env_f):
        v.reset()
    # a fused member, alone and in a group; the message names the call that takes it
    refused([fused], [env_f], "fsrl_collect_device")
    refused([fused], [env_f], "fsrl_evaluate_device", fn=evaluate_device_layered)
    refused([lay, fused], [env_l, env_f], r"member 1: .*fsrl_collect_device")
    refused([fused, lay], [env_f, env_l], r"member 0: .*fsrl_collect_device")
    # unequal hidden_sizes
    refused([lay, narrow], [env_l, env_n], r"member 1: .*hidden_sizes")
    # an env of another context
    refused([lay], [env_lb], "another context")
    refused([lay, lay_b], [env_l, env_l], "member 1")
    # what the fused calls refuse
    refused([lay], [env_l], "bound_method", bound_method=7)
    refused([lay], [env_l], "max_steps_per_launch", max_steps_per_launch=5000)
    # inside an update
    lay.collect_device_layered(env_l._h, 5, bound_method=1)
    lay.ppo_begin([0.3], 1 / 1.3, 16)
    refused([lay], [env_l], "fsrl_collect_device_layered inside an update", exc=FsrlHipError)
    refused([lay], [env_l], "fsrl_evaluate_device_layered inside an update", exc=FsrlHipError, fn=evaluate_device_layered)
    lay.ppo_abort()
    # the fused entry points keep their refusal and its text
    with pytest.raises(AssertionError, match="not supported on layered contexts yet"):
        lay.collect_device(env_l._h, 3)
    # ... and after all that the layered call still runs
    assert lay.collect_device_layered(env_l._h, 3, bound_method=1)["steps"] > 0
    close(env_l, env_lb, env_n, env_f, lay, lay_b, narrow, fused)
    # a replay context nothing was initialised on
    eng, env = rp.make("sacl", "lin8", 4, hidden_sizes=(32, 32, 32), init=False)
    env.reset()
    refused([eng], [env], "replay contexts")
    close(env, eng)


# ------------------------------------------------------------------------------------------------ 7. facade
@pytest.mark.parametrize("algo", ["ppol", "sacl"])
def test_layered_agents_learn_over_device_envs(algo, tmp_path):
    from fsrl_amd.agent import PPOLagAgent, SACLagAgent
    from fsrl_amd.data import DeviceCollector
    from fsrl_amd.env import DevicePointCircle, PointCircleEnv
    from fsrl_amd.env.device import DeviceVectorEnv
    from fsrl_amd.utils import BaseLogger
    Agent = PPOLagAgent if algo == "ppol" else SACLagAgent
    agent = Agent(PointCircleEnv(), BaseLogger(str(tmp_path), name="d"), cost_limit=10, device="cuda:0", seed=3, hidden_sizes=(32, 32, 32),
                  training_num=4)
    train = DevicePointCircle(agent.policy, 4, max_episode_steps=20, seed=1)
    seen, stepped = [], []
    orig, orig_step = DeviceCollector.collect, DeviceVectorEnv.step

    def spy(self, *a, **k):
        seen.append(self)
        return orig(self, *a, **k)

    def spy_step(self, *a, **k):
        stepped.append(self)
        return orig_step(self, *a, **k)
    DeviceCollector.collect, DeviceVectorEnv.step = spy, spy_step
    eng = agent.policy.engine
    get = (lambda: eng.get_params()) if algo == "ppol" else (lambda: eng.sac_get_params(0)[0])
    try:
        theta0 = get()
        kw = dict(repeat_per_collect=2) if algo == "ppol" else dict(update_per_step=0.1)
        ep, stat, info = agent.learn(train, None, epoch=1, episode_per_collect=4, step_per_epoch=160, batch_size=32, verbose=False,
                                     save_ckpt=False, **kw)
    finally:
        DeviceCollector.collect, DeviceVectorEnv.step = orig, orig_step
    assert ep == 1 and len(seen) >= 2 and all(isinstance(c, DeviceCollector) and c.env is train for c in seen)
    assert not stepped                                          # no call-by-call step: every training collect was a device collect
    assert np.isfinite(list(stat.values())).all() and "train/reward" in stat
    assert np.abs(get() - theta0).max() > 1e-6
    train.close()
