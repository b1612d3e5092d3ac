"""Whole collects on the GPU for the replay agents (fsrl_collect_device on SAC-Lag, DDPG-Lag and CVPO contexts) against the host model
of tests/devenv_model.py and the head arithmetic of tests/devenv_replay_model.py.  Hidden (64, 64) (one test at (256, 256)),
episodes cut at 7 steps; point-circle, the linear env at obs 8 / act 2 and obs 33 / act 8 (SAC-Lag's full 16-column head row) and
at obs 20 / act 16 (DDPG-Lag's widest head); env_num 1 / 5 / 17 / 64.

The bars are those of tests/test_gpu_devcollect.py: continuous outputs by the float64-yardstick rule of DESIGN.md 6 (the device at
most 3 x as far from float64 as the float32 restatement, never held tighter than one float32 ulp at the value's scale; the scale of
an action is max(1, |m| + |sigma eps|), which bounds the squashed action too), discontinuous outputs equal outside a band of
1e-5 x scale around the threshold that at most 2 % of the rows may lie in.  (m, sigma) of a stored row are what
Engine.sac_actor_forward gives for its observation.  Bitwise equality with FastCollector is not asked of replay contexts: the host's
tanh / exp and the device's differ in the last bits.  Stores, bookkeeping, prioritised replay's tree and the next update ARE
compared bit for bit, against the same rows pushed one vector step at a time into a twin context."""
import numpy as np
import pytest

import devenv_replay_model as rm
from devcollect_rows import action_draws, check_action, check_collect_rows

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
PC, SHAPES = rm.PC, rm.SHAPES
LAG, RESC = [0.5], 1 / 1.5
ROW_KEYS = ("obs", "act", "rew", "cost", "terminated", "truncated", "obs_next")


def make(agent, kind, n, H=64, rows_per_env=200, seed=3, sub_buffers=None, init=True, per=None, unbounded=None,
         exploration_sigma=rm.EXPLORATION_SIGMA, **cfg):
    """-> (replay engine of `agent` with fixed random actor and critic parameters, device env of `kind`).  unbounded: the actor-mean
    option of SAC-Lag and CVPO (None: the agent's default); max_action goes to the EngineConfig with the rest of cfg"""
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig
    from fsrl_amd.env import DeviceLinear, DevicePointCircle
    Do, Da = SHAPES[kind]
    kw = dict(obs_dim=Do, act_dim=Da, hidden=H, env_num=sub_buffers or n, buffer_size=(sub_buffers or n) * rows_per_env, algo=_lib.ALGO_SAC_LAG)
    kw.update(cfg)
    eng = Engine(EngineConfig(**kw), device=0)
    if init:
        if agent == "sacl":
            eng.sac_init(unbounded=unbounded)
        elif agent == "ddpgl":
            eng.sac_init(deterministic=True, exploration_sigma=exploration_sigma)
        else:
            eng.cvpo_init(qc_thres=5.0, unbounded=unbounded)
        if "hidden_sizes" not in cfg:
            eng.sac_put_params(0, rm.actor_params(eng.n_sac_actor))           # the actor of the CPU test's closed loop
            eng.sac_put_params(1, (0.15 * np.random.default_rng(8).standard_normal(eng.n_sac_critics)).astype(F32))
            eng.sac_put_params(2, eng.sac_get_params(1)[0])
        if per:
            eng.per_enable(*per)
    if kind == "pc":
        env = DevicePointCircle(eng, n, max_episode_steps=7, seed=seed, **PC)
    else:
        env = DeviceLinear(eng, like=rm.linear_host(kind, n), seed=seed)
    return eng, env


def store_rows(eng):
    """(indices, rows) of the whole store in sample(0) order: env-major, chronological"""
    idx = eng.sample0()
    return idx, eng.store_read(idx)


def same_rows(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ROW_KEYS)


def push_collects(eng, rows, queues, n, n_eps):
    """the collect loop of FastCollector fed from per-env queues of row numbers of `rows`, one push per vector step
    -> per collect (episode returns, episode lengths) in the order the loop met them"""
    out = []
    for n_ep in n_eps:
        ready, episodes, got_r, got_l = list(range(min(n, n_ep))), 0, [], []
        while episodes < n_ep:
            take = [queues[e].pop(0) for e in ready]
            ptr, er, el, ei = eng.push(np.array(ready), *(rows[k][take] for k in ROW_KEYS))
            done = rows["terminated"][take] | rows["truncated"][take]
            local = list(np.flatnonzero(done))
            if local:
                episodes += len(local)
                got_r += list(er[local]); got_l += list(el[local])
                surplus = len(ready) - (n_ep - episodes)
                if surplus > 0:
                    ready = [e for p, e in enumerate(ready) if p not in local[:surplus]]
        out.append((got_r, got_l))
    return out


# ------------------------------------------------------------------------------------------------ 1. row by row
@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("agent,kind,n,n_ep", rm.CASES)
def test_collect_row_by_row_against_the_model(agent, kind, n, n_ep, deterministic):
    """The test prints the figures; measured on an MI355X they are in DESIGN.md 3.4.1 "Replay agents": `act` at most 2.2e-7 from
    float64 in units of its scale (the float32 restatement: up to 1.6e-6), `obs_next` and `rew` the restatement's own distance, no
    row within the band.  A deterministic DDPG-Lag action sat at 1.19e-7, the one-ulp floor of the rule exactly: the host's tanh in
    (m, sigma) and the device's, each within an ulp of a value in [0.5, 1).  That the rows of these cases stay out of the band is
    also asserted without a GPU, in tests/test_devenv_replay_model.py."""
    eng, env = make(agent, kind, n, seed=rm.ENV_SEED)
    assert eng.n_sac_actor == rm.cpu_actor(agent, kind)[1]
    env.reset()
    _, t0, ord0 = env.get_state()
    assert np.all(t0 == 0) and np.all(ord0 == 1)
    res = eng.collect_device(env._h, n_ep, deterministic=deterministic, bound_method=1)
    what = f"{agent} {kind} n={n} {'deterministic' if deterministic else 'training'}"
    rows, _ = check_collect_rows(eng, env, ord0, res, n_ep, kind, rm.ENV_SEED, what,
                                 lambda rows, e, ordinal, t, key: replay_action_check(eng, agent, deterministic, what, rows, e, ordinal, t, key))
    env.close(); eng.close()


def replay_action_check(eng, agent, deterministic, what, rows, e, ordinal, t, key):
    """the stored action against the agent's formula over (m, sigma) of the row's observation (Engine.sac_actor_forward) and the
    model's draw of (env, ordinal, t, dim)"""
    mu, sigma = eng.sac_actor_forward(rows["obs"])
    eps64, eps32, nscale = action_draws(rows, e, ordinal, t, key, eng.cfg.act_dim)
    dist = check_action(agent, rows["act"], mu, sigma, eps64, eps32, deterministic, nscale, what + " act")
    if agent == "sacl":
        assert np.abs(rows["act"]).max() <= 1.0 and 0.05 < np.mean(np.abs(rows["act"]) < 0.99)      # squashed, and not all saturated
    if not deterministic:
        assert np.abs(rows["act"].astype(F64) - rm.action(agent, mu, sigma, 0 * eps64, True, F64)).max() > 1e-3      # the noise is in
    return dist


# ------------------------------------------------------------------------------------------------ 2. the store is as pushes would leave it
def test_store_bookkeeping_and_the_next_update_are_what_pushes_leave():
    n, n_eps = 5, (12, 4)
    # A: the row stream, from a store that never wraps
    eng_a, env_a = make("sacl", "pc", n, rows_per_env=400)
    env_a.reset()
    for n_ep in n_eps:
        eng_a.collect_device(env_a._h, n_ep, deterministic=False, bound_method=1)
    idx_a, rows_a = store_rows(eng_a)
    sub_a, _ = eng_a.store_geometry()
    # B: the same collects into 9-row sub-buffers; C: A's rows pushed one vector step at a time into the same geometry
    eng_b, env_b = make("sacl", "pc", n, rows_per_env=9)
    env_b.reset()
    res_b = [eng_b.collect_device(env_b._h, n_ep, deterministic=False, bound_method=1) for n_ep in n_eps]
    eng_c, env_c = make("sacl", "pc", n, rows_per_env=9)
    queues = {e: list(np.flatnonzero(idx_a // sub_a == e)) for e in range(n)}
    pushed = push_collects(eng_c, rows_a, queues, n, n_eps)
    assert all(len(q) == 0 for q in queues.values())           # the model loop consumed exactly the rows the device stored
    for r, (gr, gl) in zip(res_b, pushed):
        assert r["ep_rews"].tolist() == gr and r["ep_lens"].tolist() == gl            # in the order the loop met them
    (ib, rb), (ic, rc) = store_rows(eng_b), store_rows(eng_c)
    assert np.array_equal(ib, ic) and same_rows(rb, rc) and eng_b.store_sizes().max() == 9        # a sub-buffer wrapped
    assert np.array_equal(eng_b.store_sizes(), eng_c.store_sizes()) and len(eng_b) == len(eng_c)
    # the next update: the library's sampler over the books both ways of storing left, and everything a push invalidates
    st_b, st_c = eng_b.sac_update(16, LAG, RESC), eng_c.sac_update(16, LAG, RESC)
    assert np.isfinite(st_b).all() and np.array_equal(st_b, st_c)
    assert np.array_equal(eng_b.sac_last_sample(16)[0], eng_c.sac_last_sample(16)[0])
    pb, pc = eng_b.sac_get_params(0)[0], eng_c.sac_get_params(0)[0]
    assert np.array_equal(pb, pc) and not np.array_equal(pb, eng_a.sac_get_params(0)[0])
    # the bookkeeping behind it: one more push reports the same slot and running episode on both
    one = (np.array([1]), np.zeros((1, 6), F32), np.zeros((1, 2), F32), np.array([0.25]), np.array([1.0]), np.array([False]), np.array([False]),
           np.ones((1, 6), F32))
    assert all(np.array_equal(x, y) for x, y in zip(eng_b.push(*one), eng_c.push(*one)))
    for x in (env_a, env_b, env_c, eng_a, eng_b, eng_c):
        x.close()


# ------------------------------------------------------------------------------------------------ 3. prioritised replay
@pytest.mark.parametrize("rows_per_env", [60, 9], ids=["fits", "wraps"])
def test_prioritised_leaves_are_what_pushes_leave(rows_per_env):
    """D collects on the device; C gets the same rows by pushes.  The rows come from A, a recorder whose store never wraps and whose
    actor follows D's through the updates, so that its collects are D's."""
    n, n_eps = 5, (8, 6)
    eng_a, env_a = make("sacl", "pc", n, rows_per_env=400)
    eng_d, env_d = make("sacl", "pc", n, rows_per_env=rows_per_env, per=(0.6, 0.4))
    eng_c, env_c = make("sacl", "pc", n, rows_per_env=rows_per_env, per=(0.6, 0.4))
    env_a.reset(); env_d.reset()
    sub_a, _ = eng_a.store_geometry()
    sub, num = eng_d.store_geometry()
    taken, seen = 0, {e: 0 for e in range(n)}

    def stage(n_ep):
        nonlocal taken
        eng_a.collect_device(env_a._h, n_ep, deterministic=False, bound_method=1)
        res = eng_d.collect_device(env_d._h, n_ep, deterministic=False, bound_method=1)
        idx_a, rows_a = store_rows(eng_a)
        new = {e: list(np.flatnonzero(idx_a // sub_a == e))[seen[e]:] for e in range(n)}      # the rows of env e this collect added
        for e in range(n):
            seen[e] += len(new[e])
        n_new = sum(len(q) for q in new.values())
        taken += n_new
        pushed = push_collects(eng_c, rows_a, new, n, (n_ep, ))
        assert all(len(q) == 0 for q in new.values()) and res["steps"] == n_new
        assert (res["ep_rews"].tolist(), res["ep_lens"].tolist()) == pushed[0]
        compare()

    def compare():
        (idd, rd), (ic, rc) = store_rows(eng_d), store_rows(eng_c)
        assert np.array_equal(idd, ic) and same_rows(rd, rc)
        (ld, mxd, mnd, totd), (lc, mxc, mnc, totc) = eng_d.per_state(), eng_c.per_state()
        assert np.array_equal(ld, lc) and (mxd, mnd, totd) == (mxc, mnc, totc)
        sizes = eng_d.store_sizes()
        written = np.concatenate([e * sub + np.arange(sizes[e]) for e in range(num)])
        assert np.all(ld[written] > 0) and np.count_nonzero(ld) == len(written)
        return ld, mxd, mnd

    stage(n_eps[0])
    for _ in range(3):
        sd, sc = eng_d.sac_update(16, LAG, RESC), eng_c.sac_update(16, LAG, RESC)
        assert np.array_equal(sd, sc)
    leaves, mx, mn = compare()
    assert mx != 1.0 or mn != 1.0                               # the updates moved the priorities: the next rows take the new max_prio
    eng_a.sac_put_params(0, eng_d.sac_get_params(0)[0])          # the recorder's actor follows
    stage(n_eps[1])
    leaves2, mx2, mn2 = compare()
    assert (mx2, mn2) == (mx, mn) and np.isclose(leaves2.max(), mx ** 0.6, rtol=1e-12)
    if rows_per_env == 9:
        assert eng_d.store_sizes().max() == 9 and taken > len(eng_d)          # rows were overwritten
    for x in (env_a, env_d, env_c, eng_a, eng_d, eng_c):
        x.close()


# ------------------------------------------------------------------------------------------------ 4. launch cuts
def test_launch_cuts_change_nothing_at_256_wide():
    out = []
    for cut in (3, 0):
        eng, env = make("sacl", "lin8", 17, H=256, rows_per_env=12)
        env.reset()
        res = [eng.collect_device(env._h, n_ep, deterministic=False, bound_method=1, max_steps_per_launch=cut) for n_ep in (20, 5)]
        out.append((res, store_rows(eng), eng.store_sizes().copy(), env.get_state()))
        env.close(); eng.close()
    (ra, (ia, rows_a), sza, sta), (rb, (ib, rows_b), szb, stb) = out
    assert ra[0]["launches"] > 1 and rb[0]["launches"] == 1
    for x, y in zip(ra, rb):
        assert all(np.array_equal(x[k], y[k]) for k in x if k != "launches")
    assert np.array_equal(ia, ib) and same_rows(rows_a, rows_b) and np.array_equal(sza, szb)
    assert all(np.array_equal(x, y) for x, y in zip(sta, stb))


# ------------------------------------------------------------------------------------------------ 5. seeds
@pytest.mark.parametrize("agent", ["sacl", "ddpgl"])
def test_seeds_decide_the_rows(agent):
    def run(seed):
        eng, env = make(agent, "pc", 5, seed=seed)
        env.reset()
        eng.collect_device(env._h, 8, deterministic=False, bound_method=1)
        rows = store_rows(eng)[1]
        env.close(); eng.close()
        return rows
    a, b, c = run(3), run(3), run(4)
    assert same_rows(a, b)
    assert not np.array_equal(a["obs"][:5], c["obs"][:5]) and not np.array_equal(a["act"][:5], c["act"][:5])


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_name_their_reason_and_change_nothing():
    from fsrl_amd.engine import EngineSacGroup, TrajArchive

    def refused(eng, env, match, **kw):
        before, n_before = env.get_state(), len(eng)
        with pytest.raises(AssertionError, match=match):
            eng.collect_device(env._h, 3, **kw)
        assert all(np.array_equal(x, y) for x, y in zip(before, env.get_state())) and len(eng) == n_before

    # a layered replay context
    eng, env = make("sacl", "lin8", 4, hidden_sizes=(32, 32, 32))
    env.reset()
    refused(eng, env, "layered")
    env.close(); eng.close()
    # a member of a replay group
    eng, env = make("sacl", "lin8", 4)
    other, env_o = make("sacl", "lin8", 4)
    env.reset()
    group = EngineSacGroup([eng, other])
    refused(eng, env, "grouped")
    group.close()
    # a trajectory tap
    arch = TrajArchive(eng, 1000, 100, 50)
    arch.attach(eng)
    refused(eng, env, "trajectory tap")
    arch.detach(eng); arch.close()
    # more envs than the store has sub-buffers
    eng.store_configure(3 * 50, 3)
    refused(eng, env, "sub-buffers")
    for x in (env, env_o, eng, other):
        x.close()
    # a replay context nothing was initialised on
    eng, env = make("sacl", "lin8", 4, init=False)
    env.reset()
    refused(eng, env, "replay contexts")
    env.close(); eng.close()


# ------------------------------------------------------------------------------------------------ 7. facade
@pytest.mark.parametrize("algo,per", [("sacl", None), ("ddpgl", None), ("cvpo", None), ("sacl", dict(alpha=0.6, beta=0.4))])
def test_agents_learn_and_evaluate_over_device_envs(algo, per, tmp_path):
    from fsrl_amd.agent import CVPOAgent, DDPGLagAgent, SACLagAgent
    from fsrl_amd.data import DeviceCollector, FastCollector
    from fsrl_amd.env import DevicePointCircle, PointCircleEnv
    from fsrl_amd.utils import BaseLogger
    Agent = {"sacl": SACLagAgent, "ddpgl": DDPGLagAgent, "cvpo": CVPOAgent}[algo]
    agent = Agent(PointCircleEnv(), BaseLogger(str(tmp_path), name="d"), cost_limit=10, device="cuda:0", seed=3, hidden_sizes=(64, 64),
                  training_num=4)
    train = DevicePointCircle(agent.policy, 4, max_episode_steps=20, seed=1)
    test = DevicePointCircle(agent.policy, 2, max_episode_steps=20, seed=2)
    seen, fast = [], []
    orig, orig_fast = DeviceCollector.collect, FastCollector.collect

    def spy(self, *a, **k):
        seen.append(self)
        return orig(self, *a, **k)

    def spy_fast(self, *a, **k):
        fast.append(self)
        return orig_fast(self, *a, **k)
    DeviceCollector.collect, FastCollector.collect = spy, spy_fast
    try:
        theta0 = agent.policy.engine.sac_get_params(0)[0]
        ep, stat, info = agent.learn(train, test, epoch=1, episode_per_collect=4, step_per_epoch=160, update_per_step=0.1, batch_size=32,
                                     testing_num=2, verbose=False, save_ckpt=False, **({} if per is None else {"prioritized_replay": per}))
    finally:
        DeviceCollector.collect, FastCollector.collect = orig, orig_fast
    assert ep == 1 and len(seen) >= 2 and all(isinstance(c, DeviceCollector) and c.env is train for c in seen)
    assert all(c.env is test for c in fast)                     # every training collect went through DeviceCollector; tests did not
    assert np.isfinite(list(stat.values())).all() and "train/reward" in stat and "test/cost" in stat
    assert np.abs(agent.policy.engine.sac_get_params(0)[0] - theta0).max() > 1e-6
    if per is not None:
        leaves, mx, mn, total = agent.policy.engine.per_state()
        assert np.count_nonzero(leaves) == len(agent.policy.engine) and total > 0
    rew, length, cost = agent.evaluate(test, eval_episodes=2)          # FastCollector over DeviceVectorEnv.step
    assert 1 <= length <= 20 and np.isfinite(rew) and cost >= 0
    train.close(); test.close()
