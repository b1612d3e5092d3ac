"""Device environments and whole collects on the GPU (fsrl_devenv_*, fsrl_collect_device) against the host model of
tests/devenv_model.py and against the existing collectors.  Smallest shapes that reach every branch: hidden (64, 64) (one test at
(256, 256)), point-circle and the linear env at obs 8 / act 2 and obs 33 / act 8, env_num 1 / 5 / 16 / 17 / 64 (the tile boundaries),
episodes cut at 7 steps, radius / x_lim / cost_threshold chosen so that terminations and costs both occur, stores small enough that
sub-buffers wrap inside one collect.

The bars.  Continuous outputs are held to the float64-yardstick rule of DESIGN.md 6: with distances taken as the largest
|x - float64| / scale over the rows, the device may sit at most 3 x as far from the float64 model as the float32 restatement does, and
is never held tighter than one float32 ulp at the value's scale (scale: the sum of the magnitudes of the terms of the value, at least
1; for a normal its Box-Muller radius).  Discontinuous outputs (cost, terminated) must match except where the decision variable lies
within 1e-5 x scale of its threshold, on at most 2 % of the rows (for the injected inputs that share is asserted on the CPU, in
tests/test_devenv_model.py; for rows a collect produced it is asserted here, from the float32 restatement alone)."""
import ctypes as C

import numpy as np
import pytest

import devenv_model as dm
import devenv_replay_model as rm
from devcollect_rows import action_draws, check_action, check_collect_rows, check_continuous, check_discontinuous

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
EPS = float(np.finfo(F32).eps)
PC = dict(radius=0.12, x_lim=0.3, dt=0.1)          # resets land in [-0.5, 0.5)^2: r > 0.48 and |x| > 0.3 both happen, neither always


class Pol:
    """what the collectors read off a policy"""
    traj_buffer = None

    def __init__(self, eng, bound="clip", low_high=None, training=False):
        from fsrl_amd.env import Box
        self.engine, self.training, self._deterministic_eval = eng, training, True
        self.action_bound_method = bound
        self.action_scaling = low_high is not None
        self.action_space = Box(-1.0, 1.0, (eng.cfg.act_dim, ))
        if low_high is not None:
            self.action_space.low[:], self.action_space.high[:] = low_high


def make(kind, n, H=64, rows_per_env=200, seed=3, algo=None, sub_buffers=None, oracle_params=False, **cfg):
    """-> (engine with fixed random parameters, device env of `kind`: 'pc' or a linear shape of devenv_replay_model.SHAPES).
    oracle_params: set the fixed parameters on a context made with hidden_sizes too (two unrelated widths that the device pads),
    through the oracle's layout, which is what set_params takes"""
    from fsrl_amd.engine import Engine, EngineConfig
    from fsrl_amd.env import DeviceLinear, DevicePointCircle, SyntheticSafetyVectorEnv
    from fsrl_amd.env.synthetic import stable_coupling
    Do, Da = rm.SHAPES[kind]
    kw = dict(obs_dim=Do, act_dim=Da, hidden=H, env_num=sub_buffers or n, buffer_size=(sub_buffers or n) * rows_per_env)
    if algo is not None:
        kw["algo"] = algo
    kw.update(cfg)
    eng = Engine(EngineConfig(**kw), device=0)
    if algo is None and ("hidden_sizes" not in cfg or oracle_params):
        eng.set_params(rm.onpolicy_params(eng.n_params))
    if kind == "pc":
        env = DevicePointCircle(eng, n, max_episode_steps=7, seed=seed, **PC)
    else:
        host = SyntheticSafetyVectorEnv(env_num=n, obs_dim=Do, act_dim=Da, episode_len=7, coupling=stable_coupling(Do), cost_threshold=0.7)
        env = DeviceLinear(eng, like=host, seed=seed)
    return eng, env


def store_rows(eng):
    """(indices, rows) of the whole store in sample(0) order: env-major, chronological"""
    idx = eng.sample0()
    return idx, eng.store_read(idx)


def same_rows(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("obs", "act", "rew", "cost", "terminated", "truncated", "obs_next"))


def same_state(ea, eb):
    return all(np.array_equal(x, y) for x, y in zip(ea.get_state(), eb.get_state()))


# ------------------------------------------------------------------------------------------------ 1. the env alone
@pytest.mark.parametrize("name", ["point_circle", "linear_8_2", "linear_33_8"])
def test_env_alone_one_step_from_injected_states(name):
    """Measured on an MI355X, distance from the float64 model in units of the value's scale, device | float32 restatement:
    point-circle obs_next 9.6e-8 | 9.6e-8, rew 3.2e-8 | 3.2e-8; linear 8 / 2 obs_next 1.5e-7 | 1.5e-7, rew 1.0e-7 | 1.0e-7; linear
    33 / 8 obs_next 3.2e-7 | 3.2e-7, rew 1.5e-7 | 1.5e-7 -- the same number twice because the device computes the restatement's bits
    wherever no transcendental enters; reset normals 1.5e-7 | 4.0e-7 (the device's sincospi takes 2 u exactly, the restatement rounds
    2 pi u); rows within the discontinuity band: none.  The test prints the figures."""
    case = dm.env_alone_cases()[name]
    kind = {"point_circle": "pc", "linear_8_2": "lin8", "linear_33_8": "lin33"}[name]
    eng, env = make(kind, case["env_num"], seed=case["seed"])
    if case["kind"] == dm.POINT_CIRCLE:
        env.close()
        from fsrl_amd.env import DevicePointCircle
        env = DevicePointCircle(eng, case["env_num"], max_episode_steps=7, seed=case["seed"], radius=case["params"][0],
                                x_lim=case["params"][1], dt=case["params"][2])
    else:
        assert np.array_equal(env.A, case["A"]) and np.array_equal(env.B, case["B"]) and env.cost_threshold == case["params"][0]
    env.set_state(case["state"], case["t"], case["ordinal"])
    st, t, od = env.get_state()
    assert np.array_equal(st, case["state"]) and np.array_equal(t, case["t"]) and np.array_equal(od, case["ordinal"])
    obs, rew, term, trunc, info = env.step(case["act"])
    r64, r32 = dm.env_alone_expected(case, F64), dm.env_alone_expected(case, F32)
    check_continuous(obs, r64["obs_next"], r32["obs_next"], r32["obs_scale"], name + " obs_next")
    check_continuous(rew, r64["rew"], r32["rew"], r32["rew_scale"], name + " rew")
    check_discontinuous(info["cost"], term, r32, name)
    assert np.array_equal(trunc, r32["truncated"])
    if case["kind"] == dm.POINT_CIRCLE:               # no transcendental: the restatement's bits
        assert np.array_equal(obs, r32["obs_next"]) and np.array_equal(rew, r32["rew"])
    st2, t2, od2 = env.get_state()
    assert np.array_equal(t2, case["t"] + 1) and np.array_equal(od2, case["ordinal"])
    assert np.array_equal(st2, obs[:, :4] if case["kind"] == dm.POINT_CIRCLE else obs)
    # ---- reset draws at the injected ordinals
    obs0, _ = env.reset()
    key = dm.key_of(case["seed"])
    ids = np.arange(case["env_num"])
    if case["kind"] == dm.POINT_CIRCLE:
        want, _ = dm.point_reset(key, ids, case["ordinal"], *case["params"][:2], dtype=F64)
        assert np.all(np.abs(obs0[:, :2].astype(F64) - want[:, :2]) <= np.spacing(np.abs(want[:, :2]).astype(F32))), "uniforms: one ulp"
        assert np.all(obs0[:, 2:4] == 0)
    else:
        d = np.arange(case["obs_dim"])[None, :]
        n64 = dm.normal(key, ids[:, None], case["ordinal"][:, None], 0, dm.STREAM_RESET, d, F64)
        n32 = dm.normal(key, ids[:, None], case["ordinal"][:, None], 0, dm.STREAM_RESET, d, F32)
        check_continuous(obs0, n64, n32, dm.normal_scale(key, ids[:, None], case["ordinal"][:, None], 0, dm.STREAM_RESET, d), name + " reset normals")
    st3, t3, od3 = env.get_state()
    assert np.all(t3 == 0) and np.array_equal(od3, case["ordinal"] + 1)
    env.close(); eng.close()


# ------------------------------------------------------------------------------------------------ 2. deterministic collects
@pytest.mark.parametrize("kind,n,episodes,bound,low_high", [
    ("pc", 5, (3, 12), "clip", None),                  # below env_num, then above it: the surplus rule both ways
    ("pc", 5, (5, 5), "", (-0.5, 1.5)),                # equal to env_num; no bound method, with bounds
    ("lin8", 17, (20, 9), "clip", (-2.0, 0.5)),        # two tiles, the second with one row
    ("lin33", 16, (16, 30), "", None),                 # one full tile, wide observations (the MFMA layer 1)
    ("pc", 64, (70, 64), "clip", None),                # four full tiles
    ("lin8", 1, (2, 1), "clip", None),
])
def test_deterministic_collect_is_the_existing_path_bit_for_bit(kind, n, episodes, bound, low_high):
    deterministic_collect_twins(kind, n, episodes, bound, low_high)


def deterministic_collect_twins(kind, n, episodes, bound, low_high, **make_kw):
    """twin contexts, twin envs: FastCollector(device_actor=True) over DeviceVectorEnv.step (_collect_fused) against DeviceCollector"""
    from fsrl_amd.data import DeviceCollector, FastCollector, HipVectorReplayBuffer
    out = []
    for device in (False, True):
        eng, env = make(kind, n, rows_per_env=6, **make_kw)    # 6-row sub-buffers: a full episode (7 steps) wraps its sub-buffer
        pol = Pol(eng, bound, low_high)
        buf = HipVectorReplayBuffer(eng, n * 6, n)
        col = DeviceCollector(pol, env, buf) if device else FastCollector(pol, env, buf, device_actor=True)
        snaps = []
        for n_ep in episodes:
            stat = col.collect(n_episode=n_ep)
            idx, rows = store_rows(eng)
            snaps.append((stat, idx, rows, eng.store_sizes().copy(), len(eng), env.get_state(), buf._sizes.copy()))
        upd, _ = eng.ppo_update([0.3], 1 / 1.3, 32, 2, seed=5)
        out.append((snaps, np.asarray(upd), eng.get_params(), col.collect_step, col.collect_episode))
        env.close(); eng.close()
    (sa, ua, pa, cs_a, ce_a), (sb, ub, pb, cs_b, ce_b) = out
    for (st_a, idx_a, rows_a, sz_a, len_a, state_a, bs_a), (st_b, idx_b, rows_b, sz_b, len_b, state_b, bs_b) in zip(sa, sb):
        assert st_a == st_b, (st_a, st_b)
        assert np.array_equal(idx_a, idx_b) and same_rows(rows_a, rows_b)
        assert np.array_equal(sz_a, sz_b) and len_a == len_b and np.array_equal(bs_a, bs_b)
        assert all(np.array_equal(x, y) for x, y in zip(state_a, state_b))
    assert [s[0]["n/ep"] for s in sa] == list(episodes)
    assert (cs_a, ce_a) == (cs_b, ce_b)
    assert np.array_equal(ua, ub) and np.array_equal(pa, pb)
    assert sa[-1][3].max() == 6 and sum(s[0]["n/st"] for s in sa) > sa[-1][4]      # a sub-buffer is full and rows were overwritten


def test_deterministic_collect_under_tanh_is_the_existing_path_to_tolerance():
    """the host's tanh and the device's differ in the last bits, so this bound method is held to tolerance: linear env (no
    termination to flip), one collect of one episode per env"""
    from fsrl_amd.data import DeviceCollector, FastCollector, HipVectorReplayBuffer
    out = []
    for device in (False, True):
        eng, env = make("lin8", 5)
        pol = Pol(eng, "tanh", (-1.5, 1.0))
        buf = HipVectorReplayBuffer(eng, 5 * 200, 5)
        col = DeviceCollector(pol, env, buf) if device else FastCollector(pol, env, buf, device_actor=True)
        stat = col.collect(n_episode=5)
        out.append((stat, store_rows(eng)[1]))
        env.close(); eng.close()
    (st_a, ra), (st_b, rb) = out
    assert st_a["n/st"] == st_b["n/st"] == 35 and st_a["n/ep"] == st_b["n/ep"] == 5
    for k in ("obs", "act", "obs_next", "rew"):
        np.testing.assert_allclose(ra[k], rb[k], rtol=0, atol=2e-5)
    assert np.array_equal(ra["truncated"], rb["truncated"]) and np.mean(ra["cost"] != rb["cost"]) <= 0.03
    assert abs(st_a["rew"] - st_b["rew"]) < 1e-4


# ------------------------------------------------------------------------------------------------ 3. stochastic collects, row by row
@pytest.mark.parametrize("kind,n,n_ep", [("pc", 17, 25), ("lin33", 5, 12), ("lin8", 64, 70), ("lin8", 1, 3)])
def test_stochastic_collect_row_by_row_against_the_model(kind, n, n_ep):
    eng, env = make(kind, n, seed=11)
    env.reset()
    _, t0, ord0 = env.get_state()
    assert np.all(t0 == 0) and np.all(ord0 == 1)
    res = eng.collect_device(env._h, n_ep, deterministic=False, bound_method=1)

    def action(rows, e, ordinal, t, key):
        # the action noise: (act - mu) / sigma is the model's normal of (env, ordinal, t, dim)
        mu, sigma = eng.actor_forward(rows["obs"])
        eps64, eps32, nscale = action_draws(rows, e, ordinal, t, key, eng.cfg.act_dim)
        return check_action("onpolicy", rows["act"], mu, sigma, eps64, eps32, False, nscale, f"{kind} action noise")
    check_collect_rows(eng, env, ord0, res, n_ep, kind, 11, kind, action)
    env.close(); eng.close()


# ------------------------------------------------------------------------------------------------ 4. launch cuts
def test_launch_cuts_change_nothing_at_256_wide():
    out = []
    for cut in (3, 0):
        eng, env = make("lin8", 17, H=256, rows_per_env=12)
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
def test_seeds_decide_the_rows():
    def run(seed, reseed=None):
        eng, env = make("pc", 5, seed=seed)
        if reseed is not None:
            env.seed(reseed)
        env.reset()
        eng.collect_device(env._h, 8, deterministic=False, bound_method=1)
        rows = store_rows(eng)[1]
        env.close(); eng.close()
        return rows
    a, b, c, d, e = run(3), run(3), run(4), run(3, reseed=4), run(3, reseed=9)
    assert same_rows(a, b)
    assert not np.array_equal(a["obs"][:5], c["obs"][:5]) and not np.array_equal(a["act"][:5], c["act"][:5])
    assert same_rows(c, d)                               # fsrl_devenv_seed(s) on a fresh env is creation with seed s
    assert not np.array_equal(a["obs"][:5], e["obs"][:5])


# ------------------------------------------------------------------------------------------------ 6. the store is as pushes would leave it
def test_store_and_bookkeeping_are_what_pushes_leave():
    n, n_eps = 5, (12, 4)
    # A: the row stream, from a store that never wraps
    eng_a, env_a = make("pc", n, rows_per_env=400)
    env_a.reset()
    for n_ep in n_eps:
        eng_a.collect_device(env_a._h, n_ep, deterministic=False, bound_method=1)
    idx_a, rows_a = store_rows(eng_a)
    sub_a, _ = eng_a.store_geometry()
    # B: the same collects into 9-row sub-buffers; C: A's rows pushed one vector step at a time into the same geometry
    eng_b, env_b = make("pc", n, rows_per_env=9)
    env_b.reset()
    res_b = [eng_b.collect_device(env_b._h, n_ep, deterministic=False, bound_method=1) for n_ep in n_eps]
    eng_c, env_c = make("pc", n, rows_per_env=9)
    queues = {e: list(np.flatnonzero(idx_a // sub_a == e)) for e in range(n)}
    ep_rews, ep_lens = [], []
    for n_ep in n_eps:                                          # the collect loop, fed from the per-env row queues
        ready, episodes, got_r, got_l = list(range(min(n, n_ep))), 0, [], []
        while episodes < n_ep:
            take = [queues[e].pop(0) for e in ready]
            ptr, er, el, ei = eng_c.push(np.array(ready), *(rows_a[k][take] for k in ("obs", "act", "rew", "cost", "terminated", "truncated", "obs_next")))
            done = rows_a["terminated"][take] | rows_a["truncated"][take]
            local = list(np.flatnonzero(done))
            if local:
                episodes += len(local)
                got_r += list(er[local]); got_l += list(el[local])
                surplus = len(ready) - (n_ep - episodes)
                if surplus > 0:
                    ready = [e for p, e in enumerate(ready) if p not in local[:surplus]]
        ep_rews.append(got_r); ep_lens.append(got_l)
    assert all(len(q) == 0 for q in queues.values())           # the model loop consumed exactly the rows the device stored
    for r, gr, gl in zip(res_b, ep_rews, ep_lens):
        assert r["ep_rews"].tolist() == gr and r["ep_lens"].tolist() == gl            # in the order the loop met them
    (ib, rb), (ic, rc) = store_rows(eng_b), store_rows(eng_c)
    assert np.array_equal(ib, ic) and same_rows(rb, rc) and eng_b.store_sizes().max() == 9        # a sub-buffer wrapped
    assert np.array_equal(eng_b.store_sizes(), eng_c.store_sizes()) and len(eng_b) == len(eng_c)
    # the bookkeeping behind it: one more push reports the same slot and running episode on both, also across a reset that keeps statistics
    one = (np.array([1]), np.zeros((1, 6), F32), np.zeros((1, 2), F32), np.array([0.25]), np.array([1.0]), np.array([False]), np.array([False]),
           np.ones((1, 6), F32))
    assert all(np.array_equal(x, y) for x, y in zip(eng_b.push(*one), eng_c.push(*one)))
    eng_b.reset_store(keep_statistics=True); eng_c.reset_store(keep_statistics=True)
    assert len(eng_b) == len(eng_c) == 0
    fin = one[:5] + (np.array([True]), ) + one[6:]
    pb, pc = eng_b.push(*fin), eng_c.push(*fin)
    assert all(np.array_equal(x, y) for x, y in zip(pb, pc)) and pb[2][0] >= 2 and pb[0][0] == 9
    for x in (env_a, env_b, env_c, eng_a, eng_b, eng_c):
        x.close()


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_name_their_reason_and_change_nothing():
    from fsrl_amd import _lib
    from fsrl_amd._lib import FsrlHipError
    from fsrl_amd.engine import TrajArchive

    def refused(eng, env, match, exc=AssertionError, **kw):
        before, n_before = env.get_state(), len(eng)
        with pytest.raises(exc, match=match):
            eng.collect_device(env._h, 3, **kw)
        assert all(np.array_equal(x, y) for x, y in zip(before, env.get_state())) and len(eng) == n_before

    eng, env = make("pc", 5)
    env.reset()
    other, env_o = make("pc", 5)
    refused(other, env, "another context")
    refused(eng, env, "bound_method", bound_method=7)
    refused(eng, env, "max_steps_per_launch", max_steps_per_launch=5000)
    # a trajectory tap
    arch = TrajArchive(eng, 1000, 100, 50)
    arch.attach(eng)
    refused(eng, env, "trajectory tap")
    arch.detach(eng); arch.close()
    # inside an update
    eng.collect_device(env._h, 5, bound_method=1)
    eng.ppo_begin([0.3], 1 / 1.3, 16)
    refused(eng, env, "inside an update", exc=FsrlHipError)
    eng.ppo_abort()
    # more envs than the store has sub-buffers
    eng.store_configure(3 * 50, 3)
    refused(eng, env, "sub-buffers")
    # shapes and sizes at creation
    for bad, match in ((dict(env_num=65), "env_num"), (dict(obs_dim=7), "obs_dim"), (dict(act_dim=3), "act_dim"), (dict(kind=9), "kind")):
        cfg = _lib.DevEnvConfig()
        cfg.kind, cfg.env_num, cfg.obs_dim, cfg.act_dim, cfg.max_episode_steps = 0, 5, 6, 2, 7
        for k, v in bad.items():
            setattr(cfg, k, v)
        h = C.c_void_p()
        with pytest.raises(AssertionError, match=match):
            _lib.check(eng.lib.fsrl_devenv_create(eng._ctx, C.byref(cfg), C.byref(h)))
    for x in (env, env_o, eng, other):
        x.close()
    # replay and layered contexts
    eng, env = make("lin8", 4, algo=_lib.ALGO_SAC_LAG)
    refused(eng, env, "replay contexts")
    env.close(); eng.close()
    eng, env = make("lin8", 4, hidden_sizes=(32, 32, 32))
    refused(eng, env, "layered")
    env.close(); eng.close()


# ------------------------------------------------------------------------------------------------ 8. facade
@pytest.mark.parametrize("algo", ["ppol", "focops"])
def test_agents_learn_and_evaluate_over_device_envs(algo, tmp_path):
    from fsrl_amd.agent import FOCOPSAgent, PPOLagAgent
    from fsrl_amd.data import DeviceCollector
    from fsrl_amd.env import DevicePointCircle, PointCircleEnv
    from fsrl_amd.utils import BaseLogger
    Agent = PPOLagAgent if algo == "ppol" else FOCOPSAgent
    agent = Agent(PointCircleEnv(), BaseLogger(str(tmp_path), name="d"), cost_limit=10, device="cuda:0", seed=3, hidden_sizes=(64, 64),
                  training_num=4)
    train = DevicePointCircle(agent.policy, 4, max_episode_steps=20, seed=1)
    test = DevicePointCircle(agent.policy, 2, max_episode_steps=20, seed=2)
    seen = []
    orig = DeviceCollector.collect

    def spy(self, *a, **k):
        seen.append(self)
        return orig(self, *a, **k)
    DeviceCollector.collect = spy
    try:
        theta0 = agent.policy.engine.get_params()
        ep, stat, info = agent.learn(train, test, epoch=1, episode_per_collect=4, step_per_epoch=160, repeat_per_collect=2, batch_size=32,
                                     testing_num=2, verbose=False, save_ckpt=False)
    finally:
        DeviceCollector.collect = orig
    assert ep == 1 and len(seen) >= 2 and all(isinstance(c, DeviceCollector) for c in seen)
    assert np.isfinite(list(stat.values())).all() and "train/reward" in stat and "test/cost" in stat
    assert np.abs(agent.policy.engine.get_params() - theta0).max() > 1e-5
    rew, length, cost = agent.evaluate(test, eval_episodes=2)          # FastCollector over DeviceVectorEnv.step
    assert 1 <= length <= 20 and np.isfinite(rew) and cost >= 0
    train.close(); test.close()


def test_cpo_learns_from_a_device_collect():
    from fsrl_amd import _lib
    eng, env = make("lin8", 4, algo=_lib.ALGO_CPO)
    eng.set_params((0.3 * np.random.default_rng(7).standard_normal(eng.n_params)).astype(F32))
    env.reset()
    res = eng.collect_device(env._h, 8, deterministic=False, bound_method=1)
    assert res["steps"] == 56
    theta0 = eng.get_params()
    n = eng.tr_begin(optim_critic_iters=2, cost_limit=5.0)
    assert n == 56
    stats = eng.cpo_learn(res["total_cost"] / 8, 1)
    assert np.isfinite(stats).all() and np.abs(eng.get_params() - theta0).max() > 0
    env.close(); eng.close()
