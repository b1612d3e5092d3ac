"""The CPU preconditions of tests/test_gpu_devcollect_shapes.py and of the differing members of tests/test_gpu_devcollect_group.py,
for every case of devenv_replay_model.ALL_CASES, in training and deterministic mode.  No GPU.

Each case runs here as a closed loop of the float32 model with the oracles' CPU actors (devenv_replay_model.cpu_actor for the replay
agents, oracle/ppo_lag.py's actor over the same flat parameters for the on-policy head):
  * the share of rows whose cost / terminated decision lies inside the discontinuity band is at most dm.BAND_CAP -- the condition
    under which the GPU test may compare discontinuous outputs at all; it is a condition on the case (its seed, its env_num), not a
    measurement;
  * the inputs tell the head options apart: the action a WRONG formula would store -- the other `unbounded` mode, max_action taken
    as 1, the squash dropped or added, a neighbouring group member's max_action or exploration_sigma -- misses the yardstick bound of
    the true action by a factor of at least 100 on some row.  So a device collect that dropped or mis-sourced one of these factors
    cannot pass the row-by-row test, and a group member that read a neighbour's row of the member table cannot equal its twin;
  * with max_action above 1 some stored actions lie beyond +-1: the clip branch of map_action runs on collect-produced rows."""
import functools

import numpy as np
import pytest

import devenv_model as dm
import devenv_replay_model as rm
from devcollect_rows import action_terms

F32, F64 = np.float32, np.float64
EPS = float(np.finfo(F32).eps)
IDS = [rm.case_id(c) for c in rm.ALL_CASES]


@functools.lru_cache(maxsize=None)
def closed_loop(i, deterministic):
    """case i as a closed loop of the float32 model -> dict(n_rows, near, cost, terminated and, per row, obs / ids-derived draws)"""
    case = rm.ALL_CASES[i]
    agent, kind, n, n_ep, H, opts = case
    Do, Da = rm.SHAPES[kind]
    if kind == "pc":
        env = dm.ModelEnv(dm.POINT_CIRCLE, n, 7, rm.ENV_SEED, (rm.PC["radius"], rm.PC["x_lim"], rm.PC["dt"]), Do, Da, dtype=F32)
    else:
        host = rm.linear_host(kind, n)
        env = dm.ModelEnv(dm.LINEAR, n, 7, rm.ENV_SEED, (0.7, ), Do, Da, host.A, host.B, dtype=F32)
    actor = rm.case_actor(case)
    steps, rec = [], []
    step = env.step
    env.step = lambda act, ids=None: steps.append(step(act, ids)) or steps[-1]

    def policy(obs, ids):
        m, sigma = actor(obs)
        eps32 = env.action_noise(ids, F32)
        cnt = (ids[:, None], (env.ordinal[ids] - 1)[:, None], env.t[ids][:, None], dm.STREAM_ACT, np.arange(Da)[None, :])
        rec.append((obs.copy(), m, sigma, env.action_noise(ids, F64), eps32, dm.normal_scale(env.key, *cnt)))
        if agent == "onpolicy" and not deterministic:       # the device's arithmetic: mu + sigma * eps, each operation rounded
            act = (m + sigma * eps32).astype(F32)
        else:
            act = rm.action(rm.formula(agent), m, sigma, eps32, deterministic, F32)
        rec[-1] += (act, )
        return dm.map_action(act, 1)
    env.reset()
    rows, episodes, n_steps = dm.collect(env, n_ep, policy)
    assert episodes >= n_ep and len(steps) == n_steps and sum(len(s["rew"]) for s in steps) == len(rows)
    obs, m, sigma, eps64, eps32, nscale, act = (np.concatenate([r[j] for r in rec]) for j in range(7))
    return dict(n_rows=len(rows), near=np.concatenate([dm.band_share(s)[1] for s in steps]), cost=sum(s["cost"].sum() for s in steps),
                terminated=sum(s["terminated"].sum() for s in steps), obs=obs, m=m, sigma=sigma, eps64=eps64, eps32=eps32, nscale=nscale, act=act)


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("i", range(len(rm.ALL_CASES)), ids=IDS)
def test_closed_loop_rows_stay_out_of_the_discontinuity_band(i, deterministic):
    kind = rm.ALL_CASES[i][1]
    r = closed_loop(i, deterministic)
    print(f"{IDS[i]} deterministic={deterministic}: {r['n_rows']} rows, cost rows {r['cost']:.0f}, terminations {r['terminated']}, "
          f"within the band {r['near'].mean():.4f}")
    assert r["near"].mean() <= dm.BAND_CAP
    assert r["cost"] > 0
    if kind == "pc":
        assert r["terminated"] > 0


def wrong_formulas(i):
    """name -> (agent whose formula is applied, CPU actor) of every wrong reading of case i's head options"""
    case = rm.ALL_CASES[i]
    agent, kind, n, n_ep, H, opts = case
    out = {}
    max_action = opts.get("max_action", 1.0)
    if agent == "onpolicy":
        unbounded = bool(opts.get("unbounded", False))
    else:
        unbounded = None if agent == "ddpgl" else opts.get("unbounded", agent == "sacl")
    if unbounded is not None:
        out["the other unbounded mode"] = (agent, rm.case_actor(case, unbounded=not unbounded))
    if max_action != 1.0 and not unbounded:
        out["max_action taken as 1"] = (agent, rm.case_actor(case, max_action=1.0))
    if agent in ("sacl", "cvpo"):
        out["the squash dropped" if agent == "sacl" else "the squash added"] = ("cvpo" if agent == "sacl" else "sacl", rm.case_actor(case))
    for members in rm.GROUP_DIFF_CASES.values():
        if case in members:
            for j, other in enumerate(members):
                if other is not case:
                    for k in ("max_action", "exploration_sigma"):
                        if k in other[5] and other[5][k] != opts[k]:
                            out[f"member {j}'s {k}"] = (agent, rm.case_actor(case, **{k: other[5][k]}))
    return out


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("i", range(len(rm.ALL_CASES)), ids=IDS)
def test_the_rows_tell_a_wrong_head_formula_from_the_true_one(i, deterministic):
    agent = rm.ALL_CASES[i][0]
    r = closed_loop(i, deterministic)
    units, ref64, ref32, scale = action_terms(agent, r["m"], r["sigma"], r["eps64"], r["eps32"], deterministic, r["nscale"])
    d_r32 = float(np.max(np.abs(ref32 - ref64) / scale))
    bound = max(3.0 * d_r32, EPS)
    assert float(np.max(np.abs(units(r["act"]) - ref64) / scale)) <= bound          # the closed loop's own action is the restatement
    for name, (agent_w, actor_w) in wrong_formulas(i).items():
        if deterministic and "exploration_sigma" in name:
            continue                                         # a deterministic action has no noise term
        m_w, sigma_w = actor_w(r["obs"])
        if agent == "onpolicy" and not deterministic:
            act_w = m_w.astype(F64) + sigma_w.astype(F64) * r["eps64"]
        else:
            act_w = rm.action(rm.formula(agent_w), m_w, sigma_w, r["eps64"], deterministic, F64)
        d_w = float(np.max(np.abs(units(act_w) - ref64) / scale))
        print(f"{IDS[i]} deterministic={deterministic}: {name} sits {d_w:.3e} from the true action, the bound is {bound:.3e}")
        assert d_w >= 100 * bound, (name, d_w, bound)
    if rm.ALL_CASES[i][5].get("max_action", 1.0) > 1.0 and agent != "sacl" and not deterministic:
        # SAC-Lag's stored action is squashed; the deterministic means of these weights stay within +-0.9 at max_action 1.5
        assert np.abs(r["act"]).max() > 1.0


def test_every_non_default_head_option_has_a_wrong_formula_to_miss():
    for i, case in enumerate(rm.ALL_CASES):
        if any(k in case[5] for k in ("max_action", "unbounded", "exploration_sigma")) and case[5] != {"max_action": 1.0}:
            assert wrong_formulas(i), rm.case_id(case)
    # both unbounded modes of every Gaussian head and of the on-policy head are among the cases
    modes = {(c[0], (c[0] == "sacl") if c[5].get("unbounded") is None else c[5]["unbounded"]) for c in rm.ALL_CASES if c[0] != "ddpgl"}
    assert modes == {(a, u) for a in ("onpolicy", "sacl", "cvpo") for u in (False, True)}


def test_cpu_actor_defaults_are_what_they_were():
    """the new arguments of cpu_actor at their defaults: SAC-Lag's mean is the head, CVPO's and DDPG-Lag's tanh(head), sigma 0.1"""
    obs = np.random.default_rng(0).standard_normal((9, 8)).astype(F32)
    for agent in rm.AGENTS:
        m, sigma = rm.cpu_actor(agent, "lin8")[0](obs)
        m1, sigma1 = rm.cpu_actor(agent, "lin8", (64, 64), 1.0, None, rm.EXPLORATION_SIGMA)[0](obs)
        assert np.array_equal(m, m1) and np.array_equal(sigma, sigma1)
    head = rm.cpu_actor("sacl", "lin8")[0](obs)[0]
    np.testing.assert_allclose(rm.cpu_actor("cvpo", "lin8")[0](obs)[0], np.tanh(head.astype(F64)), rtol=0, atol=3e-7)
    assert np.array_equal(rm.cpu_actor("cvpo", "lin8", unbounded=True)[0](obs)[0], head)
    np.testing.assert_allclose(rm.cpu_actor("sacl", "lin8", max_action=1.5, unbounded=False)[0](obs)[0], 1.5 * np.tanh(head.astype(F64)), rtol=0, atol=3e-7)


def test_a_bounded_mean_at_max_action_above_one_misses_the_one_ulp_floor_in_float32_already():
    """Why no deterministic case pairs max_action 1.5 with heads of |tanh| >= 0.5 (the moved DDPG-Lag case on obs 20 / act 16).  A
    deterministic action IS the mean, which the row-by-row test takes from the batch forward as its float64 value: the restatement's
    distance is 0 and the bound the one-ulp floor at scale max(1, |m|).  But m = max_action tanh(head) is a float32 evaluation on both
    sides.  At max_action 1 the floor covers it (|m| < 1: half an ulp of a value in [0.5, 1)); at 1.5 the float32 restatement of the
    mean alone sits more than one such ulp from float64 where |tanh| >= 0.5, and two float32 tanh that sit an ulp either side of the exact
    value end two floors apart."""
    raw = np.random.default_rng(3).uniform(-1.2, 1.2, 20000).astype(F32)
    far = {}
    for ma in (1.0, 1.5):
        m32, m64 = rm.head_mean(raw, ma, True, F32), rm.head_mean(raw, ma, True, F64)
        d = np.abs(m32.astype(F64) - m64) / np.maximum(1.0, np.abs(m64))
        far[ma] = d.max() / EPS
        if ma == 1.5:
            assert np.all(np.abs(np.tanh(raw.astype(F64)))[d > EPS] >= 0.5)
    print(f"float32 restatement of the bounded mean, in one-ulp floors: max_action 1.0 {far[1.0]:.2f}, 1.5 {far[1.5]:.2f}")
    assert far[1.0] <= 0.5 and far[1.5] > 1.0
    t = np.tanh(raw).astype(F32)
    a, b = (F32(1.5) * t).astype(F32), (F32(1.5) * np.nextafter(np.nextafter(t, F32(2)), F32(2))).astype(F32)
    assert (np.abs(a.astype(F64) - b) / np.maximum(1.0, np.abs(a))).max() >= 1.5 * EPS
