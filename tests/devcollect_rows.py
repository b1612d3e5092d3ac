"""What the row-by-row device-collect tests share (tests/test_gpu_devcollect.py, test_gpu_devcollect_replay.py,
test_gpu_devcollect_shapes.py) and what their CPU twin (tests/test_devcollect_shapes_model.py) measures with.  TEST INFRASTRUCTURE ONLY.
numpy; no GPU is touched here: the engine and the env arrive as arguments.

The bars are those of DESIGN.md 6.  Continuous outputs: the device at most 3 x as far from the float64 model as the float32
restatement, never held tighter than one float32 ulp at the value's scale.  Discontinuous outputs: equal outside a band of
1e-5 x scale around the threshold that at most 2 % of the rows may lie in."""
import numpy as np

import devenv_model as dm
import devenv_replay_model as rm

F32, F64 = np.float32, np.float64


def check_discontinuous(dev_cost, dev_term, r32, what):
    share, near = dm.band_share(r32)
    print(f"{what}: rows within the band {share:.4f}")
    assert share <= dm.BAND_CAP, what
    assert np.array_equal(np.asarray(dev_cost)[~near], r32["cost"][~near]), what
    assert np.array_equal(np.asarray(dev_term, bool)[~near], r32["terminated"][~near]), what


def check_continuous(dev, r64, r32, scale, what):
    d_dev, d_r32, bound = dm.yardstick(dev, r64, r32, scale)
    print(f"{what}: device {d_dev:.3e} from float64, float32 restatement {d_r32:.3e}, bound {bound:.3e}")
    assert d_dev <= bound, (what, d_dev, d_r32)
    return d_dev, d_r32


def rows_with_counters(eng, ord0, rows_idx, rows):
    """(env, ordinal, t) of every stored row: rows of an env are chronological, the first one continues at (ord0 - 1, 0)"""
    sub, _ = eng.store_geometry()
    e = (rows_idx // sub).astype(np.int64)
    ordinal, t = np.zeros(len(e), np.int64), np.zeros(len(e), np.int64)
    first = np.zeros(len(e), bool)
    cur = {}
    for i, ei in enumerate(e):
        o, tt = cur.get(int(ei), (int(ord0[ei]) - 1, 0))
        ordinal[i], t[i], first[i] = o, tt, tt == 0
        done = rows["terminated"][i] or rows["truncated"][i]
        cur[int(ei)] = (o + 1, 0) if done else (o, tt + 1)
    return e, ordinal, t, first


# ---------------------------------------------------------------------------------------------- the action, in the units it is measured in
def action_terms(agent, mu, sigma, eps64, eps32, deterministic, nscale):
    """-> (units, ref64, ref32, scale): `units(act)` is held to ref64 by the yardstick rule with ref32 the float32 restatement.
    The on-policy head in training mode is measured as the existing test measures it, in units of the noise -- (act - mu) / sigma
    against the model's normal; every other case in units of the action, by the agent's formula of tests/devenv_replay_model.py."""
    if agent == "onpolicy" and not deterministic:
        mu, sigma = np.asarray(mu, F64), np.asarray(sigma, F64)
        act32 = (mu.astype(F32) + sigma.astype(F32) * eps32).astype(F32)
        scale = np.maximum(nscale, (np.abs(mu) + np.abs(sigma * eps64)) / sigma)
        return (lambda act: (np.asarray(act, F64) - mu) / sigma), eps64, (act32.astype(F64) - mu) / sigma, scale
    f = rm.formula(agent)
    return ((lambda act: np.asarray(act, F64)), rm.action(f, mu, sigma, eps64, deterministic, F64),
            rm.action(f, mu, sigma, eps32, deterministic, F32), rm.action_scale(mu, sigma, eps64, deterministic))


def check_action(agent, act, mu, sigma, eps64, eps32, deterministic, nscale, what):
    units, r64, r32, scale = action_terms(agent, mu, sigma, eps64, eps32, deterministic, nscale)
    return check_continuous(units(act), r64, r32, scale, what)


# ---------------------------------------------------------------------------------------------- one collect's rows against the model
def check_collect_rows(eng, env, ord0, res, n_ep, kind, seed, what, action_check):
    """Everything the row-by-row tests assert of ONE collect from freshly reset envs except the action itself, which
    action_check(rows, e, ordinal, t, key) holds to its agent's formula: episode and statistics bookkeeping, obs_next and rew under
    the yardstick rule, cost and terminated outside the band, chaining, reset draws, the resets at the end of the collect.
    -> (rows, distances): distances[name] = (device, float32 restatement), both from the float64 model"""
    PC = rm.PC
    idx = eng.sample0()
    rows = eng.store_read(idx)
    key = dm.key_of(seed)
    Do = eng.cfg.obs_dim
    e, ordinal, t, first = rows_with_counters(eng, ord0, idx, rows)
    done = rows["terminated"] | rows["truncated"]
    dist = {}
    # ---- episode count, time limit, statistics
    assert done.sum() == n_ep == len(res["ep_rews"]) and res["steps"] == len(idx)
    assert np.array_equal(rows["truncated"], t == 6) and np.all(t <= 6)
    ep_rew, ep_len, acc = [], [], {}
    for i in range(len(idx)):                                   # float64 sums over the stored rows, in order
        r_, l_ = acc.get(int(e[i]), (0.0, 0))
        r_, l_ = r_ + rows["rew"][i], l_ + 1
        if done[i]:
            ep_rew.append(r_); ep_len.append(l_); r_, l_ = 0.0, 0
        acc[int(e[i])] = (r_, l_)
    assert sorted(ep_rew) == sorted(res["ep_rews"].tolist()) and sorted(ep_len) == sorted(res["ep_lens"].tolist())
    assert res["total_cost"] == rows["cost"].sum() and res["terminated"] == rows["terminated"].sum() and res["truncated"] == rows["truncated"].sum()
    # ---- the action: the agent's formula over (m, sigma) of the row's observation and the model's draw of (env, ordinal, t, dim)
    dist["act"] = action_check(rows, e, ordinal, t, key)
    # ---- the transition: obs_next, rew, cost, terminated from (obs, mapped act, model noise)
    env_act = dm.map_action(rows["act"], 1)
    if kind == "pc":
        r64 = dm.point_step(rows["obs"][:, :4], env_act, PC["radius"], PC["x_lim"], PC["dt"], F64)
        r32 = dm.point_step(rows["obs"][:, :4], env_act, PC["radius"], PC["x_lim"], PC["dt"], F32)
    else:
        dd = np.arange(Do)[None, :]
        nz = [dm.normal(key, e[:, None], ordinal[:, None], t[:, None], dm.STREAM_STEP, dd, dt_) for dt_ in (F64, F32)]
        r64 = dm.linear_step(rows["obs"], env_act, env.A, env.B, nz[0], env.cost_threshold, F64)
        r32 = dm.linear_step(rows["obs"], env_act, env.A, env.B, nz[1], env.cost_threshold, F32)
    dist["obs_next"] = check_continuous(rows["obs_next"], r64["obs_next"], r32["obs_next"], r32["obs_scale"], what + " obs_next")
    dist["rew"] = check_continuous(rows["rew"], r64["rew"], r32["rew"], r32["rew_scale"], what + " rew")
    check_discontinuous(rows["cost"], rows["terminated"], r32, what)
    if kind == "pc":
        assert rows["cost"].sum() > 0 and rows["terminated"].sum() > 0
    # ---- chaining: inside an episode obs_next[t] is obs[t + 1], bit for bit; an episode starts at the model's reset draw
    same_env_next = (e[1:] == e[:-1]) & ~done[:-1]
    assert np.array_equal(rows["obs_next"][:-1][same_env_next], rows["obs"][1:][same_env_next]) and same_env_next.sum() > 0
    if kind == "pc":
        st0, ob0 = dm.point_reset(key, e[first], ordinal[first], PC["radius"], PC["x_lim"], F32)
        assert np.array_equal(rows["obs"][first], ob0)
    else:
        dd = np.arange(Do)[None, :]
        ef, of = e[first][:, None], ordinal[first][:, None]
        dist["first obs"] = check_continuous(rows["obs"][first], dm.normal(key, ef, of, 0, dm.STREAM_RESET, dd, F64),
                                             dm.normal(key, ef, of, 0, dm.STREAM_RESET, dd, F32),
                                             dm.normal_scale(key, ef, of, 0, dm.STREAM_RESET, dd), what + " first obs")
    # every env was reset at the end of the collect
    _, t1, ord1 = env.get_state()
    assert np.all(t1 == 0) and np.all(ord1 >= 2)
    return rows, dist


def action_draws(rows, e, ordinal, t, key, Da):
    """the model's action-stream normals of the rows, float64 and float32, and the scale of a normal"""
    d = np.arange(Da)[None, :]
    eps64 = dm.normal(key, e[:, None], ordinal[:, None], t[:, None], dm.STREAM_ACT, d, F64)
    eps32 = dm.normal(key, e[:, None], ordinal[:, None], t[:, None], dm.STREAM_ACT, d, F32)
    return eps64, eps32, dm.normal_scale(key, e[:, None], ordinal[:, None], t[:, None], dm.STREAM_ACT, d)
