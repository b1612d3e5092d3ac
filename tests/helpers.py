"""Shared helpers for the parity tests (golden-case loading)."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_npz(name):
    return dict(np.load(os.path.join(GOLDEN, name), allow_pickle=False))


def ppo_case(name):
    """-> (cfg dict, golden arrays) for tests/golden/ppo_<name>.npz"""
    g = load_npz(f"ppo_{name}.npz")
    cfg = json.loads(str(g["cfg_json"]))
    return cfg, g


def end_flag_of(g):
    """done | unfinished tail, in sample(0) order (fsrl/policy/base_policy.py:409-411)."""
    end = np.logical_or(g["buf_terminated"], g["buf_truncated"])
    end[np.isin(g["indices"], g["unfinished_index"])] = True
    return end


def oracle_cfg_and_data(cfg, g):
    from oracle.ppo_lag import OnPolicyData, PPOLagConfig
    ocfg = PPOLagConfig(obs_dim=cfg["obs_dim"], act_dim=cfg["act_dim"], hidden=tuple(cfg["hidden"]),
                        max_action=cfg["max_action"], gamma=cfg["gamma"],
                        gae_lambda=cfg["gae_lambda"], eps_clip=cfg["eps_clip"],
                        dual_clip=cfg["dual_clip"], vf_coef=cfg["vf_coef"],
                        max_grad_norm=cfg["max_grad_norm"], target_kl=cfg["target_kl"],
                        advantage_normalization=cfg["advantage_normalization"],
                        use_lagrangian=cfg["use_lagrangian"], lr=cfg["lr"],
                        recompute_advantage=bool(cfg.get("recompute_advantage", False)),
                        unbounded=bool(cfg.get("unbounded", False)),
                        reward_normalization=bool(cfg.get("reward_normalization", False)),
                        value_clip=bool(cfg.get("value_clip", False)))
    data = OnPolicyData(obs=g["buf_obs"], act=g["buf_act"], rew=g["buf_rew"], cost=g["buf_cost"],
                        terminated=g["buf_terminated"], truncated=g["buf_truncated"],
                        obs_next=g["buf_obs_next"], end_flag=end_flag_of(g))
    return ocfg, data


def synth_rollout(seed, env_num, ep_lens_per_env, obs_dim, act_dim, term_prob=0.3, cost_prob=0.1):
    """Seeded synthetic rollouts as lock-step vector steps [(ids, obs, act, rew, cost, term, trunc, obs_next)], the way
    FastCollector pushes them (fast_collector.py:333).  ep_lens_per_env[e] = episode lengths of env e; a negative last entry
    -k = k steps left unfinished.  The full-size fixtures (tests/golden/gen_golden.py `full`) store only the seed and a
    checksum of what this function returns; the generator script and the GPU tests both call it."""
    rng = np.random.default_rng(seed)
    plan = []
    for e in range(env_num):
        steps = []
        for L in ep_lens_per_env[e]:
            unfinished = L < 0
            L = abs(L)
            terminated_end = rng.random() < term_prob
            for t in range(L):
                last = (t == L - 1) and not unfinished
                steps.append((last and terminated_end, last and not terminated_end))
        plan.append(steps)
    T = max(len(p) for p in plan)
    cur = rng.standard_normal((env_num, obs_dim)).astype(np.float32)
    out = []
    for t in range(T):
        ids = [e for e in range(env_num) if t < len(plan[e])]
        k = len(ids)
        obs = cur[ids].copy()
        nxt = rng.standard_normal((k, obs_dim)).astype(np.float32)
        act = (0.3 * rng.standard_normal((k, act_dim))).astype(np.float32)
        rew = rng.normal(0.5, 0.5, k)
        cost = (rng.random(k) < cost_prob).astype(np.float64)
        term = np.array([plan[e][t][0] for e in ids])
        trunc = np.array([plan[e][t][1] for e in ids])
        out.append((ids, obs, act, rew, cost, term, trunc, nxt))
        cur[ids] = nxt
        for j, e in enumerate(ids):
            if term[j] or trunc[j]:
                cur[e] = rng.standard_normal(obs_dim).astype(np.float32)
    return out


def rollout_checksum(steps):
    """float64 sums of every column of synth_rollout's output: guards the fixture against a drift of numpy's generators"""
    return np.array([sum(float(np.asarray(s[c], np.float64).sum()) for s in steps) for c in range(1, 8)])


def rollout_env_major(steps, env_num):
    """the rows in sample(0) order (env-major, time-ordered inside each env) + end_flag = done | unfinished tail"""
    cols = [[[] for _ in range(env_num)] for _ in range(7)]
    for ids, *rest in steps:
        for j, e in enumerate(ids):
            for c, a in enumerate(rest):
                cols[c][e].append(a[j])
    cat = [np.concatenate([np.asarray(cols[c][e]) for e in range(env_num)]) for c in range(7)]
    obs, act, rew, cost, term, trunc, nxt = cat
    end = term | trunc
    off = np.cumsum([len(cols[0][e]) for e in range(env_num)])
    end[off - 1] = True                       # unfinished tails (base_policy.py:409-411); finished ones are set already
    return dict(obs=obs, act=act, rew=rew, cost=cost, terminated=term, truncated=trunc, obs_next=nxt, end_flag=end)


def ppo_full_case(name):
    """tests/golden/ppo_{c2full,c5rank}.npz: BASELINE-size PPO-Lagrangian updates of the unmodified reference (256x256, clip 0.5,
    N = 20 000, 4 passes).  -> (cfg, golden arrays incl. theta0 and int64 perms, the regenerated rollout steps)"""
    cfg, g = ppo_case(name)
    if "theta0" not in g:
        g["theta0"] = load_npz(str(g["theta0_from"]))["theta0"]
    g["perms"] = g["perms"].astype(np.int64)
    env_num = int(g["env_num"])
    steps = synth_rollout(int(g["rollout_seed"]), env_num, [list(g["ep_lens"])] * env_num, cfg["obs_dim"], cfg["act_dim"])
    assert np.array_equal(rollout_checksum(steps), g["rollout_checksum"]), "numpy's generators no longer reproduce the fixture's rollout"
    return cfg, g, steps


def synth_theta(seed, shapes, bias_scale=0.05, head_scale=1.0):
    """A seeded parameter vector for the full-size fixtures (NOT stored in them: regenerated here, checksum in the fixture):
    `shapes` = the shapes of a module's parameters() in order; matrices ~ N(0, 1 / fan_in), vectors ~ bias_scale * N(0, 1);
    a (Da, 1) tensor is the on-policy actor's sigma_param (= -0.5, ppo_lag_agent.py:147).  head_scale: factor on the head
    matrices (<= 16 output rows): the multi-seed learning-curve fixtures start from small mean actions (0.1), like the agents'
    `last_layer_scale` option (ppo_lag_agent.py:155-161), instead of a saturated tanh."""
    rng = np.random.default_rng(seed)
    parts = []
    for sh in shapes:
        sh = tuple(int(x) for x in sh)
        if len(sh) == 2 and sh[1] == 1 and sh[0] <= 16:
            parts.append(np.full(sh[0], -0.5, np.float32))
        elif len(sh) == 2:
            w = (rng.standard_normal(sh) / np.sqrt(sh[1])).astype(np.float32)
            if sh[0] <= 16 and head_scale != 1.0:
                w = (w * np.float32(head_scale)).astype(np.float32)
            parts.append(w.reshape(-1))
        else:
            parts.append((bias_scale * rng.standard_normal(sh)).astype(np.float32).reshape(-1))
    return np.concatenate(parts)


def theta_checksum(theta):
    th = np.asarray(theta, np.float64)
    return np.array([th.sum(), np.abs(th).sum(), (th * np.arange(1, th.size + 1)).sum()])


def full_rollout_arrays(g, obs_dim, act_dim):
    """the regenerated rollout of a full-size fixture as the arrays the small fixtures store: env-major rows (sample(0) order)
    under the small fixtures' keys (buf_* and st_*), env_rows, slots, indices, unfinished_index"""
    env_num = int(g["env_num"])
    ep_lens = [int(x) for x in g["ep_lens"]]
    steps = synth_rollout(int(g["rollout_seed"]), env_num, [ep_lens] * env_num, obs_dim, act_dim)
    assert np.array_equal(rollout_checksum(steps), g["rollout_checksum"]), "numpy's generators no longer reproduce the fixture's rollout"
    em = rollout_env_major(steps, env_num)
    rows = sum(abs(x) for x in ep_lens)
    sub = int(g["sub_size"])
    slots = np.concatenate([e * sub + np.arange(rows) for e in range(env_num)])
    out = {"env_rows": np.full(env_num, rows), "slots": slots, "indices": slots.copy(),
           "unfinished_index": np.array([e * sub + rows - 1 for e in range(env_num) if ep_lens[-1] < 0], np.int64)}
    for k in ("obs", "act", "rew", "cost", "terminated", "truncated", "obs_next"):
        out["buf_" + k] = out["st_" + k] = em[k]
    return out, steps


def trust_full_case(name):
    """tests/golden/cpo_c3full.npz: BASELINE configs[2] (obs 60, act 2, 256x256, N = 20 000 full batch) through one repeat of the
    unmodified CPO.update; rollout and theta0 regenerated from seeds.  -> the dict the small-fixture tests take"""
    g = load_npz(f"cpo_{name}.npz")
    cfg = json.loads(str(g["cfg_json"]))
    arr, _ = full_rollout_arrays(g, cfg["obs_dim"], cfg["act_dim"])
    g.update(arr)
    shapes = [tuple(s) for s in json.loads(str(g["theta_shapes_json"]))]
    g["theta0"] = synth_theta(int(g["theta_seed"]), shapes)
    assert np.array_equal(theta_checksum(g["theta0"]), g["theta0_checksum"])
    g["perms"] = g["perms"].astype(np.int64)
    return g


def sac_full_case(name):
    """tests/golden/sac_c4full.npz: BASELINE configs[3]'s shape (obs 33, act 8, 256x256, batch 1024, n_step 2) over a 97 000-row
    store regenerated from a seed; parameters regenerated from seeds; the tanh of the rollout's raw actions is what is stored"""
    g = load_npz(f"sac_{name}.npz")
    cfg = json.loads(str(g["cfg_json"]))
    arr, _ = full_rollout_arrays(g, cfg["obs_dim"], cfg["act_dim"])
    arr["st_act"] = arr["buf_act"] = np.tanh(arr["st_act"])
    del arr["indices"]                                   # the fixture's own `indices` are the recorded buffer.sample draws
    g.update(arr)
    for key in ("actor", "critics"):
        shapes = [tuple(s) for s in json.loads(str(g[f"theta_{key}_shapes_json"]))]
        g[f"theta_{key}0"] = synth_theta(int(g[f"theta_{key}_seed"]), shapes)
        assert np.array_equal(theta_checksum(g[f"theta_{key}0"]), g[f"theta_{key}0_checksum"])
    return g


def focops_case(name):
    """tests/golden/focops_<name>.npz -> (cfg, arrays).  The compact case (`wide`) stores neither its rollout nor theta0: they are
    regenerated from the stored seeds (checksums stored), and its theta_final holds the actor in full and every
    theta_final_stride-th entry of the critics.  theta_final_idx: the entries of the parameter vector theta_final holds."""
    g = load_npz(f"focops_{name}.npz")
    cfg = json.loads(str(g["cfg_json"]))
    if "rollout_seed" in g:
        arr, _ = full_rollout_arrays(g, cfg["obs_dim"], cfg["act_dim"])
        g.update(arr)
        shapes = [tuple(s) for s in json.loads(str(g["theta_shapes_json"]))]
        g["theta0"] = synth_theta(int(g["theta_seed"]), shapes)
        assert np.array_equal(theta_checksum(g["theta0"]), g["theta0_checksum"])
    n = g["theta0"].size
    if "theta_final_stride" in g:
        nf = int(g["theta_final_n_full"])
        g["theta_final_idx"] = np.concatenate([np.arange(nf), np.arange(nf, n, int(g["theta_final_stride"]))])
    else:
        g["theta_final_idx"] = np.arange(n)
    assert g["theta_final"].size == g["theta_final_idx"].size
    return cfg, g


def replay_last_write_wins(steps, env_num, sub, obs_dim, act_dim):
    """Lock-step vector steps (synth_rollout's format) replayed into SLOT-indexed arrays the way a ring of `sub` rows per env
    keeps them: row n of env e lands in slot e * sub + n % sub, the last write wins.
    -> (store dict for the oracles, heads [(size, index, last_index)] per env, the slot of every pushed row per step)"""
    store = {k: np.zeros((env_num * sub, ) + s, d) for k, s, d in (
        ("obs", (obs_dim, ), np.float32), ("obs_next", (obs_dim, ), np.float32), ("act", (act_dim, ), np.float32),
        ("rew", (), np.float64), ("cost", (), np.float64), ("terminated", (), bool), ("truncated", (), bool))}
    count = np.zeros(env_num, np.int64)
    slots = []
    for ids, obs, act, rew, cost, term, trunc, nxt in steps:
        at = np.array([e * sub + count[e] % sub for e in ids], np.int64)
        for k, v in (("obs", obs), ("act", act), ("rew", rew), ("cost", cost), ("terminated", term), ("truncated", trunc),
                     ("obs_next", nxt)):
            store[k][at] = v
        count[list(ids)] += 1
        slots.append(at)
    heads = np.array([[min(n, sub), n % sub, (n - 1) % sub if n else 0] for n in count], np.int64)
    return store, heads, slots


def sac_wrapped_case(name):
    """tests/golden/sac_wrapped.npz: SACLagrangian.update of the unmodified reference over a VectorReplayBuffer whose sub-buffers
    were overwritten about 2.5 times with three different write heads (n_step 3).  The rollout is regenerated from its seed
    (checksum in the fixture); the stored actions are the tanh of the rollout's.  g["steps"]: the vector steps to push in order."""
    g = load_npz(f"sac_{name}.npz")
    cfg = json.loads(str(g["cfg_json"]))
    env_num = int(g["env_num"])
    steps = synth_rollout(int(g["rollout_seed"]), env_num, json.loads(str(g["ep_lens_json"])), cfg["obs_dim"], cfg["act_dim"])
    assert np.array_equal(rollout_checksum(steps), g["rollout_checksum"]), "numpy's generators no longer reproduce the fixture's rollout"
    g["steps"] = [(ids, obs, np.tanh(act), rew, cost, term, trunc, nxt) for ids, obs, act, rew, cost, term, trunc, nxt in steps]
    return g


def replay_problem(rng, engines, rows, obs_dim, act_dim, act_of, sub=128):
    """A random replay store for the SAC-Lag / DDPG-Lag / CVPO variant tests, pushed in lock step (env e gets rows[e] rows, the
    envs drop out as they run dry) into every engine of `engines` and mirrored into SLOT-indexed arrays for the oracles.
    act_of: standard normal draws [k, act_dim] -> the stored actions (tanh, scaled tanh, clip).  The draws of a step come in the
    order obs, act, rew, cost, terminated, obs_next.  -> (store dict, oracle.sac_lag.ReplayIndex, the valid slots)"""
    from oracle.sac_lag import ReplayIndex
    E = len(rows)
    store = {k: np.zeros((E * sub, ) + s, d) for k, s, d in (("obs", (obs_dim, ), np.float32), ("obs_next", (obs_dim, ), np.float32),
             ("act", (act_dim, ), np.float32), ("rew", (), np.float64), ("cost", (), np.float64),
             ("terminated", (), bool), ("truncated", (), bool))}
    for t in range(max(rows)):
        ids = [e for e in range(E) if t < rows[e]]
        k = len(ids)
        row = dict(obs=rng.standard_normal((k, obs_dim)).astype(np.float32),
                   act=act_of(rng.standard_normal((k, act_dim))).astype(np.float32), rew=rng.normal(0, 1, k),
                   cost=(rng.random(k) < 0.3).astype(np.float64), terminated=rng.random(k) < 0.1,
                   truncated=np.full(k, t % 11 == 10), obs_next=rng.standard_normal((k, obs_dim)).astype(np.float32))
        for eng in engines:
            eng.push(ids, row["obs"], row["act"], row["rew"], row["cost"], row["terminated"], row["truncated"], row["obs_next"])
        for e, j in zip(ids, range(k)):
            for key in store:
                store[key][e * sub + t] = row[key][j]
    index = ReplayIndex(rows, sub, store["terminated"] | store["truncated"])
    valid = np.concatenate([e * sub + np.arange(r) for e, r in enumerate(rows)])
    return store, index, valid


def fan_in_params(rng, spec):
    """A flat parameter vector over `spec` (name -> shape, torch parameters() order): W ~ N(0, 1 / fan_in), b ~ 0.1 N(0, 1) -- the
    heads stay off the tails of tanh at any depth and width"""
    return np.concatenate([(rng.standard_normal(shp) / np.sqrt(shp[1]) if len(shp) == 2 else 0.1 * rng.standard_normal(shp)).ravel()
                           for shp in spec.values()]).astype(np.float32)


# ---- the replay agents' oracle runs (tests/test_gpu_layered_replay.py, tests/branch_problems.py): a case is a dict with Do, Da, hidden,
# and the options n_step, auto_alpha, use_lag (SAC-Lag), K, double (CVPO)
SAC_KEYS = ["loss/rescaling", "loss/lagrangian", "loss/actor_safety", "loss/alpha_loss", "loss/alpha_value",
            "loss/actor_rew", "loss/actor_total", "loss/q0", "loss/q1", "loss/q_total"]
CVPO_KEYS = ["loss/estep_loss", "estep/dual0", "estep/dual1", "mstep/mstep_kl_mu", "mstep/mstep_kl_std", "mstep/mstep_loss_kl",
             "mstep/mstep_loss_mle", "mstep/mstep_loss_total", "mstep/mstep_dual_mu", "mstep/mstep_dual_std", "mstep/entropy",
             "loss/loss_q0", "estep/val_q0", "loss/loss_q1", "estep/val_q1", "estep/thres_q1", "loss/q_total"]
ROW_BAR = {"sac": (1e-4, 1e-5), "ddpg": (1e-4, 1e-5), "cvpo": (2e-4, 2e-5)}          # rel, abs
VEC_BAR = {"sac": (5e-6, 3e-3), "ddpg": (5e-6, 3e-3), "cvpo": (1e-5, 5e-3)}          # q99, max


def replay_cvpo_cfg(c):
    from oracle.cvpo import CVPOConfig
    return CVPOConfig(obs_dim=c["Do"], act_dim=c["Da"], hidden=tuple(c["hidden"]), max_action=1.0, gamma=0.97, n_step=2, tau=0.1,
                      double_critic=c.get("double", False), sample_act_num=c["K"], estep_iter_num=1, mstep_iter_num=1, cost_limit=0.5,
                      max_episode_steps=50, mstep_kl_mu=1e-4, mstep_kl_std=1e-5, actor_lr=1e-3)


def replay_oracles(kind, c):
    """the fp32 oracle and its float64 twin"""
    import torch
    if kind == "sac":
        from oracle.sac_lag import SACConfig, SACLagOracle
        cfg = SACConfig(obs_dim=c["Do"], act_dim=c["Da"], hidden=tuple(c["hidden"]), gamma=0.98, n_step=c.get("n_step", 2), tau=0.1,
                        alpha=0.05, auto_alpha=c.get("auto_alpha", True), use_lagrangian=c.get("use_lag", True))
        return SACLagOracle(cfg), SACLagOracle(cfg, dtype=torch.float64)
    if kind == "ddpg":
        from oracle.ddpg_lag import DDPGConfig, DDPGLagOracle
        cfg = DDPGConfig(obs_dim=c["Do"], act_dim=c["Da"], hidden=tuple(c["hidden"]), max_action=1.0, gamma=0.98, n_step=2, tau=0.1,
                         actor_lr=1e-3, critic_lr=1e-3, use_lagrangian=True)
        return DDPGLagOracle(cfg), DDPGLagOracle(cfg, dtype=torch.float64)
    from oracle.cvpo import CVPOOracle
    return CVPOOracle(replay_cvpo_cfg(c)), CVPOOracle(replay_cvpo_cfg(c), dtype=torch.float64)


def replay_vectors(kind, o):
    v = {"actor": o.actor_flat(), "critics": o.critics_flat(), "critics_old": o.critics_flat(old=True)}
    if kind != "sac":
        v["actor_old"] = o.actor_flat(old=True)
    return v


def replay_row_items(kind, row):
    """(key, value) of a logged row -- an oracle's dict or a device row (CVPO: with the duals)"""
    keys = CVPO_KEYS if kind == "cvpo" else SAC_KEYS
    if isinstance(row, dict):
        items = [(k, float(row[k])) for k in keys if k in row]
        duals = row.get("duals")
    else:
        st, duals = row if kind == "cvpo" else (row, None)
        items = [(k, float(st[j])) for j, k in enumerate(keys)]
    if duals is not None:
        items += [(f"duals[{j}]", float(d)) for j, d in enumerate(duals)]
    return dict(items)
