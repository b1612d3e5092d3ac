"""Grouped FOCOPS updates (fsrl_group_* over FOCOPS contexts): k FOCOPS agents of one shape stepped in lock step, every launch
of the minibatch step carrying all members.  Per member the update must be Engine.focops_update on that member alone: bit for
bit wherever the grouped launch runs the member's solo tile height (a group of one; groups small enough to keep 4-row tiles;
minibatches large enough that the solo pass already runs 16-row tiles), within test_gpu_group.py's tolerances otherwise.
Both plans are covered: three launches per step (ppo_wgrad) and four (split-K weight gradients + their sum)."""
import json

import numpy as np
import pytest

from helpers import load_npz

pytestmark = pytest.mark.gpu

FIXTURES = ["small", "c1", "earlystop", "unbounded", "recompute"]     # the non-layered golden FOCOPS cases


def _case(name):
    g = load_npz(f"focops_{name}.npz")
    return json.loads(str(g["cfg_json"])), g


def _engine(cfg, g, i=0, four_launch=0, steps=None, init=True, **foc):
    """member i on the golden store (its first `steps` vector steps): theta0 perturbed by seed i for i > 0"""
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig
    eng = Engine(EngineConfig(algo=_lib.ALGO_FOCOPS, obs_dim=cfg["obs_dim"], act_dim=cfg["act_dim"], hidden_sizes=tuple(cfg["hidden"]),
                              n_critics=2, env_num=cfg["env_num"], max_action=cfg["max_action"], gamma=cfg["gamma"],
                              gae_lambda=cfg["gae_lambda"], norm_adv=cfg["advantage_normalization"], target_kl=None,
                              unbounded=bool(cfg.get("unbounded", False)),
                              recompute_adv=bool(cfg.get("recompute_advantage", False))))
    kw = dict(actor_lr=cfg["actor_lr"], critic_lr=cfg["critic_lr"], l2_reg=cfg["l2_reg"], delta=cfg["delta"], eta=cfg["eta"],
              tem_lambda=cfg["tem_lambda"], max_grad_norm=cfg["max_grad_norm"])
    kw.update(foc)
    if init:
        eng.focops_init(**kw)
        eng.focops_set_plan(four_launch)
    th = g["theta0"] + (0.01 * np.random.default_rng(100 + i).standard_normal(g["theta0"].size)).astype(np.float32) * (i > 0)
    eng.set_params(th)
    rows = g["env_rows"]; off = np.concatenate([[0], np.cumsum(rows)])
    T = rows.max() if steps is None else min(steps, rows.max())
    for t in range(T):
        ids = [e for e in range(len(rows)) if t < rows[e]]
        sel = np.array([off[e] + t for e in ids])
        eng.push(ids, g["buf_obs"][sel], g["buf_act"][sel], g["buf_rew"][sel], g["buf_cost"][sel], g["buf_terminated"][sel],
                 g["buf_truncated"][sel], g["buf_obs_next"][sel])
    return eng


def _nu(g, i):
    """member i's (nu, nu_loss): member 0 the golden host-side nu step, the others their own"""
    return float(g["stats_nu"][0][1]) * (1.0 + 0.5 * i), float(g["stats_nu"][0][0]) - 0.1 * i


def _chunks(n, size):
    from fsrl_amd.policy.ppo_lag import _chunk_sizes
    return _chunk_sizes(n, size) if n else []


def _exact(sizes, k):
    """True per member when every grouped launch runs the member's solo tile height whichever members are still active:
    the solo pass takes 4-row tiles while 4 * tiles * 3 <= CUs, the group while 4 * max tiles * 3 * active members <= CUs"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_mb = max(len(s) for s in sizes)
    tmax = [max(((s[j] + 15) // 16 if j < len(s) else 0) for s in sizes) for j in range(n_mb)]
    return [all(12 * ((s[j] + 15) // 16) > cus or 12 * tmax[j] * k <= cus for j in range(len(s))) for s in sizes]


def _close_params(a, b, lr, bulk=0.05, tail=1.0):
    # 16-row vs 4-row tiles round differently; Adam turns rounding-noise gradients into +-lr steps on a few entries
    # (test_gpu_group.py).  Looser than test_gpu_group.py's clipped bound (1 % / a fifth of a step), as its unclipped one:
    # FOCOPS's loss keeps a row only while KL(new || old) <= eta, and a last-bit difference flips that mask for rows at the
    # threshold, which moves the gradient by a whole row's share.  99 % of the entries within 5 % of a learning-rate step,
    # none beyond one step.
    d = np.abs(a - b)
    assert np.quantile(d, 0.99) <= bulk * lr and d.max() <= tail * lr, (np.quantile(d, 0.99), d.max())


def _perms(g, cfg, k, sizes, seed=5):
    R = cfg["repeat"]
    rng = np.random.default_rng(seed)
    perms = [[rng.permutation(n) for _ in range(R)] for n in sizes]
    if sizes[0] == len(g["indices"]):                # member 0 replays the golden permutations (all the passes it recorded)
        for j, pj in enumerate(g["perms"][:R]):
            perms[0][j] = np.asarray(pj)
    return perms


@pytest.mark.parametrize("four_launch", [0, 1])
@pytest.mark.parametrize("name", FIXTURES)
def test_group_of_one_is_the_single_focops_update_bit_for_bit(name, four_launch):
    from fsrl_amd.engine import EngineGroup
    cfg, g = _case(name)
    R, B = cfg["repeat"], cfg["batch_size"]
    nu, nl = _nu(g, 0)
    perms = _perms(g, cfg, 1, [len(g["indices"])])[0]
    solo = _engine(cfg, g, four_launch=four_launch)
    want = [solo.focops_update(nu, nl, B, R, perms=perms) for _ in range(2)]          # Adam state and pp parity carried over
    eng = _engine(cfg, g, four_launch=four_launch)
    grp = EngineGroup([eng])
    for st_w, sp_w in want:
        st, sp = grp.focops_update([nu], [nl], B, R, perms=[perms])
        assert sp[0] == sp_w and np.array_equal(st[0], st_w), name
    assert np.array_equal(eng.get_params(), solo.get_params())
    np.testing.assert_allclose(want[0][0], np.concatenate([g["stats_nu"], g["stats_actor"], g["stats_critic"]], 1),
                               rtol=3e-5, atol=3e-5)      # the golden case itself (its first update)
    # the member's own update while grouped, and after the group is gone
    for close in (False, True):
        if close:
            grp.close()
        s1, p1 = solo.focops_update(nu, nl, B, R, perms=perms)
        s2, p2 = eng.focops_update(nu, nl, B, R, perms=perms)
        assert p1 == p2 and np.array_equal(s1, s2) and np.array_equal(eng.get_params(), solo.get_params())
    for e in (eng, solo):
        e.close()


@pytest.mark.parametrize("four_launch", [0, 1])
@pytest.mark.parametrize("name,k", [("small", 2), ("c1", 3), ("earlystop", 3), ("unbounded", 8), ("recompute", 8), ("c1", 8)])
def test_grouped_focops_equals_member_by_member(name, k, four_launch):
    from fsrl_amd.engine import EngineGroup
    cfg, g = _case(name)
    R, B = cfg["repeat"], cfg["batch_size"]
    n = len(g["indices"])
    perms = _perms(g, cfg, k, [n] * k)
    nus = [_nu(g, i) for i in range(k)]
    want = []
    for i in range(k):
        e = _engine(cfg, g, i, four_launch)
        a = e.focops_update(*nus[i], B, R, perms=perms[i])
        b = e.focops_update(*nus[i], B, R, perms=perms[i])
        want.append((a, b, e.get_params()))
        e.close()
    engs = [_engine(cfg, g, i, four_launch) for i in range(k)]
    grp = EngineGroup(engs)
    got_a = grp.focops_update([x[0] for x in nus], [x[1] for x in nus], B, R, perms=perms)
    got_b = grp.focops_update([x[0] for x in nus], [x[1] for x in nus], B, R, perms=perms)
    exact = _exact([_chunks(n, B)] * k, k)
    for i in range(k):
        (sa, pa), (sb, pb), th = want[i]
        assert got_a[1][i] == pa and got_b[1][i] == pb, (i, got_a[1], got_b[1], pa, pb)
        assert got_a[0][i].shape == sa.shape and got_b[0][i].shape == sb.shape
        if exact[i]:
            assert np.array_equal(got_a[0][i], sa) and np.array_equal(got_b[0][i], sb), i
            assert np.array_equal(engs[i].get_params(), th), i
        else:
            np.testing.assert_allclose(got_a[0][i], sa, rtol=2e-5, atol=2e-5)
            np.testing.assert_allclose(got_b[0][i], sb, rtol=2e-4, atol=2e-4)
            _close_params(engs[i].get_params(), th, max(cfg["actor_lr"], cfg["critic_lr"]))
    np.testing.assert_allclose(got_a[0][0], np.concatenate([g["stats_nu"], g["stats_actor"], g["stats_critic"]], 1),
                               rtol=3e-5, atol=3e-5)      # member 0 == the reference's golden update
    grp.close()
    for e in engs:
        e.close()


@pytest.mark.parametrize("four_launch", [0, 1])
def test_large_minibatches_are_bit_identical_at_k8(four_launch):
    """minibatches whose solo pass already runs 16-row tiles (380 rows: 24 tiles x 3 networks x 4 rows > the CUs; three
    minibatches of c1's 1140 rows, all at most 512 rows, so the three-launch plan stays on): the group of 8 runs the same tiles,
    so every member is its solo run bit for bit"""
    from fsrl_amd.engine import EngineGroup
    cfg, g = _case("c1")
    k, B, R = 8, 380, 2
    n = len(g["indices"])
    rng = np.random.default_rng(11)
    perms = [[rng.permutation(n) for _ in range(R)] for _ in range(k)]
    assert all(_exact([_chunks(n, B)] * k, k))
    nus = [_nu(g, i) for i in range(k)]
    want = []
    for i in range(k):
        e = _engine(cfg, g, i, four_launch, delta=1e9)
        want.append((e.focops_update(*nus[i], B, R, perms=perms[i])[0], e.get_params()))
        e.close()
    engs = [_engine(cfg, g, i, four_launch, delta=1e9) for i in range(k)]
    grp = EngineGroup(engs)
    st, sp = grp.focops_update([x[0] for x in nus], [x[1] for x in nus], B, R, perms=perms)
    for i in range(k):
        assert sp[i] == -1 and np.array_equal(st[i], want[i][0]) and np.array_equal(engs[i].get_params(), want[i][1]), i
    grp.close()
    for e in engs:
        e.close()


@pytest.mark.parametrize("four_launch", [0, 1])
def test_ragged_members_an_empty_member_and_a_kl_stop(four_launch):
    """members with different store lengths (different minibatch counts, merged last minibatches), one member without rows
    that sits out (it carries a stale plan from an earlier update), and one member whose learning rate trips the delta KL
    check in its first pass while the others go on: every member's rows and stopped pass are its solo run's"""
    from fsrl_amd.engine import EngineGroup
    cfg, g = _case("small")
    B, R = cfg["batch_size"], 3
    steps = [127, 60, 90, 127]                         # vector steps of the store: 381, 180, 270 and 381 rows
    over = [dict(), dict(), dict(), dict(actor_lr=0.1)]
    nus = [_nu(g, i) for i in range(5)]

    def members():
        es = [_engine(cfg, g, i, four_launch, steps=steps[i], **over[i]) for i in range(4)]
        empty = _engine(cfg, g, 4, four_launch)
        empty.focops_update(*nus[4], B, 1, seed=3)     # leaves a plan behind ...
        empty.reset_store()                            # ... and then no rows
        return es + [empty]

    solo = members()
    sizes = [len(e) for e in solo]
    assert sizes[4] == 0 and len(set(sizes[:3])) == 3
    rng = np.random.default_rng(2)
    perms = [[rng.permutation(n) for _ in range(R)] for n in sizes]
    want = [e.focops_update(*nus[i], B, R, perms=perms[i]) for i, e in enumerate(solo)]
    assert want[3][1] >= 0 and all(w[1] == -1 for w in want[:3]), [w[1] for w in want]
    engs = members()
    grp = EngineGroup(engs)
    st, sp = grp.focops_update([x[0] for x in nus], [x[1] for x in nus], B, R, perms=perms)
    assert st[4].shape[0] == 0 and sp[4] == -1
    exact = _exact([_chunks(n, B) for n in sizes[:4]], 4)
    for i in range(4):
        assert sp[i] == want[i][1] and st[i].shape == want[i][0].shape, (i, sp, [w[1] for w in want])
        if exact[i]:
            assert np.array_equal(st[i], want[i][0]) and np.array_equal(engs[i].get_params(), solo[i].get_params()), i
        else:
            np.testing.assert_allclose(st[i], want[i][0], rtol=2e-5, atol=2e-5)
            _close_params(engs[i].get_params(), solo[i].get_params(), max(cfg["actor_lr"], cfg["critic_lr"]))
    grp.close()
    for e in engs + solo:
        e.close()


GROUP_SHAPES = [  # Do, Da, hidden, rows per env of each member, batch, repeat
    # 256 wide: 256-row minibatches take 4-row tiles solo and 16-row tiles in the group of three; 324 / 390 / 510-row merged ones
    (33, 6, 256, ([300, 280], [200, 190], [260, 250]), 256, 2),
    # minibatches over 512 rows: every member on the four-launch step, focops_wgrad_split_group_kernel; act_dim > 4
    (20, 9, 128, ([700, 650], [560, 600], [900, 800]), 600, 2),
]


@pytest.mark.parametrize("Do,Da,h,member_rows,B,R", GROUP_SHAPES)
def test_grouped_members_vs_their_own_fp32_oracle(Do, Da, h, member_rows, B, R):
    """k = 3 members with ragged N, their own theta0, nu and permutations: each member's rows, stopped pass and parameters
    against its own fp32 oracle run at test_gpu_focops_shapes.py's bars (not only against its solo run, which shares the HIP
    kernels' arithmetic)"""
    import torch
    from fsrl_amd.engine import EngineGroup
    from test_gpu_focops_shapes import _engine as engine_on, _oracle, _plan, _rollout, _theta0, check_update
    torch.set_num_threads(4)
    foc = dict(actor_lr=5e-4, critic_lr=1e-3, l2_reg=1e-3, delta=0.02, eta=0.02, tem_lambda=0.95, max_grad_norm=0.5)
    k = len(member_rows)
    engs, refs, nus, perms = [], [], [], []
    for i, rows in enumerate(member_rows):
        seed = 300 + 17 * i + Do
        cols, data = _rollout(seed, rows, Do, Da, 45)
        o = _oracle(Do, Da, h, **foc)
        theta0 = _theta0(o, seed + 1)
        o.set_params(theta0, nu=0.1 + 0.2 * i)
        rng = np.random.default_rng(seed + 2)
        perms.append([rng.permutation(len(data)) for _ in range(R)])
        pb, orows, ostopped = o.update(data, 20.0 + 5 * i, B, R, perms[i])
        want = np.array([[sn["loss/nu_loss"], sn["loss/nu_value"], sa["loss/actor_loss"], sa["loss/kl"], sa["loss/entropy"],
                          sc["loss/vf0"], sc["loss/vf1"], sc["loss/vf_total"]] for sn, sa, sc in orows])
        refs.append((pb, want, ostopped, o))
        nus.append((want[0, 1], want[0, 0]))
        e = engine_on(Do, Da, h, rows, cols, **foc)
        e.set_params(theta0)
        engs.append(e)
    sizes = [sum(r) for r in member_rows]
    assert len(set(sizes)) == k
    exact = _exact([_chunks(n, B) for n in sizes], k)
    if B <= 256:
        assert not all(exact), exact                        # the group changes some member's tile height
    else:
        assert not any(_plan(h, n, B, 0)[0] for n in sizes)   # four-launch members
    grp = EngineGroup(engs)
    st, sp = grp.focops_update([x[0] for x in nus], [x[1] for x in nus], B, R, perms=perms)
    for i in range(k):
        pb, want, ostopped, o = refs[i]
        check_update(st[i], sp[i], engs[i], None, want, ostopped, o)
    grp.close()
    for e in engs:
        e.close()


def test_refusals_name_their_reason():
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig, EngineGroup
    cfg, g = _case("small")
    a, b = _engine(cfg, g, 0), _engine(cfg, g, 1)

    def refused(engs, *words):
        with pytest.raises(Exception) as ei:
            EngineGroup(engs)
        msg = str(ei.value)
        assert all(w in msg for w in words), msg

    ppo = Engine(EngineConfig(obs_dim=cfg["obs_dim"], act_dim=cfg["act_dim"], hidden=64, env_num=cfg["env_num"], target_kl=None))
    refused([a, ppo], "one algorithm")
    bare = _engine(cfg, g, 3, init=False)
    refused([a, bare], "fsrl_focops_init")
    for key, val in (("l2_reg", 1e-2), ("delta", 0.5), ("eta", 0.5), ("tem_lambda", 0.5), ("max_grad_norm", 1.0)):
        c = _engine(cfg, g, 2, **{key: val})
        refused([a, c], "l2_reg, delta, eta, tem_lambda and max_grad_norm")
        c.close()
    c = _engine(cfg, g, 2, actor_lr=1e-2, critic_lr=1e-2)          # learning rates may differ
    EngineGroup([a, c]).close()
    c.focops_set_plan(1)
    refused([a, c], "fsrl_focops_set_plan")
    lay = Engine(EngineConfig(algo=_lib.ALGO_FOCOPS, obs_dim=cfg["obs_dim"], act_dim=cfg["act_dim"], hidden_sizes=(64, 64, 64),
                              n_critics=2, env_num=cfg["env_num"], target_kl=None))
    lay.focops_init()
    refused([a, lay], "layered")
    # checked again at update time: fsrl_focops_init may be called again in between
    grp = EngineGroup([a, b])
    b.focops_init(actor_lr=cfg["actor_lr"], critic_lr=cfg["critic_lr"], l2_reg=cfg["l2_reg"] * 2, delta=cfg["delta"],
                  eta=cfg["eta"], tem_lambda=cfg["tem_lambda"], max_grad_norm=cfg["max_grad_norm"])
    with pytest.raises(Exception) as ei:
        grp.focops_update([0.1, 0.1], [0.0, 0.0], cfg["batch_size"], 1, seed=1)
    assert "l2_reg" in str(ei.value)
    grp.close()
    for e in (a, b, c, ppo, bare, lay):
        e.close()


def _agents(tmp_path, tag, envs, ep_len):
    from fsrl_amd.agent import FOCOPSAgent
    from fsrl_amd.data import FastCollector, HipVectorReplayBuffer
    from fsrl_amd.env import SyntheticSafetyVectorEnv
    from fsrl_amd.utils import BaseLogger
    agents, cols = [], []
    for s, (e, L) in enumerate(zip(envs, ep_len)):
        env = SyntheticSafetyVectorEnv(env_num=e, obs_dim=8, act_dim=2, episode_len=L, seed=s)
        ag = FOCOPSAgent(env, BaseLogger(str(tmp_path / f"{tag}{s}"), name=f"{tag}{s}"), cost_limit=10.0, device="cuda:0", seed=s,
                         hidden_sizes=(128, 128), training_num=e)
        ag.policy.train()
        buf = HipVectorReplayBuffer(ag.policy.engine, None, e)
        agents.append(ag); cols.append(FastCollector(ag.policy, env, buf, device_actor=True))
    return agents, cols


def test_group_collector_is_each_focops_members_fast_collector(tmp_path):
    """GroupCollector over FOCOPS members == each member's own FastCollector on an identically seeded twin (k = 3, ragged env
    counts, stochastic actions): the same stats, stored rows and observations, collect after collect"""
    from fsrl_amd.data import GroupCollector
    from fsrl_amd.policy import PolicyGroup
    envs, ep_len = (5, 12, 3), (30, 17, 41)
    solo_agents, solo_cols = _agents(tmp_path, "solo", envs, ep_len)
    grp_agents, grp_cols = _agents(tmp_path, "grp", envs, ep_len)
    group = PolicyGroup([ag.policy for ag in grp_agents])
    gc = GroupCollector(group, grp_cols)
    for rnd, n_ep in enumerate((7, 4)):
        got = gc.collect(n_episode=n_ep)
        want = [c.collect(n_episode=n_ep) for c in solo_cols]
        assert got == want, rnd
        for x, y in zip(solo_cols, grp_cols):
            assert (x.collect_step, x.collect_episode) == (y.collect_step, y.collect_episode)
            assert np.array_equal(x.buffer._sizes, y.buffer._sizes)
            assert np.array_equal(x._obs, y._obs)
        for x, y in zip(solo_cols, grp_cols):
            a, b = x.policy.engine, y.policy.engine
            ia, ib = a.sample0(), b.sample0()
            assert np.array_equal(ia, ib)
            ra, rb = a.store_read(ia), b.store_read(ib)
            for key in ra:
                assert np.array_equal(ra[key], rb[key]), key
    assert group.group.actor_resident_stats()["requests"] > 0
    group.close()
    for ag in solo_agents + grp_agents:
        ag.policy.engine.close()


def test_policy_group_of_focops_agents_trains_in_lock_step(tmp_path):
    """PolicyGroup over FOCOPSAgent policies: each member's nu step is FOCOPS.process_fn's, and its logger gets the keys
    and row count of its solo FOCOPS.update"""
    from fsrl_amd.policy import FOCOPS, PolicyGroup
    from fsrl_amd.policy.focops import FOCOPS_KEYS
    envs, ep_len = (4, 4, 6), (25, 25, 25)
    solo_agents, solo_cols = _agents(tmp_path, "s", envs, ep_len)
    grp_agents, grp_cols = _agents(tmp_path, "g", envs, ep_len)

    class Cap:
        def __init__(self): self.rows, self.printed = [], []
        def store(self, tab=None, **kw): self.rows.append(dict(kw))
        def print(self, *a, **k): self.printed.append(a)
    for ag in solo_agents + grp_agents:
        ag.policy.logger = Cap()
        ag.policy.pre_update_fn({"cost": 3.0})
    group = PolicyGroup([ag.policy for ag in grp_agents])
    for _ in range(2):
        for c in solo_cols + grp_cols:
            c.collect(n_episode=8)
        res_s = [ag.policy.update(0, c.buffer, batch_size=64, repeat=2) for ag, c in zip(solo_agents, solo_cols)]
        res_g = group.update([c.buffer for c in grp_cols], batch_size=64, repeat=2)
        for a, b, rs, rg in zip(solo_agents, grp_agents, res_s, res_g):
            assert rs["gradient_steps"] == rg["gradient_steps"] and a.policy.gradient_steps == b.policy.gradient_steps
            assert float(a.policy._nu) == float(b.policy._nu)
            ka = [tuple(sorted(r)) for r in a.policy.logger.rows]
            kb = [tuple(sorted(r)) for r in b.policy.logger.rows]
            assert ka == kb
            assert set(FOCOPS_KEYS) <= {k for r in b.policy.logger.rows for k in r}
            assert not b.policy.updating and np.isfinite(b.policy.engine.get_params()).all()
    assert all(isinstance(ag.policy, FOCOPS) for ag in grp_agents)
    group.close()
    for ag in solo_agents + grp_agents:
        ag.policy.engine.close()
