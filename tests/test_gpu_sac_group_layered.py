"""Groups of LAYERED SAC-Lagrangian / DDPG-Lagrangian contexts (any `hidden_sizes`): fsrl_sac_group_update and fsrl_collect_group_*
with layered members, EngineSacGroup / EngineCollectGroup / SACPolicyGroup / DDPGPolicyGroup / GroupCollector over them.

A layered grouped update runs the launch sequence of the member's own layered fsrl_sac_update with every launch carrying all
members.  lin_body gives every output element as one accumulator over ascending k whatever the launch shape, and the replay agents
pass no squared-norm partials, so -- unlike the fused groups, whose tile height changes with k -- every member is BIT-IDENTICAL to
its solo twin at every k and batch size: the three parameter vectors (and DDPG's target actor), alpha and every statistics row are
compared with np.array_equal.  No tolerance anywhere in this file.

Twin pattern of tests/test_gpu_sac_group.py: the same parameters, pushes and Philox key (one own update on both twins first), then
grouped against solo.  Members differ in parameters, data, store length (T = 120 + 37 i), lambda, learning rates and n_updates."""
import numpy as np
import pytest

from test_gpu_group_collect import _close, _random_step, _same_stores, _step_b
from test_gpu_collect_group import _same_step, _solo_steps

pytestmark = pytest.mark.gpu

N8 = [5, 3, 0, 5, 2, 4, 1, 5]


def _engine(hs, Do, Da, kind="sacl", n_step=2, auto_alpha=True, use_lag=True, seed=0, T=150, env_num=4, lr=(5e-4, 1e-3), tau=0.05,
            force=False, key=None):
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig
    eng = Engine(EngineConfig(algo=_lib.ALGO_SAC_LAG, obs_dim=Do, act_dim=Da, hidden_sizes=tuple(hs), n_critics=2, env_num=env_num,
                              buffer_size=env_num * 400, gamma=0.99, target_kl=None, force_layered=force))
    if kind == "cvpo":
        eng.cvpo_init(0.1)
        return eng
    eng.sac_init(actor_lr=lr[0], critic_lr=lr[1], tau=tau, n_step=n_step, auto_alpha=auto_alpha, use_lagrangian=use_lag,
                 deterministic=(kind == "ddpgl"))
    rng = np.random.default_rng(100 + seed)
    eng.sac_set_params(0.1 * rng.standard_normal(eng.n_sac_actor).astype(np.float32),
                       0.1 * rng.standard_normal(eng.n_sac_critics).astype(np.float32), float(np.log(0.2)))
    ids = np.arange(env_num)
    for t in range(T):
        obs = rng.standard_normal((env_num, Do)).astype(np.float32)
        act = np.tanh(rng.standard_normal((env_num, Da))).astype(np.float32)
        term = rng.random(env_num) < 0.03
        trunc = np.full(env_num, (t + 1) % 50 == 0) & ~term
        eng.push(ids, obs, act, rng.normal(0.5, 0.5, env_num), (rng.random(env_num) < 0.2).astype(np.float64), term, trunc,
                 rng.standard_normal((env_num, Do)).astype(np.float32))
    if key is not None:
        eng.actor_sample(np.zeros((1, Do), np.float32), seed=key)      # keys the collector's noise stream
    return eng


def _state(eng, kind="sacl"):
    a, alpha = eng.sac_get_params(0)
    out = [a, eng.sac_get_params(1)[0], eng.sac_get_params(2)[0]]
    if kind == "ddpgl":
        out.append(eng.sac_get_params(3)[0])
    return out, alpha, eng.sac_drain()


def _same(x, y, tag=None):
    for j, (u, v) in enumerate(zip(x[0], y[0])):
        assert np.array_equal(u, v), (tag, j, np.abs(u - v).max())
    assert x[1] == y[1], tag
    assert x[2].shape == y[2].shape, tag
    assert np.array_equal(x[2], y[2]), tag


def _run(hs, Do, Da, B, k, n, kind="sacl", use_lag=True, auto_alpha=True, n_step=2, force=False):
    from fsrl_amd.engine import EngineSacGroup
    lam = [0.1 * (i + 1) for i in range(k)]
    mk = lambda i: _engine(hs, Do, Da, kind, n_step, auto_alpha, use_lag, seed=i, T=120 + 37 * i, lr=(5e-4 * (1 + 0.1 * i), 1e-3),
                           force=force)
    grouped, solo = [mk(i) for i in range(k)], [mk(i) for i in range(k)]
    resc = [1.0 / (1.0 + l) for l in lam]
    for i in range(k):                             # key each member's Philox stream (one own update on both twins)
        for e in (grouped[i], solo[i]):
            e.sac_update(B, [lam[i]] if use_lag else [], resc[i], seed=11 + i, sync=False)
    g = EngineSacGroup(grouped)
    g.update(B, n, [[l] for l in lam] if use_lag else None, resc)
    for i in range(k):
        for _ in range(n[i]):
            solo[i].sac_update(B, [lam[i]] if use_lag else [], resc[i], sync=False)
    out = [(_state(grouped[i], kind), _state(solo[i], kind)) for i in range(k)]
    g.close()
    _close(grouped, solo)
    return out


CASES = {
    # a member sitting out, unequal counts
    "sacl-deep3": dict(hs=(64, 48, 32), Do=8, Da=2, B=64, k=3, n=[5, 3, 0]),
    # widths and obs that fail the float4 check (scalar path); a 16-row tile plus a 4-row tail; 96 weight-side jobs
    "sacl-ragged-k8": dict(hs=(50, 30), Do=33, Da=8, B=20, k=8, n=N8, n_step=3, auto_alpha=False),
    # one layer wider than the fused kernels; 17 tiles, a ragged 64-row tile
    "sacl-wide1": dict(hs=(320, ), Do=8, Da=2, B=272, k=2, n=[4, 4], use_lag=False),
    # a two-layer network through the layered kernels
    "sacl-forced": dict(hs=(64, 64), Do=8, Da=2, B=64, k=2, n=[3, 3], force=True),
    # eight hidden layers: the solo twin's 36 weight-side jobs of the four Q-networks exceed the 32-entry job table of a launch and go
    # out as two launches of whole networks (lay_wgrad_k); the group's table is in device memory, one launch
    "sacl-eight-k2": dict(hs=(24, 17, 32, 9, 40, 4, 28, 12), Do=20, Da=8, B=64, k=2, n=[3, 2]),
    # 16-wide deterministic head, the target actor's Polyak update
    "ddpgl-deep3": dict(hs=(64, 48, 32), Do=20, Da=16, B=64, k=3, n=[4, 0, 2], kind="ddpgl", n_step=1),
    "ddpgl-ragged-k8": dict(hs=(50, 30), Do=8, Da=2, B=20, k=8, n=N8, kind="ddpgl", use_lag=False),
}


@pytest.mark.parametrize("name", list(CASES))
def test_members_are_bit_identical_to_their_solo_twins(name):
    case = dict(CASES[name])
    n = case["n"]
    res = _run(**case)
    for i, (x, y) in enumerate(res):
        assert len(x[2]) == n[i] + 1
        _same(x, y, (name, i))


@pytest.mark.parametrize("kind", ["sacl", "ddpgl"])
def test_group_of_one(kind):
    (x, y), = _run((64, 48, 32), 8, 2, 256, 1, [20], kind=kind)
    assert len(x[2]) == 21
    _same(x, y, kind)


def test_interleaved_own_updates_pushes_uploads_and_a_larger_batch():
    """Between grouped calls: a member's own sac_update, pushes that wrap a member's store, sac_put_params on one member; the last
    grouped call has a larger batch, so the members' working sets regrow and the group's tables are rebuilt."""
    from fsrl_amd.engine import EngineSacGroup
    hs, Do, Da = (64, 48, 32), 8, 2
    a = [_engine(hs, Do, Da, seed=i, T=120 + 37 * i) for i in range(3)]
    b = [_engine(hs, Do, Da, seed=i, T=120 + 37 * i) for i in range(3)]
    lam, resc = [0.2, 0.5, 0.3], [1 / 1.2, 1 / 1.5, 1 / 1.3]
    for i in range(3):
        for e in (a[i], b[i]):
            e.sac_update(64, [lam[i]], resc[i], seed=11 + i, sync=False)
    g = EngineSacGroup(a)
    rng = np.random.default_rng(5)
    ids = np.arange(4)
    th = (0.1 * rng.standard_normal(a[2].n_sac_actor)).astype(np.float32)
    for r, (B, n) in enumerate(((64, [3, 2, 1]), (64, [1, 0, 2]), (200, [2, 3, 2]))):
        g.update(B, n, [[x] for x in lam], resc)
        for i in range(3):
            for _ in range(n[i]):
                b[i].sac_update(B, [lam[i]], resc[i], sync=False)
        for e in (a[0], b[0]):                     # an own update between grouped ones
            e.sac_update(B, [lam[0]], resc[0], sync=False)
        for t in range(450 if r == 0 else 3):      # member 1's store (400 per environment) wraps in the first round
            rows = [rng.standard_normal((4, Do)).astype(np.float32) for _ in range(2)]
            for e in (a[1], b[1]):
                e.push(ids, rows[0], np.zeros((4, Da), np.float32), np.ones(4), np.zeros(4), np.zeros(4, bool),
                       np.full(4, t % 40 == 39), rows[1])
        if r == 1:
            for e in (a[2], b[2]):
                e.sac_put_params(0, th)
    g.close()
    for i in range(3):
        _same(_state(a[i]), _state(b[i]), i)
    _close(a, b)


def test_rejections_and_a_member_closed_before_its_group():
    from fsrl_amd.engine import EngineSacGroup
    Do, Da, B = 8, 2, 64
    lay = lambda hs=(64, 48, 32), **kw: _engine(hs, Do, Da, T=130, **kw)
    a, a2, twin = lay(seed=0), lay(seed=1), lay(seed=1)
    fused = lay((64, 64))
    others = [lay((64, 48, 16)), lay((64, 48, 32, 32)), lay(kind="ddpgl"), lay(kind="cvpo"), lay((64, 64), force=True)]
    cases = [([fused, a], "layered"), ([a, fused], "layered"), ([a, others[0]], "one network shape"), ([a, others[1]], "one network shape"),
             ([a, others[2]], "DDPG-Lagrangian"), ([a, others[3]], "CVPO"), ([others[3]], "CVPO"), ([fused, others[4]], "layered"),
             ([a, a], "listed twice")]
    for bad, reason in cases:
        with pytest.raises(AssertionError, match=reason):      # FSRL_EINVAL, with the reason in the message
            EngineSacGroup(bad)
    g = EngineSacGroup([a, a2])
    with pytest.raises(AssertionError, match="already in a SAC group"):
        EngineSacGroup([a2])
    for e in (a2, twin):
        e.sac_update(B, [0.1], 1.0, seed=5, sync=False)
    g.update(B, [1, 2], [[0.1], [0.1]], [1.0, 1.0])
    for _ in range(2):
        twin.sac_update(B, [0.1], 1.0, sync=False)
    a.close()                                      # a member destroyed before its group
    with pytest.raises(RuntimeError, match="destroyed"):
        g.update(B, [1, 1], [[0.1], [0.1]], [1.0, 1.0])
    for e in (a2, twin):                           # the survivor is an ordinary context
        e.sac_update(B, [0.1], 1.0, sync=False)
    _same(_state(a2), _state(twin))
    g.close()
    _close([a2, twin, fused], others)


# ---------------------------------------------------------------- lock-step collection
def _pair(kind, envs, hs, Do, Da, T=0):
    from fsrl_amd.engine import EngineCollectGroup
    mk = lambda i, e: _engine(hs, Do, Da, kind, seed=i, T=T, env_num=e, lr=(5e-4 * (1 + 0.1 * i), 1e-3), key=1000 + i)
    a = [mk(i, e) for i, e in enumerate(envs)]
    b = [mk(i, e) for i, e in enumerate(envs)]
    return a, b, EngineCollectGroup(b)


@pytest.mark.parametrize("kind,envs,hs,Do,Da", [
    ("sacl", (3, 20, 1), (64, 48, 32), 8, 2),
    ("ddpgl", (3, 20, 1), (128, 64, 32), 20, 16),          # 16 raw columns from the mean head: rows 8 - 15 of a tile exist
])
def test_collect_group_step_is_every_members_collect_step_bit_for_bit(kind, envs, hs, Do, Da):
    """A scripted run with random row counts per member (steps in which a member has no rows among them), deterministic /
    bound_method / bounds varied per step: actions, env actions, ptr / ep_* outputs and the stores identical to the members' own
    collect_step; one request per grouped call with rows, no resident kernel."""
    a, b, cg = _pair(kind, envs, hs, Do, Da)
    cg.actor_set_resident(True, idle_timeout_us=100.0)         # accepted, no effect
    rng = np.random.default_rng(7)
    low = -1.0 - rng.random((len(envs), Da)).astype(np.float32)
    high = 1.0 + rng.random((len(envs), Da)).astype(np.float32)
    script = []
    for step in range(30):
        prevs, oas = _random_step(rng, envs, Do, Da, k_act_zero=0.25)
        if step == 4:
            oas[1] = None                                      # one step in which a member has no rows
            oas[0] = rng.standard_normal((3, Do)).astype(np.float32)
        lo, hi = (low, high) if step % 2 else (None, None)
        script.append((prevs, oas, step % 7 == 3, (1, 2, 0)[step % 3], lo, hi))
    want = _solo_steps(a, script)
    n_req = 0
    for step, (prevs, oas, det, bound, lo, hi) in enumerate(script):
        _same_step(want[step], _step_b(cg, prevs, oas, det, bound, lo, hi), step)
        n_req += any(o is not None for o in oas)
    st = cg.actor_resident_stats()
    assert st["requests"] == n_req and not st["live"], st
    cg.actor_release()
    _same_stores(a, b)
    _close(cg, a, b)


@pytest.mark.parametrize("kind", ["sacl", "ddpgl"])
def test_collect_group_across_updates_uploads_and_own_calls(kind):
    """collect -> update -> collect, three cycles: the members of set B are in an EngineSacGroup too and update grouped (set A: each
    member's own updates -- the layered grouped update is bit-identical), one member runs an own update in the middle of a collect,
    another has its actor overwritten (sac_put_params), and a member's own collect_step comes between grouped steps.  Each of these
    re-orders the group's stream behind the members'; actions, stores and parameters stay those of the member-by-member run."""
    from fsrl_amd.engine import EngineSacGroup
    envs, hs, Do, Da, B = (3, 20, 1), (64, 48, 32), 8, 2, 64
    a, b, cg = _pair(kind, envs, hs, Do, Da, T=60)
    lam, resc = [0.3, 0.5, 0.7], [1.0, 0.8, 0.9]
    for i in range(3):
        for e in (a[i], b[i]):
            e.sac_update(B, [lam[i]], resc[i], seed=11 + i, sync=False)
    rng = np.random.default_rng(5)
    n_upd = [3, 1, 2]
    th = (0.2 * rng.standard_normal(a[1].n_sac_actor)).astype(np.float32)
    scripts = [[_random_step(rng, envs, Do, Da, k_act_zero=0.0) + (False, 1, None, None) for _ in range(9)] for _ in range(3)]

    def run(engs, step_fn, ug):
        out = []
        for cycle in range(3):
            res = step_fn(scripts[cycle][:4])
            if cycle == 1:
                engs[1].sac_put_params(0, th)
            if cycle == 2:
                engs[0].sac_update(B, [lam[0]], resc[0], sync=False)
            res += step_fn(scripts[cycle][4:8])
            prevs, oas = scripts[cycle][8][:2]                 # a member's own collect_step between grouped steps
            own = [np.array(x, copy=True) for x in engs[1].collect_step(prevs[1], oas[1], False, 1)]
            engs[1].actor_release()
            if ug is not None:
                ug.update(B, n_upd, [[l] for l in lam], resc)
            else:
                for i, e in enumerate(engs):
                    for _ in range(n_upd[i]):
                        e.sac_update(B, [lam[i]], resc[i], sync=False)
            out.append((res, own, [_state(e, kind) for e in engs]))
        return out

    want = run(a, lambda sc: _solo_steps(a, sc), None)
    ug = EngineSacGroup(b)
    got = run(b, lambda sc: [_step_b(cg, *st) for st in sc], ug)
    for cycle, ((ra, oa, sa), (rb, ob, sb)) in enumerate(zip(want, got)):
        for step, (x, y) in enumerate(zip(ra, rb)):
            _same_step(x, y, (cycle, step))
        for u, v in zip(oa, ob):
            assert np.array_equal(u, v), cycle
        for i in range(3):
            _same(sa[i], sb[i], (cycle, i))
    _same_stores(a, b)
    ug.close()
    _close(cg, a, b)


def test_collect_group_rejections_and_teardown_orders():
    from fsrl_amd.engine import EngineCollectGroup
    envs, hs, Do, Da = (3, 20, 1), (64, 48, 32), 8, 2
    a, b, cg = _pair("sacl", envs, hs, Do, Da)
    free = _engine(hs, Do, Da, seed=9, T=0, key=5)
    bad = [_engine((64, 64), Do, Da, T=0), _engine((64, 48, 16), Do, Da, T=0), _engine(hs, Do, Da, "ddpgl", T=0),
           _engine(hs, Do, Da, "cvpo", T=0)]
    for other, reason in zip(bad, ["layered", "one network shape", "one kind", "CVPO"]):
        with pytest.raises(Exception, match=reason):
            EngineCollectGroup([free, other])
    with pytest.raises(Exception, match="layered"):
        EngineCollectGroup([bad[0], free])
    with pytest.raises(Exception, match="already in a collect group"):
        EngineCollectGroup([free, b[0]])
    rng = np.random.default_rng(1)
    oas = [rng.standard_normal((e, Do)).astype(np.float32) for e in envs]
    want = [eng.collect_step(None, o, False, 1)[0].copy() for eng, o in zip(a, oas)]
    got = cg.collect_step([None] * 3, oas, False, 1)
    for m in range(3):
        assert np.array_equal(want[m], got[m][0]), m
    b[0].close()                                   # a member closed before its group
    with pytest.raises(Exception, match="destroyed"):
        cg.collect_step([None] * 3, oas, False, 1)
    for eng, o in zip(b[1:], oas[1:]):
        assert np.isfinite(eng.collect_step(None, o, True, 1)[0]).all()
    cg.close()
    cg2 = EngineCollectGroup(b[1:])                # the survivors group again; this group is closed BEFORE its members
    cg2.collect_step([None] * 2, oas[1:], False, 1)
    cg2.close()
    for eng, o in zip(b[1:], oas[1:]):
        assert np.isfinite(eng.collect_step(None, o, True, 1)[0]).all()
    _close(a, b[1:], [free], bad)


# ---------------------------------------------------------------- policy level
@pytest.mark.parametrize("algo", ["sacl", "ddpgl"])
def test_policy_group_and_group_collector_match_each_seeds_sequential_run(algo, tmp_path):
    """Three layered seeds (hidden_sizes (64, 64, 32), 4 envs) through SACPolicyGroup / DDPGPolicyGroup + GroupCollector over an
    EngineCollectGroup against each seed's sequential run (FastCollector.collect, policy.update): the collected statistics, the
    stores, the parameters and the logged update rows are equal."""
    import torch
    from fsrl_amd.agent import DDPGLagAgent, SACLagAgent
    from fsrl_amd.data import FastCollector, GroupCollector, HipVectorReplayBuffer
    from fsrl_amd.engine import EngineCollectGroup
    from fsrl_amd.env import SyntheticSafetyVectorEnv
    from fsrl_amd.policy import DDPGPolicyGroup, SACPolicyGroup
    Agent, Group = {"sacl": (SACLagAgent, SACPolicyGroup), "ddpgl": (DDPGLagAgent, DDPGPolicyGroup)}[algo]

    class _Log:
        def __init__(self):
            self.rows = []

        def store(self, tab=None, **kw):
            self.rows.append(sorted(kw.items()))

        def store_rows(self, keys, rows):
            self.rows.append((list(keys), np.asarray(rows).tolist()))

        def print(self, *a):
            pass

    def build(grouped):
        agents, bufs, cols, logs = [], [], [], []
        for s in range(3):
            env = SyntheticSafetyVectorEnv(env_num=4, episode_len=30 + 3 * s, seed=10 + s)
            ag = Agent(env, None, cost_limit=10, device="cuda:0", seed=1 + s, hidden_sizes=(64, 64, 32), training_num=4, buffer_size=2000)
            ag.policy.logger = _Log()
            ag.policy.train()
            buf = HipVectorReplayBuffer(ag.policy.engine, 2000, 4)
            agents.append(ag); bufs.append(buf); logs.append(ag.policy.logger)
            cols.append(FastCollector(ag.policy, env, buf, exploration_noise=True, device_actor=True))
        grp = cg = gc = None
        if grouped:
            grp = Group([a.policy for a in agents])
            cg = EngineCollectGroup([a.policy.engine for a in agents])
            gc = GroupCollector(cg, cols)
        stats = []
        for cyc in range(2):
            for ag in agents:
                ag.policy.engine.actor_sample(np.zeros((1, ag.policy.engine.cfg.obs_dim), np.float32), seed=40 + cyc)
            sts = gc.collect(n_episode=4) if grouped else [c.collect(n_episode=4) for c in cols]
            stats.append(sts)
            n = []
            for ag, st in zip(agents, sts):
                ag.policy.pre_update_fn(stats_train={"cost": 15.0 + cyc})
                n.append(round(0.1 * st["n/st"]))
            if grouped:
                grp.update(bufs, 64, n)
            else:
                for ag, buf, ni in zip(agents, bufs, n):
                    for _ in range(ni):
                        ag.policy.update(64, buf)
            for ag in agents:
                ag.policy.post_update_fn(stats_train={"cost": 15.0 + cyc})
        out = [({k: v.detach().cpu().numpy().copy() for k, v in ag.policy.state_dict().items() if torch.is_tensor(v)}, lg.rows)
               for ag, lg in zip(agents, logs)]
        if grouped:
            assert cg.actor_resident_stats()["requests"] > 0
            grp.close(); cg.close()
        return out, stats, agents

    (got, gst, gag), (want, wst, wag) = build(True), build(False)
    assert gst == wst
    _same_stores([a.policy.engine for a in wag], [a.policy.engine for a in gag])
    for (sg, lg), (sw, lw) in zip(got, want):
        assert sg.keys() == sw.keys()
        for key in sg:
            assert np.array_equal(sg[key], sw[key]), key
        assert lg == lw
    for ag in gag + wag:
        ag.policy.engine.close()
