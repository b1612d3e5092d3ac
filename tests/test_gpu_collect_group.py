"""Lock-step collection of replay-agent seeds (fsrl_collect_group_*, actor_group_resident_kernel<H, true>, EngineCollectGroup,
GroupCollector over it): one library call and one resident-actor request per vector step for k SAC-Lag, DDPG-Lag or CVPO members.
Per member everything must be what the member's own fsrl_collect_step gives, bit for bit: actions, env actions, ptr / ep_* outputs,
stored rows, the member's noise stream -- across updates, uploads, a member's own calls, idle timeouts and teardown.

Pattern throughout: two sets of identically built and identically keyed engines, A driven member by member through
Engine.collect_step, B through the collect group; everything compared with np.array_equal."""
import time

import numpy as np
import pytest

from test_gpu_group_collect import _close, _random_step, _same_stores, _step_b

pytestmark = pytest.mark.gpu

RAGGED8 = (64, 1, 16, 17, 20, 20, 48, 5)


def _member(kind, H, Do, Da, env_num, seed, T=0):
    """a replay context of its own parameters, noise stream and (T > 0) stored transitions; kind: sacl / ddpgl / cvpo"""
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig
    eng = Engine(EngineConfig(algo=_lib.ALGO_SAC_LAG, obs_dim=Do, act_dim=Da, hidden_sizes=(H, H), n_critics=2, env_num=env_num,
                              buffer_size=env_num * 200, gamma=0.99, target_kl=None))
    if kind == "sacl":
        eng.sac_init(actor_lr=5e-4 * (1 + 0.1 * seed))
    elif kind == "ddpgl":
        eng.sac_init(deterministic=True, exploration_sigma=0.1 + 0.01 * seed)
    else:
        eng.cvpo_init(0.1 + 0.02 * seed)
    rng = np.random.default_rng(100 + seed)
    eng.sac_set_params(0.2 * rng.standard_normal(eng.n_sac_actor).astype(np.float32),
                       0.1 * rng.standard_normal(eng.n_sac_critics).astype(np.float32), float(np.log(0.2)))
    if kind == "cvpo":
        eng.cvpo_post_update()                     # actor_old <- actor
        eng.cvpo_pre_update()
    ids = np.arange(env_num)
    for t in range(T):
        term = rng.random(env_num) < 0.03
        eng.push(ids, rng.standard_normal((env_num, Do)).astype(np.float32), np.tanh(rng.standard_normal((env_num, Da))).astype(np.float32),
                 rng.normal(0.5, 0.5, env_num), (rng.random(env_num) < 0.2).astype(np.float64), term,
                 np.full(env_num, (t + 1) % 50 == 0) & ~term, rng.standard_normal((env_num, Do)).astype(np.float32))
    eng.actor_sample(np.zeros((1, Do), np.float32), seed=1000 + seed)          # keys member i's noise stream
    return eng


def _pair(kind, envs, H=128, Do=8, Da=2, T=0, idle_us=2.0e5):
    """engine sets A (member by member) and B (through the collect group `cg`)"""
    from fsrl_amd.engine import EngineCollectGroup
    a = [_member(kind, H, Do, Da, e, i, T) for i, e in enumerate(envs)]
    b = [_member(kind, H, Do, Da, e, i, T) for i, e in enumerate(envs)]
    cg = EngineCollectGroup(b)
    cg.actor_set_resident(True, idle_timeout_us=idle_us)
    return a, b, cg


def _solo_steps(a, script, release=True):
    """set A: every step of `script` member by member through Engine.collect_step.  A resident actor occupies a hardware queue of the
    process for as long as it lives, and a launch that lands on that queue waits for its idle timeout; with 1 + k of them live at
    once (the group's and every twin's) the streams of the two sets would queue behind each other's kernels.  So the twins run
    their whole script BEFORE the group runs it, and each ends its own resident actor after its call, as FastCollector does at the
    end of a collect (the next call launches it again: still the solo resident kernel's answer)."""
    out = []
    for prevs, oas, det, bound, lo, hi in script:
        res = []
        for i, eng in enumerate(a):
            act, ea, er, el = eng.collect_step(prevs[i], oas[i], det, bound, None if lo is None else lo[i], None if hi is None else hi[i])
            k = 0 if prevs[i] is None else len(prevs[i][0])
            st = eng._collect_stage["a"]
            res.append((act, ea, er.copy(), el.copy(), st["ptr"][:k].copy(), st["ei"][:k].copy()))
            if release:
                eng.actor_release()
        out.append(res)
    return out


def _same_step(ra, rb, tag):
    for i, (x, y) in enumerate(zip(ra, rb)):
        for j, (u, v) in enumerate(zip(x, y)):
            assert np.array_equal(u, v), (tag, i, j)


@pytest.mark.parametrize("kind,envs,H,Do,Da,a_resident", [
    ("sacl", (20, ), 256, 8, 2, True),
    ("sacl", (20, 7, 33), 128, 27, 8, True),                  # raw_cols 16
    ("cvpo", RAGGED8, 64, 8, 2, False),                       # set A on the launched path: not the solo resident kernel's answer alone
    ("ddpgl", RAGGED8, 256, 8, 16, True),                     # raw_cols 16 from the mean head alone: four storing waves per full tile
])
def test_collect_group_step_is_every_members_collect_step_bit_for_bit(kind, envs, H, Do, Da, a_resident):
    """About 60 vector steps with random row counts per member (0, partial tiles, full tiles up to 64), deterministic / bound_method /
    bounds varied per step: actions, env actions, ptr / ep_* outputs and the stores identical; every grouped call with rows to act
    on is one request of the group's kernel, which is launched a few times at most."""
    a, b, cg = _pair(kind, envs, H, Do, Da)
    if not a_resident:
        for e in a:
            e.actor_set_resident(False)
    rng = np.random.default_rng(7)
    low = -1.0 - rng.random((len(envs), Da)).astype(np.float32)
    high = 1.0 + rng.random((len(envs), Da)).astype(np.float32)
    script = []
    for step in range(60):
        prevs, oas = _random_step(rng, envs, Do, Da)
        lo, hi = (low, high) if step % 2 else (None, None)
        script.append((prevs, oas, step % 7 == 3, (1, 2, 0)[step % 3], lo, hi))
    want = _solo_steps(a, script)
    n_req = 0
    for step, (prevs, oas, det, bound, lo, hi) in enumerate(script):
        _same_step(want[step], _step_b(cg, prevs, oas, det, bound, lo, hi), step)
        n_req += any(o is not None for o in oas)
    # one request per call with rows; few launches (an idle timeout while first-launch code loading holds the host up is legitimate)
    st = cg.actor_resident_stats()
    assert st["requests"] == n_req and st["live"] and 1 <= st["launches"] <= 6, st
    cg.actor_release()
    assert not cg.actor_resident_stats()["live"]
    _same_stores(a, b)
    _close(cg, a, b)


def _params(eng, kind):
    return [eng.sac_get_params(w)[0] for w in ((0, 1, 2, 3) if kind != "sacl" else (0, 1, 2))]


@pytest.mark.parametrize("kind", ["sacl", "cvpo", "ddpgl"])
def test_collect_group_across_updates_and_uploads(kind):
    """collect -> update -> collect, three cycles.  SAC-Lag members are also in an EngineSacGroup, CVPO members in an EngineCvpoGroup
    (both sets update grouped, so the comparison is about collection), DDPG-Lag members run their own sac_updates; in the middle of a
    collect one member's actor is overwritten (sac_put_params).  Each of these ends the collect group's kernel, and actions, stores
    and parameters stay those of the member-by-member run."""
    from fsrl_amd.engine import EngineCvpoGroup, EngineSacGroup
    envs, H, Do, Da, B = (20, 7, 33), 128, 8, 2, 64
    a, b, cg = _pair(kind, envs, H, Do, Da, T=60)
    lam, resc = [0.3, 0.5, 0.7], [1.0, 0.8, 0.9]
    for i in range(3):                             # key each member's Philox stream: one own update on both twins
        for e in (a[i], b[i]):
            if kind == "cvpo":
                e.cvpo_update(B, seed=11 + i, sync=False)
            else:
                e.sac_update(B, [lam[i]], resc[i], seed=11 + i, sync=False)
    rng = np.random.default_rng(5)
    n_upd = [3, 1, 2]
    th = (0.2 * rng.standard_normal(a[1].n_sac_actor)).astype(np.float32)
    scripts = [[_random_step(rng, envs, Do, Da, k_act_zero=0.0) + (False, 1, None, None) for _ in range(16)] for _ in range(3)]

    def run(engs, step_fn, group=None):
        """three cycles on one set; -> per cycle (step results, parameters, drained rows)"""
        ug = None
        if kind == "sacl":
            ug = EngineSacGroup(engs)
        elif kind == "cvpo":
            ug = EngineCvpoGroup(engs)
        out = []
        for cycle in range(3):
            res = step_fn(scripts[cycle][:8])
            if cycle == 1:
                engs[1].sac_put_params(0, th)
                assert group is None or not group.actor_resident_stats()["live"]
            res += step_fn(scripts[cycle][8:])
            assert group is None or group.actor_resident_stats()["live"]
            if kind == "sacl":
                ug.update(B, n_upd, [[l] for l in lam], resc)
            elif kind == "cvpo":
                ug.update(B, n_upd)
            else:
                for i, e in enumerate(engs):
                    for _ in range(n_upd[i]):
                        e.sac_update(B, [lam[i]], resc[i], sync=False)
            assert group is None or not group.actor_resident_stats()["live"]
            if kind == "cvpo":
                for e in engs:
                    e.cvpo_post_update(); e.cvpo_pre_update()
            out.append((res, [_params(e, kind) for e in engs], [e.sac_drain() for e in engs]))
        if ug is not None:
            ug.close()
        return out

    want = run(a, lambda sc: _solo_steps(a, sc))
    got = run(b, lambda sc: [_step_b(cg, *st) for st in sc], cg)
    for cycle, ((ra, pa, da), (rb, pb, db)) in enumerate(zip(want, got)):
        for step, (x, y) in enumerate(zip(ra, rb)):
            _same_step(x, y, (cycle, step))
        for i in range(3):
            for x, y in zip(pa[i], pb[i]):
                assert np.array_equal(x, y), (cycle, i)
            assert np.array_equal(da[i], db[i]), (cycle, i)
    _same_stores(a, b)
    _close(cg, a, b)


def test_a_members_own_collect_step_between_grouped_steps():
    """A member's own collect_step ends the group's kernel (it may be followed by anything on the member's stream), returns the
    member's solo bits, and the next grouped step relaunches the kernel and matches again."""
    envs, Do, Da = (20, 7, 33), 8, 2
    a, b, cg = _pair("sacl", envs, 128, Do, Da)
    rng = np.random.default_rng(3)
    script = [_random_step(rng, envs, Do, Da, k_act_zero=0.0) + (False, 1, None, None) for _ in range(6)]
    want = []
    for rnd in range(3):
        want += _solo_steps(a, script[2 * rnd:2 * rnd + 1])
        prevs, oas = script[2 * rnd + 1][:2]
        want.append([np.array(x, copy=True) for x in a[1].collect_step(prevs[1], oas[1], False, 1)])     # ep_* are staging views
        a[1].actor_release()
    for rnd in range(3):
        _same_step(want[2 * rnd], _step_b(cg, *script[2 * rnd]), ("grouped", rnd))
        st = cg.actor_resident_stats()
        assert st["live"] and st["launches"] == rnd + 1, st
        prevs, oas = script[2 * rnd + 1][:2]
        xb = b[1].collect_step(prevs[1], oas[1], False, 1)
        for u, v in zip(want[2 * rnd + 1], xb):
            assert np.array_equal(np.asarray(u), np.asarray(v))
        assert not cg.actor_resident_stats()["live"]
        assert b[1].actor_resident_stats()["live"]             # membership leaves the member its own resident actor
    _same_stores(a, b)
    _close(cg, a, b)


def test_collect_group_actor_calls_spaced_around_its_idle_timeout():
    """The end / relaunch protocol of the group kernel under its race (the short form the on-policy group uses): k = 3, idle timeout
    120 us, calls 0.6 .. 1.4 timeouts apart, so that workgroups give up while a doorbell is being rung.  Every answer equals the
    member's own."""
    envs, Do, Da = (20, 64, 7), 8, 2
    a, b, cg = _pair("sacl", envs, 256, Do, Da, idle_us=120.0)
    rng = np.random.default_rng(2)
    n = 1500
    inputs = [[rng.standard_normal((int(rng.integers(1, min(e, 64) + 1)), Do)).astype(np.float32) for e in envs] for _ in range(n)]
    for e in a:
        e.actor_set_resident(False)                            # the launched path: nothing of set A stays on a hardware queue
    want = [[eng.collect_step(None, o, True, 0)[0] for eng, o in zip(a, oas)] for oas in inputs]
    for i, oas in enumerate(inputs):
        gap = rng.uniform(0.6, 1.4) * 120e-6 if i % 3 else 0.0
        t = time.perf_counter()
        while time.perf_counter() - t < gap:
            pass
        rb = cg.collect_step([None] * 3, oas, True, 0)
        for m in range(3):
            assert np.array_equal(want[i][m], rb[m][0]), (i, m)
    st = cg.actor_resident_stats()
    assert st["requests"] == n and 10 < st["launches"] < n, st          # the timeouts did fire, and not before every call
    _close(cg, a, b)


def test_teardown_orders():
    """A member destroyed under a live kernel: the group is broken (a grouped call raises), the survivors' own calls work and the
    group's destroy is harmless.  A group destroyed with its kernel live returns cleanly.  A member of a SAC update group AND a
    collect group destroyed first, then both groups."""
    from fsrl_amd.engine import EngineCollectGroup, EngineSacGroup
    envs, Do, Da = (20, 7, 33), 8, 2
    a, b, cg = _pair("sacl", envs, 128, Do, Da)
    rng = np.random.default_rng(1)
    oas = [rng.standard_normal((e, Do)).astype(np.float32) for e in envs]
    cg.collect_step([None] * 3, oas, False, 1)
    assert cg.actor_resident_stats()["live"]
    b[0].close()
    with pytest.raises(Exception, match="destroyed"):
        cg.collect_step([None] * 3, oas, False, 1)
    for eng, o in zip(b[1:], oas[1:]):
        act, ea, _, _ = eng.collect_step(None, o, True, 1)
        assert act.shape == (len(o), Da) and np.isfinite(act).all()
    cg.close()
    for eng, o in zip(b[1:], oas[1:]):
        assert np.isfinite(eng.collect_step(None, o, True, 1)[0]).all()
    # the survivors can be grouped again, and that group is destroyed with its kernel live
    cg2 = EngineCollectGroup(b[1:])
    cg2.collect_step([None] * 2, oas[1:], False, 1)
    assert cg2.actor_resident_stats()["live"]
    cg2.close()
    for eng, o in zip(b[1:], oas[1:]):
        assert np.isfinite(eng.collect_step(None, o, True, 1)[0]).all()
    # a member of an update group and a collect group goes first
    ug, cg3 = EngineSacGroup(a), EngineCollectGroup(a)
    cg3.collect_step([None] * 3, oas, False, 1)
    assert cg3.actor_resident_stats()["live"]
    a[2].close()
    with pytest.raises(Exception, match="destroyed"):
        cg3.collect_step([None] * 3, oas, False, 1)
    ug.close(); cg3.close()
    for eng, o in zip(a[:2], oas[:2]):
        assert np.isfinite(eng.collect_step(None, o, True, 1)[0]).all()
    _close(a[:2], b[1:])


def test_rejections():
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineCollectGroup, EngineConfig
    H, Do, Da = 128, 8, 2
    a, a2 = _member("sacl", H, Do, Da, 4, 0), _member("sacl", H, Do, Da, 4, 1)
    mk = lambda hs, **kw: Engine(EngineConfig(algo=_lib.ALGO_SAC_LAG, obs_dim=Do, act_dim=Da, hidden_sizes=hs, n_critics=2, env_num=4,
                                              buffer_size=800, target_kl=None, **kw))
    ppo = Engine(EngineConfig(obs_dim=Do, act_dim=Da, hidden=H, env_num=4, buffer_size=800, target_kl=None))
    lay = mk((64, 64, 64)); lay.cvpo_init(0.1)
    raw = mk((H, H))
    ddpg = _member("ddpgl", H, Do, Da, 4, 2)
    cvpo = _member("cvpo", H, Do, Da, 4, 3)
    wide = _member("sacl", 256, Do, Da, 4, 4)
    cases = [([a, ppo], "fsrl_group_create"), ([a, lay], "layered"), ([a, raw], "fsrl_sac_init"), ([a, ddpg], "one kind"),
             ([a, cvpo], "one kind"), ([ddpg, cvpo], "one kind"), ([a, wide], "one network shape"), ([a, a2, a], "listed twice")]
    for bad, reason in cases:
        with pytest.raises(Exception, match=reason):           # FSRL_EINVAL, with the reason in the message
            EngineCollectGroup(bad)
    g = EngineCollectGroup([a])
    with pytest.raises(Exception, match="already in a collect group"):
        EngineCollectGroup([a2, a])
    g.close()
    many = [_member("sacl", 64, Do, Da, 2, i) for i in range(17)]
    with pytest.raises(Exception, match="1..16 members"):
        EngineCollectGroup(many)
    g16 = EngineCollectGroup(many[:16])                        # sixteen is the most
    g16.close()
    g = EngineCollectGroup([a, a2])                            # and the rejected members are still free to join
    g.close()
    _close([a, a2, ppo, lay, raw, ddpg, cvpo, wide], many)


@pytest.mark.parametrize("algo", ["sacl", "cvpo", "ddpgl"])
def test_group_collector_over_replay_agents_is_each_members_fast_collector(algo, tmp_path):
    """GroupCollector(EngineCollectGroup, collectors).collect(n) against each member's own FastCollector.collect(n) on an identically
    seeded twin (k = 3, ragged env counts and episode lengths, stochastic actions), two collects with each member's own updates
    between them: the same stats, counters, fill levels, next observations and stored rows."""
    from fsrl_amd.agent import CVPOAgent, DDPGLagAgent, SACLagAgent
    from fsrl_amd.data import FastCollector, GroupCollector, HipVectorReplayBuffer
    from fsrl_amd.engine import EngineCollectGroup
    from fsrl_amd.env import SyntheticSafetyVectorEnv
    from fsrl_amd.utils import BaseLogger
    Agent = {"sacl": SACLagAgent, "cvpo": CVPOAgent, "ddpgl": DDPGLagAgent}[algo]
    envs, ep_len = (5, 12, 3), (30, 17, 41)

    def build(tag):
        agents, cols = [], []
        for s, (e, L) in enumerate(zip(envs, ep_len)):
            env = SyntheticSafetyVectorEnv(env_num=e, obs_dim=8, act_dim=2, episode_len=L, seed=s)
            ag = Agent(env, BaseLogger(str(tmp_path / f"{tag}{s}"), name=f"{tag}{s}"), cost_limit=10.0, device="cuda:0", seed=s,
                       hidden_sizes=(128, 128), training_num=e)
            ag.policy.train()
            buf = HipVectorReplayBuffer(ag.policy.engine, None, e)
            agents.append(ag); cols.append(FastCollector(ag.policy, env, buf, exploration_noise=True, device_actor=True))
        return agents, cols

    solo_agents, solo_cols = build("solo")
    grp_agents, grp_cols = build("grp")
    for x, y in zip(solo_agents, grp_agents):
        assert np.array_equal(x.policy.engine.sac_get_params(0)[0], y.policy.engine.sac_get_params(0)[0])
    cg = EngineCollectGroup([ag.policy.engine for ag in grp_agents])
    gc = GroupCollector(cg, grp_cols)
    for rnd, n_ep in enumerate((7, 4)):
        got = gc.collect(n_episode=n_ep)
        want = [c.collect(n_episode=n_ep) for c in solo_cols]
        assert got == want, rnd
        assert not cg.actor_resident_stats()["live"]
        for x, y in zip(solo_cols, grp_cols):
            assert (x.collect_step, x.collect_episode) == (y.collect_step, y.collect_episode)
            assert np.array_equal(x.buffer._sizes, y.buffer._sizes)
            assert np.array_equal(x._obs, y._obs)
        _same_stores([c.policy.engine for c in solo_cols], [c.policy.engine for c in grp_cols])
        if rnd == 0:                               # an update between the collects: every member's own, on both twins
            for agents, cols, sts in ((solo_agents, solo_cols, want), (grp_agents, grp_cols, got)):
                for ag, col, st in zip(agents, cols, sts):
                    ag.policy.pre_update_fn(stats_train=st)
                    for _ in range(2):
                        ag.policy.update(64, col.buffer)
                    ag.policy.post_update_fn(stats_train=st)
            for x, y in zip(solo_agents, grp_agents):
                assert np.array_equal(x.policy.engine.sac_get_params(0)[0], y.policy.engine.sac_get_params(0)[0])
    assert cg.actor_resident_stats()["requests"] > 0
    cg.close()
    for ag in solo_agents + grp_agents:
        ag.policy.engine.close()
