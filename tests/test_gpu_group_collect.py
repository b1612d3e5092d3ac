"""Lock-step collection of a group (fsrl_group_collect_step, actor_group_resident_kernel, GroupCollector): one library call and one
actor request per vector step for every member.  Per member everything must be what the member's own fsrl_collect_step gives, bit for
bit: stored rows and slots, actions, episode outputs, the library-RNG stream."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _engines(envs, H, Do, Da, unbounded, seed):
    """k engines of one shape, member i with its own parameters and noise stream (the same for every call of this function)"""
    from fsrl_amd.engine import Engine, EngineConfig
    rng = np.random.default_rng(seed)
    engs = []
    for i, e in enumerate(envs):
        eng = Engine(EngineConfig(obs_dim=Do, act_dim=Da, hidden=H, env_num=e, buffer_size=64 * e, max_grad_norm=0.5, target_kl=None,
                                  unbounded=unbounded))
        eng.set_params((0.2 * rng.standard_normal(eng.n_params)).astype(np.float32))
        eng.actor_sample(np.zeros((1, Do), np.float32), seed=1000 + i)        # seeds member i's noise stream
        engs.append(eng)
    return engs


def _pair(envs, H=128, Do=8, Da=2, unbounded=False, seed=0, idle_us=2.0e5):
    """two groups of identical engines: A is driven member by member (fsrl_collect_step), B through fsrl_group_collect_step"""
    from fsrl_amd.engine import EngineGroup
    a, b = _engines(envs, H, Do, Da, unbounded, seed), _engines(envs, H, Do, Da, unbounded, seed)
    ga, gb = EngineGroup(a), EngineGroup(b)
    gb.actor_set_resident(True, idle_timeout_us=idle_us)
    return a, b, ga, gb


def _random_step(rng, envs, Do, Da, k_act_zero=0.15):
    """per member: a random subset of envs with finished transitions (0 .. all) and 0 .. min(env_num, 64) rows to act on"""
    prevs, oas = [], []
    for e in envs:
        k = int(rng.integers(0, e + 1)) if rng.random() > 0.1 else 0
        ids = np.sort(rng.choice(e, k, replace=False)).astype(np.int32)
        prevs.append(None if k == 0 else (ids, rng.standard_normal((k, Do)).astype(np.float32),
                                          rng.standard_normal((k, Da)).astype(np.float32), rng.standard_normal(k),
                                          (rng.random(k) < 0.2).astype(np.float64), rng.random(k) < 0.05, rng.random(k) < 0.05,
                                          rng.standard_normal((k, Do)).astype(np.float32)))
        ka = 0 if rng.random() < k_act_zero else int(rng.integers(1, min(e, 64) + 1))
        oas.append(rng.standard_normal((ka, Do)).astype(np.float32) if ka else None)
    return prevs, oas


def _step_a(a, prevs, oas, det, bound, low, high):
    """group A: the members' own calls; -> per member (act, env_act, ep_rew, ep_len, ptr, ep_idx)"""
    out = []
    for i, eng in enumerate(a):
        act, ea, er, el = eng.collect_step(prevs[i], oas[i], det, bound, None if low is None else low[i],
                                           None if high is None else high[i])
        k = 0 if prevs[i] is None else len(prevs[i][0])
        st = eng._collect_stage["a"]
        out.append((act, ea, er.copy(), el.copy(), st["ptr"][:k].copy(), st["ei"][:k].copy()))
    return out


def _step_b(gb, prevs, oas, det, bound, low, high):
    res = gb.collect_step(prevs, oas, det, bound, low, high)
    ptr, ei = gb.collect_step_outputs()
    out, o = [], 0
    for i, (act, ea, er, el) in enumerate(res):
        k = 0 if prevs[i] is None else len(prevs[i][0])
        out.append((act, ea, er.copy(), el.copy(), ptr[o:o + k].copy(), ei[o:o + k].copy()))
        o += k
    return out


def _same_stores(a, b):
    for ea, eb in zip(a, b):
        ia, ib = ea.sample0(), eb.sample0()
        assert np.array_equal(ia, ib)
        ra, rb = ea.store_read(ia), eb.store_read(ib)
        for key in ra:
            assert np.array_equal(ra[key], rb[key]), key


def _close(*objs):
    for o in objs:
        if isinstance(o, (list, tuple)):
            for x in o:
                x.close()
        else:
            o.close()


@pytest.mark.parametrize("envs,H,Do,Da,unbounded", [
    ((20, ), 256, 8, 2, False),
    ((20, 7, 33), 128, 27, 8, False),
    ((64, 1, 16, 17, 20, 20, 48, 5), 64, 8, 2, True),
    ((64, 1, 16, 17, 20, 20, 48, 5), 256, 8, 2, False),
])
def test_group_collect_step_is_every_members_collect_step_bit_for_bit(envs, H, Do, Da, unbounded):
    """About 60 vector steps with random row counts per member (0, partial tiles, full tiles up to 64): group B's one call per step
    against group A's member-by-member calls.  Actions, env actions, ptr / ep_* outputs and the stores must be identical, and every
    grouped call with rows to act on is one request of the group's resident kernel."""
    a, b, ga, gb = _pair(envs, H, Do, Da, unbounded, seed=len(envs) + H)
    rng = np.random.default_rng(7)
    low = -1.0 - rng.random((len(envs), Da)).astype(np.float32)
    high = 1.0 + rng.random((len(envs), Da)).astype(np.float32)
    n_req = 0
    for step in range(60):
        prevs, oas = _random_step(rng, envs, Do, Da)
        det = step % 7 == 3
        bound = (1, 2, 0)[step % 3]
        lo, hi = (low, high) if step % 2 else (None, None)
        ra = _step_a(a, prevs, oas, det, bound, lo, hi)
        rb = _step_b(gb, prevs, oas, det, bound, lo, hi)
        n_req += any(o is not None for o in oas)
        for i, (x, y) in enumerate(zip(ra, rb)):
            for j, (u, v) in enumerate(zip(x, y)):
                assert np.array_equal(u, v), (step, i, j)
    # one request per call; few launches (an idle timeout while first-launch code loading holds the host up is legitimate)
    st = gb.actor_resident_stats()
    assert st["requests"] == n_req and st["live"] and 1 <= st["launches"] <= 6, st
    gb.actor_release()
    assert not gb.actor_resident_stats()["live"]
    _same_stores(a, b)
    _close(ga, gb, a, b)


def test_group_collect_across_updates_and_uploads():
    """collect -> grouped update -> collect, three cycles, one member's set_params in the middle: the update and the upload end the
    group's kernel (it holds the weights in registers), and parameters and actions stay identical to the member-by-member run."""
    envs, Do, Da = (20, 7, 33), 8, 2
    a, b, ga, gb = _pair(envs, 128, Do, Da, False, seed=11)
    rng = np.random.default_rng(5)
    for cycle in range(3):
        for step in range(16):
            if cycle == 1 and step == 8:
                th = (0.2 * rng.standard_normal(a[1].n_params)).astype(np.float32)
                a[1].set_params(th); b[1].set_params(th)
                assert not gb.actor_resident_stats()["live"]
            prevs, oas = _random_step(rng, envs, Do, Da, k_act_zero=0.0)
            ra = _step_a(a, prevs, oas, False, 1, None, None)
            rb = _step_b(gb, prevs, oas, False, 1, None, None)
            for i, (x, y) in enumerate(zip(ra, rb)):
                for j, (u, v) in enumerate(zip(x, y)):
                    assert np.array_equal(u, v), (cycle, step, i, j)
        assert gb.actor_resident_stats()["live"]
        lag, resc = np.full((3, 1), 0.3), [1.0, 0.8, 0.9]
        sa, _ = ga.ppo_update(lag, resc, 64, 2, seed=5 + cycle)
        sb, _ = gb.ppo_update(lag, resc, 64, 2, seed=5 + cycle)
        assert not gb.actor_resident_stats()["live"]
        for x, y in zip(sa, sb):
            assert np.array_equal(x, y)
        for ea, eb in zip(a, b):
            assert np.array_equal(ea.get_params(), eb.get_params())
    _same_stores(a, b)
    _close(ga, gb, a, b)


def test_group_actor_calls_spaced_around_its_idle_timeout():
    """The end / relaunch protocol of the group kernel under its race (the short form of
    test_resident_actor_calls_spaced_around_its_idle_timeout): k = 3, calls 0.6 .. 1.4 idle timeouts apart, so that workgroups give
    up while a doorbell is being rung.  Every answer equals the launched path's."""
    envs, Do, Da = (20, 64, 7), 8, 2
    a, b, ga, gb = _pair(envs, 256, Do, Da, False, seed=3, idle_us=120.0)
    rng = np.random.default_rng(2)
    n = 1500
    for i in range(n):
        gap = rng.uniform(0.6, 1.4) * 120e-6 if i % 3 else 0.0
        t = time.perf_counter()
        while time.perf_counter() - t < gap:
            pass
        oas = [rng.standard_normal((int(rng.integers(1, min(e, 64) + 1)), Do)).astype(np.float32) for e in envs]
        rb = gb.collect_step([None] * 3, oas, True, 0)
        ra = [eng.collect_step(None, o, True, 0) for eng, o in zip(a, oas)]
        for m in range(3):
            assert np.array_equal(ra[m][0], rb[m][0]), (i, m)
    st = gb.actor_resident_stats()
    assert st["requests"] == n and 10 < st["launches"] < n, st          # the timeouts did fire, and not before every call
    _close(ga, gb, a, b)


def test_destroying_a_member_under_a_live_group_kernel():
    """A member destroyed while the group's kernel is live: the group is broken (a grouped call raises), the survivors' own calls
    still work, and destroying the broken group is harmless.  A group destroyed with a live kernel returns cleanly too."""
    envs, Do, Da = (20, 7, 33), 8, 2
    a, b, ga, gb = _pair(envs, 128, Do, Da, False, seed=4)
    rng = np.random.default_rng(1)
    oas = [rng.standard_normal((e, Do)).astype(np.float32) for e in envs]
    gb.collect_step([None] * 3, oas, False, 1)
    assert gb.actor_resident_stats()["live"]
    b[0].close()
    with pytest.raises(Exception):
        gb.collect_step([None] * 3, oas, False, 1)
    for eng, o in zip(b[1:], oas[1:]):
        act, ea, _, _ = eng.collect_step(None, o, True, 1)
        assert act.shape == (len(o), Da) and np.isfinite(act).all()
    gb.close()
    for eng, o in zip(b[1:], oas[1:]):
        assert np.isfinite(eng.collect_step(None, o, True, 1)[0]).all()
    # a healthy group destroyed with its kernel live
    ga.collect_step([None] * 3, oas, False, 1)
    assert ga.actor_resident_stats()["live"]
    ga.close()
    for eng, o in zip(a, oas):
        assert np.isfinite(eng.collect_step(None, o, True, 1)[0]).all()
    _close(a, b[1:])


def test_group_collector_is_each_members_fast_collector(tmp_path):
    """GroupCollector.collect(n) against each member's own FastCollector.collect(n) on an ungrouped, identically seeded twin
    (k = 3, ragged env counts, stochastic actions): the same stats, the same stored rows, and the same member RNG state afterwards
    (the second collect matches too)."""
    from fsrl_amd.agent import PPOLagAgent
    from fsrl_amd.data import FastCollector, GroupCollector, HipVectorReplayBuffer
    from fsrl_amd.env import SyntheticSafetyVectorEnv
    from fsrl_amd.policy import PolicyGroup
    from fsrl_amd.utils import BaseLogger
    envs, ep_len = (5, 12, 3), (30, 17, 41)

    def build(tag):
        agents, cols = [], []
        for s, (e, L) in enumerate(zip(envs, ep_len)):
            env = SyntheticSafetyVectorEnv(env_num=e, obs_dim=8, act_dim=2, episode_len=L, seed=s)
            ag = PPOLagAgent(env, BaseLogger(str(tmp_path / f"{tag}{s}"), name=f"{tag}{s}"), cost_limit=10.0, device="cuda:0", seed=s,
                             hidden_sizes=(128, 128), training_num=e)
            ag.policy.train()
            buf = HipVectorReplayBuffer(ag.policy.engine, None, e)
            agents.append(ag); cols.append(FastCollector(ag.policy, env, buf, device_actor=True))
        return agents, cols

    solo_agents, solo_cols = build("solo")
    grp_agents, grp_cols = build("grp")
    for x, y in zip(solo_agents, grp_agents):
        assert np.array_equal(x.policy.engine.get_params(), y.policy.engine.get_params())
    group = PolicyGroup([ag.policy for ag in grp_agents])
    gc = GroupCollector(group, grp_cols)
    for rnd, n_ep in enumerate((7, 4)):
        got = gc.collect(n_episode=n_ep)
        want = [c.collect(n_episode=n_ep) for c in solo_cols]
        assert got == want, rnd
        assert not group.group.actor_resident_stats()["live"]
        for x, y in zip(solo_cols, grp_cols):
            assert (x.collect_step, x.collect_episode) == (y.collect_step, y.collect_episode)
            assert np.array_equal(x.buffer._sizes, y.buffer._sizes)
            assert np.array_equal(x._obs, y._obs)
        _same_stores([c.policy.engine for c in solo_cols], [c.policy.engine for c in grp_cols])
    assert group.group.actor_resident_stats()["requests"] > 0
    group.close()
    for ag in solo_agents + grp_agents:
        ag.policy.engine.close()
