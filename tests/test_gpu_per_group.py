"""Grouped prioritised updates (fsrl_sac_group_update over members that all have fsrl_per_enable on) against solo twins stepped by
fsrl_sac_update and against the exact CPU model of tests/test_per_model.py.

A member's kernels are the solo prioritised update's bodies inlined, so wherever the group takes the solo run's tile heights --
fused members while 4 * ceil(B / 16) * n_q * k <= 256 and 8 * ceil(B / 16) * k <= 256 (4-row tiles on both sides), batches above 1024
rows (16-row tiles on both sides), layered members at every size -- every member is held to its twin with np.array_equal:
parameters, targets, alpha, statistics rows, the tree (leaves, max_prio, min_prio, root) and the last sample, chain, weights and TD
averages.  Where the tile height differs (fused SAC-Lag, B = 33, k = 8: 16-row tiles in the group, 4-row tiles alone) a last-bit
change in a TD error changes later samples, so no twin is compared: every member is held to the model loaded with the device's own
leaves, at the bars of tests/test_gpu_per.py (its _check_sample and _check_priorities: sample element for element, weights at
relative 1e-6, new leaves and scalars at relative 1e-12, the root exactly).

Stores: 4 x 8 and 3 x 7 slots, partly filled and wrapped; obs 5 / act 2; hidden (64, 64) fused and (32, 16, 8) layered."""
import numpy as np
import pytest

from test_gpu_per import Rig, _check_priorities, _check_sample, _close
from test_per_model import PerModel, priorities, rollout

pytestmark = pytest.mark.gpu

NAMES = ["p2_wrap", "np2_wrap", "p2_part", "np2_part"]
PERS = [(0.6, 0.4, True), (0.6, 0.9, False), (1.0, 0.4, True)]
FUSED, LAYERED = (64, 64), (32, 16, 8)


def _member(i, kind, hidden, B, per=None, name=None):
    """member i: its own store, rollout, parameters, (alpha, beta, weight_norm), priorities and Philox key (one own update)"""
    r = Rig(name or NAMES[i % len(NAMES)], kind, hidden, n_step=2, per=per or PERS[i % len(PERS)], fill=False)
    try:
        rng = np.random.default_rng(200 + i)
        r.eng.sac_set_params((0.3 * rng.standard_normal(r.eng.n_sac_actor)).astype(np.float32),
                             (0.3 * rng.standard_normal(r.eng.n_sac_critics)).astype(np.float32), float(np.log(0.2 + 0.05 * i)))
        for step in rollout(r.name, seed=i):
            r.push(step)
        r.eng.per_update_weight(*priorities(r.name, seed=2 + i))
        r.lam, r.resc = 0.1 * (i + 1), 1.0 / (1.0 + 0.1 * (i + 1))
        _solo(r, B, seed=11 + i)
    except Exception:
        r.close()
        raise
    return r


def _solo(r, B, seed=0):
    if seed:
        from oracle import sampler as S
        r.key = S.key_of(seed)
    r.eng.sac_update(B, [r.lam], r.resc, seed=seed, sync=False)
    r.count += 1


def _grouped(g, rigs, B, n):
    g.update(B, n, [[r.lam] for r in rigs], [r.resc for r in rigs])
    for r, ni in zip(rigs, n):
        r.count += ni


def _state(r, B):
    eng = r.eng
    out = [eng.sac_get_params(w)[0] for w in ((0, 1, 2, 3) if r.kind == "ddpg" else (0, 1, 2))]
    out.append(np.float64(eng.sac_get_params(0)[1]))
    out.append(eng.sac_drain())
    out.extend(np.asarray(x) for x in eng.per_state())
    out.extend(eng.sac_last_sample(B))
    out.extend(eng.sac_last_chain(B, r.n_step))
    out.append(eng.per_last_weights(B))
    out.append(eng.per_last_td(B))
    return out


def _assert_same(x, y, who):
    assert len(x) == len(y)
    for j, (u, v) in enumerate(zip(x, y)):
        assert np.shape(u) == np.shape(v) and np.array_equal(u, v), (who, j, np.abs(np.asarray(u, np.float64) - v).max())


@pytest.fixture
def made():
    rigs, groups = [], []
    yield rigs, groups
    for g in groups:
        g.close()
    for r in rigs:
        r.close()


def _twins(made, k, kind, hidden, B, **kw):
    a = [_member(i, kind, hidden, B, **kw) for i in range(k)]
    made[0].extend(a)
    b = [_member(i, kind, hidden, B, **kw) for i in range(k)]
    made[0].extend(b)
    return a, b


def _group(made, rigs):
    from fsrl_amd.engine import EngineSacGroup
    g = EngineSacGroup([r.eng for r in rigs])
    made[1].append(g)
    return g


# ------------------------------------------------------------------------------------------------ 1: bit-identity with solo twins
EXACT = [("sac", FUSED, 16, 8), ("ddpg", FUSED, 16, 8), ("sac", FUSED, 33, 3), ("ddpg", FUSED, 33, 3), ("sac", FUSED, 1040, 2),
         ("sac", LAYERED, 33, 8), ("ddpg", LAYERED, 33, 8)]


@pytest.mark.parametrize("kind,hidden,B,k", EXACT)
def test_members_equal_their_solo_twins_where_the_tile_heights_agree(made, kind, hidden, B, k):
    a, b = _twins(made, k, kind, hidden, B)
    n = [3, 2, 0, 3, 1, 2, 0, 3][:k]
    before = None
    if k > 2:                   # the member with no updates, as it is before the call (both twins: a look drains the statistics ring)
        before = _state(a[2], B)
        _state(b[2], B)
    _grouped(_group(made, a), a, B, n)
    for r, ni in zip(b, n):
        for _ in range(ni):
            _solo(r, B)
    for i in range(k):
        x, y = _state(a[i], B), _state(b[i], B)
        # the statistics rows: the keying update's (drained above for the idle member) and the call's
        assert len(x[len(x) - 12]) == n[i] + (0 if before is not None and i == 2 else 1)
        _assert_same(x, y, i)
        if n[i]:
            assert np.ptp(x[-2]) > 0 and np.abs(x[-1]).max() > 0       # weights that differ, TD averages that are there
    if before is not None:      # ... its tree, parameters and the last update's buffers untouched bit for bit
        after = _state(a[2], B)
        before[len(before) - 12] = after[len(after) - 12]       # (the keying update's row went with the first look)
        _assert_same(before, after, "idle")


# ------------------------------------------------------------------------------------------------ 2: where the tile height differs
def test_members_follow_the_model_where_the_tile_height_differs(made):
    """fused SAC-Lag, B = 33, k = 8: 4 * 3 * 4 * 8 = 384 > 256, so the group's Q launches take 16-row tiles and a solo run 4-row
    tiles.  Three one-update calls, every member against the model loaded with its own leaves from before the call."""
    B, k = 33, 8
    per = [(0.6, 0.4, True), (1.0, 0.4, True), (0.3, 0.9, True)]          # _check_sample expects weight_norm (w.max() == 1)
    rigs = [_member(i, "sac", FUSED, B, per=per[i % 3]) for i in range(k)]
    made[0].extend(rigs)
    g = _group(made, rigs)
    for call in range(3):
        models = [r.model() for r in rigs]
        _grouped(g, rigs, B, [1] * k)
        for r, m in zip(rigs, models):
            idx, _, _, w = _check_sample(r, B, m)
            assert np.ptp(w) > 0
            _check_priorities(r, B, m, idx)


# ------------------------------------------------------------------------------------------------ 3: interleaving
def _extra_steps(r, seed, n):
    """n more vector steps for every sub-buffer of r's store (a wrapped store overwrites slots)"""
    return rollout(r.name, seed=seed)[:n]


@pytest.mark.parametrize("kind,hidden", [("sac", FUSED), ("ddpg", LAYERED)])
def test_pushes_host_priorities_beta_and_own_updates_between_grouped_calls(made, kind, hidden):
    B, k = 16, 2
    a, b = _twins(made, k, kind, hidden, B)               # stores p2_wrap and np2_wrap: both wrapped
    g = _group(made, a)
    for rnd in range(3):
        n = [2, 1] if rnd != 1 else [1, 3]
        _grouped(g, a, B, n)
        for r, ni in zip(b, n):
            for _ in range(ni):
                _solo(r, B)
        for i in range(k):                               # pushes that overwrite slots of the wrapped stores
            for step in _extra_steps(a[i], 50 + 10 * rnd + i, 3):
                for r in (a[i], b[i]):
                    r.push(step)
        idx, w = priorities(a[0].name, seed=30 + rnd)
        for r in (a[0], b[0]):                           # priorities from the host
            r.eng.per_update_weight(idx[:7], w[:7])
        for r in (a[1], b[1]):                           # beta moves: the next sample's weights
            r.eng.per_set_beta(0.5 + 0.1 * rnd)
        for r in (a[0], b[0]):                           # an own update of one member
            _solo(r, B)
    _grouped(g, a, B, [1, 1])
    for r in b:
        _solo(r, B)
    for i in range(k):
        _assert_same(_state(a[i], B), _state(b[i], B), i)


def test_a_push_right_before_and_right_behind_a_grouped_call_is_ordered_against_its_tree_writes(made):
    """no synchronisation between a push and the grouped call on either side of it: the pushed rows' leaves (max_prio ** alpha as
    of the push) are in the tree the call samples from, and rows pushed behind the call land on top of its priorities"""
    B, k = 16, 3
    per = (0.6, 0.4, True)
    rigs = [_member(i, "sac", FUSED, B, per=per, name=["p2_wrap", "np2_wrap", "p2_wrap"][i]) for i in range(k)]
    made[0].extend(rigs)
    g = _group(made, rigs)
    models = [r.model() for r in rigs]                   # (waits: everything before is done)
    for r, m in zip(rigs, models):
        for step in _extra_steps(r, 77, 2):
            m.add(r.push(step))
    _grouped(g, rigs, B, [1] * k)                        # right behind the pushes
    behind = [[r.push(step) for step in _extra_steps(r, 78, 2)] for r in rigs]      # right behind the call
    devs = [r.model() for r in rigs]                     # flushes the rows pushed behind the call: their leaves follow its priorities
    for r, m, ptrs, dev in zip(rigs, models, behind, devs):
        idx, _, _ = r.eng.sac_last_sample(B)
        assert np.array_equal(idx, m.sample(r.key, r.count - 1, B))
        assert _close(r.eng.per_last_weights(B), m.weights(idx), 1e-6)
        m.update_weight(idx, r.eng.per_last_td(B))
        for ptr in ptrs:
            m.add(ptr)
        assert _close(dev.leaves, m.leaves) and _close(dev.max_prio, m.max_prio) and _close(dev.min_prio, m.min_prio)
        assert (dev.leaves[np.concatenate(ptrs)] == dev.leaves[ptrs[-1][0]]).all()      # the pushed rows carry max_prio ** alpha


# ------------------------------------------------------------------------------------------------ 4: refusals and teardown
def test_refusals_and_teardown(made):
    from fsrl_amd.engine import EngineCvpoGroup, EngineSacGroup
    B = 16
    a, b, c = (_member(i, "sac", FUSED, B, name="p2_part") for i in range(3))
    made[0].extend([a, b, c])
    plain = Rig("p2_part", per=None)
    made[0].append(plain)
    with pytest.raises(AssertionError, match="member 0 has prioritised replay on and member 1 does not: "):
        EngineSacGroup([a.eng, plain.eng])
    with pytest.raises(AssertionError, match="member 1 has prioritised replay on and member 0 does not: "):
        EngineSacGroup([plain.eng, a.eng])
    with pytest.raises(AssertionError, match="prioritised replay"):
        EngineCvpoGroup([a.eng, b.eng])
    g = EngineSacGroup([a.eng, b.eng])
    made[1].append(g)
    with pytest.raises(AssertionError, match="already in a group"):
        a.eng.per_enable(0.5, 0.5)
    _grouped(g, [a, b], B, [1, 1])
    b.close()                                            # a member destroyed before its group
    with pytest.raises(RuntimeError, match="destroyed"):
        g.update(B, [1, 1], [[0.1], [0.1]], [1.0, 1.0])
    g.close()                                            # destroy still works
    a.eng.per_enable(0.5, 0.5)                           # out of the group again: allowed
    g2 = EngineSacGroup([a.eng, c.eng])                  # ... and a group of prioritised members again
    made[1].append(g2)
    m = PerModel(a.E * a.sub, 0.5, 0.5).load(*a.eng.per_state()[:3])
    a.per = (0.5, 0.5, True)
    _grouped(g2, [a, c], B, [1, 1])
    _check_sample(a, B, m)


# ------------------------------------------------------------------------------------------------ 5: policy level
@pytest.mark.parametrize("algo", ["sac", "ddpg"])
def test_policy_group_over_prioritized_buffers_equals_sequential_policy_updates(algo):
    """tests/test_gpu_sac_group.py's test_policy_group_matches_sequential_policy_updates with HipPrioritizedVectorReplayBuffers:
    hidden (64, 64), batch 64, two members -- 4 * 4 * 4 * 2 = 128 and 8 * 4 * 2 = 64 workgroups, the solo tile heights"""
    import torch
    from fsrl_amd.agent import DDPGLagAgent, SACLagAgent
    from fsrl_amd.data import FastCollector, HipPrioritizedVectorReplayBuffer
    from fsrl_amd.env import SyntheticSafetyVectorEnv
    from fsrl_amd.policy import DDPGPolicyGroup, SACPolicyGroup
    agent_cls, group_cls = (SACLagAgent, SACPolicyGroup) if algo == "sac" else (DDPGLagAgent, DDPGPolicyGroup)

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
        for s in range(2):
            env = SyntheticSafetyVectorEnv(env_num=4, episode_len=30, seed=10 + s)
            ag = agent_cls(env, None, cost_limit=10, device="cuda:0", seed=1 + s, hidden_sizes=(64, 64), training_num=4, buffer_size=2000)
            ag.policy.logger = _Log()
            ag.policy.train()
            buf = HipPrioritizedVectorReplayBuffer(ag.policy.engine, 2000, 4, alpha=0.6 + 0.2 * s, beta=0.4 + 0.3 * s, weight_norm=s == 0)
            agents.append(ag); bufs.append(buf); logs.append(ag.policy.logger)
            cols.append(FastCollector(ag.policy, env, buf, exploration_noise=True))
        grp = group_cls([a.policy for a in agents]) if grouped else None
        for cyc in range(2):
            n = []
            for ag, col in zip(agents, cols):
                ag.policy.engine.actor_sample(np.zeros((1, ag.policy.engine.cfg.obs_dim), np.float32), seed=40 + cyc)
                st = col.collect(n_episode=4)
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
        out = [({k: v.detach().cpu().numpy().copy() for k, v in ag.policy.state_dict().items() if torch.is_tensor(v)}, lg.rows,
                ag.policy.engine.per_state(), ag.policy.engine.per_last_weights(64))
               for ag, lg in zip(agents, logs)]
        if grp is not None:
            grp.close()
        for ag in agents:
            ag.policy.engine.close()
        return out

    got, want = build(True), build(False)
    for (sg, lg, tg, wg), (sw, lw, tw, ww) in zip(got, want):
        assert sg.keys() == sw.keys()
        for key in sg:
            assert np.array_equal(sg[key], sw[key]), key
        assert lg == lw
        assert all(np.array_equal(x, y) for x, y in zip(tg, tw)) and np.array_equal(wg, ww)
        assert tg[1] > 1.0 > tg[2] > 0.0 and np.ptp(wg) > 0           # priorities moved, weights differ


def test_policy_group_refuses_a_mix_of_prioritized_and_uniform_buffers():
    from fsrl_amd.agent import SACLagAgent
    from fsrl_amd.data import HipPrioritizedVectorReplayBuffer, HipVectorReplayBuffer
    from fsrl_amd.env import SyntheticSafetyVectorEnv
    from fsrl_amd.policy import SACPolicyGroup
    agents = [SACLagAgent(SyntheticSafetyVectorEnv(env_num=4, episode_len=30, seed=s), None, cost_limit=10, device="cuda:0", seed=s,
                          hidden_sizes=(64, 64), training_num=4, buffer_size=2000) for s in range(2)]
    try:
        HipPrioritizedVectorReplayBuffer(agents[0].policy.engine, 2000, 4)
        HipVectorReplayBuffer(agents[1].policy.engine, 2000, 4)
        with pytest.raises(AssertionError, match="HipPrioritizedVectorReplayBuffer"):
            SACPolicyGroup([a.policy for a in agents])
    finally:
        for a in agents:
            a.policy.engine.close()
