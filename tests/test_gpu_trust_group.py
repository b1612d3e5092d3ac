"""Grouped trust-region seeds: CPO / TRPO-Lag engines in an EngineCollectGroup (fsrl_collect_group_* over on-policy members: the
group actor kernel of the PPO-Lag group launched from a group whose members keep their own streams; layered members: L + 2 launches
per request), GroupCollector over it, and TrustPolicyGroup (the members' own updates on a thread each).

Pattern throughout: "twins" -- two sets of identically built and identically seeded members.  Set A collects with each member's own
FastCollector and updates the members one after the other; set B collects in lock step and updates through the group.  Everything is
compared with np.array_equal: per member the grouped run IS the member's own run."""
import numpy as np
import pytest

from test_gpu_group_collect import _close, _same_stores

pytestmark = pytest.mark.gpu

ENVS = (3, 5, 20)           # ragged; the last member has two 16-row tiles


class _Log:
    def __init__(self):
        self.rows = []

    def store(self, tab=None, **kw):
        self.rows.append((tab, sorted((k, repr(v)) for k, v in kw.items())))     # repr: exact for floats, and nan == nan

    def print(self, *a):
        pass


def _agent_cls(algo):
    from fsrl_amd.agent import CPOAgent, TRPOLagAgent
    return {"cpo": CPOAgent, "trpol": TRPOLagAgent}[algo]


class _Set:
    """k members: agent, env, buffer, collector, log and the record of every collect_step answer a member got"""

    def __init__(self, algos, envs=ENVS, hs=(64, 64), Do=8, Da=2, grouped=False, resident=True, reference_rng=False):
        from fsrl_amd.data import FastCollector, GroupCollector, HipVectorReplayBuffer
        from fsrl_amd.engine import EngineCollectGroup
        from fsrl_amd.env import SyntheticSafetyVectorEnv
        self.envs, self.grouped = envs, grouped
        self.agents, self.bufs, self.cols, self.logs = [], [], [], []
        self.recs = [[] for _ in envs]
        for s, (algo, e) in enumerate(zip(algos, envs)):
            env = SyntheticSafetyVectorEnv(env_num=e, obs_dim=Do, act_dim=Da, episode_len=25 + 2 * s, seed=10 + s)
            ag = _agent_cls(algo)(env, None, cost_limit=10, device="cuda:0", seed=1 + s, hidden_sizes=hs, training_num=e,
                                  buffer_size=e * 200)
            ag.policy.logger = _Log()
            ag.policy._reference_rng = reference_rng
            ag.policy.train()
            buf = HipVectorReplayBuffer(ag.policy.engine, e * 200, e)
            ag.policy.engine.actor_sample(np.zeros((1, Do), np.float32), seed=40 + s)       # keys member s's noise stream
            self.agents.append(ag); self.bufs.append(buf); self.logs.append(ag.policy.logger)
            self.cols.append(FastCollector(ag.policy, env, buf, exploration_noise=True, device_actor=True))
        self.engines = [a.policy.engine for a in self.agents]
        self.policies = [a.policy for a in self.agents]
        self.cg = self.gcol = None
        if grouped:
            self.cg = EngineCollectGroup(self.engines)
            self.cg.actor_set_resident(resident, idle_timeout_us=2.0e5)
            self.gcol = GroupCollector(self.cg, self.cols)
            self._record_group()
        else:
            for i, eng in enumerate(self.engines):
                eng.actor_set_resident(resident, idle_timeout_us=2.0e5)
                self._record_solo(i, eng)

    def _record_solo(self, i, eng):
        inner = eng.collect_step

        def step(prev, obs_act, *a, **kw):
            act, ea, er, el = inner(prev, obs_act, *a, **kw)
            k = 0 if prev is None else len(prev[0])
            st = eng._collect_stage["a"]
            self.recs[i].append((act.copy(), ea.copy(), er.copy(), el.copy(), st["ptr"][:k].copy(), st["ei"][:k].copy()))
            return act, ea, er, el
        eng.collect_step = step

    def _record_group(self):
        cg, inner = self.cg, self.cg.collect_step

        def step(prevs, obs_acts, *a, **kw):
            res = inner(prevs, obs_acts, *a, **kw)
            ptr, ei = cg.collect_step_outputs()
            o = 0
            for i, (act, ea, er, el) in enumerate(res):
                k = 0 if prevs[i] is None else len(prevs[i][0])
                if prevs[i] is not None or obs_acts[i] is not None:      # a member that has its episodes sits the call out
                    self.recs[i].append((act.copy(), ea.copy(), er.copy(), el.copy(), ptr[o:o + k].copy(), ei[o:o + k].copy()))
                o += k
            return res
        cg.collect_step = step

    def collect(self, per_env=2):
        n = [per_env * e for e in self.envs]
        return self.gcol.collect(n_episode=n) if self.grouped else [c.collect(n_episode=x) for c, x in zip(self.cols, n)]

    def next_actions(self):
        """what every member draws next from ITS noise stream, through its own actor call"""
        rng = np.random.default_rng(3)
        out = []
        for eng, e in zip(self.engines, self.envs):
            obs = rng.standard_normal((e, eng.cfg.obs_dim)).astype(np.float32)
            out.append(eng.actor_sample(obs).copy())
            eng.actor_release()
        return out

    def close(self):
        if self.cg is not None:
            self.cg.close()
        for e in self.engines:
            e.close()


def _same_records(a, b):
    for i, (ra, rb) in enumerate(zip(a.recs, b.recs)):
        assert len(ra) == len(rb) and len(ra) > 0, (i, len(ra), len(rb))
        for s, (x, y) in enumerate(zip(ra, rb)):
            for j, (u, v) in enumerate(zip(x, y)):
                assert np.array_equal(u, v), (i, s, j)


def _same_collect(a, b, sa, sb):
    """stats (episode returns and lengths), every call's actions / env actions / write pointers / episode outputs, the stores"""
    assert sa == sb
    _same_records(a, b)
    _same_stores(a.engines, b.engines)


def _twins(algos, **kw):
    """set A first: 1 + k resident kernels live at once would queue behind each other's hardware queues (test_gpu_collect_group)"""
    return _Set(algos, grouped=False, **kw), _Set(algos, grouped=True, **kw)


# ---------------------------------------------------------------------------------------------------- lock-step collection
@pytest.mark.parametrize("algos", [("cpo", ) * 3, ("trpol", ) * 3, ("cpo", "trpol", "trpol")], ids=["cpo", "trpol", "mixed"])
def test_lock_step_collection_is_every_members_own_collect(algos):
    """k = 3 fused members (64, 64) with 3 / 5 / 20 envs, two episodes per env"""
    a, b = _twins(algos)
    sa = a.collect()
    sb = b.collect()
    _same_collect(a, b, sa, sb)
    st = b.cg.actor_resident_stats()
    assert st["requests"] == max(len(r) for r in b.recs) - 1 and 1 <= st["launches"] <= 6 and not st["live"], st
    for x, y in zip(a.next_actions(), b.next_actions()):
        assert np.array_equal(x, y)
    _close(a, b)


@pytest.mark.parametrize("resident", [True, False])
def test_second_half_of_a_tile_and_the_widest_head(resident):
    """act_dim 16, hidden (128, 128), one member with 12 rows in every request: rows 8 .. 15 of a tile, sixteen means per row"""
    a, b = _twins(("cpo", ), envs=(12, ), hs=(128, 128), Da=16, resident=resident)
    sa = a.collect(per_env=1)
    sb = b.collect(per_env=1)
    _same_collect(a, b, sa, sb)
    assert (b.cg.actor_resident_stats()["requests"] > 0) == resident
    assert a.recs[0][0][0].shape == (12, 16)
    _close(a, b)


def test_a_member_asking_for_more_rows_than_its_tiles_falls_back_to_the_members_own_calls():
    """env_num 80 has min(4, ceil(80 / 16)) = 4 tiles: 64 rows.  80 rows in a request: every member's own actor call, same bits."""
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineCollectGroup, EngineConfig
    envs, Do, Da = (80, 3), 8, 2

    def members():
        rng, out = np.random.default_rng(5), []
        for i, e in enumerate(envs):
            eng = Engine(EngineConfig(algo=_lib.ALGO_CPO, obs_dim=Do, act_dim=Da, hidden_sizes=(64, 64), env_num=e, buffer_size=e * 50,
                                      target_kl=None))
            eng.set_params((0.2 * rng.standard_normal(eng.n_params)).astype(np.float32))
            eng.actor_sample(np.zeros((1, Do), np.float32), seed=70 + i)
            out.append(eng)
        return out
    a, b = members(), members()
    rng = np.random.default_rng(6)
    script = [[rng.standard_normal((k, Do)).astype(np.float32) for k in ks] for ks in ((64, 3), (80, 3), (80, 1), (10, 2))]
    want = []
    for oas in script:
        want.append([eng.collect_step(None, o, False, 1)[:2] for eng, o in zip(a, oas)])
        for eng in a:
            eng.actor_release()
    cg = EngineCollectGroup(b)
    requests = []
    for oas, w in zip(script, want):
        got = cg.collect_step([None] * 2, oas, False, 1)
        requests.append(cg.actor_resident_stats()["requests"])
        for m in range(2):
            assert np.array_equal(w[m][0], got[m][0]) and np.array_equal(w[m][1], got[m][1]), m
    assert requests == [1, 1, 1, 2]            # the two 80-row steps went member by member
    _close(cg, a, b)


def test_layered_members_collect_through_one_launch_sequence_per_request():
    a, b = _twins(("cpo", "trpol", "cpo"), hs=(64, 48, 32))
    sa = a.collect()
    sb = b.collect()
    _same_collect(a, b, sa, sb)
    st = b.cg.actor_resident_stats()
    n_req = max(len(r) for r in b.recs) - 1    # the last call of the longest member stores rows and asks for none
    assert st["launches"] == st["requests"] == n_req and not st["live"], (st, n_req)
    for x, y in zip(a.next_actions(), b.next_actions()):
        assert np.array_equal(x, y)
    _close(a, b)


# ---------------------------------------------------------------------------------------------------- ordering against updates
@pytest.mark.parametrize("hs,change", [((64, 64), "learn"), ((64, 48, 32), "learn"), ((64, 64), "params"), ((64, 48, 32), "params")])
def test_a_members_update_between_two_collects_is_seen_by_that_member_alone(hs, change):
    """collect in lock step; member 1 ALONE runs tr_begin + cpo_learn (or gets new parameters); collect again: every member's second
    collect is its twin's -- member 1 acted with its new parameters, the others with unchanged ones.  What this needs: the group's
    stream behind member 1's compute stream before the kernel's prologue reads the parameters (the `ready` events; layered: the
    `reorder` mark), and the kernel ended before the update (the release hook of ENTER_DEV)."""
    a, b = _twins(("cpo", ) * 3, hs=hs)
    sa = a.collect(per_env=1)
    sb = b.collect(per_env=1)
    _same_collect(a, b, sa, sb)
    before = [s.engines[1].get_params() for s in (a, b)]
    na = a.engines[1].n_actor_params
    for s in (a, b):
        eng = s.engines[1]
        if change == "learn":
            eng.tr_begin(target_kl=0.01, critic_lr=1e-3, optim_critic_iters=3, l2_reg=0.001, cost_limit=5.0)
            eng.cpo_learn(12.0, 1)
        else:
            eng.set_params((before[0] + np.float32(0.05) * np.random.default_rng(8).standard_normal(before[0].size)).astype(np.float32))
    after = [s.engines[1].get_params() for s in (a, b)]
    assert np.array_equal(after[0], after[1]) and not np.array_equal(before[0][:na], after[0][:na])      # the actor moved
    first = [len(r) for r in b.recs]
    sa = a.collect(per_env=1)
    sb = b.collect(per_env=1)
    _same_collect(a, b, sa, sb)
    assert all(len(r) > f for r, f in zip(b.recs, first))
    for i in (0, 2):
        assert np.array_equal(a.engines[i].get_params(), b.engines[i].get_params())
    _close(a, b)


# ---------------------------------------------------------------------------------------------------- grouped update
def _state(pol):
    import torch
    return {k: v.detach().cpu().numpy().copy() for k, v in pol.state_dict().items() if torch.is_tensor(v)}


@pytest.mark.parametrize("algo,batch_size,reference_rng", [("cpo", 99999, False), ("trpol", 99999, False), ("cpo", 60, False),
                                                           ("trpol", 60, True)])
def test_trust_policy_group_update_is_the_members_updates_one_after_the_other(algo, batch_size, reference_rng):
    """Two cycles of collect -> pre_update_fn -> update(repeat=2) -> reset_buffer: TrustPolicyGroup (learn calls on a thread per
    member) against the twins updated one after the other under the same np.random.seed.  Per member: parameters, logged rows,
    gradient_steps and the line-search evaluations equal bit for bit.  The critics' Adam step count has no getter in the C ABI; it
    enters every critic step's bias correction, so the second cycle's parameters are equal only if the first cycle left the same
    count.  reference_rng: torch's global stream ends where the twins' does."""
    import torch
    from fsrl_amd.policy import TrustPolicyGroup
    a, b = _twins((algo, ) * 3, reference_rng=reference_rng)
    group = TrustPolicyGroup(b.policies, collect_group=b.cg)
    ends = []
    for s in (a, b):
        evals = []
        for cyc in range(2):
            sts = s.collect()
            for pol, st in zip(s.policies, sts):
                pol.pre_update_fn(stats_train={"cost": 8.0 + 3.0 * cyc + st["cost"] * 0.0})
            np.random.seed(100 + cyc)
            torch.manual_seed(200 + cyc)
            if s.grouped:
                res = group.update(s.bufs, batch_size=batch_size, repeat=2)
            else:
                res = [pol.update(0, buf, batch_size=batch_size, repeat=2) for pol, buf in zip(s.policies, s.bufs)]
            evals.append([eng.tr_linesearch_evals().copy() for eng in s.engines])
            assert all(r["gradient_steps"] >= 2 for r in res)
            if batch_size < 99999:
                assert all(r["gradient_steps"] > 2 for r in res)             # several minibatches: the permutations were used
            for col in s.cols:
                col.reset_buffer(keep_statistics=True)
        ends.append((evals, torch.get_rng_state().clone(), np.random.get_state()[1].copy()))
    for i, (pa, pb) in enumerate(zip(a.policies, b.policies)):
        sa, sb = _state(pa), _state(pb)
        assert sa.keys() == sb.keys()
        for key in sa:
            assert np.array_equal(sa[key], sb[key]), (i, key)
        assert a.logs[i].rows == b.logs[i].rows and len(a.logs[i].rows) > 4, i
        assert pa.gradient_steps == pb.gradient_steps > 0
        assert not pb.updating and pb._pending is None
    for ea, eb in zip(ends[0][0], ends[1][0]):
        for x, y in zip(ea, eb):
            assert np.array_equal(x, y) and len(x) > 0
    assert torch.equal(ends[0][1], ends[1][1]) and np.array_equal(ends[0][2], ends[1][2])
    _same_records(a, b)
    group.close()
    _close(a, b)


# ---------------------------------------------------------------------------------------------------- refusals, teardown
def _engine(algo, hs=(64, 64), env_num=4, **kw):
    from fsrl_amd.engine import Engine, EngineConfig
    return Engine(EngineConfig(algo=algo, obs_dim=8, act_dim=2, hidden_sizes=hs, env_num=env_num, buffer_size=400, target_kl=None, **kw))


def test_refusals_name_the_member_and_the_reason():
    from fsrl_amd import _lib
    from fsrl_amd.engine import EngineCollectGroup, EngineGroup
    from fsrl_amd.policy import TrustPolicyGroup
    cpo, trpo = _engine(_lib.ALGO_CPO), _engine(_lib.ALGO_TRPO_LAG)
    ppo = _engine(_lib.ALGO_PPO_LAG)
    ug = EngineGroup([ppo])                                       # ppo now shares that group's stream
    sac = _engine(_lib.ALGO_SAC_LAG)
    sac.sac_init()
    lay = _engine(_lib.ALGO_CPO, hs=(64, 48, 32))
    loud = _engine(_lib.ALGO_CPO, max_action=2.0)
    free = _engine(_lib.ALGO_CPO, unbounded=True)
    wide = _engine(_lib.ALGO_CPO, hs=(128, 128))
    cases = [([cpo, ppo], "member 1 is in an fsrl_group"), ([cpo, sac], "member 1 is a replay context and member 0 an on-policy one"),
             ([sac, cpo], "member 1 is an on-policy context and member 0 a replay one"),
             ([cpo, lay], "member 1 is a layered context and member 0 a fused one"),
             ([lay, trpo], "member 1 is a fused context and member 0 a layered one"), ([cpo, trpo, loud], "member 2: members must share max_action"),
             ([cpo, free], "member 1: members must share unbounded"), ([cpo, wide], "member 1: members must have one network shape"),
             ([cpo, trpo, cpo], "member 2 is listed twice")]
    for bad, reason in cases:
        with pytest.raises(Exception, match=reason):
            EngineCollectGroup(bad)
    g = EngineCollectGroup([cpo, trpo])                           # CPO and TRPO-Lag members share a group
    with pytest.raises(Exception, match="member 0 is already in a collect group"):
        EngineCollectGroup([trpo])
    g.close()
    ug.close()
    g2 = EngineCollectGroup([cpo, ppo])                           # out of its fsrl_group a PPO-Lag context is a member like any other
    g2.close()
    a, b = _Set(("cpo", ), envs=(3, )), _Set(("trpol", ), envs=(3, ))
    with pytest.raises(AssertionError, match="all CPO or all TRPOLagrangian"):
        TrustPolicyGroup(a.policies + b.policies)
    _close(a, b, [cpo, trpo, ppo, sac, lay, loud, free, wide])


def test_a_member_destroyed_before_its_group():
    from fsrl_amd import _lib
    from fsrl_amd.engine import EngineCollectGroup
    rng = np.random.default_rng(2)
    engs = [_engine(_lib.ALGO_CPO), _engine(_lib.ALGO_TRPO_LAG)]
    for e in engs:
        e.set_params((0.2 * rng.standard_normal(e.n_params)).astype(np.float32))
    oas = [rng.standard_normal((4, 8)).astype(np.float32) for _ in engs]
    cg = EngineCollectGroup(engs)
    cg.collect_step([None] * 2, oas, False, 1)
    assert cg.actor_resident_stats()["live"]
    engs[0].close()
    with pytest.raises(Exception, match="destroyed"):
        cg.collect_step([None] * 2, oas, False, 1)
    cg.close()                                                    # destroying the group still works
    act, ea, _, _ = engs[1].collect_step(None, oas[1], True, 1)   # the survivor collects on its own
    assert act.shape == (4, 2) and np.isfinite(act).all()
    engs[1].close()
