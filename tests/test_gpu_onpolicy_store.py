"""The on-policy data plane on wrapped, re-cut and reset stores: fsrl_store_push -> store_scatter_kernel -> sample0() ->
batch_gather_kernel -> mlp_infer_kernel / lay_infer -> gae_kernel -> ret_rms_update_kernel, against an exact host model of the
store (tests/onpolicy_store_problems.py: a mirror kept by tests/golden/ref_shim.VectorReplayBuffer) and the float64 oracle.

After every stage of a scenario's script:

* bit-exact against the mirror: every push return (ptr, ep_rew, ep_len, ep_idx), len, the fill levels, the geometry, sample0()
  and all seven columns of every stored slot;
* process_fn (ppo_begin) against PPOLagOracle(float64) on the mirror's batch: values, advs, rets, logp_old within
  5e-6 * max(1, max|x|) per array, without and with reward normalisation (from a non-trivial ret_rms; the running statistics
  afterwards at rtol 1e-5, atol 1e-7);
* one short update (2 passes, batch 64, given permutations) against the fp32 oracle at the bars of tests/test_gpu_shapes.py.

The bar is the one the project uses for the same four arrays against the fp32 oracle; tests/test_onpolicy_store_host.py keeps the
fp32 oracle within a tenth of it of float64, and shows that a batch read from slot 0 or without its unfinished-tail flags would
miss it a hundred times over.  The device's own distance from float64, in units of the bar (bound: 1), as measured on an
MI355X (ROCm 7.0.2) -- largest over the stages of each scenario, plain / with reward normalisation:

    wrapped_ragged      0.061 / 0.061        reset_keep          0.029 / 0.029
    one_over            0.050 / 0.050        reset_drop          0.029 / 0.029
    tiny_sub            0.012 / 0.017        recut               0.032 / 0.032
    windows             0.035 / 0.035        layered_wrapped     0.018 / 0.018
    one_critic          0.061 / 0.061        one_critic_layered  0.016 / 0.016

(largest: 0.061 bars = 3.1e-7 of scale; the fp32 oracle itself sits at 0.03 bars on the same batches)

The other on-policy entry points take the wrapped batch too: tr_begin / cpo_learn, FOCOPS, a grouped PPO update with one wrapped
member; and the single-critic contexts (n_critics = 1), fused and layered."""
import numpy as np
import pytest
import torch

import onpolicy_store_problems as P

pytestmark = pytest.mark.gpu

COLUMNS = ("obs", "act", "rew", "cost", "terminated", "truncated", "obs_next")
SEEN = {}                     # scenario -> largest |device - float64| / bar (plain, reward-normalised)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for name, (a, b) in sorted(SEEN.items()):
        print(f"distance from float64 in bars: {name:20s} {a:.3f} / {b:.3f}")


def _same_push(got, want):
    """every engine's push return is the shim's add: slot, episode reward, length and start index, bit for bit"""
    for g in got:
        for a, b in zip(g, want):
            assert np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64)), (g, want)


def check_store(eng, s):
    """the engine's store against the mirror's stage `s`, bit-exact"""
    assert len(eng) == len(s.batch) == int(s.sizes.sum())
    assert eng.store_geometry() == (s.sub, s.num)
    sizes = eng.store_sizes()
    assert np.array_equal(sizes[:s.num], s.sizes) and not sizes[s.num:].any()
    assert np.array_equal(eng.sample0(), s.indices)
    if s.valid.size:
        got = eng.store_read(s.valid)
        for k in COLUMNS:
            assert got[k].dtype == s.columns[k].dtype and np.array_equal(got[k], s.columns[k]), k


def check_process(scn, eng, s, rew_norm):
    """ppo_begin's products against the float64 oracle on the mirror's batch; leaves the update open.  -> largest distance in bars"""
    o64 = scn.oracle(torch.float64, rew_norm)
    want = o64.process(s.batch)
    lag, resc = scn.lagrangians()
    n = eng.ppo_begin(lag, resc, 64)
    assert n == len(s.batch)
    worst = 0.0
    for k in P.PRODUCTS:
        ref = want[k].numpy()
        got = eng.batch_get(k)
        assert got.shape == ref.shape, (k, got.shape, ref.shape)
        d = float(np.abs(got.astype(np.float64) - ref).max()) / P.bar_of(ref)
        print(f"{s.name} rew_norm={rew_norm} {k}: |device - float64| = {d:.3f} bars")
        worst = max(worst, d)
    for k in P.PRODUCTS:
        ref = want[k].numpy()
        np.testing.assert_allclose(eng.batch_get(k), ref, rtol=0, atol=P.bar_of(ref), err_msg=f"{s.name} {k} rew_norm={rew_norm}")
    if rew_norm:
        got = eng.ret_rms_get()
        assert got.shape == (scn.n_critics, 3)
        np.testing.assert_allclose(got, o64.ret_rms, rtol=1e-5, atol=1e-7)
    return worst


def check_update(scn, eng, s):
    """2 passes at batch 64 with given permutations, on the update check_process left open, against the fp32 oracle
    (tests/test_gpu_shapes.py's bars)"""
    o = scn.oracle()
    lag, resc = scn.lagrangians()
    n = len(s.batch)
    rng = np.random.default_rng(n)
    perms = [rng.permutation(n) for _ in range(2)]
    _, ostats, _ = o.update(s.batch, lag, resc, 64, 2, perms=perms)
    for p in perms:
        assert eng.ppo_pass(p) is False
    stats = eng.ppo_end_stats(2 * max(1, -(-n // 64)))
    ostats = np.asarray(ostats)
    assert stats.shape == ostats.shape
    np.testing.assert_allclose(stats, ostats, rtol=3e-5, atol=3e-5)
    d = np.abs(eng.get_params() - o.get_params())
    assert np.quantile(d, 0.999) <= 5e-6 and d.max() <= 1e-4, (np.quantile(d, 0.999), d.max())
    return stats


def run_scenario(name, on_refuse=None):
    scn = P.SCENARIOS[name]
    eng, engn = scn.engine(), scn.engine(rew_norm=True)
    seen = [0.0, 0.0]
    rows = []

    def on_stage(s, mirror):
        assert np.array_equal(s.book, s.want_book)
        for e in (eng, engn):
            check_store(e, s)
        if not len(s.batch):
            assert eng.ppo_begin(*scn.lagrangians(), 64) == 0
            eng.ppo_abort()
            return
        for j, e in enumerate((eng, engn)):
            scn.start(e)                                       # every stage from theta0, a fresh optimiser, RMS0
            seen[j] = max(seen[j], check_process(scn, e, s, rew_norm=bool(j)))
        rows.append(check_update(scn, eng, s))
        engn.ppo_end()
        for e in (eng, engn):
            check_store(e, s)                                  # an update leaves the store as it was

    try:
        stages, adds = scn.play([eng, engn], on_push=_same_push, on_stage=on_stage, on_refuse=on_refuse and (lambda op: on_refuse(op, (eng, engn))))
    finally:
        eng.close(); engn.close()
    SEEN[name] = tuple(seen)
    return scn, stages, adds, rows


@pytest.mark.parametrize("name", ["wrapped_ragged", "one_over", "tiny_sub", "windows", "layered_wrapped"])
def test_store_and_process_fn_follow_the_mirror(name):
    torch.set_num_threads(4)
    scn, stages, adds, rows = run_scenario(name)
    assert len(rows) == 1 and np.isfinite(rows[0]).all()


@pytest.mark.parametrize("name", ["reset_keep", "reset_drop"])
def test_reset_between_updates_with_episodes_in_flight(name):
    """OnpolicyTrainer's reset after every update: the next batch holds only the new rows, and the first finished episode of every
    env reports the reward and length carried across the reset (keep_statistics) or counted from it -- equal to the shim's, which
    run_scenario asserts for every push; here: that the two differ the way the scenario says"""
    torch.set_num_threads(4)
    scn, stages, adds, rows = run_scenario(name)
    assert [s.name for s in stages] == ["before", "emptied", "after"] and len(rows) == 2
    after = stages[-1]
    assert len(after.batch) == 30 * scn.E and np.array_equal(after.indices, np.concatenate([e * scn.sub + np.arange(30) for e in range(scn.E)]))
    n_before = int(stages[0].sizes.sum())
    seen = np.zeros(scn.E, np.int64)
    first = {}
    for a in adds:
        for ptr, ep_rew, ep_len, ep_idx in zip(*a):
            e = int(ptr) // scn.sub
            seen[e] += 1
            if seen.sum() > n_before and ep_len > 0 and e not in first:
                first[e] = (int(ep_len), int(seen[e]) - 50)
    assert sorted(first) == list(range(scn.E))
    for e, (ep_len, since_reset) in first.items():
        assert (ep_len > since_reset) if name == "reset_keep" else (ep_len == since_reset), (e, ep_len, since_reset)


def test_recut_store_follows_the_mirror():
    """fsrl_store_configure to fewer sub-buffers and to a ceil(total / num) size: the geometry, the emptying, the content after
    each cut; an env id beyond the active sub-buffers and a geometry beyond the allocation are refused and change nothing"""
    torch.set_num_threads(4)
    refused = []

    def on_refuse(op, engines):
        for eng in engines:
            before = (len(eng), eng.store_geometry(), eng.sample0().copy())
            z = np.zeros
            with pytest.raises(AssertionError):
                if op[0] == "refuse_push":
                    eng.push([op[1]], z((1, 4), np.float32), z((1, 2), np.float32), z(1), z(1), z(1, bool), z(1, bool), z((1, 4), np.float32))
                else:
                    eng.store_configure(op[1], op[2])
            assert (len(eng), eng.store_geometry()) == before[:2] and np.array_equal(eng.sample0(), before[2])
        refused.append(op)

    scn, stages, adds, rows = run_scenario("recut", on_refuse)
    assert len(refused) == 4 and len(rows) == 3
    assert [(s.sub, s.num) for s in stages] == [(130, 3), (130, 3), (3, 3), (3, 3), (100, 4)]


# ------------------------------------------------------------------------------------------------ the other entry points
def _wrapped_engine(**over):
    """an engine holding wrapped_ragged's store + the mirror's stage"""
    scn = P.SCENARIOS["wrapped_ragged"]
    eng = scn.engine(**over)
    try:
        stages, _ = scn.play([eng], on_push=_same_push)
    except BaseException:
        eng.close()
        raise
    return scn, eng, stages[-1]


def test_trust_region_begin_and_cpo_learn_on_the_wrapped_batch():
    from oracle.trust_region import CPOConfig, CPOOracle
    from test_gpu_trust import CPO_KEYS
    torch.set_num_threads(4)
    scn, eng, s = _wrapped_engine()
    kw = P.CPO_KW
    o = CPOOracle(CPOConfig(obs_dim=scn.Do, act_dim=scn.Da, hidden=scn.hidden, max_action=1.5, **kw))
    o.set_params(scn.theta0(o.n_params))
    pb, rows = o.update(s.batch, P.CPO_COST, 1)
    n = eng.tr_begin(target_kl=kw["target_kl"], backtrack_coeff=kw["backtrack_coeff"], damping=kw["damping_coeff"], l2_reg=kw["l2_reg"],
                     critic_lr=kw["lr"], max_backtracks=kw["max_backtracks"], optim_critic_iters=kw["optim_critic_iters"], norm_adv=True,
                     cost_limit=kw["cost_limit"])
    assert n == len(s.batch)
    np.testing.assert_allclose(eng.batch_get("advs"), pb["advs"].numpy(), rtol=0, atol=2e-5)
    stats = eng.cpo_learn(P.CPO_COST, 1)
    assert stats.shape[0] == 1 and np.isfinite(stats).all()
    assert stats[0, CPO_KEYS.index("loss/optim_case")] == rows[0][0]["loss/optim_case"]
    eng.close()


def test_focops_update_on_the_wrapped_batch():
    from fsrl_amd import _lib
    from test_gpu_focops_shapes import _oracle, _theta0, check_update as focops_check
    torch.set_num_threads(4)
    scn = P.SCENARIOS["wrapped_ragged"]
    foc = dict(actor_lr=5e-4, critic_lr=1e-3, l2_reg=1e-3, delta=0.02, eta=0.02, tem_lambda=0.95, max_grad_norm=0.5)
    eng = scn.engine(start=False, algo=_lib.ALGO_FOCOPS, max_action=1.0, max_grad_norm=None)
    eng.focops_init(**foc)
    stages, _ = scn.play([eng], on_push=_same_push)
    s = stages[-1]
    check_store(eng, s)
    o = _oracle(scn.Do, scn.Da, scn.hidden, **foc)
    theta0 = _theta0(o, 5)
    o.set_params(theta0, nu=0.3)
    N, B, R = len(s.batch), 64, 2
    rng = np.random.default_rng(6)
    perms = [rng.permutation(N) for _ in range(R)]
    pb, orows, ostopped = o.update(s.batch, 25.0, B, R, perms)
    want = np.array([[sn["loss/nu_loss"], sn["loss/nu_value"], sa["loss/actor_loss"], sa["loss/kl"], sa["loss/entropy"],
                      sc["loss/vf0"], sc["loss/vf1"], sc["loss/vf_total"]] for sn, sa, sc in orows])
    eng.set_params(theta0)
    stats, stopped = eng.focops_update(want[0, 1], want[0, 0], B, R, perms=perms)
    focops_check(stats, stopped, eng, pb, want, ostopped, o)
    eng.close()


def test_grouped_update_with_one_wrapped_member_equals_the_solo_updates():
    """k = 2, only member 1's store has wrapped: per member bit-identical to its own update (both plans run 4-row tiles at these
    sizes: 4 tiles x 4 x 3 networks x 2 members fit the chip in one round)"""
    from fsrl_amd.engine import EngineGroup
    scns = [P.UNWRAPPED, P.SCENARIOS["wrapped_ragged"]]
    assert 4 * 4 * 3 * 2 <= torch.cuda.get_device_properties(0).multi_processor_count
    B, R = 32, 2
    lags, resc = np.array([[0.4], [0.9]]), [1 / 1.4, 1 / 1.9]

    def members():
        out = []
        for i, scn in enumerate(scns):
            eng = scn.engine()
            th = scn.theta0(eng.n_params)
            eng.set_params(th + (0.01 * np.random.default_rng(100 + i).standard_normal(th.size)).astype(np.float32) * (i > 0))
            stages, _ = scn.play([eng], on_push=_same_push)
            check_store(eng, stages[-1])
            out.append((eng, stages[-1]))
        return out
    solo = members()
    assert not solo[0][1].wrapped.any() and solo[1][1].wrapped.all()
    rng = np.random.default_rng(5)
    perms = [[rng.permutation(len(s.batch)) for _ in range(R)] for _, s in solo]
    want = []
    for i, (eng, s) in enumerate(solo):
        st, stop = eng.ppo_update(lags[i], resc[i], B, R, perms=perms[i])
        st2, _ = eng.ppo_update(lags[i], resc[i], B, R, perms=perms[i])              # Adam state carried over
        want.append((st, stop, st2, eng.get_params(), eng.batch_get("advs")))
        eng.close()
    grouped = members()
    engs = [e for e, _ in grouped]
    grp = EngineGroup(engs)
    st_a, stop_a = grp.ppo_update(lags, resc, B, R, perms=perms)
    st_b, _ = grp.ppo_update(lags, resc, B, R, perms=perms)
    for i, eng in enumerate(engs):
        st, stop, st2, th, advs = want[i]
        assert stop_a[i] == stop == -1 and np.isfinite(st).all()
        assert np.array_equal(st_a[i], st) and np.array_equal(st_b[i], st2), i
        assert np.array_equal(eng.get_params(), th) and np.array_equal(eng.batch_get("advs"), advs), i
    grp.close()
    for e in engs:
        e.close()


# ------------------------------------------------------------------------------------------------ one critic
@pytest.mark.parametrize("name", ["one_critic", "one_critic_layered"])
def test_single_critic_context(name):
    """n_critics = 1: one column per batch array, 3 running statistics, process_fn and the update against
    PPOLagOracle(n_critics=1); the cost columns of the logged rows are exactly 0; the other algorithms refuse the context"""
    from oracle.ppo_lag import STAT_KEYS
    torch.set_num_threads(4)
    scn, stages, adds, rows = run_scenario(name)
    assert scn.n_critics == 1 and len(rows) == 1
    st = rows[0]
    col = {k: st[:, j] for j, k in enumerate(STAT_KEYS)}
    for k in ("loss/lagrangian", "loss/actor_safety", "loss/vf1"):
        assert not col[k].any(), k
    assert np.array_equal(col["loss/vf_total"], col["loss/vf0"]) and (col["loss/vf0"] > 0).all()
    assert (col["loss/rescaling"] == 1.0).all()
    eng = scn.engine()
    stages, _ = scn.play([eng])
    n = eng.ppo_begin([], 1.0, 64)
    for k in ("values", "advs", "rets"):
        assert eng.batch_get(k).shape == (n, 1)
    assert eng.batch_get("logp_old").shape == (n, )
    eng.ppo_end()
    with pytest.raises(AssertionError, match="CPO / TRPO-Lag need a reward and one cost critic"):
        eng.tr_begin()
    check_store(eng, stages[-1])                              # the refusal left the store alone
    eng.close()
    from fsrl_amd import _lib
    foc = scn.engine(start=False, algo=_lib.ALGO_FOCOPS)
    with pytest.raises(AssertionError, match="FOCOPS uses a reward and a cost critic"):
        foc.focops_init()
    foc.close()


class _Cap:
    def __init__(self):
        self.rows = []

    def store(self, tab=None, **kw):
        self.rows.append({(tab + "/" + k if tab else k): float(v) for k, v in kw.items()})

    def print(self, *a, **k):
        pass


def _facade_policy(Do, Da, E, n_critics, buffer_size, logger):
    from torch.distributions import Independent, Normal
    from fsrl_amd.env import Box
    from fsrl_amd.policy import PPOLagrangian
    from fsrl_amd.utils.net import ActorCritic, ActorProb, Critic, Net
    torch.manual_seed(3)
    actor = ActorProb(Net((Do, ), hidden_sizes=(64, 64)), (Da, ), max_action=1.0)
    critics = [Critic(Net((Do, ), hidden_sizes=(64, 64))) for _ in range(n_critics)]
    pol = PPOLagrangian(actor, critics, torch.optim.Adam(ActorCritic(actor, critics).parameters(), lr=5e-4),
                        lambda *l: Independent(Normal(*l), 1), logger=logger, target_kl=None, max_grad_norm=0.5, cost_limit=10.0,
                        observation_space=Box(-np.inf, np.inf, (Do, )), action_space=Box(-1, 1, (Da, )), device=0, env_num=E,
                        buffer_size=buffer_size)
    pol.train()
    return pol


def test_facade_with_one_critic_logs_no_cost_columns():
    from fsrl_amd.data import FastCollector, HipVectorReplayBuffer
    from fsrl_amd.env import SyntheticSafetyVectorEnv
    log = _Cap()
    pol = _facade_policy(8, 2, 3, 1, 3 * 40, log)
    assert pol.engine.cfg.n_critics == 1 and pol.lagrangians_and_rescaling() == ([], 1.0)
    env = SyntheticSafetyVectorEnv(env_num=3, episode_len=25, seed=5)
    buf = HipVectorReplayBuffer(pol.engine, 3 * 40, 3)
    torch.manual_seed(11); np.random.seed(11)
    FastCollector(pol, env, buf, exploration_noise=True).collect(n_episode=12)          # 100 rows per env: the store wraps
    assert len(buf) == 120
    out = pol.update(0, buf, batch_size=64, repeat=2)
    assert out["gradient_steps"] == 2
    keys = set().union(*[set(r) for r in log.rows])
    assert "loss/vf0" in keys and "loss/vf_total" in keys and "loss/actor_rew" in keys
    assert not keys & {"loss/vf1", "loss/lagrangian", "loss/actor_safety"}, keys
    assert all(np.isfinite(list(r.values())).all() for r in log.rows)
    pol.engine.close()


# ------------------------------------------------------------------------------------------------ facade
class _Recording:
    """a HipVectorReplayBuffer and a shim buffer fed the same rows; every add's return compared"""

    def __init__(self, buf, mirror):
        self.buf, self.mirror, self.buffer_num, self.engine = buf, mirror, buf.buffer_num, buf.engine

    def add(self, batch, buffer_ids=None):
        got = self.buf.add(batch, buffer_ids)
        want = self.mirror.add(buffer_ids, batch.obs, batch.act, batch.rew, batch.cost, batch.terminated, batch.truncated, batch.obs_next)
        _same_push([got], want)
        return got

    def reset(self, keep_statistics=False):
        self.buf.reset(keep_statistics)
        self.mirror.reset(keep_statistics)

    def __len__(self):
        return len(self.buf)


def test_facade_collector_wraps_the_store_like_the_reference_buffer():
    """HipVectorReplayBuffer + FastCollector over 3 envs of 25-step episodes into 3 x 40 slots: 100 rows per env; sample_indices(0)
    and len equal a shim buffer's fed the same rows, before and after reset(keep_statistics=True) and a second collect"""
    from fsrl_amd.data import FastCollector, HipVectorReplayBuffer
    from fsrl_amd.env import SyntheticSafetyVectorEnv
    E, sub = 3, 40
    pol = _facade_policy(8, 2, E, 2, E * sub, _Cap())
    env = SyntheticSafetyVectorEnv(env_num=E, episode_len=25, seed=5)
    hip = HipVectorReplayBuffer(pol.engine, E * sub, E)
    assert hip.maxsize == E * sub and pol.engine.store_geometry() == (sub, E)
    mirror = P.StoreMirror(E, sub, 8, 2)
    rec = _Recording(hip, mirror)
    torch.manual_seed(11); np.random.seed(11)
    col = FastCollector(pol, env, rec, exploration_noise=True)
    st = col.collect(n_episode=12)
    assert st["n/st"] == 300 and st["n/ep"] == 12

    def same():
        assert len(hip) == len(mirror.buf) and np.array_equal(hip.sample_indices(0), mirror.indices())
        got = pol.engine.store_read(mirror.valid())
        want = mirror.store()
        for k in COLUMNS:
            assert np.array_equal(got[k], want[k][mirror.valid()]), k
    same()
    assert len(hip) == E * sub and np.array_equal(mirror.book, [[40, 20, 19]] * 3)
    col.reset_buffer(keep_statistics=True)
    assert len(hip) == 0 and hip.sample_indices(0).size == 0
    st = col.collect(n_episode=6)                             # 50 rows per env into the emptied store: wraps again
    assert st["n/st"] == 150
    same()
    assert np.array_equal(mirror.book, [[40, 10, 9]] * 3)
    pol.engine.close()
