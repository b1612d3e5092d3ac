"""Prioritised replay: the exact CPU model the device's sum tree is held against (tests/test_gpu_per.py), checked on its own.

The model restates tianshou 0.5 PrioritizedReplayBuffer / SegmentTree in float64 numpy (tianshou is not installed):

    one tree over the whole store: bound = the next power of two at or above buffer_num * sub_size, tree = float64[2 * bound],
    leaf of global slot s = tree[bound + s], every internal node exactly left + right
    add             leaf = max_prio ** alpha                               (max_prio = min_prio = 1 at the start)
    sample          scalar = u * tree[1], u = word 0 of Philox block (row, 0, update count) * 2^-32;
                    i = 1; while i < bound: i *= 2; l = tree[i]; d = l < scalar; scalar -= l * d; i += d;   slot = i - bound
    weight          (leaf / min_prio) ** (-beta), divided by the batch maximum with weight_norm, as float32
    update_weight   p = |td| + float32 eps; leaf[idx] = p ** alpha (numpy fancy assignment: of duplicates the last wins);
                    max_prio = max(max_prio, p.max()), min_prio = min(min_prio, p.min())

It also holds a float32 torch restatement of ONE weighted update (loss per Q-network = mean(td^2 * w)) built from the oracles' public
pieces; with w = 1 it must reproduce SACLagOracle.update / DDPGLagOracle.update bit for bit, which is what makes it a yardstick.
The stores, seeds and priorities the GPU tests use are defined here, and checked here to make the model land on filled slots only."""
import numpy as np
import pytest
import torch

from oracle import sampler as S
from oracle.ddpg_lag import DDPGConfig, DDPGLagOracle, mlp
from oracle.sac_lag import ReplayIndex, SACConfig, SACLagOracle
from oracle.scans import nstep_return_np
from test_oracle_sampler import Mirror

F32_EPS = float(np.finfo(np.float32).eps)


# ------------------------------------------------------------------------------------------------ the model
class PerModel:
    def __init__(self, slots, alpha, beta, weight_norm=True):
        self.slots, self.alpha, self.beta, self.weight_norm = int(slots), float(alpha), float(beta), bool(weight_norm)
        self.bound = 1
        while self.bound < self.slots:
            self.bound *= 2
        self.reset()

    def reset(self):
        self.tree = np.zeros(2 * self.bound, np.float64)
        self.max_prio = self.min_prio = 1.0

    @property
    def leaves(self):
        return self.tree[self.bound:self.bound + self.slots]

    @property
    def total(self):
        return float(self.tree[1])

    def rebuild(self):
        """every internal node = left + right, one IEEE add each: a pure function of the leaves"""
        t = self.tree
        n = self.bound
        while n > 1:
            half = n // 2
            t[half:n] = t[n:2 * n:2] + t[n + 1:2 * n:2]
            n = half
        if self.bound == 1:
            pass                     # the root is the only leaf

    def load(self, leaves, max_prio=None, min_prio=None):
        self.tree[:] = 0.0
        self.tree[self.bound:self.bound + self.slots] = np.asarray(leaves, np.float64)
        self.rebuild()
        if max_prio is not None:
            self.max_prio, self.min_prio = float(max_prio), float(min_prio)
        return self

    def add(self, slots):
        self.tree[self.bound + np.asarray(slots, np.int64)] = self.max_prio**self.alpha
        self.rebuild()

    def update_weight(self, idx, td):
        p = np.abs(np.asarray(td, np.float64)) + F32_EPS
        self.tree[self.bound + np.asarray(idx, np.int64)] = p**self.alpha          # fancy assignment: the last duplicate wins
        self.rebuild()
        self.max_prio = max(self.max_prio, float(p.max()))
        self.min_prio = min(self.min_prio, float(p.min()))

    def uniforms(self, key, counter, B):
        key, counter = int(key), int(counter)
        ctr = np.stack([np.arange(B, dtype=np.uint64), np.zeros(B, np.uint64), np.full(B, counter & 0xFFFFFFFF, np.uint64),
                        np.full(B, counter >> 32, np.uint64)], -1)
        w0 = S.philox4x32_10(ctr, (key & 0xFFFFFFFF, key >> 32))[:, 0]
        return w0.astype(np.float64) * 2.0**-32

    def descend(self, scalar, with_margin=False):
        scalar = np.asarray(scalar, np.float64).copy()
        i = np.ones(scalar.shape, np.int64)
        margin = np.full(scalar.shape, np.inf)
        while i[0] < self.bound:
            i *= 2
            l = self.tree[i]
            margin = np.minimum(margin, np.abs(l - scalar))
            d = l < scalar
            scalar -= l * d
            i += d
        slot = i - self.bound
        return (slot, margin) if with_margin else slot

    def sample(self, key, counter, B, with_margin=False):
        return self.descend(self.uniforms(key, counter, B) * self.tree[1], with_margin)

    def weights(self, idx):
        w = (self.tree[self.bound + np.asarray(idx, np.int64)] / self.min_prio)**(-self.beta)
        if self.weight_norm:
            w = w / w.max()
        return w.astype(np.float32)


def td_average(q, y, pair_shift):
    """critics_loss's td_average from the Q values [n_q][B] and the targets [2][B] of an update: float32, summed in network order,
    then divided by the number of Q-networks (sac_lag.py:191-208, ddpg_lag.py:170-184)"""
    q, y = np.asarray(q, np.float32), np.asarray(y, np.float32)
    t = np.zeros(q.shape[1], np.float32)
    for j in range(q.shape[0]):
        t = t + (q[j] - y[j >> pair_shift])
    return t / np.float32(q.shape[0])


# ------------------------------------------------------------------------------------------------ the inputs the GPU tests use
OBS_DIM, ACT_DIM = 5, 2
STORES = {            # name: (buffer_num, sub_size, rows pushed per sub-buffer); 3 x 7 = 21 slots: bound 32
    "p2_part": (4, 8, [5, 8, 3, 6]),
    "p2_wrap": (4, 8, [19, 8, 11, 21]),
    "np2_part": (3, 7, [4, 7, 2]),
    "np2_wrap": (3, 7, [16, 9, 15]),
}
ALPHA, BETA = 0.6, 0.4
SAMPLER_SEEDS = (3, 11)              # x counters 0 .. 2, B in SAMPLE_BATCHES
SAMPLE_BATCHES = (16, 33, 1040)
UPDATE_SEED = 5


def rollout(name, seed=1):
    """the vector steps that fill store `name`, in lock step; sub-buffer 1 sits out every 7th step, so the write heads differ"""
    E, sub, rows = STORES[name]
    rng = np.random.default_rng(seed)
    left = np.array(rows, np.int64)
    steps, t = [], 0
    while (left > 0).any():
        ids = [e for e in range(E) if left[e] > 0 and not (e == 1 and t % 7 == 3)]
        if ids:
            k = len(ids)
            term = rng.random(k) < 0.1
            trunc = (rng.random(k) < 0.1) & ~term
            steps.append((ids, rng.standard_normal((k, OBS_DIM)).astype(np.float32),
                          np.tanh(rng.standard_normal((k, ACT_DIM))).astype(np.float32), rng.normal(0, 1, k),
                          (rng.random(k) < 0.3).astype(np.float64), term, trunc, rng.standard_normal((k, OBS_DIM)).astype(np.float32)))
            left[ids] -= 1
        t += 1
    return steps


def priorities(name, seed=2):
    """the non-uniform priorities the GPU tests set through fsrl_per_update_weight: one per filled slot, a repeated index among them
    (its last entry wins), signs mixed (update_weight takes the absolute value)"""
    E, sub, rows = STORES[name]
    valid = np.concatenate([e * sub + np.arange(min(r, sub)) for e, r in enumerate(rows)])
    rng = np.random.default_rng(seed)
    idx = np.concatenate([valid, valid[:3]])
    w = rng.uniform(0.05, 3.0, idx.size) * rng.choice([-1.0, 1.0], idx.size)
    return idx, w


def build(name, alpha=ALPHA, beta=BETA, weight_norm=True, prio=True):
    """the mirror of store `name` and the model after the pushes (and the priorities)"""
    E, sub, rows = STORES[name]
    mirror, model = Mirror(E, sub, OBS_DIM, ACT_DIM), PerModel(E * sub, alpha, beta, weight_norm)
    for step in rollout(name):
        model.add(mirror.push(*step))
    if prio:
        model.update_weight(*priorities(name))
    return mirror, model


# ------------------------------------------------------------------------------------------------ the model on its own
def _assert_invariant(m):
    t = m.tree
    for i in range(1, m.bound):
        assert t[i] == t[2 * i] + t[2 * i + 1], i
    assert (m.tree[m.bound + m.slots:] == 0).all()


@pytest.mark.parametrize("name", sorted(STORES))
def test_tree_invariant_through_adds_updates_and_reset(name):
    mirror, m = build(name, prio=False)
    assert m.bound == 32 and m.tree.size == 64
    _assert_invariant(m)
    valid = mirror.valid()
    assert (m.leaves[valid] == 1.0).all() and m.leaves.sum() == len(valid) == m.total
    m.update_weight(*priorities(name))
    _assert_invariant(m)
    idx, w = priorities(name)
    assert m.max_prio == np.abs(w).max() + F32_EPS and m.min_prio == np.abs(w).min() + F32_EPS
    m.add(valid[:2])                                     # a push after an update takes the max_prio the update left
    assert (m.leaves[valid[:2]] == m.max_prio**ALPHA).all()
    _assert_invariant(m)
    m.reset()
    assert (m.tree == 0).all() and m.max_prio == 1.0 and m.min_prio == 1.0


def test_duplicate_indices_the_last_one_wins():
    m = PerModel(21, 0.5, 0.4)
    m.add(np.arange(21))
    m.update_weight([4, 9, 4, 4, 9], [9.0, 1.0, 0.25, 4.0, -16.0])
    assert m.leaves[4] == (4.0 + F32_EPS)**0.5 and m.leaves[9] == (16.0 + F32_EPS)**0.5
    assert m.max_prio == 16.0 + F32_EPS and m.min_prio == 0.25 + F32_EPS          # the extremes run over the losing entries too
    _assert_invariant(m)


def test_descent_is_the_prefix_sum_search():
    """integer leaves (sums exact): the descent lands on the first slot whose inclusive prefix sum reaches the scalar"""
    rng = np.random.default_rng(0)
    m = PerModel(21, 1.0, 0.4)
    leaves = rng.integers(0, 5, 21).astype(np.float64)
    leaves[[0, 20]] = 3.0
    m.load(leaves)
    cum = np.cumsum(leaves)
    scalar = np.concatenate([rng.uniform(0, cum[-1], 500), cum[:-1], cum[:-1] + 0.5, [1e-9]])
    want = np.searchsorted(cum, scalar, side="left")
    assert np.array_equal(m.descend(scalar), want)
    assert (leaves[want] > 0).all()


def test_weights_mix_leaf_and_raw_min_prio():
    m = PerModel(8, 0.5, 1.0, weight_norm=False)
    m.add(np.arange(8))
    m.update_weight([1, 2], [4.0 - F32_EPS, 0.25 - F32_EPS])
    w = m.weights([1, 2, 3])
    np.testing.assert_allclose(w, [(2.0 / 0.25)**-1.0, (0.5 / 0.25)**-1.0, (1.0 / 0.25)**-1.0], rtol=1e-6)
    m.weight_norm = True
    assert m.weights([1, 2, 3]).max() == 1.0


@pytest.mark.parametrize("name", sorted(STORES))
def test_gpu_inputs_land_on_filled_slots_only(name):
    """every (store, priorities, seed, update count, batch) the GPU tests sample with: the model's slots are filled ones, and no
    comparison of a descent is closer than 1e-9 of the root to a tie -- so a device leaf one ulp off numpy's pow cannot turn one"""
    for prio in (False, True):
        mirror, m = build(name, prio=prio)
        valid = mirror.valid()
        for seed in SAMPLER_SEEDS + (UPDATE_SEED, ):
            for counter in range(3):
                for B in SAMPLE_BATCHES:
                    slot, margin = m.sample(S.key_of(seed), counter, B, with_margin=True)
                    assert np.isin(slot, valid).all(), (prio, seed, counter, B)
                    assert margin.min() > 1e-9 * m.total, (prio, seed, counter, B, margin.min())


# ------------------------------------------------------------------------------------------------ one weighted update, restated
def _chains(index, indices, n_step):
    chain = [np.asarray(indices)]
    for _ in range(n_step - 1):
        chain.append(index.next(chain[-1]))
    chain = np.stack(chain)
    end_flag = index.done.copy()
    end_flag[index.unfinished_index()] = True
    return chain, end_flag


def _polyak(pairs, tau):
    with torch.no_grad():
        for tgt, src in pairs:
            for k in src:
                tgt[k].copy_(tau * src[k].data + (1 - tau) * tgt[k].data)


def weighted_sac_update(o: SACLagOracle, store, index: ReplayIndex, indices, eps_target, eps_pi, lagrangians, rescaling, w):
    """SACLagOracle.update with critics_loss's `weight` = w [B] (sac_lag.py:189-201) -> (stats_a, stats_c, td_average [B])"""
    cfg, B = o.cfg, len(indices)
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=o.dtype)  # noqa: E731
    chain, end_flag = _chains(index, indices, cfg.n_step)
    terminal = chain[-1]
    value_mask = (~np.asarray(store["terminated"], bool)[terminal]).reshape(-1, 1)
    with torch.no_grad():
        obs_n = t(store["obs_next"][terminal])
        a_n, logp_n = o.pi(obs_n, t(eps_target))
        targets = []
        for i in range(2):
            q1, q2 = o.q_pair(o.critics_old[i], obs_n, a_n)
            targets.append(torch.min(q1, q2) - o.alpha * logp_n)
    metrics = [np.asarray(store["rew"], np.float64), np.asarray(store["cost"]).astype(np.float64)]
    rets = [torch.from_numpy(nstep_return_np(metrics[i], end_flag, targets[i].reshape(B, -1).numpy() * value_mask, chain, cfg.gamma,
                                             cfg.n_step)).to(o.dtype) for i in range(2)]
    obs, act = t(store["obs"][indices]), t(store["act"][indices])
    weight = t(w)
    stats_c, loss_c, td_avg = {}, 0, 0
    for i in range(2):
        y = rets[i].flatten()
        q = o.q_pair(o.critics[i], obs, act)
        li = 0
        for j in range(2):
            td = q[j].flatten() - y
            td_avg = td_avg + td.detach()
            li = li + (td.pow(2) * weight).mean()
        loss_c = loss_c + li
        stats_c["loss/q" + str(i)] = li.item()
    td_avg = td_avg / 4
    o.critic_optim.zero_grad()
    loss_c.backward()
    o.critic_optim.step()
    stats_c["loss/q_total"] = loss_c.item()
    a_pi, logp = o.pi(obs, t(eps_pi))
    qr = o.q_pair(o.critics[0], obs, a_pi)
    loss_rew = (o.alpha * logp.flatten() - torch.min(qr[0], qr[1]).flatten()).mean()
    stats_a = {"loss/rescaling": rescaling}
    loss_safety = 0.0
    if cfg.use_lagrangian:
        qc = o.q_pair(o.critics[1], obs, a_pi)
        ls = torch.mean(torch.min(qc[0], qc[1]).flatten() * lagrangians[0])
        loss_safety = loss_safety + ls
        stats_a["loss/lagrangian"] = lagrangians[0]
        stats_a["loss/actor_safety"] = ls.item()
    loss_a = rescaling * (loss_rew + loss_safety)
    o.actor_optim.zero_grad()
    for cr in o.critics:
        for p in cr.values():
            p.grad = None
    loss_a.backward()
    o.actor_optim.step()
    if cfg.auto_alpha:
        alpha_loss = -(o.log_alpha * (logp.detach() + o.target_entropy)).mean()
        o.alpha_optim.zero_grad()
        alpha_loss.backward()
        o.alpha_optim.step()
        o.alpha = o.log_alpha.detach().exp()
        stats_a.update({"loss/alpha_loss": alpha_loss.item(), "loss/alpha_value": o.alpha.item()})
    stats_a.update({"loss/actor_rew": loss_rew.item(), "loss/actor_total": loss_a.item()})
    _polyak(zip(o.critics_old, o.critics), cfg.tau)
    return stats_a, stats_c, td_avg.numpy().copy()


def weighted_ddpg_update(o: DDPGLagOracle, store, index: ReplayIndex, indices, lagrangians, rescaling, w):
    """DDPGLagOracle.update with critics_loss's `weight` = w [B] (ddpg_lag.py:170-179) -> (stats_a, stats_c, td_average [B])"""
    cfg, B = o.cfg, len(indices)
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=o.dtype)  # noqa: E731
    chain, end_flag = _chains(index, indices, cfg.n_step)
    terminal = chain[-1]
    value_mask = (~np.asarray(store["terminated"], bool)[terminal]).reshape(-1, 1)
    with torch.no_grad():
        obs_n = t(store["obs_next"][terminal])
        a_n = o.pi(o.actor_old, obs_n)
        targets = [mlp(o.critics_old[i], torch.cat([obs_n, a_n], 1)) for i in range(2)]
    metrics = [np.asarray(store["rew"], np.float64), np.asarray(store["cost"]).astype(np.float64)]
    rets = [torch.from_numpy(nstep_return_np(metrics[i], end_flag, targets[i].reshape(B, -1).numpy() * value_mask, chain, cfg.gamma,
                                             cfg.n_step)).to(o.dtype) for i in range(2)]
    obs, act = t(store["obs"][indices]), t(store["act"][indices])
    x = torch.cat([obs, act], 1)
    weight = t(w)
    stats_c, loss_c, td_avg = {}, 0, 0
    for i in range(2):
        td = mlp(o.critics[i], x).flatten() - rets[i].flatten()
        td_avg = td_avg + td.detach()
        li = (td.pow(2) * weight).mean()
        loss_c = loss_c + li
        stats_c["loss/q" + str(i)] = li.item()
    td_avg = td_avg / 2
    o.critic_optim.zero_grad()
    loss_c.backward()
    o.critic_optim.step()
    stats_c["loss/q_total"] = loss_c.item()
    xa = torch.cat([obs, o.pi(o.actor, obs)], 1)
    loss_rew = -mlp(o.critics[0], xa).mean()
    stats_a = {"loss/rescaling": rescaling}
    loss_safety = 0.0
    if cfg.use_lagrangian:
        ls = torch.mean(mlp(o.critics[1], xa).mean() * lagrangians[0])
        loss_safety = loss_safety + ls
        stats_a["loss/lagrangian"] = lagrangians[0]
        stats_a["loss/actor_safety"] = ls.item()
    loss_a = rescaling * (loss_rew + loss_safety)
    o.actor_optim.zero_grad()
    for cr in o.critics:
        for p in cr.values():
            p.grad = None
    loss_a.backward()
    o.actor_optim.step()
    stats_a.update({"loss/actor_rew": loss_rew.item(), "loss/actor_total": loss_a.item()})
    _polyak([(o.actor_old, o.actor)] + list(zip(o.critics_old, o.critics)), cfg.tau)
    return stats_a, stats_c, td_avg.numpy().copy()


def make_oracle(kind, hidden, n_step, seed=0):
    """an oracle of `kind` (sac | ddpg) with seeded parameters -> (oracle, actor_flat, critics_flat)"""
    if kind == "sac":
        o = SACLagOracle(SACConfig(obs_dim=OBS_DIM, act_dim=ACT_DIM, hidden=tuple(hidden), gamma=0.98, n_step=n_step))
    else:
        o = DDPGLagOracle(DDPGConfig(obs_dim=OBS_DIM, act_dim=ACT_DIM, hidden=tuple(hidden), gamma=0.98, n_step=n_step))
    r = np.random.default_rng(seed)
    a = (0.3 * r.standard_normal(o.n_actor)).astype(np.float32)
    c = (0.3 * r.standard_normal(2 * o.n_critic)).astype(np.float32)
    o.set_params(a, c)
    return o, a, c


def oracle_store(mirror):
    return mirror.store(), ReplayIndex(None, mirror.sub, mirror.done, heads=mirror.book)


def restated_update(kind, o, store, index, idx, eps_t, eps_p, lag, resc, w):
    if kind == "sac":
        return weighted_sac_update(o, store, index, idx, eps_t, eps_p, lag, resc, w)
    return weighted_ddpg_update(o, store, index, idx, lag, resc, w)


@pytest.mark.parametrize("kind,hidden", [("sac", (64, 64)), ("sac", (32, 16, 8)), ("ddpg", (64, 64)), ("ddpg", (32, 16, 8))])
@pytest.mark.parametrize("name,n_step", [("p2_wrap", 2), ("np2_part", 1)])
def test_restatement_with_unit_weights_is_the_oracles_update(kind, hidden, name, n_step):
    torch.set_num_threads(1)
    mirror, _ = build(name)
    store, index = oracle_store(mirror)
    a, _, _ = make_oracle(kind, hidden, n_step)
    b, _, _ = make_oracle(kind, hidden, n_step)
    rng = np.random.default_rng(4)
    valid, B, lag, resc = mirror.valid(), 33, [0.5], 1 / 1.5
    for u in range(3):
        idx = rng.choice(valid, B)
        et, ep = rng.standard_normal((B, ACT_DIM)).astype(np.float32), rng.standard_normal((B, ACT_DIM)).astype(np.float32)
        if kind == "sac":
            sa, sc, _ = a.update(store, index, idx, et, ep, lag, resc)
        else:
            sa, sc, _ = a.update(store, index, idx, lag, resc)
        ra, rc, td = restated_update(kind, b, store, index, idx, et, ep, lag, resc, np.ones(B, np.float32))
        assert sa == ra and sc == rc
        assert td.dtype == np.float32 and td.shape == (B, ) and np.isfinite(td).all()
    assert np.array_equal(a.actor_flat(), b.actor_flat()) and np.array_equal(a.critics_flat(), b.critics_flat())
    assert np.array_equal(a.critics_flat(old=True), b.critics_flat(old=True))


def test_restated_weights_scale_the_loss_and_its_gradient():
    """w = c for every row scales each loss/q* by c; a row of weight 0 drops out of the critics' gradient"""
    torch.set_num_threads(1)
    mirror, _ = build("p2_wrap")
    store, index = oracle_store(mirror)
    rng = np.random.default_rng(6)
    valid, B = mirror.valid(), 16
    idx = rng.choice(valid, B)
    et, ep = rng.standard_normal((B, ACT_DIM)).astype(np.float32), rng.standard_normal((B, ACT_DIM)).astype(np.float32)
    outs = []
    for w in (np.ones(B, np.float32), np.full(B, 0.25, np.float32)):
        o, _, _ = make_oracle("sac", (64, 64), 2)
        _, sc, _ = weighted_sac_update(o, store, index, idx, et, ep, [0.5], 1 / 1.5, w)
        outs.append(sc)
    for k in outs[0]:
        assert abs(outs[1][k] - 0.25 * outs[0][k]) <= 1e-6 * abs(outs[0][k])


# ------------------------------------------------------------------------------------------------ the training state's PER section
def test_train_state_refuses_a_per_section_that_disagrees_with_the_context(tmp_path):
    """fsrl_amd/csrc/train_state.hpp as a stand-alone program (tests/host/per_state_sim.cpp, built with the address / undefined-
    behaviour sanitizers, nothing loaded into Python): a blob with the prioritised-replay section against a context without it,
    the reverse, and a section whose head, length or leaves are wrong"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "per_state_sim")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan", "-I" + os.path.join(root, "fsrl_amd", "csrc"),
           os.path.join(root, "tests", "host", "per_state_sim.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr
    oks = [ln.split()[1] for ln in out.stdout.splitlines() if ln.startswith("ok ")]
    assert oks == ["agree", "blob_has_context_has_not", "context_has_blob_has_not", "section"], out.stdout
    assert "ok section refused=%d" % (16 + 48) in out.stdout
