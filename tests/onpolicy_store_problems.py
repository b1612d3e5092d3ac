"""Scenarios for the on-policy store and process_fn on wrapped, re-cut and reset stores (tests/test_onpolicy_store_host.py on the
host, tests/test_gpu_onpolicy_store.py on the device).

A scenario is a seeded script of push / reset / configure calls.  `play` applies it to a mirror of the store kept by
tests/golden/ref_shim.VectorReplayBuffer (tianshou's index semantics, written independently of the library's store) and to any
engines passed in, and hands out, FROM THE MIRROR ALONE, after every stage of the script:

* the reference batch: oracle.ppo_lag.OnPolicyData in `buf.sample_indices(0)` order with
  end_flag = done[idx] | isin(idx, buf.unfinished_index())              (fsrl/policy/base_policy.py:409-411);
* the per-slot columns of the stored rows, the book (size, write head, slot written last) and the fill levels;
* the (ptr, ep_rew, ep_len, ep_idx) every add returned.

Only the buffer classes of ref_shim are used: nothing of the reference is imported, so the module runs on the GPU machine too.

Rollouts (`rollout`): per env a chain of observations (obs_next of a row is obs of the next one, a fresh draw after an episode
end), actions 0.3 N(0, 1), rewards N(0.5, 0.5), costs Bernoulli(0.2); `truncated` after every `ep` rows of an episode,
`terminated` by a seeded coin on the other rows.  Pushed in lock step the way FastCollector does (fast_collector.py:333), env e
taking rows[e] rows; the lagging env sits out every 7th step (as test_oracle_sampler.fill_flags), so the write heads differ.

Conditions every scenario meets (asserted by tests/test_onpolicy_store_host.py; the seeds were chosen on the host so they hold):

* it ends every stage in the book it states;
* terminated rows, truncated rows and unfinished tails are each present in the batch, at least 2 rows each where the geometry
  allows (TINY: 7 rows in the tiny_sub batch, one of each kind);
* sensitivity: the reference batch rebuilt with ONE defect moves the float64 oracle's advantages by at least 100 x the
  comparison bar.  Defect (a) reads every sub-buffer from slot 0 instead of from its write head; it changes the batch only where
  a sub-buffer has wrapped onto a head other than 0, and is asserted at those stages.  Defect (b) drops the unfinished-tail
  flags; it is asserted at every stage (every stage has unfinished tails);
* the fp32 oracle's process products lie within ONE TENTH of the comparison bar of the float64 oracle's.

The comparison bar: 5e-6 * max(1, max|x|) per array -- what the project uses for the same four arrays against the fp32 oracle
(tests/test_gpu_ppo.py, tests/test_gpu_shapes.py), here measured against float64."""
import numpy as np

from test_oracle_sampler import Mirror

BAR = 5e-6                       # x max(1, max|x|), per array
PRODUCTS = ("values", "advs", "rets", "logp_old")
RMS0 = np.array([[1.3, 4.0, 700.0], [0.2, 0.5, 700.0]])          # a non-trivial BasePolicy.ret_rms to start from
LAG, RESC = np.array([0.4]), 1 / 1.4
# CPO on the wrapped batch (tests/test_gpu_onpolicy_store.py): an episode cost of 25 against a limit of 10 -> the infeasible branch
CPO_KW = dict(target_kl=0.01, backtrack_coeff=0.8, damping_coeff=0.1, max_backtracks=10, optim_critic_iters=3, l2_reg=1e-3, cost_limit=10.0,
              lr=1e-3)
CPO_COST = 25.0
STAGE_CAP = 4096                 # rows of one staging window of the library (fsrl_ctx::STAGE_CAP)


def bar_of(x):
    return BAR * max(1.0, float(np.abs(np.asarray(x, np.float64)).max())) if np.size(x) else BAR


# ------------------------------------------------------------------------------------------------ the mirror
class StoreMirror(Mirror):
    """test_oracle_sampler.Mirror + what the on-policy half needs: the full return of add, reset, the sample(0) batch."""

    def add(self, ids, obs, act, rew, cost, term, trunc, nxt):
        term, trunc = np.asarray(term, bool), np.asarray(trunc, bool)
        return self.buf.add({"obs": np.asarray(obs, np.float32), "act": np.asarray(act, np.float32), "rew": np.asarray(rew, np.float64),
                             "terminated": term, "truncated": trunc, "done": term | trunc,
                             "obs_next": np.asarray(nxt, np.float32), "info.cost": np.asarray(cost, np.float64)}, list(ids))

    def reset(self, keep_statistics):
        self.buf.reset(keep_statistics)

    def indices(self):
        return np.asarray(self.buf.sample_indices(0), np.int64)

    def indices_from_slot0(self):
        """defect (a): every sub-buffer read from slot 0, not from its write head"""
        return self.valid().astype(np.int64)

    def wrapped(self):
        """sub-buffers that are full with a write head other than 0: where sample(0) order differs from slot order"""
        return np.array([n == self.sub and i != 0 for n, i, _ in self.book], bool)

    def batch(self, idx=None, tails=True):
        """OnPolicyData of the rows `idx` (default: sample_indices(0)); tails=False is defect (b)"""
        from oracle.ppo_lag import OnPolicyData
        idx = self.indices() if idx is None else idx
        if idx.size == 0:
            z = np.zeros
            return OnPolicyData(obs=z((0, self.Do), np.float32), act=z((0, self.Da), np.float32), rew=z(0), cost=z(0),
                                terminated=z(0, bool), truncated=z(0, bool), obs_next=z((0, self.Do), np.float32), end_flag=z(0, bool))
        st = self.store()
        end = self.done[idx].copy()
        if tails:
            end |= np.isin(idx, self.buf.unfinished_index())
        return OnPolicyData(obs=st["obs"][idx], act=st["act"][idx], rew=st["rew"][idx], cost=st["cost"][idx],
                            terminated=st["terminated"][idx], truncated=st["truncated"][idx], obs_next=st["obs_next"][idx],
                            end_flag=end)


class Stage:
    """what the mirror says after one stage of a script"""

    def __init__(self, name, m):
        self.name, self.sub, self.num = name, m.sub, m.E
        self.book, self.sizes, self.indices, self.valid = m.book, m.sizes, m.indices(), m.valid().astype(np.int64)
        self.wrapped = m.wrapped()
        self.batch = m.batch()
        self.batch_from_slot0 = m.batch(m.indices_from_slot0())
        self.batch_without_tails = m.batch(tails=False)
        self.unfinished = np.asarray(m.buf.unfinished_index(), np.int64)
        st = m.store() if self.valid.size else None
        self.columns = {k: st[k][self.valid] for k in st} if st else {}


# ------------------------------------------------------------------------------------------------ scenarios
class Scenario:
    """geometry + network + script.  script: a list of
         ("push", rows per env, lagging env)     a rollout continued from the scenario's one generator state (so episodes carry on)
         ("reset", keep_statistics)
         ("configure", total_size, buffer_num)
         ("refuse_push", env id) / ("refuse_configure", total_size, buffer_num)   the engines must refuse; the mirror is untouched
         ("stage", name, book the mirror must show)"""

    def __init__(self, E, sub, Do, Da, hidden, script, seed, n_critics=2, force_layered=False, ep=13, term_p=0.05, alloc=None):
        self.E, self.sub, self.Do, self.Da, self.hidden, self.script, self.seed = E, sub, Do, Da, tuple(hidden), script, seed
        self.n_critics, self.force_layered, self.ep, self.term_p = n_critics, force_layered, ep, term_p
        self.alloc = alloc or (E * sub, E)                   # (buffer_size, env_num) the engine allocates

    # ---- the networks
    def oracle(self, dtype=None, rew_norm=False):
        import torch
        from oracle.ppo_lag import PPOLagConfig, PPOLagOracle
        o = PPOLagOracle(PPOLagConfig(obs_dim=self.Do, act_dim=self.Da, hidden=self.hidden, n_critics=self.n_critics, max_grad_norm=0.5,
                                      target_kl=1e9, max_action=1.5, reward_normalization=rew_norm), dtype=dtype or torch.float32)
        o.set_params(self.theta0(o.n_params))
        if rew_norm:
            o.ret_rms[:] = RMS0[:self.n_critics]
        return o

    def theta0(self, n):
        return (0.15 * np.random.default_rng(1000 + self.seed).standard_normal(n)).astype(np.float32)

    def engine(self, rew_norm=False, start=True, **over):
        from fsrl_amd.engine import Engine, EngineConfig
        kw = dict(obs_dim=self.Do, act_dim=self.Da, hidden_sizes=self.hidden, force_layered=self.force_layered, n_critics=self.n_critics,
                  env_num=self.alloc[1], buffer_size=self.alloc[0], max_grad_norm=0.5, target_kl=None, max_action=1.5, rew_norm=rew_norm)
        kw.update(over)
        eng = Engine(EngineConfig(**kw))
        if start:
            self.start(eng)
        return eng

    def start(self, eng):
        """theta0, a fresh optimiser and, with reward normalisation, RMS0"""
        eng.set_params(self.theta0(eng.n_params))
        eng.optim_reset()
        if eng.cfg.rew_norm:
            eng.ret_rms_set(RMS0[:self.n_critics])

    def lagrangians(self):
        return (LAG, RESC) if self.n_critics == 2 else (np.zeros(0), 1.0)

    # ---- the script
    def play(self, engines=(), on_push=None, on_stage=None, on_refuse=None):
        """Run the script on a fresh mirror and on `engines`.  on_push(engine returns [per engine], the mirror's add return),
        on_stage(Stage, mirror), on_refuse(op) are called as the script goes.  -> (stages, every add return of the mirror)"""
        m = StoreMirror(self.alloc[1], -(-self.alloc[0] // self.alloc[1]), self.Do, self.Da)
        stages, adds, n_roll = [], [], 0
        carry = None                   # the rollout generator's state across pushes: episodes carry on over a reset
        for op in self.script:
            if op[0] == "push":
                _, rows, lag_env = op
                steps, carry = rollout(self.seed, n_roll, carry, rows, self.Do, self.Da, lag_env, self.ep, self.term_p)
                n_roll += 1
                for step in steps:
                    want = m.add(*step)
                    adds.append(want)
                    got = [eng.push(*step) for eng in engines]
                    if on_push is not None:
                        on_push(got, want)
            elif op[0] == "reset":
                m.reset(op[1])
                for eng in engines:
                    eng.reset_store(op[1])
            elif op[0] == "configure":
                _, total, num = op
                m = StoreMirror(num, -(-total // num), self.Do, self.Da)
                for eng in engines:
                    eng.store_configure(total, num)
                carry = None
            elif op[0] in ("refuse_push", "refuse_configure"):
                if on_refuse is not None:
                    on_refuse(op)
            elif op[0] == "stage":
                s = Stage(op[1], m)
                s.want_book = np.array(op[2], np.int64)
                stages.append(s)
                if on_stage is not None:
                    on_stage(s, m)
            else:
                raise ValueError(op)
        return stages, adds


def rollout(seed, n_roll, carry, rows, Do, Da, lag_env, ep, term_p):
    """push number n_roll of a script -> ([(ids, obs, act, rew, cost, terminated, truncated, obs_next)] vector steps, carry).  Env e
    contributes rows[e] rows; the envs continue where the previous push left them (`carry`: observation and episode age), so an
    episode in flight at a reset goes on after it"""
    rng = np.random.default_rng([seed, n_roll])
    E = len(rows)
    left = np.array(rows, np.int64)
    if carry is None or len(carry[0]) != E:
        carry = (rng.standard_normal((E, Do)).astype(np.float32), np.zeros(E, np.int64))
    cur, age = carry[0].copy(), carry[1].copy()
    out, t = [], 0
    while (left > 0).any():
        ids = [e for e in range(E) if left[e] > 0 and not (e == lag_env and t % 7 == 0)]
        t += 1
        if not ids:
            continue
        k = len(ids)
        obs = cur[ids].copy()
        nxt = rng.standard_normal((k, Do)).astype(np.float32)
        act = (0.3 * rng.standard_normal((k, Da))).astype(np.float32)
        rew = rng.normal(0.5, 0.5, k)
        cost = (rng.random(k) < 0.2).astype(np.float64)
        age[ids] += 1
        trunc = age[ids] >= ep
        term = (rng.random(k) < term_p) & ~trunc
        out.append((ids, obs, act, rew, cost, term, trunc, nxt))
        cur[ids] = nxt
        for j, e in enumerate(ids):
            if term[j] or trunc[j]:
                cur[e] = rng.standard_normal(Do).astype(np.float32)
                age[e] = 0
        left[ids] -= 1
    return out, (cur, age)


def _wrapped(hidden, seed=1, **kw):
    # E=3, sub=40, rows 100 / 86 / 93, env 1 lags: three write heads in the middle of their slot ranges, ~2.5 times round
    return Scenario(3, 40, 7, 3, hidden, [("push", [100, 86, 93], 1), ("stage", "wrapped", [[40, 20, 19], [40, 6, 5], [40, 13, 12]])],
                    seed, **kw)


def _reset(keep):
    # 50 rows per env, an update, reset(keep_statistics), 30 rows per env: episodes of 20 rows straddle the reset in every env
    return Scenario(3, 64, 6, 2, (64, 64), [("push", [50, 50, 50], 2), ("stage", "before", [[50, 50, 49]] * 3), ("reset", keep),
                                            ("stage", "emptied", [[0, 0, 0]] * 3),
                                            ("push", [30, 30, 30], 2), ("stage", "after", [[30, 30, 29]] * 3)], 2, ep=20, term_p=0.03)


SCENARIOS = {
    "wrapped_ragged": _wrapped((64, 64)),
    # a full sub-buffer with index 0 beside one with index 1
    "one_over": Scenario(2, 16, 12, 16, (128, 128), [("push", [16, 17], None), ("stage", "over", [[16, 0, 15], [16, 1, 0]])], 2, ep=5,
                         term_p=0.15),
    # the `staged == sub_size` flush, ~16 times with no update in between; an empty sub-buffer
    "tiny_sub": Scenario(4, 3, 3, 1, (64, 64), [("push", [50, 3, 1, 0], None),
                                                ("stage", "tiny", [[3, 2, 1], [3, 0, 2], [1, 1, 0], [0, 0, 0]])], 1, ep=4, term_p=0.2),
    # 8 400 rows, 59 or 60 per push: both window switches fall inside a push call; the second one waits on the first window
    "windows": Scenario(60, 160, 5, 2, (64, 64), [("push", [140] * 60, 7), ("stage", "windows", [[140, 140, 139]] * 60)], 1),
    "reset_keep": _reset(True),
    "reset_drop": _reset(False),
    # engine with env_num=4, buffer_size=400: three sub-buffers of 130, then of 3 (wrapped), then four of 100
    "recut": Scenario(3, 130, 4, 2, (64, 64), [
        ("configure", 390, 3), ("stage", "cut_130_empty", [[0, 0, 0]] * 3),
        ("push", [40, 33, 37], 1), ("stage", "cut_130", [[40, 40, 39], [33, 33, 32], [37, 37, 36]]),
        ("refuse_push", 3), ("refuse_configure", 406, 3), ("refuse_configure", 400, 5),
        ("configure", 7, 3), ("stage", "cut_3_empty", [[0, 0, 0]] * 3),
        ("push", [8, 7, 4], 1), ("stage", "cut_3", [[3, 2, 1], [3, 1, 0], [3, 1, 0]]),
        ("refuse_push", 3),
        ("configure", 400, 4), ("push", [30, 25, 28, 27], 2),
        ("stage", "cut_100", [[30, 30, 29], [25, 25, 24], [28, 28, 27], [27, 27, 26]])], 2, ep=6, term_p=0.1, alloc=(400, 4)),
    "layered_wrapped": _wrapped((40, 24, 56)),
    "one_critic": _wrapped((64, 64), n_critics=1),
    "one_critic_layered": _wrapped((40, 24), n_critics=1, force_layered=True),
}


# wrapped_ragged's geometry and network with no sub-buffer wrapped (113 rows: as many 16-row tiles as wrapped_ragged's 120)
UNWRAPPED = Scenario(3, 40, 7, 3, (64, 64), [("push", [39, 36, 38], 1), ("stage", "plain", [[39, 39, 38], [36, 36, 35], [38, 38, 37]])], 3)


def push_offsets(steps):
    """rows pushed before each vector step and after the last: where the staging windows (STAGE_CAP rows) switch"""
    return np.concatenate([[0], np.cumsum([len(s[0]) for s in steps])])
