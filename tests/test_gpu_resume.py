"""The engine's full training state through Engine.train_state / load_train_state / copy_train_state_from (fsrl_train_state_*) and
learn(resume=True) on top of it: a context that imports another's state continues EXACTLY as that one does -- parameters, logged
rows, drawn actions and sampled indices bit for bit -- for every algorithm, fused and layered; the store travels with its
sub-buffer books; refused blobs change nothing; a resident actor is ended and relaunched; group members move between groups.

Shapes: obs 8, act 2, fused width 64, layered (64, 48, 32); on-policy 2 envs x 75 vector steps, minibatches of 64, 2 passes; replay
stores of 4 sub-buffers x 50 rows, batch 32."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

Do, Da = 8, 2
LAYERED = (64, 48, 32)
ONPOLICY = ("ppo", "ppo_layered", "focops", "cpo", "trpo_layered")
REPLAY = ("sac", "sac_layered", "ddpg", "cvpo")


def _engine(kind, theta_seed):
    """a context of `kind` with its *_init done and parameters drawn from theta_seed"""
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig
    hs = LAYERED if kind.endswith("_layered") else (64, 64)
    rng = np.random.default_rng(theta_seed)
    base = kind.split("_")[0]
    if kind in ONPOLICY:
        algo = {"ppo": _lib.ALGO_PPO_LAG, "focops": _lib.ALGO_FOCOPS, "cpo": _lib.ALGO_CPO, "trpo": _lib.ALGO_TRPO_LAG}[base]
        kw = dict(rew_norm=True, max_grad_norm=0.5) if base == "ppo" else dict(target_kl=None) if base in ("cpo", "trpo") else {}
        eng = Engine(EngineConfig(algo=algo, obs_dim=Do, act_dim=Da, hidden_sizes=hs, env_num=2, buffer_size=150, lr=1e-3, **kw))
        if base == "focops":
            eng.focops_init()
        eng.set_params((0.2 * rng.standard_normal(eng.n_params)).astype(np.float32))
        return eng
    eng = Engine(EngineConfig(algo=_lib.ALGO_SAC_LAG, obs_dim=Do, act_dim=Da, hidden_sizes=hs, env_num=4, buffer_size=200, target_kl=None))
    if base == "cvpo":
        eng.cvpo_init(qc_thres=0.4, sample_act_num=8)
    else:
        eng.sac_init(auto_alpha=True, n_step=2, deterministic=base == "ddpg")
    eng.sac_set_params((0.2 * rng.standard_normal(eng.n_sac_actor)).astype(np.float32),
                       (0.2 * rng.standard_normal(eng.n_sac_critics)).astype(np.float32), 0.1)
    return eng


def _steps(seed, n, env_num, open_end=False):
    """n lock-step vector steps of random transitions; an episode ends every 25 steps (not at the very end if open_end)"""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(n):
        done = (t % 25 == 24) and not (open_end and t == n - 1)
        out.append((np.arange(env_num), rng.standard_normal((env_num, Do)).astype(np.float32),
                    np.tanh(rng.standard_normal((env_num, Da))).astype(np.float32), rng.normal(0.5, 0.5, env_num),
                    (rng.random(env_num) < 0.2).astype(np.float64), np.full(env_num, done and t % 50 == 24), np.full(env_num, done and t % 50 != 24),
                    rng.standard_normal((env_num, Do)).astype(np.float32)))
    return out


def _push(eng, steps):
    for s in steps:
        eng.push(*s)


def _update(eng, kind, first=False):
    """one update of the kind -> everything it logs, as bytes-comparable arrays"""
    base = kind.split("_")[0]
    if base == "ppo":
        stats, stopped = eng.ppo_update([0.3], 0.8, 64, 2, perms=None)
        return [stats, np.array([stopped])]
    if base == "focops":
        stats, stopped = eng.focops_update(0.2, 0.1, 64, 2, perms=None)
        return [stats, np.array([stopped])]
    if base in ("cpo", "trpo"):
        eng.tr_begin(target_kl=0.01, critic_lr=1e-3, optim_critic_iters=3, l2_reg=0.001, cost_limit=5.0)
        return [eng.cpo_learn(12.0, 2, batch_size=64) if base == "cpo" else eng.trpo_learn([0.3], 0.8, 2, batch_size=64)]
    seed = 7 if first else 0                                        # the Philox stream is keyed once; afterwards the key is state
    if base == "cvpo":
        eng.cvpo_pre_update()
        row = eng.cvpo_update(32, seed=seed)
        eng.cvpo_post_update()
        return [row, eng.cvpo_duals(), *eng.sac_last_sample(32), eng.cvpo_last_particles(32)]
    row = eng.sac_update(32, [0.3], 0.8, seed=seed)
    return [row, *eng.sac_last_sample(32)]                          # the sampled indices and both noise blocks


def _params(eng, kind):
    if kind in ONPOLICY:
        out = [eng.get_params()]
        if kind.startswith("ppo"):
            out.append(eng.ret_rms_get())
        return out
    which = (0, 1, 2) if kind.startswith("sac") else (0, 1, 2, 3)
    return [x for w in which for x in (eng.sac_get_params(w)[0], np.array([eng.sac_get_params(w)[1]]))]


def _collect(eng, seed, n, env_num):
    """n collect_step calls with device noise, each storing the previous step's transition -> the drawn actions"""
    steps = _steps(seed, n, env_num)
    acts, prev = [], None
    for s in steps:
        act, env_act, _, _ = eng.collect_step(prev, s[1], deterministic=False, bound_method=1)
        acts += [act, env_act]
        prev = s
    eng.collect_step(prev, None)
    return acts


def _warm_up(eng, kind):
    """pushes, two updates, a few collect_steps -> the blob taken after the FIRST update (one update early) for the negative check"""
    n_env = eng.cfg.env_num
    early = None
    for i in range(2):
        if kind in ONPOLICY:
            eng.reset_store(keep_statistics=True)
            _push(eng, _steps(100 + i, 75, n_env))
        else:
            _push(eng, _steps(100 + i, 30, n_env))
        _update(eng, kind, first=i == 0)
        if i == 0:
            early = eng.train_state()
    if kind in ONPOLICY:
        eng.reset_store(keep_statistics=True)
    _collect(eng, 200, 3, n_env)
    return early


def _continuation(eng, kind):
    """more collect_steps, pushes, two updates -> every observable result"""
    n_env = eng.cfg.env_num
    out = _collect(eng, 300, 3, n_env)
    for i in range(2):
        _push(eng, _steps(400 + i, 69 if kind in ONPOLICY else 30, n_env, open_end=True))       # on-policy: inside the sub-buffer's 75 rows
        out += _update(eng, kind)
        if kind in ONPOLICY:
            eng.reset_store(keep_statistics=True)
    out += _collect(eng, 500, 2, n_env)
    return out + _params(eng, kind)


def _differ(a, b):
    """indices of the entries of two result lists that are not equal bit for bit (dtype included)"""
    if len(a) != len(b):
        return [-1]
    return [i for i, (x, y) in enumerate(zip(a, b))
            if np.asarray(x).dtype != np.asarray(y).dtype or np.asarray(x).tobytes() != np.asarray(y).tobytes()]


def _same(a, b):
    return not _differ(a, b)


@pytest.mark.parametrize("kind", ONPOLICY + REPLAY)
def test_an_imported_state_continues_exactly(kind):
    a = _engine(kind, 1)
    early = _warm_up(a, kind)
    blob = a.train_state()
    assert a.train_state() == blob and blob != early                       # a pure function of the state; an update moved it
    want = _continuation(a, kind)
    b = _engine(kind, 2)                                                   # same configuration, other parameters
    b.load_train_state(blob)
    assert b.train_state() == blob                                         # export(import(b)) == b, byte for byte
    got = _continuation(b, kind)
    assert _same(got, want), _differ(got, want)
    assert b.train_state() == a.train_state()
    # the comparison can fail: without the import, and from a state one update early, the continuation differs
    c = _engine(kind, 2)
    assert not _same(_continuation(c, kind), want)
    c.load_train_state(early)
    assert c.train_state() == early
    assert not _same(_continuation(c, kind), want)
    # a blob without the store carries the same learner state (the continuation above needs the store: not run here)
    lean = a.train_state(with_store=False)
    assert len(lean) < len(a.train_state()) and a.train_state(with_store=False) == lean
    c.load_train_state(lean)
    assert c.train_state(with_store=False) == lean
    for e in (a, b, c):
        e.close()


def _uneven_store(eng, seed):
    """sub-buffer 0 wrapped past its 50 rows (70 pushed), 1 empty, 2 with an episode in progress (20 rows, 5 into an episode),
    3 exactly full.  -> the rewards of sub-buffer 2's open episode"""
    rng = np.random.default_rng(seed)
    rows = {0: 70, 2: 20, 3: 50}
    open_rew = []
    for t in range(70):
        ids = np.array([e for e, n in rows.items() if t < n])
        k = len(ids)
        rew = rng.normal(0.5, 0.5, k)
        done = np.array([(t + 1) % 15 == 0 or (e == 3 and t == 49) for e in ids])
        eng.push(ids, rng.standard_normal((k, Do)).astype(np.float32), np.tanh(rng.standard_normal((k, Da))).astype(np.float32), rew,
                 (rng.random(k) < 0.2).astype(np.float64), done & (t % 2 == 0), done & (t % 2 == 1),
                 rng.standard_normal((k, Do)).astype(np.float32))
        if 2 in ids and t >= 15:
            open_rew.append(float(rew[list(ids).index(2)]))
    return open_rew


def _store_view(eng):
    idx = eng.sample0()
    rows = eng.store_read(idx)
    return [idx, eng.store_sizes(), np.array(eng.store_geometry()), np.array([len(eng)])] + [rows[k] for k in sorted(rows)]


def test_the_store_travels_with_its_books():
    a, b, c = _engine("sac", 1), _engine("sac", 2), _engine("sac", 3)
    open_rew = _uneven_store(a, 11)
    assert list(a.store_sizes()) == [50, 0, 20, 50] and len(open_rew) == 5
    _push(b, _steps(12, 7, 4))                                             # rows of its own, to be replaced
    blob = a.train_state()
    b.load_train_state(blob)
    assert b.train_state() == blob
    assert _same(_store_view(b), _store_view(a))
    assert np.array_equal(a.sample0()[:50], np.concatenate([np.arange(20, 50), np.arange(20)]))     # sub-buffer 0 starts at its write head
    # the rest of the open episode: same return and length in both, and they count the rows pushed before the export
    rng = np.random.default_rng(13)
    for t in range(3):
        row = (np.array([2]), rng.standard_normal((1, Do)).astype(np.float32), np.zeros((1, Da), np.float32), np.array([0.25 * (t + 1)]),
               np.zeros(1), np.array([False]), np.array([t == 2]), rng.standard_normal((1, Do)).astype(np.float32))
        ra, rb = a.push(*row), b.push(*row)
        assert _same(list(ra), list(rb))
    assert rb[2][0] == 8 and rb[1][0] == pytest.approx(sum(open_rew) + 0.25 + 0.5 + 0.75, abs=1e-12) and rb[3][0] == 2 * 50 + 15
    assert _same(_store_view(b), _store_view(a))
    # one update from the same state over the imported store: the same sample, the same result
    assert _same(_update(a, "sac", first=True) + _params(a, "sac"), _update(b, "sac", first=True) + _params(b, "sac"))
    # a blob without the store leaves the importing context's store as it was
    _push(c, _steps(14, 9, 4, open_end=True))
    before = _store_view(c)
    c.load_train_state(a.train_state(with_store=False))
    assert _same(_store_view(c), before)
    assert _same(_params(c, "sac"), _params(a, "sac"))
    for e in (a, b, c):
        e.close()


def test_refused_imports_leave_the_context_as_it_was():
    from fsrl_amd._lib import FsrlHipError
    from fsrl_amd.engine import Engine, EngineConfig
    a = _engine("ppo", 1)
    _push(a, _steps(1, 75, 2))
    _update(a, "ppo")
    before = a.train_state()
    other = _engine("ppo", 2).train_state()
    # inside an update: the state error, for import and export alike
    a.ppo_begin([0.3], 0.8, 64)
    with pytest.raises(FsrlHipError, match=r"\[-1\].*inside an update"):
        a.load_train_state(other)
    with pytest.raises(FsrlHipError, match=r"\[-1\].*inside an update"):
        a.train_state()
    a.ppo_abort()
    ref = _engine("ppo", 3)                     # fsrl_ppo_begin itself moves state (the running return statistics): the twin begins too
    ref.load_train_state(before)
    ref.ppo_begin([0.3], 0.8, 64)
    ref.ppo_abort()
    assert a.train_state() == ref.train_state() != before
    before = a.train_state()
    # another width: the field is named with both values
    wide = Engine(EngineConfig(obs_dim=Do, act_dim=Da, hidden_sizes=(48, 64), env_num=2, buffer_size=150, lr=1e-3, rew_norm=True,
                               max_grad_norm=0.5))
    with pytest.raises(AssertionError, match=r"hidden_sizes\[0\] differs: the blob has 48, this context 64"):
        a.load_train_state(wide.train_state())
    assert a.train_state() == before
    layered = _engine("ppo_layered", 1)
    with pytest.raises(AssertionError, match=r"layered differs: the blob has 1, this context 0"):
        a.load_train_state(layered.train_state())
    assert a.train_state() == before
    # truncated, extended, one flipped bit in a payload, not a blob at all
    bad = bytearray(other)
    bad[len(bad) // 2] ^= 0x10
    for blob, why in ((other[:-8], "checksum"), (other[:len(other) // 2], "checksum|multiple of 8"), (other + b"\0" * 8, "checksum"),
                      (bytes(bad), "checksum"), (b"", "too few"), (b"not a training state" * 40, "magic")):
        with pytest.raises(AssertionError, match=why):
            a.load_train_state(blob)
        assert a.train_state() == before
    # and the state still works: the next update is its twin's
    t = _engine("ppo", 3)
    t.load_train_state(before)
    assert _same(_update(a, "ppo") + _params(a, "ppo"), _update(t, "ppo") + _params(t, "ppo"))
    for e in (a, t, ref, wide, layered):
        e.close()


def test_export_and_import_end_a_resident_actor_and_the_next_step_relaunches_it():
    a, twin, src = _engine("ppo", 1), _engine("ppo", 1), _engine("ppo", 1)
    rng = np.random.default_rng(5)
    obs = [rng.standard_normal((2, Do)).astype(np.float32) for _ in range(4)]
    for e in (a, twin):
        e.actor_set_resident(True)
    act1, _, _, _ = a.collect_step(None, obs[0])
    assert a.actor_resident_stats()["live"]
    blob = a.train_state()                                                 # holds the noise stream as it stands after one step
    assert not a.actor_resident_stats()["live"]
    a.collect_step(None, obs[1])
    launches = a.actor_resident_stats()["launches"]
    assert a.actor_resident_stats()["live"] and launches == 2
    a.load_train_state(blob)
    assert not a.actor_resident_stats()["live"]
    act3, _, _, _ = a.collect_step(None, obs[2])
    assert a.actor_resident_stats()["live"] and a.actor_resident_stats()["launches"] == launches + 1
    t1, _, _, _ = twin.collect_step(None, obs[0])
    t3, _, _, _ = twin.collect_step(None, obs[2])                          # the twin never drew for obs[1]: the import rewound that draw
    assert _same([act1, act3], [t1, t3])
    # imported PARAMETERS reach the relaunched kernel (it held the old ones in registers)
    src.set_params((0.3 * rng.standard_normal(src.n_params)).astype(np.float32))
    a.load_train_state(src.train_state())
    act4, _, _, _ = a.collect_step(None, obs[3])
    s4, _, _, _ = src.collect_step(None, obs[3])
    assert _same([act4], [s4]) and not _same([act4], [twin.collect_step(None, obs[3])[0]])
    for e in (a, twin, src):
        e.actor_release()
        e.close()


def test_group_members_move_into_a_fresh_group_between_two_grouped_updates():
    from fsrl_amd.engine import EngineGroup
    first = [_engine("ppo_layered", 10 + i) for i in range(3)]
    g1 = EngineGroup(first)
    for i, e in enumerate(first):
        _push(e, _steps(20 + i, 75, 2))
    lags, resc = [[0.3], [0.1], [0.0]], [0.8, 0.9, 1.0]
    g1.ppo_update(lags, resc, 64, 2, perms=None)
    blobs = [e.train_state() for e in first]                               # members export between grouped calls
    want = g1.ppo_update(lags, resc, 64, 2, perms=None)
    second = [_engine("ppo_layered", 30 + i) for i in range(3)]
    g2 = EngineGroup(second)
    for e, blob in zip(second, blobs):
        e.load_train_state(blob)
        assert e.train_state() == blob
    got = g2.ppo_update(lags, resc, 64, 2, perms=None)
    for i in range(3):
        assert _same([got[0][i], np.array(got[1][i])], [want[0][i], np.array(want[1][i])])
        assert _same(_params(second[i], "ppo"), _params(first[i], "ppo"))
        assert second[i].train_state() == first[i].train_state()
    g1.close(); g2.close()
    for e in first + second:
        e.close()


@pytest.mark.parametrize("kind", ("sac", "trpo_layered"))
def test_copy_between_two_contexts_on_one_device(kind):
    a, b = _engine(kind, 1), _engine(kind, 2)
    _warm_up(a, kind)
    blob = a.train_state()
    b.copy_train_state_from(a)
    assert a.train_state() == blob and b.train_state() == blob             # the source is unchanged, the copy is complete
    assert _same(_continuation(b, kind), _continuation(a, kind))
    other = _engine("ddpg" if kind == "sac" else "cpo", 3)
    with pytest.raises(AssertionError, match="differs: the source has"):
        other.copy_train_state_from(a)
    with pytest.raises(AssertionError, match="onto itself"):
        a.copy_train_state_from(a)
    for e in (a, b, other):
        e.close()


@pytest.mark.parametrize("algo", ("ppo", "sac"))
def test_learn_resume_continues_the_run(algo, tmp_path, monkeypatch):
    import torch
    from fsrl_amd.agent import PPOLagAgent, SACLagAgent
    from fsrl_amd.env import SyntheticSafetyVectorEnv
    from fsrl_amd.trainer.base_trainer import BaseTrainer
    from fsrl_amd.utils import BaseLogger

    def agent_and_learn(seed, env_seed, **lk):
        env = SyntheticSafetyVectorEnv(env_num=4, episode_len=25, seed=env_seed)
        logger = BaseLogger(str(tmp_path), name="run")
        if algo == "ppo":
            agent = PPOLagAgent(env, logger, cost_limit=10, device="cuda:0", seed=seed, hidden_sizes=(64, 64), training_num=4)
            return agent, agent.learn(env, None, episode_per_collect=4, step_per_epoch=200, repeat_per_collect=2, batch_size=64,
                                      save_interval=1, verbose=False, device_actor=True, **lk)
        agent = SACLagAgent(env, logger, cost_limit=10, device="cuda:0", seed=seed, hidden_sizes=(64, 64), training_num=4, buffer_size=200)
        return agent, agent.learn(env, None, episode_per_collect=4, step_per_epoch=200, update_per_step=0.1, batch_size=32,
                                  save_interval=1, verbose=False, device_actor=True, **lk)

    epochs, seen = [], {}
    nxt = BaseTrainer.__next__
    monkeypatch.setattr(BaseTrainer, "__next__", lambda self: (lambda out: (epochs.append(out[0]), out)[1])(nxt(self)))
    # fires when the saved state has just been loaded, before the first collect
    monkeypatch.setattr(BaseTrainer, "on_resumed", lambda self, state: seen.update(
        saved=state, blob=self.policy.engine.train_state(True), epoch=self.epoch, env_step=self.env_step, best=self.best_perf_rew,
        cum=(self.cum_cost, self.cum_episode), gsteps=self.policy.gradient_steps, lag=self.policy.lagrangians_and_rescaling()))
    a1, (ep1, _, info1) = agent_and_learn(3, 1, epoch=2)
    assert ep1 == 2 and epochs == [1, 2] and not seen
    path = os.path.join(str(tmp_path), "run", "checkpoint", "train_state.pt")
    saved = torch.load(path, weights_only=False)
    assert saved["trainer"]["epoch"] == 2 and saved["trainer"]["env_step"] >= 400
    model = torch.load(os.path.join(str(tmp_path), "run", "checkpoint", "model.pt"), weights_only=False)
    assert list(model) == ["model"] and list(model["model"]) == list(a1.policy.state_dict())
    del epochs[:]
    a2, (ep2, _, info2) = agent_and_learn(4, 2, epoch=4, resume=True)      # another seed, a fresh env, the same log_dir
    assert epochs == [3, 4] and ep2 == 4
    assert seen["epoch"] == 2 and seen["env_step"] == saved["trainer"]["env_step"] and seen["best"] == saved["trainer"]["best_reward"]
    assert seen["cum"] == (saved["trainer"]["cum_cost"], saved["trainer"]["cum_episode"])
    assert seen["gsteps"] == saved["policy"]["gradient_steps"] == a1.policy.gradient_steps
    assert seen["lag"] == a1.policy.lagrangians_and_rescaling()
    assert seen["blob"] == bytes(saved["policy"]["engine"].numpy().tobytes())       # the engine holds the saved state, byte for byte
    assert seen["blob"] == a1.policy.engine.train_state(True)                       # ... which is where the first run stopped
    assert info2["best_reward"] >= saved["trainer"]["best_reward"]
    lines = open(os.path.join(str(tmp_path), "run", "progress.txt")).read().splitlines()
    assert sum(ln.startswith("Steps\t") for ln in lines) == 1
    steps = [int(ln.split("\t")[0]) for ln in lines[1:]]
    assert len(steps) == 4 and all(x < y for x, y in zip(steps, steps[1:])) and steps[1] == saved["trainer"]["env_step"]
    for a in (a1, a2):
        a.policy.engine.close()
