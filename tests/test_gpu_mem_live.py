"""Nothing leaks: every device and pinned block the library allocates goes through one owner (fsrl_amd/csrc/dev_mem.hpp), and
fsrl_mem_live reads the process-wide counters at that choke point.  Every case takes the counters as its baseline (suites create
engines before it), builds one kind of object, runs the steps that reach its allocations -- first use, a regrow, the optional
buffers -- asserts that the counters stood ABOVE the baseline while the objects lived, closes everything explicitly, and asserts
that all four counters are back at the baseline exactly.  Shapes are the smallest that reach every allocation: obs_dim 6, act_dim 2,
hidden 64, 2 envs, a store of 256 rows, batch 32 (and 96: the regrow)."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F32 = np.float32
DO, DA, H, ENVS, ROWS, B, B2 = 6, 2, 64, 2, 256, 32, 96
LAYERED = (24, 17, 32)


def live():
    """the counters with no garbage behind them: an engine that an earlier test left unclosed in a reference cycle is freed here,
    not between a case's baseline and its last reading"""
    from fsrl_amd.engine import mem_live
    gc.collect()
    return mem_live()


def back_at(base, *closed):
    """everything is closed: the four counters are the baseline's, exactly"""
    del closed
    gc.collect()
    now = live()
    assert now == base, (now, base)


def above(base):
    now = live()
    assert now["dev_blocks"] > base["dev_blocks"] and now["dev_bytes"] > base["dev_bytes"], (now, base)
    assert now["pinned_blocks"] > base["pinned_blocks"] and now["pinned_bytes"] > base["pinned_bytes"], (now, base)
    return now


def engine(algo=None, hidden_sizes=None, seed=0, **kw):
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig
    cfg = dict(obs_dim=DO, act_dim=DA, env_num=ENVS, buffer_size=ROWS, n_critics=2, target_kl=None)
    cfg.update(hidden_sizes=hidden_sizes) if hidden_sizes else cfg.update(hidden=H)
    if algo is not None:
        cfg["algo"] = getattr(_lib, algo)
    cfg.update(kw)
    eng = Engine(EngineConfig(**cfg), device=0)
    if algo != "ALGO_SAC_LAG":
        eng.set_params((0.2 * np.random.default_rng(seed).standard_normal(eng.n_params)).astype(F32))
    return eng


def replay_params(eng, seed=0):
    rng = np.random.default_rng(50 + seed)
    eng.sac_set_params((0.2 * rng.standard_normal(eng.n_sac_actor)).astype(F32), (0.2 * rng.standard_normal(eng.n_sac_critics)).astype(F32))


def fill(eng, steps=60, seed=0, ep=10):
    """`steps` vector steps of both envs, an episode end every `ep` steps: 120 rows, twelve finished episodes"""
    rng = np.random.default_rng(seed)
    ids = np.arange(ENVS)
    obs = rng.standard_normal((ENVS, DO)).astype(F32)
    for t in range(steps):
        nxt = rng.standard_normal((ENVS, DO)).astype(F32)
        end = np.full(ENVS, (t + 1) % ep == 0)
        eng.push(ids, obs, rng.uniform(-1, 1, (ENVS, DA)).astype(F32), rng.standard_normal(ENVS), rng.uniform(0, 1, ENVS),
                 end & (t % 20 < 10), end & (t % 20 >= 10), nxt)
        obs = nxt


def finite(x):
    assert np.isfinite(np.asarray(x, np.float64)).all()


# ------------------------------------------------------------------------------------------------ on-policy contexts
def onpolicy_steps(eng, update):
    fill(eng)
    update(B)
    update(B2)          # the minibatch working set regrows
    eng.state_snapshot()
    eng.state_restore()


@pytest.mark.parametrize("hidden_sizes", [None, LAYERED], ids=["fused", "layered"])
def test_ppo_lag(hidden_sizes):
    base = live()
    eng = engine(hidden_sizes=hidden_sizes, max_grad_norm=0.5)
    if hidden_sizes is None:
        eng.ppo_set_clip_fuse(1)        # the clipped step in two launches: its slots and its snapshot
    onpolicy_steps(eng, lambda b: finite(eng.ppo_update([0.1], 1.0, b, 2, seed=3)[0]))
    if hidden_sizes is None:
        assert eng.ppo_clip_fuse_stats()["steps"] > 0
    above(base)
    eng.close()
    back_at(base, eng)


def test_ppo_lag_reward_normalization_and_actor_calls():
    """the buffers only some options reach: the float64 returns of reward_normalization, the pinned staging of the actor calls"""
    base = live()
    eng = engine(rew_norm=True)
    fill(eng)
    finite(eng.ppo_update([0.1], 1.0, B, 1, seed=3)[0])
    obs = np.random.default_rng(1).standard_normal((ENVS, DO)).astype(F32)
    finite(eng.actor_forward(obs)[0])
    eng.actor_set_resident(False)
    finite(eng.collect_step(None, obs, False, 1)[0])
    finite(eng.get_grads())
    above(base)
    eng.close()
    back_at(base, eng)


def test_focops():
    base = live()
    eng = engine("ALGO_FOCOPS")
    eng.focops_init()
    onpolicy_steps(eng, lambda b: finite(eng.focops_update(0.1, 0.0, b, 2, seed=3)[0]))
    above(base)
    eng.close()
    back_at(base, eng)


@pytest.mark.parametrize("algo", ["ALGO_CPO", "ALGO_TRPO_LAG"])
@pytest.mark.parametrize("hidden_sizes", [None, LAYERED], ids=["fused", "layered"])
def test_trust_region(algo, hidden_sizes):
    base = live()
    eng = engine(algo, hidden_sizes=hidden_sizes)       # n_critics 2: the critic lane's slabs exist
    fill(eng)
    assert eng.tr_begin(optim_critic_iters=2, cost_limit=5.0) == 120      # fill's rows
    finite(eng.cpo_learn(1.0, 1) if algo == "ALGO_CPO" else eng.trpo_learn([0.1], 1.0, 1))
    above(base)
    eng.close()
    back_at(base, eng)


# ------------------------------------------------------------------------------------------------ replay contexts
@pytest.mark.parametrize("deterministic", [False, True], ids=["sac", "ddpg"])
@pytest.mark.parametrize("hidden_sizes", [None, LAYERED], ids=["fused", "layered"])
def test_sac_and_ddpg(deterministic, hidden_sizes):
    base = live()
    eng = engine("ALGO_SAC_LAG", hidden_sizes=hidden_sizes)
    eng.sac_init(deterministic=deterministic)
    replay_params(eng)
    fill(eng)
    if not deterministic:
        eng.per_enable(0.6, 0.4)
    for b in (B, B2):
        finite(eng.sac_update(b, [0.1], 1.0))
    if not deterministic:
        eng.per_update_weight(np.arange(8), np.linspace(0.5, 2.0, 8))
    held = above(base)
    eng.sac_init(deterministic=deterministic)          # a second init on the same context: the old state goes
    replay_params(eng)
    finite(eng.sac_update(B, [0.1], 1.0))
    again = live()
    assert again["dev_blocks"] <= held["dev_blocks"] and again["dev_bytes"] < held["dev_bytes"], (again, held)   # one state at batch 32, not two
    eng.close()
    back_at(base, eng)


@pytest.mark.parametrize("hidden_sizes", [None, LAYERED], ids=["fused", "layered"])
def test_cvpo(hidden_sizes):
    base = live()
    eng = engine("ALGO_SAC_LAG", hidden_sizes=hidden_sizes)
    eng.cvpo_init(0.1, sample_act_num=4)
    replay_params(eng)
    fill(eng)
    eng.cvpo_pre_update()
    for b in (B, B2):
        finite(eng.cvpo_update(b))
    eng.cvpo_post_update()
    above(base)
    eng.close()
    back_at(base, eng)


# ------------------------------------------------------------------------------------------------ device envs
def device_env(eng, seed=3):
    from fsrl_amd import _lib
    A = (0.9 * np.eye(DO)).astype(F32)
    Bm = np.full((DA, DO), 0.1, F32)
    h = eng.devenv_create(_lib.DEVENV_LINEAR, ENVS, 7, seed, (0.7, ), A, Bm)
    eng.devenv_reset(h, ENVS)
    return h


@pytest.mark.parametrize("env_first", [True, False], ids=["env_then_context", "context_then_env"])
def test_device_env(env_first):
    base = live()
    eng = engine()
    h = device_env(eng)
    assert eng.collect_device(h, 2, max_steps_per_launch=4)["steps"] > 0
    assert eng.collect_device(h, 2, max_steps_per_launch=16)["steps"] > 0        # the log regrows
    above(base)
    if env_first:
        eng.devenv_destroy(h)
        mid = live()
        assert mid["dev_blocks"] > base["dev_blocks"]
        eng.close()
    else:
        lib = eng.lib
        eng.close()
        mid = live()
        assert mid["dev_blocks"] > base["dev_blocks"] and mid["pinned_blocks"] > base["pinned_blocks"], (mid, base)  # the env's own
        lib.fsrl_devenv_destroy(h)
    back_at(base, eng)


# ------------------------------------------------------------------------------------------------ the trajectory archive
@pytest.mark.parametrize("detach", [True, False], ids=["detached", "tap_attached"])
def test_trajectory_archive(detach):
    from fsrl_amd.engine import TrajArchive
    base = live()
    eng = engine()
    arch = TrajArchive(eng, 256, 32, 16)
    assert arch.attach(eng) == 0
    fill(eng, steps=30)
    arch.flush()
    assert len(arch.episodes()[0]) > 0
    above(base)
    if detach:
        arch.detach(eng)
    arch.close()            # with the tap still attached: the archive takes it off the context
    fill(eng, steps=10, seed=1)
    eng.close()
    back_at(base, eng, arch)


def test_trajectory_archive_outlives_its_context():
    from fsrl_amd.engine import TrajArchive
    base = live()
    eng, other = engine(), engine(seed=1)
    arch = TrajArchive(other, 256, 32, 16)
    arch.attach(eng)
    fill(eng, steps=30)
    eng.close()             # the context goes first: its finished episodes are archived, the tap goes with it
    arch.flush()
    assert len(arch.episodes()[0]) > 0 and arch.export()["observations"].shape[1] == DO
    arch.close(); other.close()
    back_at(base, eng, other, arch)


# ------------------------------------------------------------------------------------------------ groups
def group_cases():
    """name -> (members, group, one grouped update or collect)"""
    from fsrl_amd.engine import EngineCollectGroup, EngineCvpoGroup, EngineGroup, EngineSacGroup, collect_device_group
    obs = [np.random.default_rng(i).standard_normal((ENVS, DO)).astype(F32) for i in range(2)]

    def onpolicy(algo, hs):
        def make():
            engs = [engine(algo, hidden_sizes=hs, seed=i) for i in range(2)]
            for i, e in enumerate(engs):
                if algo == "ALGO_FOCOPS":
                    e.focops_init()
                fill(e, seed=i)
            g = EngineGroup(engs)

            def run():
                if algo == "ALGO_FOCOPS":
                    stats, _ = g.focops_update([0.1, 0.2], [0.0, 0.0], B, 1, seed=3)
                else:
                    stats, _ = g.ppo_update([[0.1], [0.2]], [1.0, 1.0], B, 1, seed=3)
                for s in stats:
                    finite(s)
                for act, _, _, _ in g.collect_step([None] * 2, obs, False, 1):
                    finite(act)
            return engs, g, run
        return make

    def replay(kind, hs, collect=False):
        def make():
            engs = [engine("ALGO_SAC_LAG", hidden_sizes=hs) for _ in range(2)]
            for i, e in enumerate(engs):
                e.cvpo_init(0.1, sample_act_num=4) if kind == "cvpo" else e.sac_init(deterministic=kind == "ddpg")
                replay_params(e, i)
                fill(e, seed=i)
            if collect:
                g = EngineCollectGroup(engs)

                def run():
                    for act, _, _, _ in g.collect_step([None] * 2, obs, False, 1):
                        finite(act)
            else:
                g = (EngineCvpoGroup if kind == "cvpo" else EngineSacGroup)(engs)

                def run():
                    g.update(B, [1, 1]) if kind == "cvpo" else g.update(B, [1, 1], [[0.1], [0.2]])
                    for e in engs:
                        finite(e.sac_drain())
            return engs, g, run
        return make

    def device_collect():
        class Envs:
            def __init__(self, engs):
                self.engs, self.hs = engs, [device_env(e, seed=3 + i) for i, e in enumerate(engs)]

            def close(self):
                for e, h in zip(self.engs, self.hs):
                    e.lib.fsrl_devenv_destroy(h)

        engs = [engine(seed=i) for i in range(2)]
        envs = Envs(engs)

        def run():
            for r in collect_device_group(engs, envs.hs, 2, max_steps_per_launch=4):
                assert r["steps"] > 0
        return engs, envs, run

    return {"ppo": onpolicy(None, None), "ppo_layered": onpolicy(None, LAYERED), "focops": onpolicy("ALGO_FOCOPS", None),
            "focops_layered": onpolicy("ALGO_FOCOPS", LAYERED), "sac": replay("sac", None), "ddpg": replay("ddpg", None),
            "sac_layered": replay("sac", LAYERED), "cvpo": replay("cvpo", None), "cvpo_layered": replay("cvpo", LAYERED),
            "collect": replay("sac", None, collect=True), "collect_layered": replay("sac", LAYERED, collect=True),
            "device_collect": device_collect}


GROUPS = ["ppo", "ppo_layered", "focops", "focops_layered", "sac", "ddpg", "sac_layered", "cvpo", "cvpo_layered", "collect",
          "collect_layered", "device_collect"]


@pytest.mark.parametrize("group_first", [True, False], ids=["group_then_members", "member_then_group"])
@pytest.mark.parametrize("name", GROUPS)
def test_groups(name, group_first):
    base = live()
    engs, group, run = group_cases()[name]()
    run()
    above(base)
    if group_first:
        group.close()
        for e in engs:
            e.close()
    else:
        engs[0].close()         # a member before its group: the group detaches it and is broken, not leaked
        group.close()
        engs[1].close()
    back_at(base, group, *engs)


# ------------------------------------------------------------------------------------------------ the resident actor
def test_context_destroyed_while_its_actor_kernel_is_live():
    base = live()
    eng = engine()
    obs = np.random.default_rng(1).standard_normal((ENVS, DO)).astype(F32)
    finite(eng.collect_step(None, obs, False, 1)[0])
    assert eng.actor_resident_stats()["live"]
    above(base)
    eng.close()
    back_at(base, eng)


# ------------------------------------------------------------------------------------------------ the hot path allocates nothing
def test_a_third_identical_update_allocates_nothing():
    base = live()
    ppo = engine(max_grad_norm=0.5)
    sac = engine("ALGO_SAC_LAG"); sac.sac_init(); replay_params(sac)
    cpo = engine("ALGO_CPO")
    for e in (ppo, sac, cpo):
        fill(e)

    def cpo_update():
        cpo.tr_begin(optim_critic_iters=2, cost_limit=5.0)
        finite(cpo.cpo_learn(1.0, 1))

    updates = [lambda: finite(ppo.ppo_update([0.1], 1.0, B, 2, seed=3)[0]),
               lambda: finite(sac.sac_update(B, [0.1], 1.0)),      # 32 rows: no rider blocks, so no change of buffer set either
               cpo_update]
    for u in updates:
        u(); u()
        steady = live()
        u()
        assert live() == steady, (live(), steady)
    for e in (ppo, sac, cpo):
        e.close()
    back_at(base, ppo, sac, cpo)
