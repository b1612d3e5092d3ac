"""Groups of LAYERED CVPO contexts (any `hidden_sizes`): fsrl_cvpo_group_update and fsrl_collect_group_* with layered CVPO members,
EngineCvpoGroup / EngineCollectGroup over them.

A layered grouped update runs the launch sequence of the member's own layered fsrl_cvpo_update with every launch carrying all
members (the actor's second forward of an M iteration, which recomputes the first, is left out).  lin_body gives every output
element as one accumulator over ascending k whatever the launch shape and layered launches have no tile-height plan, so -- unlike
the fused CVPO groups -- every member is BIT-IDENTICAL to its solo twin at every k and batch size: the four parameter vectors
(actor, critics, target critics, actor_old), the four duals, every statistics row and the last particles are compared with
np.array_equal.  No tolerance anywhere in this file.

Twin pattern of tests/test_gpu_sac_group_layered.py: the same parameters, pushes and Philox key (one own update on both twins
first), then grouped against solo.  Members differ in parameters, data, store length (T = 120 + 37 i), learning rates, tau,
qc_thres and n_updates."""
import numpy as np
import pytest

from test_gpu_group_collect import _close, _random_step, _same_stores, _step_b
from test_gpu_collect_group import _same_step, _solo_steps

pytestmark = pytest.mark.gpu

N8 = [5, 3, 0, 5, 2, 4, 1, 5]
NAMES = ("actor", "critics", "critics_old", "actor_old", "duals", "rows", "particles")


def _engine(hs, Do, Da, seed=0, T=150, env_num=4, sub=200, force=False, kind="cvpo", key=None, **cv):
    """A layered CVPO context with parameters, data, learning rates, tau and qc_thres of its own (kind "sacl": a SAC-Lag one)."""
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine, EngineConfig
    eng = Engine(EngineConfig(algo=_lib.ALGO_SAC_LAG, obs_dim=Do, act_dim=Da, hidden_sizes=tuple(hs), n_critics=2, env_num=env_num,
                              buffer_size=env_num * sub, gamma=0.98, target_kl=None, force_layered=force))
    if kind == "sacl":
        eng.sac_init()
        return eng
    kw = dict(actor_lr=5e-4 * (1 + 0.1 * seed), critic_lr=1e-3 * (1 + 0.05 * seed), tau=0.05 + 0.01 * seed)
    kw.update(cv)
    eng.cvpo_init(0.1 + 0.02 * seed, **kw)
    rng = np.random.default_rng(100 + seed)
    eng.sac_set_params(0.1 * rng.standard_normal(eng.n_sac_actor).astype(np.float32),
                       0.1 * rng.standard_normal(eng.n_sac_critics).astype(np.float32), 0.0)
    eng.cvpo_post_update()                         # actor_old <- actor
    eng.cvpo_pre_update()
    ids = np.arange(env_num)
    for t in range(T):                             # T > sub: the sub-buffers wrap
        obs = rng.standard_normal((env_num, Do)).astype(np.float32)
        act = np.tanh(rng.standard_normal((env_num, Da))).astype(np.float32)
        term = rng.random(env_num) < 0.03
        trunc = np.full(env_num, (t + 1) % 50 == 0) & ~term
        eng.push(ids, obs, act, rng.normal(0.5, 0.5, env_num), (rng.random(env_num) < 0.2).astype(np.float64), term, trunc,
                 rng.standard_normal((env_num, Do)).astype(np.float32))
    if key is not None:
        eng.actor_sample(np.zeros((1, Do), np.float32), seed=key)      # keys the collector's noise stream
    return eng


def _state(eng, B=None):
    """actor, critics, target critics, actor_old, the four duals, the drained rows, the last update's particles"""
    out = [eng.sac_get_params(w)[0] for w in (0, 1, 2, 3)] + [eng.cvpo_duals(), eng.sac_drain()]
    out.append(eng.cvpo_last_particles(B) if B else np.zeros(0, np.float32))
    return out


def _same(x, y, tag=None):
    for j, name in enumerate(NAMES):
        assert x[j].shape == y[j].shape, (tag, name, x[j].shape, y[j].shape)
        assert np.array_equal(x[j], y[j]), (tag, name, np.abs(x[j] - y[j]).max())


def _run(hs, Do, Da, B, k, n, force=False, **cv):
    from fsrl_amd.engine import EngineCvpoGroup
    mk = lambda i: _engine(hs, Do, Da, seed=i, T=120 + 37 * i, force=force, **cv)
    grouped, solo = [mk(i) for i in range(k)], [mk(i) for i in range(k)]
    for i in range(k):                             # key each member's Philox stream (one own update on both twins)
        for e in (grouped[i], solo[i]):
            e.cvpo_update(B, seed=11 + i, sync=False)
    g = EngineCvpoGroup(grouped)
    g.update(B, n)
    for i in range(k):
        for _ in range(n[i]):
            solo[i].cvpo_update(B, sync=False)
    out = [(_state(grouped[i], B), _state(solo[i], B)) for i in range(k)]
    g.close()
    _close(grouped, solo)
    return out


CASES = {
    # a member sitting out, unequal counts
    "deep3": dict(hs=(64, 48, 32), Do=8, Da=2, B=64, k=3, n=[5, 3, 0], sample_act_num=4),
    # widths and obs that fail the float4 check (scalar path); a 16-row tile plus a 4-row tail; K * B = 60 is no multiple of 16; a
    # 16-output head; the iteration table with M > 1
    "ragged-k8": dict(hs=(50, 30), Do=33, Da=8, B=20, k=8, n=N8, sample_act_num=3, mstep_iter_num=2, n_step=3),
    # one layer wider than the fused kernels; four Q-networks (pair_shift 1); 17 tiles, a ragged 64-row tile
    "wide1-double": dict(hs=(320, ), Do=8, Da=2, B=272, k=2, n=[4, 4], sample_act_num=2, double_critic=True),
    # a two-layer network through the layered kernels
    "forced": dict(hs=(64, 64), Do=8, Da=2, B=64, k=2, n=[3, 3], sample_act_num=4, force=True),
    # eight hidden layers, four Q-networks: the solo twin's 36 weight-side jobs of the critics exceed the 32-entry job table of a
    # launch and go out as two launches of whole networks (lay_wgrad_k); the group's table is in device memory, one launch
    "eight-k2": dict(hs=(24, 17, 32, 9, 40, 4, 28, 12), Do=20, Da=8, B=64, k=2, n=[3, 2], sample_act_num=2, double_critic=True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_members_are_bit_identical_to_their_solo_twins(name):
    case = dict(CASES[name])
    n = case["n"]
    res = _run(**case)
    for i, (x, y) in enumerate(res):
        assert x[5].shape == (n[i] + 1, 17)
        _same(x, y, (name, i))


def test_group_of_one():
    (x, y), = _run((64, 48, 32), 8, 2, 256, 1, [20], sample_act_num=8)
    assert x[5].shape == (21, 17)
    _same(x, y)


def test_interleaved_member_calls_and_own_updates():
    """Between two grouped calls: cvpo_pre_update / cvpo_post_update / cvpo_set_thres and an own update on some members (the same on
    the twins), pushes on another.  Orders a member's stream against the group's stream in both directions."""
    from fsrl_amd.engine import EngineCvpoGroup
    hs, Do, Da, B = (64, 48, 32), 8, 2, 64
    a = [_engine(hs, Do, Da, seed=i, T=120 + 37 * i, sample_act_num=4, mstep_iter_num=2) for i in range(3)]
    b = [_engine(hs, Do, Da, seed=i, T=120 + 37 * i, sample_act_num=4, mstep_iter_num=2) for i in range(3)]
    for i in range(3):
        for e in (a[i], b[i]):
            e.cvpo_update(B, seed=31 + i, sync=False)
    g = EngineCvpoGroup(a)
    rng = np.random.default_rng(5)
    ids = np.arange(4)
    for r, n in enumerate(([3, 2, 1], [1, 0, 2], [2, 3, 2])):
        g.update(B, n)
        for i in range(3):
            for _ in range(n[i]):
                b[i].cvpo_update(B, sync=False)
        for e in (a[0], b[0]):                     # member calls right behind the grouped call, then an own update
            e.cvpo_post_update(); e.cvpo_pre_update(); e.cvpo_set_thres(0.3 + 0.1 * r)
            e.cvpo_update(B, sync=False)
        for e in (a[2], b[2]):
            e.cvpo_pre_update()
        rows = [rng.standard_normal((4, Do)).astype(np.float32) for _ in range(2)]
        for e in (a[1], b[1]):                     # pushes in between
            e.push(ids, rows[0], np.zeros((4, Da), np.float32), np.ones(4), np.ones(4), np.zeros(4, bool), np.zeros(4, bool), rows[1])
    g.close()
    for i in range(3):
        _same(_state(a[i], B), _state(b[i], B), i)
    _close(a, b)


def test_rejections_a_member_closed_before_its_group_and_a_member_made_sac():
    from fsrl_amd.engine import EngineCvpoGroup, EngineSacGroup
    Do, Da, B = 8, 2, 64
    lay = lambda hs=(64, 48, 32), **kw: _engine(hs, Do, Da, T=130, **kw)
    a, a2, twin = lay(seed=0), lay(seed=1), lay(seed=1)
    fused = lay((64, 64))
    others = [lay((64, 48, 16)), lay((64, 48, 32, 32)), lay((64, 64), force=True), lay(kind="sacl"), lay(sample_act_num=8),
              lay(mstep_iter_num=2), lay(n_step=3), lay(double_critic=True)]
    cases = [([a, others[0]], "one network shape"), ([a, others[1]], "one network shape"), ([fused, others[2]], "layered"),
             ([others[2], fused], "layered"), ([a, fused], "layered"), ([a, others[3]], "SAC-Lagrangian"),
             ([a, others[4]], "sample_act_num"), ([a, others[5]], "mstep_iter_num"), ([a, others[6]], "n_step"),
             ([a, others[7]], "double_critic"), ([a, a], "listed twice")]
    for bad, reason in cases:
        with pytest.raises(AssertionError, match=reason):      # FSRL_EINVAL, with the reason in the message
            EngineCvpoGroup(bad)
    with pytest.raises(AssertionError, match="CVPO"):          # a SAC group still refuses a layered CVPO member
        EngineSacGroup([others[3], a])
    g = EngineCvpoGroup([a, a2])
    with pytest.raises(AssertionError, match="already in a CVPO group"):
        EngineCvpoGroup([a2])
    for e in (a2, twin):
        e.cvpo_update(B, seed=5, sync=False)
    g.update(B, [1, 2])
    for _ in range(2):
        twin.cvpo_update(B, sync=False)
    a.close()                                      # a member destroyed before its group
    with pytest.raises(RuntimeError, match="destroyed"):
        g.update(B, [1, 1])
    for e in (a2, twin):                           # the survivor is an ordinary context
        e.cvpo_update(B, sync=False)
    _same(_state(a2, B), _state(twin, B))
    g.close()
    c, d = lay(seed=2), lay(seed=3)                # a member re-initialised as SAC-Lag under a live group
    g2 = EngineCvpoGroup([c, d])
    g2.update(B, [1, 1])
    d.sac_init()
    with pytest.raises(AssertionError, match="SAC-Lagrangian|no longer a context of the group's kind"):
        g2.update(B, [1, 1])
    g2.close()
    _close([a2, twin, fused, c, d], others)


# ---------------------------------------------------------------- lock-step collection
def _pair(envs, hs, Do, Da, T=0):
    from fsrl_amd.engine import EngineCollectGroup
    mk = lambda i, e: _engine(hs, Do, Da, seed=i, T=T, env_num=e, sub=400, key=1000 + i, sample_act_num=4)
    a = [mk(i, e) for i, e in enumerate(envs)]
    b = [mk(i, e) for i, e in enumerate(envs)]
    return a, b, EngineCollectGroup(b)


def test_collect_group_step_is_every_members_collect_step_bit_for_bit():
    """A scripted run with random row counts per member (steps in which a member has no rows among them), deterministic /
    bound_method / bounds varied per step: actions, env actions, ptr / ep_* outputs and the stores identical to the members' own
    collect_step; one request per grouped call with rows, no resident kernel."""
    envs, hs, Do, Da = (3, 20, 1), (64, 48, 32), 8, 2
    a, b, cg = _pair(envs, hs, Do, Da)
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


def test_collect_grouped_update_collect_matches_the_solo_twins():
    """One closed cycle: lock-step collection, a grouped update, lock-step collection again; set A runs each member's own
    collect_step and cvpo_update.  Actions, stores and every piece of the members' state stay those of the member-by-member run."""
    from fsrl_amd.engine import EngineCvpoGroup
    envs, hs, Do, Da, B = (3, 20, 1), (64, 48, 32), 8, 2, 64
    a, b, cg = _pair(envs, hs, Do, Da, T=60)
    for i in range(3):
        for e in (a[i], b[i]):
            e.cvpo_update(B, seed=11 + i, sync=False)
    rng = np.random.default_rng(5)
    n_upd = [3, 1, 2]
    scripts = [[_random_step(rng, envs, Do, Da, k_act_zero=0.0) + (False, 1, None, None) for _ in range(6)] for _ in range(2)]
    want = [_solo_steps(a, scripts[0])]
    for i, e in enumerate(a):
        e.cvpo_pre_update()
        for _ in range(n_upd[i]):
            e.cvpo_update(B, sync=False)
        e.cvpo_post_update()
    want.append(_solo_steps(a, scripts[1]))
    ug = EngineCvpoGroup(b)
    got = [[_step_b(cg, *st) for st in scripts[0]]]
    for e in b:
        e.cvpo_pre_update()
    ug.update(B, n_upd)
    for e in b:
        e.cvpo_post_update()
    got.append([_step_b(cg, *st) for st in scripts[1]])
    for cycle in range(2):
        for step, (x, y) in enumerate(zip(want[cycle], got[cycle])):
            _same_step(x, y, (cycle, step))
    for i in range(3):
        _same(_state(a[i], B), _state(b[i], B), i)
    _same_stores(a, b)
    ug.close()
    _close(cg, a, b)
