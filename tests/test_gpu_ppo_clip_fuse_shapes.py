"""The two-launch clipped PPO-Lagrangian step over the case table of tests/clip_fuse_problems.py: every ClipPend slot of the dW1 role and
both sides of each slot's edge, H 64 / 128 / 256, one and two critics, heads of 1 and 16 actions, minibatches from 7 to 512 rows, the
coefficient-1 branch, updates that clip in some steps only, option combinations, the refusals, and the forced fallback from every place
the host reads the control block.  tests/test_gpu_ppo_clip_fuse.py has the mode at one shape family; this file has the table.

Two yardsticks.  (1) The three-launch step of the same library: one summation routine and one Adam routine serve both routes, so the
logged statistics, the parameters, the training-state blob (step count, random streams, P with its mirrors, M, V), the last gradient norm
and the KL stop are compared bit for bit.  (2) The float64 oracle, with the fp32 oracle's own distance to it as the unit.

Every context gets its mode from ppo_set_clip_fuse, so nothing depends on the automatic rule, which has a test of its own in a child
process.  The wait limit is the default or 0 (every workgroup gives up before its first poll: the fallback on demand); any small positive
limit would make the outcome depend on timing."""
import contextlib
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import clip_fuse_problems as cf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FALLBACK_SHAPES = ["o17", "o33a16"]


@contextlib.contextmanager
def _engines():
    """make(case, mode, limit, fill=True, **EngineConfig overrides) -> Engine; every engine made is closed on the way out"""
    from fsrl_amd.engine import Engine, EngineConfig
    made = []

    def make(case, mode, limit=-1, fill=True, **over):
        eng = Engine(EngineConfig(**cf.engine_kwargs(case, **over)), device=0)
        made.append(eng)
        eng.ppo_set_clip_fuse(mode, limit)
        if fill:
            cf.fill(eng, case)
        return eng
    try:
        yield make
    finally:
        for eng in made:
            eng.close()


def _result(eng, stats, stopped):
    return dict(stats=np.array(stats), stopped=stopped, params=eng.get_params().copy(), state=eng.train_state(with_store=False),
                cf=eng.ppo_clip_fuse_stats())


def _update(eng, case, passes=None, perms="table", seed=0):
    passes = case.passes if passes is None else passes
    if isinstance(perms, str):
        perms = cf.problem(case)["perms"][:passes]
    stats, stopped = eng.ppo_update(cf.lagrangians(case), cf.RESCALING, case.batch, passes, perms=perms, seed=seed)
    return _result(eng, stats, stopped)


def _same(a, b):
    assert a["stats"].shape == b["stats"].shape, (a["stats"].shape, b["stats"].shape)
    assert np.isfinite(a["stats"]).all() and np.isfinite(a["params"]).all()
    assert np.array_equal(a["stats"], b["stats"]), int((a["stats"] != b["stats"]).sum())
    assert np.array_equal(a["params"], b["params"]), int((a["params"] != b["params"]).sum())
    assert a["state"] == b["state"]                                     # adam_t, random streams, P with mirrors, M, V
    assert a["stopped"] == b["stopped"]
    assert a["cf"]["grad_norm"].tobytes() == b["cf"]["grad_norm"].tobytes(), (a["cf"], b["cf"])
    assert a["cf"]["grad_norm"] > 0


@functools.lru_cache(maxsize=None)
def _pair(cid):
    """one update of the case with the two-launch step forced on, and one with it off: run once, shared by the tests below"""
    case = cf.CASES[cid]
    out = []
    for mode in (1, 0):
        with _engines() as make:
            out.append(_update(make(case, mode), case))
    return tuple(out)


# ------------------------------------------------------------------------------------------------ 1. the two routes agree bit for bit
@pytest.mark.parametrize("cid", list(cf.CASES))
def test_modes_agree_bit_for_bit(cid):
    case = cf.CASES[cid]
    on, off = _pair(cid)
    assert on["stats"].shape == (case.steps, 11), on["stats"].shape
    want = dict(fallbacks=0, steps=case.fused_steps, last_update_fused=not case.refused)
    assert on["cf"] == dict(on["cf"], **want), (on["cf"], want)
    assert off["cf"] == dict(off["cf"], available=False, fallbacks=0, steps=0, last_update_fused=False), off["cf"]
    assert on["stopped"] == case.stop_pass
    _same(on, off)
    assert not np.array_equal(on["params"], cf.problem(case)["theta"])


# ------------------------------------------------------------------------------------------------ 2. against float64
@pytest.mark.parametrize("cid", [*cf.SHAPES, *cf.CLIP_BRANCH, *cf.OPTIONS])
def test_two_launch_step_against_float64(cid):
    """Bars: the first ten steps' statistics within max(3 x the fp32 oracle's distance to float64, 2e-5 * scale + 1e-6) (the floor is what
    test_gpu_ppo.py holds its first ten steps to); parameters after the update at test_gpu_shapes.py's bar (0.999-quantile 5e-6, max
    1e-4); the last step's gradient norm within max(3 x the fp32 oracle's, 2e-5) relative.  The measured distances are printed."""
    case = cf.CASES[cid]
    on, _ = _pair(cid)
    r64, r32 = cf.oracle_run(case, True), cf.oracle_run(case, False)
    assert on["stats"].shape == r64["stats"].shape and on["stopped"] == r64["stopped"] == -1
    k = min(10, case.steps)
    scale = np.maximum(np.abs(r64["stats"]).max(0), 1e-2)
    e_ref = np.abs(r32["stats"][:k] - r64["stats"][:k]).max(0)
    e_dev = np.abs(on["stats"][:k].astype(np.float64) - r64["stats"][:k]).max(0)
    bar = np.maximum(3.0 * e_ref, 2e-5 * scale + 1e-6)
    d = np.abs(on["params"].astype(np.float64) - r64["params"])
    d_ref = np.abs(r32["params"].astype(np.float64) - r64["params"])
    g64 = r64["norms"][-1]
    g_dev, g_ref = abs(float(on["cf"]["grad_norm"]) - g64) / g64, abs(r32["norms"][-1] - g64) / g64
    print(f"\n{cid}: route {'three launches (refused)' if case.refused else 'two launches'}, {on['cf']['steps']} two-launch steps of "
          f"{case.steps}; statistics / scale vs f64: device {(e_dev / scale).max():.2e} fp32 oracle {(e_ref / scale).max():.2e}; "
          f"parameters vs f64: device q999 {np.quantile(d, 0.999):.2e} max {d.max():.2e}, fp32 oracle q999 "
          f"{np.quantile(d_ref, 0.999):.2e} max {d_ref.max():.2e}; last gradient norm {float(on['cf']['grad_norm']):.6g} rel. vs f64: "
          f"device {g_dev:.2e} fp32 oracle {g_ref:.2e}")
    assert (e_dev <= bar).all(), (e_dev, bar)
    assert np.quantile(d, 0.999) <= 5e-6 and d.max() <= 1e-4, (np.quantile(d, 0.999), d.max())
    assert g_dev <= max(3.0 * g_ref, 2e-5), (g_dev, g_ref)


@pytest.mark.parametrize("cid", ["o49tiny-loose", "o17-loose"])
def test_loose_threshold_equals_the_unclipped_fused_adam_form(cid):
    """coefficient exactly 1: g * 1.0f == g, so the parameters are those of a max_grad_norm=None context (Adam inside the weight-gradient
    launch, no exchange) bit for bit"""
    case = cf.CASES[cid]
    on, _ = _pair(cid)
    with _engines() as make:
        plain = _update(make(case, 0, max_grad_norm=None), case)
    assert np.array_equal(on["params"], plain["params"]), int((on["params"] != plain["params"]).sum())
    assert np.array_equal(on["stats"], plain["stats"])


# ------------------------------------------------------------------------------------------------ 3. switching routes
@pytest.mark.parametrize("cid", FALLBACK_SHAPES)
def test_switching_routes_within_a_contexts_life(cid):
    """two launches, three, two again on one context against three launches throughout: the slot tags after a gap, and the forward-fragment
    mirror of W2 that both routes write"""
    case = cf.CASES[cid]
    with _engines() as make:
        a, b = make(case, 1), make(case, 0)
        for u, mode in enumerate((1, 0, 1)):
            a.ppo_set_clip_fuse(mode, -1)
            ra, rb = _update(a, case), _update(b, case)
            assert ra["cf"]["last_update_fused"] == bool(mode) and ra["cf"]["fallbacks"] == 0, (u, ra["cf"])
            assert ra["cf"]["steps"] == case.fused_steps * (1 + u // 2), (u, ra["cf"])
            _same(ra, rb)


# ------------------------------------------------------------------------------------------------ 4. the forced fallback
def _fell_back(r):
    assert r["cf"] == dict(r["cf"], available=False, fallbacks=1, last_update_fused=False), r["cf"]


@pytest.mark.parametrize("cid", FALLBACK_SHAPES)
def test_fallback_with_library_drawn_permutations(cid):
    """perms=None: the replay uploads the permutations the passes ran with and leaves the shuffle stream where the three-launch context
    leaves it (the state blob holds it); the next update draws the same permutations on both"""
    case = cf.CASES[cid]
    with _engines() as make:
        a, b = make(case, 1, 0), make(case, 0)
        ra, rb = _update(a, case, perms=None, seed=7), _update(b, case, perms=None, seed=7)
        _fell_back(ra)
        _same(ra, rb)
        assert not np.array_equal(ra["stats"], _pair(cid)[0]["stats"])          # not the table's permutations
        _same(_update(a, case, perms=None), _update(b, case, perms=None))


@pytest.mark.parametrize("cid", list(cf.KL))
def test_fallback_under_the_kl_stop(cid):
    """target_kl on: the first pass's verdict reads the control block, replays that pass and the update goes on in three launches to the
    same stop"""
    case = cf.CASES[cid]
    with _engines() as make:
        ra, rb = _update(make(case, 1, 0), case), _update(make(case, 0), case)
    _fell_back(ra)
    assert ra["stopped"] == case.stop_pass and ra["stats"].shape[0] == case.steps, (ra["stopped"], ra["stats"].shape)
    assert ra["cf"]["steps"] == len(case.minibatches), ra["cf"]                 # the first pass only ran two-launch steps
    _same(ra, rb)


@pytest.mark.parametrize("limit", [-1, 0])
@pytest.mark.parametrize("cid", list(cf.KL))
def test_stepwise_passes_without_waiting(cid, limit):
    """ppo_begin / ppo_pass(wait=False) / ppo_pass_result / ppo_end_stats, the policy facade's sequence: the verdict is collected by
    ppo_pass_result, the third place that looks at the control block"""
    case = cf.CASES[cid]
    perms = cf.problem(case)["perms"]
    with _engines() as make:
        a = make(case, 1, limit)
        assert a.ppo_begin(cf.lagrangians(case), cf.RESCALING, case.batch) == case.n
        stopped = -1
        for k in range(case.passes):
            assert a.ppo_pass(perms[k], wait=False) is False
            if a.ppo_pass_result():
                stopped = k
                break
        ra = _result(a, a.ppo_end_stats(case.passes * len(case.minibatches)), stopped)
        rb = _update(make(case, 0), case)
    if limit == 0:
        _fell_back(ra)
    else:
        assert ra["cf"] == dict(ra["cf"], fallbacks=0, steps=case.fused_steps, last_update_fused=True), ra["cf"]
    assert ra["stopped"] == case.stop_pass
    _same(ra, rb)


def test_fallback_replays_a_pass_that_holds_a_split_k_step():
    case = cf.CASES["o64mix"]
    with _engines() as make:
        ra = _update(make(case, 1, 0), case)
    _fell_back(ra)
    _same(ra, _pair("o64mix")[1])


@pytest.mark.parametrize("cid", FALLBACK_SHAPES)
def test_state_of_a_fallen_back_context_runs_two_launches_elsewhere(cid):
    """the training state carries nothing of the fallback: a fresh context that imports it takes the two-launch step again and goes on
    bit-identically to three launches"""
    case = cf.CASES[cid]
    with _engines() as make:
        a, b = make(case, 1, 0), make(case, 0)
        ra, rb = _update(a, case), _update(b, case)
        _fell_back(ra)
        _same(ra, rb)
        fresh = make(case, 1, fill=False)
        fresh.load_train_state(a.train_state(with_store=True))
        rf, rb2 = _update(fresh, case), _update(b, case)
        assert rf["cf"] == dict(rf["cf"], available=True, fallbacks=0, steps=case.fused_steps, last_update_fused=True), rf["cf"]
        _same(rf, rb2)
        assert not np.array_equal(rf["params"], ra["params"])


# ------------------------------------------------------------------------------------------------ 5. the benchmark's region
@pytest.mark.parametrize("limit", [-1, 0])
@pytest.mark.parametrize("cid", FALLBACK_SHAPES)
def test_restore_then_update_is_idempotent(cid, limit):
    """bench.py times state_restore + ppo_update: snapshot, update, restore, update gives the same update twice, equal to three launches,
    also when the first of the two fell back"""
    case = cf.CASES[cid]
    with _engines() as make:
        a = make(case, 1, limit)
        a.state_snapshot()
        first = _update(a, case)
        a.state_restore()
        second = _update(a, case)
    if limit == 0:
        _fell_back(first); _fell_back(second)
        assert second["cf"]["steps"] == first["cf"]["steps"]
    else:
        assert second["cf"] == dict(second["cf"], fallbacks=0, steps=2 * case.fused_steps, last_update_fused=True), second["cf"]
    _same(first, second)
    _same(second, _pair(cid)[1])


# ------------------------------------------------------------------------------------------------ 6. the automatic rule on the device
def _automatic_rule_child():
    """a lone context in mode -1, then with a second context alive, then alone again: one line of JSON per update"""
    sys.path.insert(0, ROOT)
    case = cf.CASES["o17"]
    with _engines() as make:
        a = make(case, -1)
        out = [_update(a, case)["cf"]]
        other = make(case, -1, fill=False)
        out.append(_update(a, case)["cf"])
        other.close()
        out.append(_update(a, case)["cf"])
    for s in out:
        print("CLIP_FUSE_STATS " + json.dumps(dict(s, grad_norm=float(s["grad_norm"]))), flush=True)


def test_automatic_rule_counts_the_contexts_alive_on_the_device():
    """in a process of its own: the suite's process may hold contexts that earlier tests left unclosed"""
    case = cf.CASES["o17"]
    res = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    s = [json.loads(line.split(" ", 1)[1]) for line in res.stdout.splitlines() if line.startswith("CLIP_FUSE_STATS ")]
    assert len(s) == 3, res.stdout[-2000:]
    assert s[0] == dict(s[0], available=True, fallbacks=0, steps=case.fused_steps, last_update_fused=True), s
    assert s[1] == dict(s[1], available=True, fallbacks=0, steps=case.fused_steps, last_update_fused=False), s
    assert s[2] == dict(s[2], available=True, fallbacks=0, steps=2 * case.fused_steps, last_update_fused=True), s
    assert all(x["grad_norm"] > 0 for x in s)


if __name__ == "__main__":
    _automatic_rule_child()
