"""Grouped trust-region seeds on the host (no GPU): the multi-seed example's arguments, TrustPolicyGroup's argument checks and its
update over stub engines (process_fn in member order, the device parts beside each other on worker threads, all of them joined
before a member's error is raised with its index, everything that logs or draws random numbers on the calling thread in member
order), and the agreement of include/fsrl_hip.h, the library's exports and the ctypes table (the feature adds no symbol)."""
import importlib.util
import os
import re
import subprocess
import threading

import numpy as np
import pytest

from fsrl_amd.policy import TrustPolicyGroup
from fsrl_amd.policy.cpo import CPO
from fsrl_amd.policy.trpo_lag import TRPOLagrangian

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "fsrl_amd", "libfsrl_hip.so")


# ---------------------------------------------------------------------------------------------------- the example's arguments
def _example():
    spec = importlib.util.spec_from_file_location("train_multi_seed", os.path.join(ROOT, "examples", "train_multi_seed.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("algo", ["cpo", "trpol"])
@pytest.mark.parametrize("hidden", ["128x128", "64x48x32"])
def test_example_takes_grouped_trust_region_seeds(algo, hidden):
    mod = _example()
    a = mod.parse_args(["--grouped", "--algo", algo, "--hidden-sizes", hidden, "--seeds", "8"])
    assert a.grouped and a.algo == algo and a.seeds == 8 and a.hidden_sizes == tuple(int(w) for w in hidden.split("x"))
    assert algo in mod.GROUPED_ALGOS and callable(mod.run_grouped_trust)


def test_example_keeps_what_it_took_and_what_it_refused(capsys):
    mod = _example()
    assert set(mod.GROUPED_ALGOS) == {"ppol", "focops", "sacl", "ddpgl", "cvpo", "cpo", "trpol"}
    for algo in ("focops", "cvpo"):
        with pytest.raises(SystemExit):
            mod.parse_args(["--grouped", "--algo", algo, "--hidden-sizes", "64x48x32"])
        assert "do not group yet" in capsys.readouterr().err
    src = open(os.path.join(ROOT, "examples", "train_multi_seed.py")).read()
    assert "a.algo in GROUPED_ALGOS" in src and "CVPOPolicyGroup" in src and "TrustPolicyGroup" in src


# ---------------------------------------------------------------------------------------------------- TrustPolicyGroup over stubs
class _Cfg:
    def __init__(self, hs):
        self.obs_dim, self.act_dim, self.hidden, self.hidden_sizes = 8, 2, 0, hs


class _Engine:
    """the engine calls of process_fn / _learn_device; `script(engine)` runs inside the learn call, on whatever thread that is"""

    def __init__(self, i, journal, hs=(64, 64), device=0, n=40, script=None):
        self.i, self.journal, self.cfg, self.device, self.n, self.script = i, journal, _Cfg(hs), device, n, script
        self.thread = None

    def tr_begin(self, **kw):
        self.journal.append(("begin", self.i, threading.current_thread() is threading.main_thread()))
        return self.n

    def _learn(self, width, repeat, perms):
        self.thread = threading.current_thread()
        self.perms = perms
        if self.script is not None:
            self.script(self)
        return np.full((repeat, width), float(self.i), np.float32)

    def cpo_learn(self, ave_cost_return, repeat, batch_size=2**31 - 1, perms=None, seed=0):
        return self._learn(17, repeat, perms)

    def trpo_learn(self, lagrangians, rescaling, repeat, batch_size=2**31 - 1, perms=None, seed=0):
        return self._learn(11, repeat, perms)

    def tr_linesearch_evals(self, cap=64):
        return np.ones(cap - 1, np.int32)


class _Log:
    def __init__(self, i, journal):
        self.i, self.journal = i, journal

    def store(self, tab=None, **kw):
        if "gradient_steps" in kw:
            self.journal.append(("log", self.i, threading.current_thread() is threading.main_thread()))


class _Optim:
    param_groups = [{"lr": 1e-3}]


class _Buf:
    def __init__(self, p):
        self.engine = p.engine


def _policy(cls, i, journal, **kw):
    p = cls.__new__(cls)
    p.engine = _Engine(i, journal, **kw)
    p.logger, p.optim, p.lr_scheduler = _Log(i, journal), _Optim(), None
    p._reference_rng, p.gradient_steps, p._ave_cost_return, p.updating = False, 0, 3.0, False
    p._delta, p._backtrack_coeff, p._damping_coeff, p._damping, p._l2_reg = 0.01, 0.8, 0.1, 0.1, 0.001
    p._max_backtracks, p._optim_critic_iters, p._norm_adv, p._cost_limit = 10, 3, True, 10.0
    p.use_lagrangian = False
    p._mark_stale = lambda: journal.append(("stale", i, True))
    p._step_lr_scheduler = lambda: journal.append(("lr", i, threading.current_thread() is threading.main_thread()))
    return p


def test_argument_checks():
    j = []
    with pytest.raises(AssertionError, match="at least one policy"):
        TrustPolicyGroup([])
    with pytest.raises(AssertionError, match="all CPO or all TRPOLagrangian"):
        TrustPolicyGroup([_policy(CPO, 0, j), _policy(TRPOLagrangian, 1, j)])
    with pytest.raises(AssertionError, match="all CPO or all TRPOLagrangian"):
        TrustPolicyGroup([_policy(TRPOLagrangian, 0, j), _policy(CPO, 1, j)])
    with pytest.raises(AssertionError, match="one network shape"):
        TrustPolicyGroup([_policy(CPO, 0, j), _policy(CPO, 1, j, hs=(64, 48, 32))])
    with pytest.raises(AssertionError, match="one device"):
        TrustPolicyGroup([_policy(CPO, 0, j), _policy(CPO, 1, j, device=1)])
    p = _policy(CPO, 0, j)
    with pytest.raises(AssertionError, match="listed twice"):
        TrustPolicyGroup([p, p])
    g = TrustPolicyGroup([p, _policy(CPO, 1, j)])
    with pytest.raises(AssertionError, match="one buffer per policy"):
        g.update([_Buf(p)])
    with pytest.raises(AssertionError, match="buffer i must be"):
        g.update([_Buf(p), _Buf(p)])
    g.close()
    g.close()                                                    # closing twice is fine


@pytest.mark.parametrize("cls", [CPO, TRPOLagrangian])
def test_update_runs_the_device_parts_beside_each_other_and_the_rest_in_member_order(cls):
    j, k = [], 3
    barrier = threading.Barrier(k, timeout=20)                   # passes only if the k learn calls are in flight at the same time
    pols = [_policy(cls, i, j, n=40 + i, script=lambda e: barrier.wait()) for i in range(k)]
    released = []

    class _CollectGroup:
        def actor_release(self):
            released.append(len(j))

    g = TrustPolicyGroup(pols, collect_group=_CollectGroup())
    np.random.seed(7)
    out = g.update([_Buf(p) for p in pols], batch_size=16, repeat=2)
    np.random.seed(7)                                            # learn's draws, on the calling thread in member order
    want = [[np.random.permutation(40 + i) for _ in range(2)] for i in range(k)]
    assert released == [0]                                       # the collect group's kernel ends before anything else
    for i, p in enumerate(pols):
        assert p.engine.thread is not threading.main_thread() and len({q.engine.thread for q in pols}) == k
        assert all(np.array_equal(x, y) for x, y in zip(p.engine.perms, want[i]))
        assert not p.updating and p._pending is None
    assert out == [{"gradient_steps": 2}] * k
    assert [e[:2] for e in j[:k]] == [("begin", i) for i in range(k)]
    assert [e[:2] for e in j[k:]] == [x for i in range(k) for x in (("log", i), ("stale", i))] + [("lr", i) for i in range(k)]
    assert all(e[2] for e in j)                                  # all of it on the calling thread
    g.close()


def test_a_members_error_is_raised_with_its_index_after_every_call_has_ended():
    j, done = [], []
    failed = threading.Event()

    def script(e):
        if e.i == 1:
            failed.set()
            raise RuntimeError("FSRL_EHIP: device error")
        assert failed.wait(20)                                   # the others are still in flight when member 1 fails ...
        done.append(e.i)

    pols = [_policy(CPO, i, j, script=script) for i in range(3)]
    g = TrustPolicyGroup(pols)
    with pytest.raises(RuntimeError, match="member 1: FSRL_EHIP: device error"):
        g.update([_Buf(p) for p in pols], repeat=1)
    assert sorted(done) == [0, 2]                                # ... and have ended when it is raised
    assert not any(p.updating for p in pols) and [e[:2] for e in j if e[0] == "stale"] == [("stale", i) for i in range(3)]
    assert not any(e[0] == "log" for e in j)
    g.close()


def test_a_group_of_one_updates_on_the_calling_thread():
    j = []
    p = _policy(TRPOLagrangian, 0, j)
    g = TrustPolicyGroup([p])
    assert g.update([_Buf(p)], repeat=3) == [{"gradient_steps": 3}]
    assert p.engine.thread is threading.main_thread() and p.gradient_steps == 9      # optim_critic_iters per row
    g.close()


def test_learn_alone_is_its_three_parts():
    """learn() and update() on their own do what they did: prepare, device, finish on one thread"""
    j = []
    p = _policy(CPO, 0, j)
    np.random.seed(3)
    out = p.update(0, _Buf(p), batch_size=16, repeat=2)
    np.random.seed(3)
    want = [np.random.permutation(40) for _ in range(2)]
    assert out == {"gradient_steps": 2} and all(np.array_equal(x, y) for x, y in zip(p.engine.perms, want))
    assert [e[:2] for e in j] == [("begin", 0), ("log", 0), ("stale", 0), ("lr", 0)] and not p.updating
    q = _policy(CPO, 1, j, n=10)
    q.update(0, _Buf(q), batch_size=99999, repeat=1)
    assert q.engine.perms is None                                # one minibatch covers the batch: the device keeps store order


# ---------------------------------------------------------------------------------------------------- the C ABI
def test_header_exports_and_ctypes_table_agree_and_the_collect_group_has_its_six_calls():
    from fsrl_amd import _lib
    if not os.path.exists(LIB):
        pytest.fail("libfsrl_hip.so is not built (fsrl_amd/csrc/build.sh cross-compiles it without a GPU)")
    src = open(os.path.join(ROOT, "include", "fsrl_hip.h")).read()
    # the comment block above fsrl_collect_group_create names the fourth kind of member and what stays a caller error
    block = src[src.index("Lock-step collection for seeds that keep their own streams"):src.index("int fsrl_collect_group_create(")]
    for phrase in ("ON-POLICY members", "CPO", "TRPO-Lag", "fsrl_group", "max_action", "unbounded", "caller error"):
        assert phrase in block, phrase
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(fsrl_[a-z0-9_]+)\s*\(", code))
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.split()[-1].startswith("fsrl_")}
    assert declared == exported == set(_lib.SIGNATURES)
    assert {s for s in declared if s.startswith("fsrl_collect_group")} == {
        "fsrl_collect_group_create", "fsrl_collect_group_destroy", "fsrl_collect_group_step", "fsrl_collect_group_actor_set_resident",
        "fsrl_collect_group_actor_resident_stats", "fsrl_collect_group_actor_release"}
    assert not any("trust" in s for s in declared)               # the members' own fsrl_tr_* / fsrl_cpo_* / fsrl_trpo_* calls
