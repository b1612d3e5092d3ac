"""CVPOPolicyGroup on the host (no GPU): a fake engine group stands in for fsrl_cvpo_group_update.  Per member the group must pass
its count, run a fresh policy's keying update alone, keep the bookkeeping of n_i calls of policy.update (gradient_steps, pending
rows and the ring drain, lr scheduler steps, stale mirrors), and refuse what it cannot group.  Plus what can be checked of the
native side without a GPU: the C ABI's symbols, the grouped kernels in the gfx950 code object, the example's argument check."""
import ctypes
import importlib.util
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "fsrl_amd", "libfsrl_hip.so")
SYMBOLS = ("fsrl_cvpo_group_create", "fsrl_cvpo_group_destroy", "fsrl_cvpo_group_update")


class _FakeGroup:
    def __init__(self, fail=False):
        self.calls, self.fail = [], fail

    def update(self, batch_size, n_updates):
        if self.fail:
            raise RuntimeError("device error")
        self.calls.append((batch_size, list(n_updates)))

    def close(self):
        pass


class _Sched:
    def __init__(self):
        self.n = 0


def _policy(steps=1, sched=False):
    from fsrl_amd.policy.cvpo import CVPO
    p = CVPO.__new__(CVPO)
    p.engine = object()
    p._reference_rng, p._seed, p._pending = False, 0, 0
    p.gradient_steps = steps
    p.lr_scheduler = _Sched() if sched else None
    p._dirty = p._rest_dirty = False
    p.drained, p.own = 0, []
    p._step_lr_scheduler = lambda: setattr(p.lr_scheduler, "n", p.lr_scheduler.n + 1) if p.lr_scheduler else None
    p._drain = lambda: (setattr(p, "drained", p.drained + p._pending), setattr(p, "_pending", 0))
    p._mark_stale = lambda: None

    def own_update(B, buf):                        # CVPO.update of one batch: what a fresh policy's keying update runs
        p.own.append(B)
        p.gradient_steps += 1
        p._pending += 1
        p.updating = False
    p.update = own_update
    return p


class _Buf:
    def __init__(self, p):
        self.engine = p.engine


def test_passes_each_members_count():
    from fsrl_amd.policy import CVPOPolicyGroup
    pols = [_policy(), _policy(), _policy()]
    fg = _FakeGroup()
    out = CVPOPolicyGroup(pols, engine_group=fg).update([_Buf(p) for p in pols], 128, [4, 0, 2])
    assert fg.calls == [(128, [4, 0, 2])] and out == [{}, {}, {}]
    assert [p.gradient_steps for p in pols] == [5, 1, 3]
    assert [p._pending for p in pols] == [4, 0, 2]
    assert pols[0]._dirty and pols[0]._rest_dirty and not pols[1]._dirty
    assert not any(getattr(p, "updating", False) for p in pols)


def test_a_fresh_policys_first_update_runs_alone():
    from fsrl_amd.policy import CVPOPolicyGroup
    pols = [_policy(steps=0), _policy(steps=7), _policy(steps=0)]
    fg = _FakeGroup()
    CVPOPolicyGroup(pols, engine_group=fg).update([_Buf(p) for p in pols], 64, [3, 2, 0])
    assert [p.own for p in pols] == [[64], [], []]             # keyed with seed + 1 inside CVPO.learn; no update, no keying
    assert fg.calls == [(64, [2, 2, 0])]
    assert [p.gradient_steps for p in pols] == [3, 9, 0]


def test_scheduler_steps_one_update_per_call():
    from fsrl_amd.policy import CVPOPolicyGroup
    pols = [_policy(sched=True), _policy()]
    fg = _FakeGroup()
    CVPOPolicyGroup(pols, engine_group=fg).update([_Buf(p) for p in pols], 64, [3, 1])
    assert [c[1] for c in fg.calls] == [[1, 1], [1, 0], [1, 0]]
    assert pols[0].lr_scheduler.n == 3


def test_statistics_ring_is_drained_where_learn_drains_it():
    from fsrl_amd.policy import CVPOPolicyGroup
    p = _policy()
    p._pending = 2000
    fg = _FakeGroup()
    CVPOPolicyGroup([p], engine_group=fg).update([_Buf(p)], 64, 100)
    assert [c[1] for c in fg.calls] == [[48], [52]]
    assert p.drained == 2048 and p._pending == 52


def test_rejects_what_cannot_be_grouped():
    from fsrl_amd.policy import CVPOPolicyGroup
    from fsrl_amd.policy.sac_lag import SACLagrangian
    p, q = _policy(), _policy()
    q._reference_rng = True
    with pytest.raises(AssertionError, match="reference_rng"):
        CVPOPolicyGroup([p, q], engine_group=_FakeGroup())
    with pytest.raises(AssertionError, match="CVPO policies"):
        CVPOPolicyGroup([p, SACLagrangian.__new__(SACLagrangian)], engine_group=_FakeGroup())
    grp = CVPOPolicyGroup([p], engine_group=_FakeGroup())
    with pytest.raises(AssertionError, match="buffer"):
        grp.update([_Buf(_policy())], 64, [1])
    with pytest.raises(AssertionError, match="n_updates"):
        grp.update([_Buf(p)], 64, [-1])


def test_failure_marks_every_mirror_stale():
    from fsrl_amd.policy import CVPOPolicyGroup
    pols = [_policy(), _policy()]
    with pytest.raises(RuntimeError):
        CVPOPolicyGroup(pols, engine_group=_FakeGroup(fail=True)).update([_Buf(p) for p in pols], 64, [1, 1])
    assert all(p._dirty and p._rest_dirty and not p.updating for p in pols)


def test_symbols_in_header_binding_table_and_library():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fsrl_hip.h")).read(), flags=re.S)
    from fsrl_amd import _lib
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, src) and s in _lib.SIGNATURES, s
    if not os.path.exists(LIB):
        pytest.skip("libfsrl_hip.so is not built")
    lib = ctypes.CDLL(LIB)
    for s in SYMBOLS:
        assert hasattr(lib, s), s


def test_grouped_kernels_are_in_the_code_object_without_spills_or_scratch():
    if not os.path.exists(LIB):
        pytest.skip("libfsrl_hip.so is not built")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import sonotes
    notes = sonotes.kernel_notes(LIB)
    for fam, at_least in (("cvpo_sample_gather_group_kernel", 1), ("cvpo_actor_group_kernel", 18), ("cvpo_estep_group_kernel", 1),
                          ("cvpo_mdual_group_kernel", 1), ("cvpo_adam_group_kernel", 2)):
        ks = [k for n, k in notes.items() if fam in n]
        assert len(ks) >= at_least, (fam, len(ks))          # actor: 3 widths x 2 tile heights x 3 launches
        for k in ks:
            assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (fam, k)


def test_example_accepts_grouped_cvpo():
    spec = importlib.util.spec_from_file_location("train_multi_seed", os.path.join(ROOT, "examples", "train_multi_seed.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "cvpo" in mod.GROUPED_ALGOS and callable(mod.run_grouped_replay)
    src = open(os.path.join(ROOT, "examples", "train_multi_seed.py")).read()
    assert "a.algo in GROUPED_ALGOS" in src and "CVPOPolicyGroup" in src
