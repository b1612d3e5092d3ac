"""Groups of layered FOCOPS contexts on the host (no GPU): the grouped loss-head kernel in the cross-compiled gfx950 code object
(no spills, no scratch), the solo head kernel it shares its body with unchanged, and PolicyGroup over FOCOPS policies whose
engines are layered, on a fake engine group."""
import os
import sys

import pytest
import torch

from fsrl_amd.policy import PolicyGroup
from fsrl_amd.policy.focops import FOCOPS_KEYS

from test_group_focops_host import _Buf, _FakeGroup, _focops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "fsrl_amd", "libfsrl_hip.so")
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))
import sonotes  # noqa: E402


def _notes():
    if not os.path.exists(LIB):
        pytest.fail("libfsrl_hip.so is not built (fsrl_amd/csrc/build.sh cross-compiles it without a GPU)")
    return sonotes.kernel_notes(LIB)


def test_grouped_focops_head_kernel_is_in_the_code_object_without_spills():
    ks = {n: k for n, k in _notes().items() if "lay_fb_head_group_kernel" in n}
    assert len(ks) == 1, sorted(ks)
    (k, ) = ks.values()
    assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k
    assert k["max_flat_workgroup_size"] == 256, k


# (VGPRs, LDS bytes) of the solo head kernel, read from a build of the parent commit (where the kernel held its body itself): as a
# one-line call of lay_fb_head_body it compiles to what it did
PARENT = {"_Z18lay_fb_head_kernel13LayFbHeadArgs": (26, 512)}


def test_solo_head_kernel_compiles_to_what_it_did():
    notes = _notes()
    for name, (vgprs, lds) in PARENT.items():
        assert name in notes, name
        k = notes[name]
        assert (k["vgpr_count"], k["group_segment_fixed_size"]) == (vgprs, lds), (name, k)
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (name, k)


# ---------------------------------------------------------------------------------------------------- PolicyGroup over a stub
class _LayeredCfg:
    """what a policy group may look at of an engine's configuration: nothing of its network shape"""
    hidden, hidden_sizes, force_layered = 0, (64, 48, 32), False


def _layered_focops(*a, **kw):
    p = _focops(*a, **kw)
    p.engine.cfg = _LayeredCfg()
    return p


def test_policy_group_takes_focops_policies_whose_engines_are_layered():
    args = [(10.0, 3.7, 0.01), (5.0, 12.25, 0.3), (25.0, 0.5, 1.99)]
    pols = [_layered_focops(*a) for a in args]
    twins = [_focops(*a) for a in args]
    fg = _FakeGroup(steps=[6, 2, 4], stopped=[-1, 0, -1])
    grp = PolicyGroup(pols, engine_group=fg)
    out = grp.update([_Buf(p) for p in pols], batch_size=64, repeat=2)
    for t in twins:
        t.process_fn(None, _Buf(t), None, batch_size=64)
    # the nu step per member: FOCOPS.process_fn's
    assert list(zip(fg.calls[0][0], fg.calls[0][1])) == [t.engine.lib.set_nu[-1] for t in twins]
    assert all(torch.equal(p._nu, t._nu) for p, t in zip(pols, twins))
    assert out == [{"gradient_steps": 6, "early_stop_pass": -1}, {"gradient_steps": 2, "early_stop_pass": 0},
                   {"gradient_steps": 4, "early_stop_pass": -1}]
    for p, n in zip(pols, (6, 2, 4)):
        rows = p.logger.rows
        assert len(rows) == 3 * n + 1 and set().union(*rows[:-1]) == set(FOCOPS_KEYS)
        assert rows[-1] == {"gradient_steps": p.gradient_steps} and p.stale == 1 and not p.updating


def test_a_failed_update_of_layered_members_marks_mirrors_stale():
    pols = [_layered_focops(10.0, 1.0, 0.1), _layered_focops(10.0, 2.0, 0.2)]
    grp = PolicyGroup(pols, engine_group=_FakeGroup(fail=True))
    with pytest.raises(RuntimeError, match="device error"):
        grp.update([_Buf(p) for p in pols])
    assert all(p.stale == 1 and not p.updating and p.logger.rows == [] for p in pols)


def test_engine_group_focops_update_leaves_a_closed_member_to_the_grouped_call():
    """nu / nu_loss go to the members that are still alive; a closed member (null context) is left for fsrl_group_ppo_update, which
    names the destroyed member, instead of failing in fsrl_focops_set_nu with "null ctx" """
    import numpy as np
    from fsrl_amd import _lib
    from fsrl_amd.engine import EngineGroup

    class Lib:
        def __init__(self): self.set_nu = []
        def fsrl_focops_set_nu(self, ctx, nu, nl):
            assert ctx, "null ctx"
            self.set_nu.append((ctx, nu, nl))
            return 0

    class Eng:
        def __init__(self, ctx): self._ctx = ctx

    grp = EngineGroup.__new__(EngineGroup)
    grp.lib, grp.engines, grp._g = Lib(), [Eng(None), Eng(7)], None
    calls = []

    def ppo_update(lags, resc, batch_size, repeat, perms=None, seed=0):
        calls.append((batch_size, repeat, seed))
        return [np.zeros((0, _lib.PPO_NSTATS), np.float32)] * 2, [-1, -1]
    grp.ppo_update = ppo_update
    st, sp = grp.focops_update([0.2, 0.4], [0.0, 0.1], 64, 1, seed=9)
    assert grp.lib.set_nu == [(7, 0.4, 0.1)] and calls == [(64, 1, 9)]
    assert [s.shape for s in st] == [(0, _lib.FOCOPS_NSTATS)] * 2 and sp == [-1, -1]
