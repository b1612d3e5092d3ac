"""Groups of layered CVPO contexts on the host (no GPU): the new grouped head kernel in the cross-compiled gfx950 code object (no
spills, no scratch) next to the solo head it shares its body with, CVPOPolicyGroup over a stub engine group with layered engines,
and the group benchmark's `--hidden` argument."""
import importlib.util
import os
import sys

import pytest

from test_cvpo_group_host import _Buf, _FakeGroup, _policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "fsrl_amd", "libfsrl_hip.so")
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))
import sonotes  # noqa: E402


def test_layered_cvpo_group_head_is_in_the_code_object_without_spills():
    if not os.path.exists(LIB):
        pytest.fail("libfsrl_hip.so is not built (fsrl_amd/csrc/build.sh cross-compiles it without a GPU)")
    notes = sonotes.kernel_notes(LIB)
    grouped = {n: k for n, k in notes.items() if "lay_cvpo_actor_head_group_kernel" in n}
    solo = {n: k for n, k in notes.items() if "lay_cvpo_actor_head_kernel" in n}
    assert len(grouped) == 1 and len(solo) == 1, (sorted(grouped), sorted(solo))
    (g, ), (s, ) = grouped.values(), solo.values()
    for k in (g, s):
        assert k["max_flat_workgroup_size"] == 256
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k
    # one body: the same LDS (the 16 x 4 per-row sums of the MFWD head); the solo kernel's (VGPRs, LDS bytes) are those of a build
    # of the parent commit, where the body was the kernel itself
    assert (s["vgpr_count"], s["group_segment_fixed_size"]) == (35, 256), s
    assert g["group_segment_fixed_size"] == 256


class _LayeredEngine:
    """what a policy group may look at of an engine: nothing of its network shape"""

    class cfg:
        hidden, hidden_sizes, force_layered = 0, (64, 48, 32), False


def test_cvpo_policy_group_takes_policies_whose_engines_are_layered():
    from fsrl_amd.policy import CVPOPolicyGroup
    pols = [_policy(), _policy(), _policy()]
    for p in pols:
        p.engine = _LayeredEngine()
    fg = _FakeGroup()
    out = CVPOPolicyGroup(pols, engine_group=fg).update([_Buf(p) for p in pols], 64, [3, 0, 1])
    assert fg.calls == [(64, [3, 0, 1])] and out == [{}, {}, {}]        # (batch_size, n_updates) unchanged
    assert [p.gradient_steps for p in pols] == [4, 1, 2] and [p._pending for p in pols] == [3, 0, 1]


def _bench():
    spec = importlib.util.spec_from_file_location("bench_group_cvpo", os.path.join(ROOT, "tools", "bench_group_cvpo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_group_bench_parses_hidden_and_defaults_to_the_shapes_own_layers():
    mod = _bench()
    a = mod.build_parser().parse_args(["--hidden", "64x48x32", "--ks", "1,8"])
    assert a.hidden == (64, 48, 32) and a.ks == "1,8"
    assert mod.build_parser().parse_args(["--hidden", "256X256X256"]).hidden == (256, 256, 256)
    a = mod.build_parser().parse_args([])
    assert a.hidden is None and a.shapes == "default,wide"
    assert mod.SHAPES["default"]["H"] == 128 and mod.SHAPES["wide"]["H"] == 256         # what `hidden or (H, H)` falls back to
