"""Grouped prioritised replay on the host (no GPU): the new group kernels in the cross-compiled gfx950 code object (no spills, no
scratch, the solo kernels' register and LDS footprint, since they inline the same bodies), the solo kernels unchanged, the replay
policy group's rule that its members agree on prioritised replay, and the multi-seed example's --per-* arguments."""
import importlib.util
import os
import sys

import pytest

from fsrl_amd.policy import SACPolicyGroup

from test_sac_group_host import _FakeGroup, _policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "fsrl_amd", "libfsrl_hip.so")
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))
import sonotes  # noqa: E402

# (VGPRs, LDS bytes) of the solo prioritised kernels, read from a build of the parent commit: factoring their bodies out for the
# group kernels left them what they were
SOLO = {
    "_Z17per_sample_kernel13SacSampleArgs6PerDev8PerBatchi": (72, 16384),
    "_Z17per_update_kernel6PerDev6PerUpd": (74, 8192),
}
GROUP = {"per_sample_group_kernel": "per_sample_kernel", "per_update_group_kernel": "per_update_kernel"}


def test_group_kernels_are_in_the_code_object_with_the_solo_kernels_footprint():
    if not os.path.exists(LIB):
        pytest.fail("libfsrl_hip.so is not built (fsrl_amd/csrc/build.sh cross-compiles it without a GPU)")
    notes = sonotes.kernel_notes(LIB)
    for name, (vgprs, lds) in SOLO.items():
        assert name in notes, name
        k = notes[name]
        assert (k["vgpr_count"], k["group_segment_fixed_size"]) == (vgprs, lds), (name, k)
    for grouped, solo in GROUP.items():
        gk = [k for n, k in notes.items() if grouped in n]
        sk = [k for n, k in notes.items() if solo + "13Sac" in n or solo + "6PerDev" in n]
        assert len(gk) == 1 and len(sk) == 1, (grouped, solo)
        assert gk[0]["max_flat_workgroup_size"] == 1024
        assert gk[0]["group_segment_fixed_size"] == sk[0]["group_segment_fixed_size"]
        assert gk[0]["vgpr_count"] <= sk[0]["vgpr_count"] + 8, (grouped, gk[0], sk[0])
        assert gk[0]["vgpr_spill_count"] == 0 and gk[0]["private_segment_fixed_size"] == 0, (grouped, gk[0])
    gather = [k for n, k in notes.items() if "sac_gather_group_kernel" in n]
    assert len(gather) == 1 and gather[0]["vgpr_spill_count"] == 0 and gather[0]["private_segment_fixed_size"] == 0


class _Engine:
    def __init__(self, per_on):
        self.per_on = per_on


def test_replay_policy_group_members_agree_on_prioritised_replay():
    def pols(flags):
        out = [_policy(0.5) for _ in flags]
        for p, f in zip(out, flags):
            p.engine = _Engine(f)
        return out
    SACPolicyGroup(pols([True, True]), engine_group=_FakeGroup())
    SACPolicyGroup(pols([False, False]), engine_group=_FakeGroup())
    for flags in ([True, False], [False, True, True]):
        with pytest.raises(AssertionError, match="HipPrioritizedVectorReplayBuffer"):
            SACPolicyGroup(pols(flags), engine_group=_FakeGroup())


def _example():
    spec = importlib.util.spec_from_file_location("train_multi_seed", os.path.join(ROOT, "examples", "train_multi_seed.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("algo", ["sacl", "ddpgl"])
def test_example_takes_the_prioritised_replay_flags(algo):
    mod = _example()
    a = mod.parse_args(["--grouped", "--algo", algo, "--seeds", "8", "--per-alpha", "0.7", "--per-beta", "0.5", "--per-no-weight-norm"])
    assert a.grouped and mod.prioritized_replay(a) == dict(alpha=0.7, beta=0.5, weight_norm=False)
    a = mod.parse_args(["--algo", algo, "--per-alpha", "0.6"])
    assert mod.prioritized_replay(a) == dict(alpha=0.6, beta=0.4, weight_norm=True)
    assert mod.prioritized_replay(mod.parse_args(["--grouped", "--algo", algo])) is None


@pytest.mark.parametrize("argv,reason", [
    (["--grouped", "--algo", "cvpo", "--per-alpha", "0.6"], "no per-row TD error"),
    (["--algo", "cvpo", "--per-alpha", "0.6", "--per-beta", "0.4"], "no per-row TD error"),
    (["--grouped", "--algo", "ppol", "--per-alpha", "0.6"], "built for sacl and ddpgl, not ppol"),
    (["--grouped", "--algo", "sacl", "--per-beta", "0.4"], "--per-alpha switches on"),
    (["--grouped", "--algo", "sacl", "--per-no-weight-norm"], "--per-alpha switches on"),
    (["--grouped", "--algo", "sacl", "--per-alpha", "-1"], ">= 0"),
])
def test_example_refuses_the_flags_with_the_reason(argv, reason, capsys):
    mod = _example()
    with pytest.raises(SystemExit):
        mod.parse_args(argv)
    assert reason in capsys.readouterr().err
