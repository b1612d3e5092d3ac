"""Groups of layered SAC-Lag / DDPG-Lag contexts on the host (no GPU): the new group kernels in the cross-compiled gfx950 code
object (no spills, no scratch), the kernels they stand next to unchanged, the replay policy groups over a stub engine group with
layered engines, and the multi-seed example's argument handling."""
import importlib.util
import os
import sys

import pytest

from fsrl_amd.policy import DDPGPolicyGroup, SACPolicyGroup
from fsrl_amd.policy.ddpg_lag import DDPGLagrangian

from test_sac_group_host import _Buf, _FakeGroup, _policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "fsrl_amd", "libfsrl_hip.so")
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))
import sonotes  # noqa: E402


def _notes():
    if not os.path.exists(LIB):
        pytest.fail("libfsrl_hip.so is not built (fsrl_amd/csrc/build.sh cross-compiles it without a GPU)")
    return sonotes.kernel_notes(LIB)


def test_layered_replay_group_kernels_are_in_the_code_object_without_spills():
    notes = _notes()
    # template <int FORM, bool VEC, int NW> lin_sac_group_kernel: forward / activation-side / weight-side x float4 or dword loads x
    # 1, 2 or 4 column groups of waves
    lin = {n: k for n, k in notes.items() if "lin_sac_group_kernel" in n}
    for form in (0, 1, 2):
        for vec in (0, 1):
            for nw in (1, 2, 4):
                ks = [k for n, k in lin.items() if f"ILi{form}ELb{vec}ELi{nw}E" in n]
                assert len(ks) == 1, (form, vec, nw, sorted(lin))
                assert ks[0]["max_flat_workgroup_size"] == 256 * nw
    assert len(lin) == 18
    singles = ("lay_sac_actor_head_group_kernel", "lay_sac_q_head_group_kernel", "sac_sample_gather_group_kernel",
               "sac_nstep_group_kernel", "lay_raw_out_group_kernel")
    fam = dict(lin)
    for name in singles:
        ks = {n: k for n, k in notes.items() if name in n}
        assert len(ks) == 1, (name, sorted(ks))
        fam.update(ks)
    for n, k in fam.items():
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (n, k)


# (VGPRs, LDS bytes) of the kernels the new ones share their bodies with, read from a build of the parent commit: the PPO
# instantiations of lin_group_kernel and the solo heads of the layered replay update compile to what they did
PARENT = {
    "_Z16lin_group_kernelILi0ELb0ELi1EEvPK11LinGroupJobPK10GroupAgentPK9GroupStep": (164, 34816),
    "_Z16lin_group_kernelILi0ELb0ELi2EEvPK11LinGroupJobPK10GroupAgentPK9GroupStep": (98, 34816),
    "_Z16lin_group_kernelILi0ELb0ELi4EEvPK11LinGroupJobPK10GroupAgentPK9GroupStep": (58, 34816),
    "_Z16lin_group_kernelILi0ELb1ELi1EEvPK11LinGroupJobPK10GroupAgentPK9GroupStep": (156, 34816),
    "_Z16lin_group_kernelILi0ELb1ELi2EEvPK11LinGroupJobPK10GroupAgentPK9GroupStep": (87, 34816),
    "_Z16lin_group_kernelILi0ELb1ELi4EEvPK11LinGroupJobPK10GroupAgentPK9GroupStep": (53, 34816),
    "_Z16lin_group_kernelILi1ELb0ELi1EEvPK11LinGroupJobPK10GroupAgentPK9GroupStep": (180, 34816),
    "_Z16lin_group_kernelILi1ELb0ELi2EEvPK11LinGroupJobPK10GroupAgentPK9GroupStep": (108, 34816),
    "_Z16lin_group_kernelILi1ELb0ELi4EEvPK11LinGroupJobPK10GroupAgentPK9GroupStep": (71, 34816),
    "_Z16lin_group_kernelILi1ELb1ELi1EEvPK11LinGroupJobPK10GroupAgentPK9GroupStep": (168, 34816),
    "_Z16lin_group_kernelILi1ELb1ELi2EEvPK11LinGroupJobPK10GroupAgentPK9GroupStep": (97, 34816),
    "_Z16lin_group_kernelILi1ELb1ELi4EEvPK11LinGroupJobPK10GroupAgentPK9GroupStep": (61, 34816),
    "_Z16lin_group_kernelILi2ELb0ELi1EEvPK11LinGroupJobPK10GroupAgentPK9GroupStep": (196, 34832),
    "_Z16lin_group_kernelILi2ELb0ELi2EEvPK11LinGroupJobPK10GroupAgentPK9GroupStep": (124, 34848),
    "_Z16lin_group_kernelILi2ELb0ELi4EEvPK11LinGroupJobPK10GroupAgentPK9GroupStep": (106, 34880),
    "_Z16lin_group_kernelILi2ELb1ELi1EEvPK11LinGroupJobPK10GroupAgentPK9GroupStep": (200, 34832),
    "_Z16lin_group_kernelILi2ELb1ELi2EEvPK11LinGroupJobPK10GroupAgentPK9GroupStep": (134, 34848),
    "_Z16lin_group_kernelILi2ELb1ELi4EEvPK11LinGroupJobPK10GroupAgentPK9GroupStep": (86, 34880),
    "_Z21lay_sac_q_head_kernel11LaySacQArgs": (18, 0),
    "_Z25lay_sac_actor_head_kernel15LaySacActorArgs": (27, 256),
}


def test_ppo_group_and_solo_head_kernels_compile_to_what_they_did():
    notes = _notes()
    for name, (vgprs, lds) in PARENT.items():
        assert name in notes, name
        k = notes[name]
        assert (k["vgpr_count"], k["group_segment_fixed_size"]) == (vgprs, lds), (name, k)
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (name, k)


# ---------------------------------------------------------------------------------------------------- policy groups over a stub
class _LayeredEngine:
    """what a policy group may look at of an engine: nothing of its network shape"""

    class cfg:
        hidden, hidden_sizes, force_layered = 0, (64, 48, 32), False


def test_replay_policy_groups_take_policies_whose_engines_are_layered():
    pols = [_policy(0.5), _policy(2.0)]
    for p in pols:
        p.engine = _LayeredEngine()
    fg = _FakeGroup()
    grp = SACPolicyGroup(pols, engine_group=fg)
    grp.update([_Buf(p) for p in pols], 64, [3, 1])
    assert fg.calls == [(64, [3, 1], [[0.5], [2.0]], [1 / 1.5, 1 / 3.0])]
    assert [p.gradient_steps for p in pols] == [4, 2] and [p._pending for p in pols] == [3, 1]
    # the DDPG group is the same class over DDPGLagrangian policies
    d = _policy(0.25)
    d.__class__ = DDPGLagrangian
    d.engine = _LayeredEngine()
    fg = _FakeGroup()
    DDPGPolicyGroup([d], engine_group=fg).update([_Buf(d)], 32, [2])
    assert fg.calls == [(32, [2], [[0.25]], [1 / 1.25])]


# ---------------------------------------------------------------------------------------------------- the example's arguments
def _example():
    spec = importlib.util.spec_from_file_location("train_multi_seed", os.path.join(ROOT, "examples", "train_multi_seed.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("algo", ["sacl", "ddpgl", "ppol"])
def test_example_accepts_grouped_layered_seeds(algo):
    mod = _example()
    a = mod.parse_args(["--grouped", "--algo", algo, "--hidden-sizes", "64x48x32", "--seeds", "8"])
    assert a.grouped and a.algo == algo and a.hidden_sizes == (64, 48, 32) and a.seeds == 8
    assert mod.is_layered(a.hidden_sizes) and not mod.is_layered((128, 128)) and mod.is_layered((320, 64)) and mod.is_layered((64, ))


@pytest.mark.parametrize("algo", ["cvpo", "focops"])
def test_example_refuses_grouped_layered_seeds_that_do_not_group_yet(algo, capsys):
    mod = _example()
    with pytest.raises(SystemExit):
        mod.parse_args(["--grouped", "--algo", algo, "--hidden-sizes", "64x48x32"])
    assert "do not group yet" in capsys.readouterr().err
    assert mod.parse_args(["--grouped", "--algo", algo, "--hidden-sizes", "128x128"]).hidden_sizes == (128, 128)
