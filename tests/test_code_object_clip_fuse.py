"""The weight-gradient kernel that clips and steps itself (ppo_wgrad_kernel<H, false, true, true>, kernels_mlp.hpp) in the built
library's gfx950 code object, read on the host (no GPU; tools/sonotes.py as in test_code_object.py): the instantiation exists at
H = 64, 128 and 256, spills no register, uses no scratch, and stays within the 128 VGPRs and the LDS that let a 1024-thread workgroup
launch on every CU -- its workgroups wait for each other, so all of them must be resident at once."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "fsrl_amd", "libfsrl_hip.so")
PREFIX = "_Z16ppo_wgrad_kernelILi"


@pytest.fixture(scope="module")
def family():
    assert os.path.exists(LIB), "libfsrl_hip.so is not built"
    import sonotes
    fam = {n: k for n, k in sonotes.kernel_notes(LIB).items() if n.startswith(PREFIX)}
    assert fam, "no ppo_wgrad_kernel in the code object's metadata note"
    return fam


@pytest.mark.parametrize("H", [64, 128, 256])
def test_no_spill_no_scratch_and_one_workgroup_per_cu(family, H):
    want = "%s%dELb0ELb1ELb1EE" % (PREFIX, H)                 # <H, BIG = false, FUSE = true, CLIP = true>
    hits = [k for n, k in family.items() if n.startswith(want)]
    assert len(hits) == 1, (want, sorted(family))
    k = hits[0]
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k
    assert k["vgpr_count"] <= 128, k                          # 512 VGPRs per SIMD lane / 4 waves per SIMD of a 1024-thread workgroup
    assert k["max_flat_workgroup_size"] == 1024 and k["group_segment_fixed_size"] <= 64 * 1024, k


def test_the_other_forms_are_still_there(family):
    for H in (64, 128, 256):
        for fuse in (0, 1):
            assert any(n.startswith("%s%dELb0ELb%dELb0EE" % (PREFIX, H, fuse)) for n in family), (H, fuse)


def test_the_shipped_library_reads_the_switch():
    with open(LIB, "rb") as f:
        assert b"FSRL_NO_CLIP_FUSE\0" in f.read()
