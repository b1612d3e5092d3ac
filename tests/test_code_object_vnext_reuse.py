"""The two kernels of process_fn's V(obs_next) reuse in the built library's gfx950 code object, read on the host (no GPU;
tools/sonotes.py as in test_code_object.py): the gather launch with its flagging sibling (batch_gather_flag_kernel) exists beside the
plain gather, which every other caller still launches; mlp_infer_kernel, which now also walks a list of rows, keeps zero spilled
VGPRs, zero bytes of scratch and the VGPR budget of its workgroup size at every width (128 at 1024 threads); and the shipped library reads FSRL_NO_VNEXT_REUSE, so that the twin
context of tests/test_gpu_ppo_vnext_reuse.py really evaluates every row."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "fsrl_amd", "libfsrl_hip.so")


@pytest.fixture(scope="module")
def notes():
    assert os.path.exists(LIB), "libfsrl_hip.so is not built"
    import sonotes
    return sonotes.kernel_notes(LIB)


def test_both_gather_launches_exist(notes):
    for want in ("batch_gather_kernel", "batch_gather_flag_kernel"):
        fam = {n: k for n, k in notes.items() if want + "10StorePtrs" in n or n.startswith("_Z%d%s" % (len(want), want))}
        assert fam, want
        for name, k in fam.items():
            assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (name, k)


def test_infer_kernel_keeps_its_register_budget(notes):
    fam = {n: k for n, k in notes.items() if n.startswith("_Z16mlp_infer_kernelILi")}
    assert len(fam) == 3, sorted(fam)                       # hidden 64, 128, 256
    for name, k in fam.items():
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (name, k)
        # one workgroup of 4 H threads must fit a CU: 512 VGPRs per SIMD lane over its waves per SIMD (1024 threads: 128)
        assert k["vgpr_count"] <= 512 // max(1, k["max_flat_workgroup_size"] // 256), (name, k)


def test_the_shipped_library_reads_the_switch():
    with open(LIB, "rb") as f:
        assert b"FSRL_NO_VNEXT_REUSE\0" in f.read()
