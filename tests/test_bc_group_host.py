"""Grouped behaviour cloning without a GPU: fsrl_bc_update_group in the built library, the header and the bindings; the registers of
every bc_*_group_kernel instantiation in the gfx950 code object (tools/sonotes.py, as tests/test_bc_host.py reads the solo kernels')."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "fsrl_amd", "libfsrl_hip.so")

def test_bc_update_group_is_exported_declared_and_bound():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert "fsrl_bc_update_group" in {ln.split()[-1] for ln in out.stdout.splitlines() if ln.strip()}
    with open(os.path.join(ROOT, "include", "fsrl_hip.h")) as f:
        decl = re.search(r"\bint fsrl_bc_update_group\(([^;]*)\);", f.read())
    assert decl, "fsrl_bc_update_group is not declared in include/fsrl_hip.h"
    from fsrl_amd import _lib
    assert len(_lib.SIGNATURES["fsrl_bc_update_group"][1]) == decl.group(1).count(",") + 1 == 9

def test_bc_group_kernel_instantiations_do_not_spill():
    # H = 64 / 128 / 256 x the three heads, and bc_wgrad_group_kernel<H>: the member lookup costs scalar registers only -- no spills,
    # no scratch, inside the 128-VGPR cap of 4 H threads like the solo kernels
    import sonotes
    pat = re.compile(r"^_Z\d+(bc_fwd_bwd_group_kernel|bc_wgrad_group_kernel)ILi(\d+)E(?:Li(\d)E)?E")
    seen = set()
    for name, k in sonotes.kernel_notes(LIB).items():
        m = pat.match(name)
        if not m:
            continue
        seen.add((m.group(1), int(m.group(2)), m.group(3) and int(m.group(3))))
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (name, k)
        assert k["vgpr_count"] <= 128, (name, k)
    assert seen == ({("bc_fwd_bwd_group_kernel", H, head) for H in (64, 128, 256) for head in (0, 1, 2)} |
                    {("bc_wgrad_group_kernel", H, None) for H in (64, 128, 256)}), sorted(seen, key=str)
