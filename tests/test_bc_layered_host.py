"""Layered behaviour cloning without a GPU: fsrl_bc_update_layered in the built library, the header and the bindings; the registers of
every bc_lay_* kernel instantiation in the gfx950 code object (tools/sonotes.py, as tests/test_bc_host.py reads them)."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "fsrl_amd", "libfsrl_hip.so")

def test_bc_update_layered_is_exported_declared_and_bound():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert "fsrl_bc_update_layered" in {ln.split()[-1] for ln in out.stdout.splitlines() if ln.strip()}
    with open(os.path.join(ROOT, "include", "fsrl_hip.h")) as f:
        decl = re.search(r"\bint fsrl_bc_update_layered\(([^;]*)\);", f.read())
    assert decl, "fsrl_bc_update_layered is not declared in include/fsrl_hip.h"
    from fsrl_amd import _lib
    assert len(_lib.SIGNATURES["fsrl_bc_update_layered"][1]) == decl.group(1).count(",") + 1 == 7

def test_bc_lay_kernel_instantiations_do_not_spill():
    # heads x {LDS, HBM} operand homes of the tile kernel and the one weight-gradient kernel: nothing per shape, no spills, no scratch
    import sonotes
    pat = re.compile(r"^_Z\d+(bc_lay_\w+?_kernel)(?:ILi(\d)ELb([01])EE)?")
    seen = set()
    for name, k in sonotes.kernel_notes(LIB).items():
        m = pat.match(name)
        if not m:
            continue
        seen.add((m.group(1), m.group(2) and int(m.group(2)), m.group(3) and int(m.group(3))))
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (name, k)
    assert seen == ({("bc_lay_fwd_bwd_kernel", head, form) for head in (0, 1, 2) for form in (0, 1)} |
                    {("bc_lay_wgrad_kernel", None, None)}), sorted(seen, key=str)
