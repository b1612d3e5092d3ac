"""Wide device collects without a GPU: the two C ABI entry points in the built library, the header and the bindings; the registers of
every wide_collect_step_kernel instantiation in the gfx950 code object (tools/sonotes.py, as tests/test_code_object.py reads them);
and the per-position surplus rule of the kernel (fsrl_amd/csrc/devcollect_plan.hpp) against dc_episode_end as a stand-alone program,
tests/host/devcollect_wide_sim.cpp -- its own process, built with the address / undefined-behaviour sanitizers."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "fsrl_amd", "libfsrl_hip.so")
SRC = os.path.join(ROOT, "tests", "host", "devcollect_wide_sim.cpp")
ENVS = {"12DevEnvLinear", "17DevEnvPointCircle"}


def test_entry_points_are_exported_and_declared():
    assert os.path.exists(LIB), "libfsrl_hip.so is not built"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    exported = {ln.split()[-1] for ln in out.stdout.splitlines() if ln.strip()}
    assert {"fsrl_devenv_create_wide", "fsrl_collect_device_wide"} <= exported
    with open(os.path.join(ROOT, "include", "fsrl_hip.h")) as f:
        header = f.read()
    from fsrl_amd import _lib
    for name, n_args in (("fsrl_devenv_create_wide", 3), ("fsrl_collect_device_wide", 16)):
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert decl, name + " is not declared in include/fsrl_hip.h"
        assert len(_lib.SIGNATURES[name][1]) == decl.group(1).count(",") + 1 == n_args
    assert re.search(r"#define DCW_MAX_ENVS 4096\b", header) and _lib.DCW_MAX_ENVS == 4096


def test_wide_kernel_instantiations_do_not_spill():
    """wide_collect_step_kernel<H, Env, HEAD> for H = 64 / 128 / 256 x both envs x the three heads: zero spilled VGPRs, no scratch,
    inside the 128-VGPR cap of 4 H threads"""
    assert os.path.exists(LIB), "libfsrl_hip.so is not built"
    import sonotes
    pat = re.compile(r"^_Z\d+wide_collect_step_kernelILi(\d+)E(\d+[A-Za-z]+)Li(\d)EE")
    seen = set()
    for name, k in sonotes.kernel_notes(LIB).items():
        m = pat.match(name)
        if not m:
            continue
        seen.add((int(m.group(1)), m.group(2), int(m.group(3))))
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (name, k)
        assert k["vgpr_count"] <= 128, (name, k)
    assert seen == {(H, env, head) for H in (64, 128, 256) for env in ENVS for head in (0, 1, 2)}, sorted(seen)


def test_position_rule_against_dc_episode_end(tmp_path):
    exe = str(tmp_path / "devcollect_wide_sim")
    # -static-lib*san: a dynamically linked sanitizer runtime must be the first library loaded (tests/test_train_state_host.py)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "fsrl_amd", "csrc"), SRC, "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr
    assert [ln.split()[1] for ln in out.stdout.splitlines() if ln.startswith("ok ")] == ["rule", "all"], out.stdout


def test_row_cases_stay_out_of_the_discontinuity_band():
    """the precondition of the row-by-row cases of tests/test_gpu_devcollect_wide.py, from the float32 model alone: no row's cost
    decision lies in the band, costs occur, and a surplus drop takes positions out of several tiles at once"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_devcollect_wide as gw
    for case in gw.ROW_CASES:
        for deterministic in (False, True):
            rows, near = gw.model_rows(case, deterministic)
            assert len(rows) == len(near) and not near.any(), (case, deterministic, int(near.sum()))
        live, at, spread = list(range(case[2])), 0, 0        # the vector steps of the row list: a step's rows are its live list
        while at + len(live) < len(rows):
            at += len(live)
            nxt = [r[0] for r in rows[at:at + len(live)]]
            nxt = nxt[:next((i for i in range(1, len(nxt)) if nxt[i] <= nxt[i - 1]), len(nxt))]      # the list is ascending: it ends where ids stop rising
            spread = max(spread, len({p // 16 for p, e in enumerate(live) if e not in set(nxt)}))
            live = nxt
        assert spread > 1, case
