"""Wide layered device collects without a GPU: the entry point in the built library, the header and the bindings; the registers and
LDS of every wide_layered_step_kernel instantiation in the gfx950 code object (tools/sonotes.py); the collectors' routing on stub
engines; and the preconditions of the row-by-row cases of tests/test_gpu_devcollect_wide_layered.py from the float32 model."""
import os
import re
import subprocess
import sys

import test_devcollect_layered_host as lh

ROOT, LIB, ENVS = lh.ROOT, lh.LIB, lh.ENVS


def test_entry_point_is_exported_declared_and_bound():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert "fsrl_collect_device_wide_layered" in {ln.split()[-1] for ln in out.stdout.splitlines() if ln.strip()}
    header = open(os.path.join(ROOT, "include", "fsrl_hip.h")).read()
    from fsrl_amd import _lib
    from fsrl_amd.engine import Engine
    norm = lambda s: re.sub(r"\s+", " ", s).strip()
    decl, ref = (re.search(r"\bint %s\(([^;]*)\);" % n, header) for n in ("fsrl_collect_device_wide_layered", "fsrl_collect_device_wide"))
    assert decl and ref and norm(decl.group(1)) == norm(ref.group(1)) and decl.group(1).count(",") + 1 == 16
    assert _lib.SIGNATURES["fsrl_collect_device_wide_layered"] == _lib.SIGNATURES["fsrl_collect_device_wide"]
    assert callable(Engine.collect_device_wide_layered)
    plan = open(os.path.join(ROOT, "fsrl_amd", "csrc", "devcollect_plan.hpp")).read()
    assert int(re.search(r"#define DCWL_LDS_WIDTH (\d+)\b", plan).group(1)) == _lib.DCWL_LDS_WIDTH


def test_wide_layered_kernels_fit_their_launch_and_do_not_spill():
    """wide_layered_step_kernel<Env, HEAD, DEVWS>: 2 envs x 3 heads x the LDS / device-memory form = 12 kernels for every shape"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import sonotes
    from fsrl_amd._lib import DCWL_LDS_WIDTH as W
    dyn = 2 * 16 * (W if (W // 4) % 2 else W + 4) * 4          # dc_wl_lds_bytes(DCWL_LDS_WIDTH), the largest dynamic request
    pat = re.compile(r"^_Z\d+wide_layered_step_kernelI(\d+[A-Za-z]+)Li(\d)ELb([01])EE")
    seen = set()
    for name, k in sonotes.kernel_notes(LIB).items():
        m = pat.match(name)
        if not m:
            assert "wide_layered_step_kernel" not in name, name
            continue
        seen.add((m.group(1), int(m.group(2)), int(m.group(3))))
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (name, k)
        threads = k["max_flat_workgroup_size"]
        assert threads % 256 == 0 and k["vgpr_count"] <= 512 // (threads // 256), (name, k)          # waves per SIMD = threads / 64 / 4
        assert k["group_segment_fixed_size"] + (0 if int(m.group(3)) else dyn) <= 160 * 1024, (name, k)
    assert seen == {(env, head, devws) for env in ENVS for head in (0, 1, 2) for devws in (0, 1)}, sorted(seen)


class _Eng(lh._Eng):
    def devenv_create(self, *a, **kw):
        return 1

    def __getattr__(self, name):
        return self._run(name) if name in ("collect_device_wide", "collect_device_wide_layered") else super().__getattr__(name)


def test_collector_routes_a_wide_env_on_the_engines_shape():
    from fsrl_amd.data import DeviceCollector
    from fsrl_amd.env import DevicePointCircle
    for hidden_sizes, force_layered, layered in lh.SHAPES:
        eng = _Eng(hidden_sizes, force_layered)
        for wide, want in ((True, "collect_device_wide_layered" if layered else "collect_device_wide"),
                           (False, "collect_device_layered" if layered else "collect_device")):
            DeviceCollector(lh._Pol(eng), DevicePointCircle(eng, 2, wide=wide), lh._Buf()).collect(n_episode=1)
            assert eng.calls[-1] == want, (hidden_sizes, force_layered, wide)


def test_row_cases_stay_out_of_the_discontinuity_band():
    """no row's cost decision lies in the band, and a surplus drop takes positions out of several tiles at once"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_devcollect_wide_layered as gwl
    for case in gwl.ROW_CASES:
        for deterministic in (False, True):
            rows, near = gwl.model_rows(case, deterministic)
            assert len(rows) == len(near) and not near.any(), (case, deterministic, int(near.sum()))
        live, at, spread = list(range(case[2])), 0, 0        # the vector steps of the row list: a step's rows are its live list
        while at + len(live) < len(rows):
            at += len(live)
            nxt = [r[0] for r in rows[at:at + len(live)]]
            nxt = nxt[:next((i for i in range(1, len(nxt)) if nxt[i] <= nxt[i - 1]), len(nxt))]      # the list is ascending: it ends where ids stop rising
            spread = max(spread, len({p // 16 for p, e in enumerate(live) if e not in set(nxt)}))
            live = nxt
        assert spread > 1, case
