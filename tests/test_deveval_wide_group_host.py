"""Grouped wide device evaluations without a GPU: the entry point in the library, the header and the bindings, its refusals that come
before any device call, and registers and LDS of every wide_eval(_layered)_group_step_kernel instantiation (tools/sonotes.py) against
its solo counterpart."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "fsrl_amd", "libfsrl_hip.so")
ENVS = {"12DevEnvLinear", "17DevEnvPointCircle"}
NAME = "fsrl_evaluate_device_wide_group"
FSRL_MAX_GROUP = 16


def test_entry_point_is_exported_declared_and_bound_like_the_grouped_wide_collect():
    assert os.path.exists(LIB), "libfsrl_hip.so is not built"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert NAME in {ln.split()[-1] for ln in out.stdout.splitlines() if ln.strip()}
    with open(os.path.join(ROOT, "include", "fsrl_hip.h")) as f:
        header = f.read()
    from fsrl_amd import _lib, engine
    params = [re.sub(r"\s+", " ", re.search(r"\bint %s\(([^;]*)\);" % n, header).group(1)) for n in (NAME, "fsrl_collect_device_wide_group")]
    assert params[0] == params[1]
    assert [a.__name__ for a in _lib.SIGNATURES[NAME][1]] == [a.__name__ for a in _lib.SIGNATURES["fsrl_collect_device_wide_group"][1]]
    with open(os.path.join(ROOT, "fsrl_amd", "csrc", "kernels_devcollect.hpp")) as f:
        assert int(re.search(r"#define FSRL_MAX_GROUP (\d+)", f.read()).group(1)) == FSRL_MAX_GROUP
    assert callable(engine.evaluate_device_wide_group)


@pytest.mark.parametrize("k,arrays,match", [(0, True, "k 0: .*1..16 members"), (FSRL_MAX_GROUP + 1, True, "k 17: .*1..16 members"), (2, False, "null argument")])
def test_refusals_before_any_device_call(k, arrays, match):
    """a member count outside 1..FSRL_MAX_GROUP and null arrays: FSRL_EINVAL, no context is read and no device is touched"""
    from fsrl_amd import _lib
    lib = _lib.load()
    ptrs, n_ep = (C.c_void_p * 17)(), (C.c_int32 * 17)(*([3] * 17))
    rc = lib.fsrl_evaluate_device_wide_group(ptrs if arrays else None, ptrs if arrays else None, k, n_ep if arrays else None, 1, 1, None, None, 3,
                                             None, None, None, None, None, None, None, None)
    assert rc == _lib.FSRL_EINVAL
    with pytest.raises(AssertionError, match=match):
        _lib.check(rc)


def test_grouped_wide_evaluation_kernels_do_not_spill_and_take_no_more_lds_than_their_solo_kernels():
    assert os.path.exists(LIB), "libfsrl_hip.so is not built"
    import sonotes
    pat = re.compile(r"^_Z\d+wide_eval(_layered)?(_group)?_step_kernelI(?:Li(\d+)E)?(\d+[A-Za-z]+)Li(\d)E(?:Lb([01])E)?E")
    seen = {}
    for name, k in sonotes.kernel_notes(LIB).items():
        m = pat.match(name)
        if m:
            seen.setdefault((bool(m.group(1)), bool(m.group(2))), {})[(int(m.group(3) or m.group(6)), m.group(4), int(m.group(5)))] = k
    assert set(seen[False, True]) == {(H, env, head) for H in (64, 128, 256) for env in ENVS for head in (0, 1, 2)}, sorted(seen[False, True])
    assert set(seen[True, True]) == {(devws, env, head) for devws in (0, 1) for env in ENVS for head in (0, 1, 2)}, sorted(seen[True, True])
    for layered in (False, True):
        for key, k in seen[layered, True].items():
            assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (key, k)
            assert k["group_segment_fixed_size"] <= seen[layered, False][key]["group_segment_fixed_size"], (key, k)
            assert k["vgpr_count"] <= (256 if layered else 128), (key, k)          # the launch bounds: 512 and at most 1024 threads
