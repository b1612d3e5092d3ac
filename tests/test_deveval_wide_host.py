"""Wide device evaluations without a GPU: the entry points in the library, the header and the bindings; registers and LDS of every
wide_eval(_layered)_step_kernel instantiation (tools/sonotes.py); the episode-row rule as a sanitized stand-alone program."""
import os
import re
import subprocess
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "fsrl_amd", "libfsrl_hip.so")
SRC = os.path.join(ROOT, "tests", "host", "deveval_wide_sim.cpp")
ENVS = {"12DevEnvLinear", "17DevEnvPointCircle"}
NAMES = ("fsrl_evaluate_device_wide", "fsrl_evaluate_device_wide_layered")


def test_entry_points_are_exported_declared_and_bound_like_the_wide_collect():
    assert os.path.exists(LIB), "libfsrl_hip.so is not built"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert set(NAMES) <= {ln.split()[-1] for ln in out.stdout.splitlines() if ln.strip()}
    with open(os.path.join(ROOT, "include", "fsrl_hip.h")) as f:
        header = f.read()
    from fsrl_amd import _lib
    params = {name: re.sub(r"\s+", " ", re.search(r"\bint %s\(([^;]*)\);" % name, header).group(1)) for name in NAMES + ("fsrl_collect_device_wide", )}
    for name in NAMES:
        assert params[name] == params["fsrl_collect_device_wide"], name
        assert [a.__name__ for a in _lib.SIGNATURES[name][1]] == [a.__name__ for a in _lib.SIGNATURES["fsrl_collect_device_wide"][1]], name


def test_wide_evaluation_kernels_do_not_spill_and_take_no_more_lds_than_their_collects():
    assert os.path.exists(LIB), "libfsrl_hip.so is not built"
    import sonotes
    pat = re.compile(r"^_Z\d+wide_(eval|collect|eval_layered|layered)_step_kernelI(?:Li(\d+)E)?(\d+[A-Za-z]+)Li(\d)E(?:Lb([01])E)?E")
    seen = {}
    for name, k in sonotes.kernel_notes(LIB).items():
        m = pat.match(name)
        if m:
            seen.setdefault(m.group(1), {})[(int(m.group(2) or m.group(5)), m.group(3), int(m.group(4)))] = k
            if m.group(1).startswith("eval"):
                assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (name, k)
    assert set(seen["eval"]) == {(H, env, head) for H in (64, 128, 256) for env in ENVS for head in (0, 1, 2)}, sorted(seen["eval"])
    assert set(seen["eval_layered"]) == {(devws, env, head) for devws in (0, 1) for env in ENVS for head in (0, 1, 2)}, sorted(seen["eval_layered"])
    for fam, twin in (("eval", "collect"), ("eval_layered", "layered")):
        for key, k in seen[fam].items():
            assert k["group_segment_fixed_size"] <= seen[twin][key]["group_segment_fixed_size"] and k["vgpr_count"] <= (128 if fam == "eval" else 256), (fam, key, k)


def test_episode_row_rule_against_a_sequential_walk(tmp_path):
    exe = str(tmp_path / "deveval_wide_sim")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "fsrl_amd", "csrc"), SRC, "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr
    assert [ln.split()[1] for ln in out.stdout.splitlines() if ln.startswith("ok ")] == ["rows", "all"], out.stdout
