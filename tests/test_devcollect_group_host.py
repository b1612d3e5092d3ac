"""Grouped device collects without a GPU: the C ABI entry point in the built library and in the header, the group kernel's
instantiations in the gfx950 code object (registers read with tools/sonotes.py, as tests/test_code_object.py does), and the plain
host logic of fsrl_collect_device_group (fsrl_amd/csrc/devcollect_plan.hpp: episode offsets, launch cap, the "made no step" rule) as
a stand-alone program, tests/host/devcollect_group_sim.cpp -- its own process, nothing preloaded, nothing loaded into Python, built
with the address / undefined-behaviour sanitizers."""
import importlib.util
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "fsrl_amd", "libfsrl_hip.so")
SRC = os.path.join(ROOT, "tests", "host", "devcollect_group_sim.cpp")
ENVS = {"12DevEnvLinear", "17DevEnvPointCircle"}


def test_entry_point_is_exported_and_declared():
    assert os.path.exists(LIB), "libfsrl_hip.so is not built"
    with open(LIB, "rb") as f:
        blob = f.read()
    assert b"fsrl_collect_device_group\0" in blob and b"fsrl_store_version\0" in blob
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    exported = {ln.split()[-1] for ln in out.stdout.splitlines() if ln.strip()}
    assert {"fsrl_collect_device_group", "fsrl_collect_device", "fsrl_store_version"} <= exported
    with open(os.path.join(ROOT, "include", "fsrl_hip.h")) as f:
        header = f.read()
    decl = re.search(r"\bint fsrl_collect_device_group\(([^;]*)\);", header)
    assert decl, "fsrl_collect_device_group is not declared in include/fsrl_hip.h"
    args = decl.group(1)
    for name in ("fsrl_ctx** ctxs", "fsrl_devenv** envs", "int32_t k", "const int32_t* n_episode", "max_steps_per_launch", "launches_out"):
        assert name in args, name
    from fsrl_amd import _lib
    assert len(_lib.SIGNATURES["fsrl_collect_device_group"][1]) == args.count(",") + 1 == 17


def test_group_kernel_instantiations_do_not_spill():
    """collect_device_group_kernel<H, Env, HEAD> for H = 64 / 128 / 256 x both envs x the three heads: zero spilled VGPRs, no scratch,
    inside the 128-VGPR cap of 4 H threads.  It is the only storing family: the solo call is its one-member launch, and every kernel
    named collect_device* or evaluate_device* is one of the 18 + 18 table-driven ones"""
    assert os.path.exists(LIB), "libfsrl_hip.so is not built"
    import sonotes
    notes = sonotes.kernel_notes(LIB)
    pat = re.compile(r"^_Z\d+(collect_device\w*|evaluate_device\w*)ILi(\d+)E(\d+[A-Za-z]+)Li(\d)EE")
    seen = {}
    for name, k in notes.items():
        assert pat.match(name) or not re.match(r"^(_Z\d+)?(collect_device|evaluate_device)", name), name
        m = pat.match(name)
        if not m:
            continue
        seen.setdefault(m.group(1), set()).add((int(m.group(2)), m.group(3), int(m.group(4))))
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (name, k)
        assert k["vgpr_count"] <= 128, (name, k)
    want = {(H, env, head) for H in (64, 128, 256) for env in ENVS for head in (0, 1, 2)}
    assert set(seen) == {"collect_device_group_kernel", "evaluate_device_group_kernel"}, sorted(seen)
    assert seen["collect_device_group_kernel"] == want, sorted(want ^ seen["collect_device_group_kernel"])
    assert seen["evaluate_device_group_kernel"] == want, sorted(want ^ seen["evaluate_device_group_kernel"])


def test_example_takes_device_tasks_for_every_grouped_algo(capsys):
    spec = importlib.util.spec_from_file_location("train_multi_seed", os.path.join(ROOT, "examples", "train_multi_seed.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for algo in mod.GROUPED_ALGOS:
        for task in ("device-linear", "device-point-circle"):
            a = mod.parse_args(["--grouped", "--algo", algo, "--task", task, "--seeds", "4"])
            assert a.task == task and a.grouped
    assert mod.parse_args(["--grouped"]).task == "linear"
    for argv, why in ((["--task", "device-linear"], "--grouped"), (["--grouped", "--task", "device-linear", "--workers", "2"], "--workers 0"),
                      (["--grouped", "--task", "device-point-circle", "--envs", "65"], "at most 64 envs")):
        with pytest.raises(SystemExit):
            mod.parse_args(argv)
        assert why in capsys.readouterr().err
    src = open(os.path.join(ROOT, "examples", "train_multi_seed.py")).read()
    assert "GroupDeviceCollector(cols)" in src and "DeviceCollector(agent.policy, env, buf)" in src


def test_group_host_logic_against_brute_force(tmp_path):
    exe = str(tmp_path / "devcollect_group_sim")
    # -static-lib*san: a dynamically linked sanitizer runtime must be the first library loaded (tests/test_train_state_host.py)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "fsrl_amd", "csrc"), SRC, "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr
    oks = [ln.split()[1] for ln in out.stdout.splitlines() if ln.startswith("ok ")]
    assert oks == ["offsets", "cap", "stalled", "all"], out.stdout
    f = dict(kv.split("=") for kv in next(ln for ln in out.stdout.splitlines() if ln.startswith("ok stalled")).split()[2:])
    assert int(f["loops"]) >= 2000 and int(f["idle_relaunches"]) > 0 and int(f["injected"]) > 0
