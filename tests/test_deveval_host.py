"""Device evaluations without a GPU: the two C ABI entry points in the built library, in the header and in the Python prototypes;
the 18 store-less kernels in the gfx950 code object (registers read with tools/sonotes.py, as tests/test_code_object.py does); the
Python side that needs no device (the helper's choice of collector, the group collector's refusal of a mix, the example's option);
and the host replay of an evaluation (fsrl_amd/csrc/devcollect_plan.hpp dc_eval_row) against dc_replay_row as a stand-alone program,
tests/host/deveval_sim.cpp -- its own process, nothing preloaded, nothing loaded into Python, built with the address / undefined-
behaviour sanitizers."""
import importlib.util
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "fsrl_amd", "libfsrl_hip.so")
SRC = os.path.join(ROOT, "tests", "host", "deveval_sim.cpp")
ENVS = {"12DevEnvLinear", "17DevEnvPointCircle"}


def test_eval_replay_equals_the_collect_replay(tmp_path):
    exe = str(tmp_path / "deveval_sim")
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
    assert oks == ["replay", "restart", "all"], out.stdout
    f = dict(kv.split("=") for kv in next(ln for ln in out.stdout.splitlines() if ln.startswith("ok replay")).split()[2:])
    assert int(f["logs"]) >= 400 and int(f["episodes"]) > 1000 and int(f["many_env_logs"]) > 0


def test_entry_points_are_exported_declared_and_bound():
    assert os.path.exists(LIB), "libfsrl_hip.so is not built"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    exported = {ln.split()[-1] for ln in out.stdout.splitlines() if ln.strip()}
    assert {"fsrl_evaluate_device", "fsrl_evaluate_device_group"} <= exported
    with open(os.path.join(ROOT, "include", "fsrl_hip.h")) as f:
        header = f.read()
    from fsrl_amd import _lib
    for name, twin in (("fsrl_evaluate_device", "fsrl_collect_device"), ("fsrl_evaluate_device_group", "fsrl_collect_device_group")):
        decl, ref = (re.search(r"\bint %s\(([^;]*)\);" % n, header) for n in (name, twin))
        assert decl and ref, name
        norm = lambda s: re.sub(r"\s+", " ", s).strip()
        assert norm(decl.group(1)) == norm(ref.group(1)), "the evaluation takes the collect's arguments"
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[twin]


def test_storeless_kernels_are_the_table_driven_family_and_do_not_spill():
    """evaluate_device_group_kernel<H, Env, HEAD>: 3 widths x 2 envs x 3 heads = 18 kernels, no solo form; zero spilled VGPRs, no
    scratch, inside the 128-VGPR cap of 4 H threads -- next to the one storing family, which has no solo form either"""
    assert os.path.exists(LIB), "libfsrl_hip.so is not built"
    import sonotes
    notes = sonotes.kernel_notes(LIB)
    pat = re.compile(r"^_Z\d+(evaluate_device\w*|collect_device\w*)ILi(\d+)E(\d+[A-Za-z]+)Li(\d)EE")
    seen = {}
    for name, k in notes.items():
        m = pat.match(name)
        if not m:
            continue
        seen.setdefault(m.group(1), set()).add((int(m.group(2)), m.group(3), int(m.group(4))))
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (name, k)
        assert k["vgpr_count"] <= 128, (name, k)
    want = {(H, env, head) for H in (64, 128, 256) for env in ENVS for head in (0, 1, 2)}
    assert set(seen) == {"evaluate_device_group_kernel", "collect_device_group_kernel"}, sorted(seen)
    for fam, got in seen.items():
        assert got == want, (fam, sorted(want ^ got))


class _Eng:
    def __init__(self, hidden_sizes=None, force_layered=False):
        from types import SimpleNamespace
        self.cfg = SimpleNamespace(hidden_sizes=hidden_sizes, force_layered=force_layered, obs_dim=6, act_dim=2)

    def devenv_create(self, *a):
        return 1

    def devenv_destroy(self, h):
        pass

    def devenv_reset(self, h, n, ids=None):
        import numpy as np
        return np.zeros((n, 6), np.float32)


class _Pol:
    def __init__(self, eng):
        self.engine = eng


def test_helper_picks_the_storeless_collector_only_where_the_device_takes_it():
    from fsrl_amd.data import DeviceCollector, FastCollector, evaluation_collector
    from fsrl_amd.data.device_collector import _layered
    from fsrl_amd.env import DevicePointCircle, SyntheticSafetyVectorEnv
    assert [_layered(_Eng(hs, fl)) for hs, fl in ((None, False), ((64, 64), False), ((256, 48), False), ((64, 64), True), ((32, 32, 32), False),
                                                  ((512, 512), False), ((64, ), False))] == [False, False, False, True, True, True, True]
    eng = _Eng()
    pol, env = _Pol(eng), DevicePointCircle(eng, 2)
    assert evaluation_collector(pol, None) is None
    col = evaluation_collector(pol, env)
    assert isinstance(col, DeviceCollector) and col.buffer is None and col.env is env
    col.reset_buffer()                                                      # nothing to reset, nothing raised
    assert isinstance(evaluation_collector(pol, env, render=True), FastCollector)
    assert isinstance(evaluation_collector(_Pol(_Eng()), env), FastCollector)                     # an env of another engine: stepped
    lay = _Eng((32, 32, 32))
    assert isinstance(evaluation_collector(_Pol(lay), DevicePointCircle(lay, 2)), FastCollector)
    host = SyntheticSafetyVectorEnv(env_num=2, obs_dim=6, act_dim=2, episode_len=5)
    assert isinstance(evaluation_collector(pol, host), FastCollector)


def test_group_collector_refuses_a_mix_without_a_device():
    from fsrl_amd.data import DeviceCollector, GroupDeviceCollector
    from fsrl_amd.env import DevicePointCircle

    class Buf:
        buffer_num = 2

        def reset(self, keep_statistics=False):
            pass
    engs = [_Eng(), _Eng()]
    cols = [DeviceCollector(_Pol(engs[0]), DevicePointCircle(engs[0], 2)), DeviceCollector(_Pol(engs[1]), DevicePointCircle(engs[1], 2), Buf())]
    with pytest.raises(AssertionError, match="mix of store-less and storing"):
        GroupDeviceCollector(cols)
    assert GroupDeviceCollector(cols[:1]).store is False and GroupDeviceCollector(cols[1:]).store is True


def test_example_takes_test_episodes(capsys):
    spec = importlib.util.spec_from_file_location("train_multi_seed", os.path.join(ROOT, "examples", "train_multi_seed.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.parse_args(["--grouped"]).test_episodes == 0 and mod.make_evaluator(mod.parse_args(["--grouped"]), []) is None
    assert mod.parse_args(["--grouped", "--task", "device-linear", "--test-episodes", "4"]).test_episodes == 4
    for argv in (["--test-episodes", "3"], ["--grouped", "--test-episodes", "-1"]):
        with pytest.raises(SystemExit):
            mod.parse_args(argv)
        assert "--test-episodes" in capsys.readouterr().err
    src = open(os.path.join(ROOT, "examples", "train_multi_seed.py")).read()
    assert "DeviceCollector(ag.policy, env)" in src and "GroupDeviceCollector(self.cols)" in src
