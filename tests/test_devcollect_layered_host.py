"""Layered device collects without a GPU: the two C ABI entry points in the built library, in the header and in the Python prototypes;
the 12 lay_collect_kernel instantiations in the gfx950 code object (registers read with tools/sonotes.py, as
tests/test_code_object.py does); and the collectors' routing between the fused and the layered calls, on stub engines."""
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "fsrl_amd", "libfsrl_hip.so")
ENVS = {"12DevEnvLinear", "17DevEnvPointCircle"}
PAIRS = (("fsrl_collect_device_layered", "fsrl_collect_device_group"), ("fsrl_evaluate_device_layered", "fsrl_evaluate_device_group"))


def test_entry_points_are_exported_declared_and_bound():
    assert os.path.exists(LIB), "libfsrl_hip.so is not built"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    exported = {ln.split()[-1] for ln in out.stdout.splitlines() if ln.strip()}
    assert {name for name, _ in PAIRS} <= exported
    with open(os.path.join(ROOT, "include", "fsrl_hip.h")) as f:
        header = f.read()
    from fsrl_amd import _lib
    norm = lambda s: re.sub(r"\s+", " ", s).strip()
    for name, twin in PAIRS:
        decl, ref = (re.search(r"\bint %s\(([^;]*)\);" % n, header) for n in (name, twin))
        assert decl and ref, name
        assert norm(decl.group(1)) == norm(ref.group(1)), "the layered call takes its _group twin's arguments"
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[twin]
    import fsrl_amd.engine as E
    for fn in ("collect_device_layered", "evaluate_device_layered"):
        assert callable(getattr(E, fn)) and callable(getattr(E.Engine, fn))


def test_layered_collect_kernels_fit_their_launch_and_do_not_spill():
    """lay_collect_kernel<Env, HEAD, STORE>: 2 envs x 3 heads x store / store-less = 12 kernels, one for every shape; zero spilled
    VGPRs, no private segment, VGPRs within what a workgroup of its launch bound leaves a lane (512 per SIMD lane over the waves of
    one SIMD), LDS within the 160 KiB of a gfx950 CU"""
    assert os.path.exists(LIB), "libfsrl_hip.so is not built"
    import sonotes
    notes = sonotes.kernel_notes(LIB)
    pat = re.compile(r"^_Z\d+lay_collect_kernelI(\d+[A-Za-z]+)Li(\d)ELb([01])EE")
    seen = set()
    for name, k in notes.items():
        m = pat.match(name)
        if not m:
            assert "lay_collect_kernel" not in name, name
            continue
        seen.add((m.group(1), int(m.group(2)), int(m.group(3))))
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (name, k)
        threads = k["max_flat_workgroup_size"]
        assert threads % 256 == 0 and 256 <= threads <= 1024, (name, k)
        assert k["vgpr_count"] <= 512 // (threads // 256), (name, k)         # waves per SIMD = threads / 64 / 4
        assert k["group_segment_fixed_size"] <= 160 * 1024, (name, k)
    assert seen == {(env, head, store) for env in ENVS for head in (0, 1, 2) for store in (0, 1)}, sorted(seen)


# ---------------------------------------------------------------------------------------------------- routing, on stub engines
RESULT = dict(steps=7, total_cost=1.0, terminated=0, truncated=1, ep_rews=np.array([2.0]), ep_lens=np.array([7]), launches=1)


class _Eng:
    def __init__(self, hidden_sizes=None, force_layered=False):
        self.cfg = SimpleNamespace(hidden_sizes=hidden_sizes, force_layered=force_layered, obs_dim=6, act_dim=2)
        self.calls = []

    def devenv_create(self, *a):
        return 1

    def devenv_destroy(self, h):
        pass

    def devenv_reset(self, h, n, ids=None):
        return np.zeros((n, 6), np.float32)

    def _run(self, name):
        def run(h, n_episode, *a):
            self.calls.append(name)
            return dict(RESULT)
        return run

    def __getattr__(self, name):
        if name in ("collect_device", "evaluate_device", "collect_device_layered", "evaluate_device_layered"):
            return self._run(name)
        raise AttributeError(name)


class _Pol:
    training, _deterministic_eval, action_bound_method, action_scaling, action_space = True, True, "clip", False, None

    def __init__(self, eng):
        self.engine = eng


class _Buf:
    buffer_num = 2

    def reset(self, keep_statistics=False):
        pass

    def sync_sizes(self):
        pass


SHAPES = [(None, False, False), ((64, 64), False, False), ((64, 64), True, True), ((32, 32, 32), False, True), ((512, 512), False, True),
          ((64, ), False, True)]


def test_solo_collectors_route_on_the_engines_shape():
    from fsrl_amd.data import DeviceCollector
    from fsrl_amd.data.device_collector import DeviceEvalCollector
    from fsrl_amd.env import DevicePointCircle
    for hidden_sizes, force_layered, layered in SHAPES:
        eng = _Eng(hidden_sizes, force_layered)
        env = DevicePointCircle(eng, 2)
        train, test = DeviceCollector(_Pol(eng), env, _Buf()), DeviceCollector(_Pol(eng), env)
        assert isinstance(test, DeviceEvalCollector)
        assert train.collect(n_episode=1)["n/ep"] == 1 and test.collect(n_episode=1)["n/st"] == 7
        tail = "_layered" if layered else ""
        assert eng.calls == ["collect_device" + tail, "evaluate_device" + tail], (hidden_sizes, force_layered)
        assert (train.collect_step, train.collect_episode, test.collect_step) == (7, 1, 7)


def test_group_collector_routes_a_whole_group_and_refuses_a_mixed_one(monkeypatch):
    import fsrl_amd.engine as E
    from fsrl_amd.data import DeviceCollector, GroupDeviceCollector
    from fsrl_amd.env import DevicePointCircle
    calls = []
    for fn in ("collect_device_group", "evaluate_device_group", "collect_device_layered", "evaluate_device_layered"):
        def run(engines, handles, n_episodes, *a, _fn=fn):
            calls.append((_fn, len(engines), list(n_episodes)))
            return [dict(RESULT) for _ in engines]
        monkeypatch.setattr(E, fn, run)

    def cols(shapes, store):
        engs = [_Eng(*s) for s in shapes]
        return [DeviceCollector(_Pol(e), DevicePointCircle(e, 2), _Buf() if store else None) for e in engs]
    lay, fus = ((32, 32, 32), False), ((64, 64), False)
    for shapes, store, want in (([lay, lay], True, "collect_device_layered"), ([lay, lay, lay], False, "evaluate_device_layered"),
                                ([fus, fus], True, "collect_device_group"), ([fus, (None, False)], False, "evaluate_device_group"),
                                ([((64, 64), True)], True, "collect_device_layered")):
        g = GroupDeviceCollector(cols(shapes, store))
        assert g.layered == want.endswith("layered")
        stats = g.collect(n_episode=2)
        assert len(stats) == len(shapes) and calls[-1] == (want, len(shapes), [2] * len(shapes))
    with pytest.raises(AssertionError, match="member 2 is a fused engine and member 0 a layered one"):
        GroupDeviceCollector(cols([lay, lay, fus], True))
    with pytest.raises(AssertionError, match="member 1 is a layered engine and member 0 a fused one"):
        GroupDeviceCollector(cols([fus, lay], False))


def test_evaluation_collector_steps_a_layered_engine_and_the_explicit_collector_does_not():
    """evaluation_collector and the shape rule stay as they were; DeviceCollector(policy, env) is the way to a device evaluation"""
    from fsrl_amd.data import DeviceCollector, FastCollector, evaluation_collector
    from fsrl_amd.data.device_collector import _layered
    from fsrl_amd.env import DevicePointCircle
    assert [_layered(_Eng(hs, fl)) for hs, fl, _ in SHAPES] == [lay for _, _, lay in SHAPES]
    lay = _Eng((32, 32, 32))
    env = DevicePointCircle(lay, 2)
    assert isinstance(evaluation_collector(_Pol(lay), env), FastCollector)
    DeviceCollector(_Pol(lay), env).collect(n_episode=1)
    assert lay.calls == ["evaluate_device_layered"]


def test_example_help_names_the_layered_device_collect():
    src = open(os.path.join(ROOT, "examples", "train_agent.py")).read()
    assert "fsrl_collect_device_layered" in src
