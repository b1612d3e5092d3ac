"""Sweep groups on the host (no GPU): PolicyGroup.update over PPOLagrangian policies with a stand-in engine group -- ints take
EngineGroup.ppo_update exactly as before, a sequence for batch_size or repeat takes ppo_update_each with one value per member -- and
the --sweep option of examples/train_multi_seed.py."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from fsrl_amd.policy import PolicyGroup
from fsrl_amd.policy.ppo_lag import PPO_STAT_KEYS, PPOLagrangian

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _FakeGroup:
    """stands in for EngineGroup; only_ppo_update: the stand-in of the older host tests, which has no ppo_update_each"""

    def __init__(self, steps, stopped):
        self.calls, self.steps, self.stopped = [], list(steps), list(stopped)

    def _answer(self):
        return [np.full((n, len(PPO_STAT_KEYS)), float(i), np.float32) for i, n in enumerate(self.steps)], self.stopped

    def ppo_update(self, lags, resc, batch_size, repeat, perms=None, seed=0):
        self.calls.append(("ppo_update", np.asarray(lags).tolist(), list(resc), batch_size, repeat, perms, seed))
        return self._answer()

    def ppo_update_each(self, lags, resc, batch_sizes, repeats, perms=None, seed=0):
        self.calls.append(("ppo_update_each", np.asarray(lags).tolist(), list(resc), batch_sizes, repeats, perms, seed))
        return self._answer()

    def close(self):
        pass


class _OnlyPpoUpdate:
    def __init__(self, inner):
        self.ppo_update, self.close = inner.ppo_update, inner.close


class _Log:
    def __init__(self):
        self.rows, self.printed = [], []

    def store(self, tab=None, **kw):
        self.rows.append(dict(kw))

    def print(self, *a, **k):
        self.printed.append(a[0] if a else "")


class _Eng:
    pass


class _Buf:
    def __init__(self, p):
        self.engine = p.engine


def _ppol(lag, use_lagrangian=True, steps=0):
    p = PPOLagrangian.__new__(PPOLagrangian)
    torch.nn.Module.__init__(p)
    p.engine = _Eng()
    p.use_lagrangian, p.critics_num = use_lagrangian, 2
    p.lagrangians_and_rescaling = lambda: ([lag], 1.0 / (1.0 + lag))
    p.gradient_steps, p.logger, p.updating, p.stale, p.sched = steps, _Log(), False, 0, 0
    p._step_lr_scheduler = lambda: setattr(p, "sched", p.sched + 1)
    p._mark_stale = lambda: setattr(p, "stale", p.stale + 1)
    return p


def _group(steps, stopped, only_ppo_update=False):
    pols = [_ppol(0.25), _ppol(0.5, use_lagrangian=False), _ppol(1.0, steps=7)]
    fg = _FakeGroup(steps, stopped)
    return pols, fg, PolicyGroup(pols, engine_group=_OnlyPpoUpdate(fg) if only_ppo_update else fg)


def test_ints_take_ppo_update_exactly_as_before():
    pols, fg, grp = _group([4, 4, 4], [-1, -1, -1], only_ppo_update=True)      # a stand-in without ppo_update_each is enough
    grp.update([_Buf(p) for p in pols], batch_size=128, repeat=2)
    grp.update([_Buf(p) for p in pols], batch_size=np.int64(64), repeat=np.int32(3), perms=[[0]] * 3)
    (name, lags, resc, bs, rp, perms, seed), second = fg.calls
    assert name == second[0] == "ppo_update"
    assert lags == [[0.25], [0.0], [1.0]] and resc == [1 / 1.25, 1.0, 1 / 2.0]           # a member without the Lagrangian term: 0, 1
    assert (bs, rp, perms) == (128, 2, None) and seed != 0
    assert second[3:6] == (64, 3, [[0]] * 3) and second[6] == 0                            # given permutations: no shuffle seed


def test_sequences_take_ppo_update_each_with_one_value_per_member():
    pols, fg, grp = _group([4, 6, 1], [-1, 2, -1])
    perms = [[np.arange(4)] * 2, [np.arange(4)] * 3, [np.arange(4)]]
    out = grp.update([_Buf(p) for p in pols], batch_size=[64, 32, 150], repeat=(2, 3, 1), perms=perms)
    name, lags, resc, bs, rp, got_perms, seed = fg.calls[0]
    assert name == "ppo_update_each" and bs == [64, 32, 150] and rp == [2, 3, 1] and got_perms is perms and seed == 0
    assert lags == [[0.25], [0.0], [1.0]] and resc == [1 / 1.25, 1.0, 1 / 2.0]
    # per member, as with ints: its rows, gradient_steps, the early-stop message, the scheduler step, stale mirrors
    assert out == [{"gradient_steps": 4, "early_stop_pass": -1}, {"gradient_steps": 6, "early_stop_pass": 2},
                   {"gradient_steps": 1, "early_stop_pass": -1}]
    assert [p.gradient_steps for p in pols] == [4, 6, 8]
    assert [p.logger.printed for p in pols] == [[], ["Early stop at step 2 due to reaching max kl."], []]
    assert all(p.sched == 1 and p.stale == 1 and not p.updating for p in pols)
    assert [len(p.logger.rows) for p in pols] == [4 + 1, 6 + 1, 1 + 1]
    assert "loss/lagrangian" in pols[0].logger.rows[0] and "loss/lagrangian" not in pols[1].logger.rows[0]
    # one of the two may stay an int: it is repeated
    grp.update([_Buf(p) for p in pols], batch_size=256, repeat=[4, 0, 2])
    assert fg.calls[1][0] == "ppo_update_each" and fg.calls[1][3] == [256] * 3 and fg.calls[1][4] == [4, 0, 2] and fg.calls[1][6] != 0
    with pytest.raises(AssertionError, match="one batch_size and one repeat per member"):
        grp.update([_Buf(p) for p in pols], batch_size=[64, 32], repeat=2)
    assert not any(p.updating for p in pols)


def _example():
    spec = importlib.util.spec_from_file_location("train_multi_seed", os.path.join(ROOT, "examples", "train_multi_seed.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_examples_sweep_option(capsys):
    ex = _example()
    a = ex.parse_args(["--grouped", "--seeds", "3", "--sweep", "eps_clip=0.1,0.2,0.3", "--sweep", "target_kl=none,0.01,0.02",
                       "--sweep", "batch_size=64,128,256", "--sweep", "repeat_per_collect=2,4,0"])
    assert a.sweep == {"eps_clip": [0.1, 0.2, 0.3], "target_kl": [None, 0.01, 0.02], "batch_size": [64, 128, 256],
                       "repeat_per_collect": [2, 4, 0]}
    assert ex.parse_args(["--grouped", "--seeds", "3"]).sweep == {}
    every = ex.SWEEP_AGENT_KEYS + ex.SWEEP_UPDATE_KEYS
    assert every == ("eps_clip", "dual_clip", "vf_coef", "max_grad_norm", "target_kl", "lr", "gae_lambda", "gamma", "cost_limit",
                     "batch_size", "repeat_per_collect")
    for name in every:
        assert list(ex.parse_args(["--grouped", "--seeds", "2", "--sweep", name + "=1,2"]).sweep) == [name]
    bad = [(["--grouped", "--seeds", "3", "--sweep", "eps_clip=0.1,0.2"], "2 values for 3 seeds"),
           (["--grouped", "--seeds", "2", "--sweep", "l2_reg=0.1,0.2"], "NAME one of eps_clip"),
           (["--grouped", "--seeds", "2", "--sweep", "eps_clip"], "NAME=v1,v2"),
           (["--grouped", "--seeds", "2", "--sweep", "eps_clip=a,b"], "not a number"),
           (["--grouped", "--seeds", "2", "--sweep", "eps_clip=none,0.1"], "not a number"),
           (["--grouped", "--seeds", "2", "--sweep", "batch_size=0,64"], "batch_size >= 1"),
           (["--grouped", "--seeds", "2", "--sweep", "lr=1e-3,1e-4", "--sweep", "lr=1e-3,1e-4"], "given twice"),
           (["--grouped", "--seeds", "2", "--sweep", "max_grad_norm=0.5,none"], "agree on whether the clip is on"),
           (["--seeds", "2", "--sweep", "lr=1e-3,1e-4"], "PPO-Lagrangian groups only"),
           (["--grouped", "--algo", "focops", "--seeds", "2", "--sweep", "lr=1e-3,1e-4"], "PPO-Lagrangian groups only"),
           # an existing refusal and its text
           (["--grouped", "--algo", "focops", "--hidden-sizes", "64x48x32"], "layered seeds")]
    for argv, why in bad:
        with pytest.raises(SystemExit):
            ex.parse_args(argv)
        assert why in capsys.readouterr().err, (argv, why)


def test_the_new_entry_point_is_declared_with_per_member_arrays():
    from fsrl_amd import _lib
    import ctypes as C
    res, args = _lib.SIGNATURES["fsrl_group_ppo_update_each"]
    one = _lib.SIGNATURES["fsrl_group_ppo_update"][1]
    assert res is C.c_int and len(args) == len(one) == 11
    i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    assert (args[3], args[4], args[8]) == (i32p, i32p, i64p) and (one[3], one[4], one[8]) == (C.c_int32, C.c_int32, C.c_int64)
    assert [a for j, a in enumerate(args) if j not in (3, 4, 8)] == [a for j, a in enumerate(one) if j not in (3, 4, 8)]
