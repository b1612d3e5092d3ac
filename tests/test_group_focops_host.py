"""PolicyGroup over FOCOPS policies on the host (no GPU): a fake engine group stands in for fsrl_group_ppo_update.  Per member the
group must pass the nu / nu_loss FOCOPS.process_fn would compute (the host float32 nu step), keep FOCOPS.learn's bookkeeping
(FOCOPS_KEYS rows, the early-stop message, gradient_steps, lr scheduler step, stale mirrors), refuse what it cannot group, and
leave every member out of its update with stale mirrors when the grouped update fails."""
import numpy as np
import pytest
import torch

from fsrl_amd.policy import FOCOPS, PolicyGroup
from fsrl_amd.policy.focops import FOCOPS_KEYS
from fsrl_amd.policy.ppo_lag import PPOLagrangian


class _FakeGroup:
    def __init__(self, steps=(), stopped=(), fail=False):
        self.calls, self.steps, self.stopped, self.fail = [], list(steps), list(stopped), fail

    def focops_update(self, nus, nu_losses, batch_size, repeat, perms=None, seed=0):
        if self.fail:
            raise RuntimeError("device error")
        self.calls.append((list(nus), list(nu_losses), batch_size, repeat, perms, seed))
        stats = [np.arange(n * len(FOCOPS_KEYS), dtype=np.float32).reshape(n, len(FOCOPS_KEYS)) + i for i, n in enumerate(self.steps)]
        return stats, self.stopped

    def close(self):
        pass


class _Log:
    def __init__(self):
        self.rows, self.printed = [], []

    def store(self, tab=None, **kw):
        self.rows.append(dict(kw))

    def print(self, *a, **k):
        self.printed.append(a[0] if a else "")


class _Sched:
    def __init__(self):
        self.n = 0


class _Lib:
    def __init__(self):
        self.set_nu = []

    def fsrl_focops_set_nu(self, ctx, nu, nu_loss):
        self.set_nu.append((nu, nu_loss))
        return 0


class _Eng:
    def __init__(self):
        self.lib, self._ctx = _Lib(), None

    def ppo_begin(self, lag, resc, batch_size):
        return 0


def _focops(cost_limit, ave_cost, nu0, nu_lr=0.01, nu_max=2.0, steps=3, sched=False, reference_rng=False):
    p = FOCOPS.__new__(FOCOPS)
    torch.nn.Module.__init__(p)
    p.engine = _Eng()
    p.cost_limit, p._ave_cost_return = cost_limit, ave_cost
    p._nu_max, p._nu_lr, p._nu = nu_max, nu_lr, torch.zeros(1) + nu0
    p._reference_rng = reference_rng
    p.gradient_steps = steps
    p.logger = _Log()
    p.lr_scheduler = _Sched() if sched else None
    p.updating = False
    p.stale = 0
    p._step_lr_scheduler = lambda: setattr(p.lr_scheduler, "n", p.lr_scheduler.n + 1) if p.lr_scheduler else None
    p._mark_stale = lambda: setattr(p, "stale", p.stale + 1)
    return p


class _Buf:
    def __init__(self, p):
        self.engine = p.engine


def test_passes_each_member_the_nu_step_of_process_fn():
    args = [(10.0, 3.7, 0.01), (5.0, 12.25, 0.3), (25.0, 0.5, 1.99)]
    pols = [_focops(*a) for a in args]
    twins = [_focops(*a) for a in args]
    fg = _FakeGroup(steps=[4, 4, 4], stopped=[-1, -1, -1])
    grp = PolicyGroup(pols, engine_group=fg)
    for rnd in range(2):                                  # nu carries over from one update to the next
        grp.update([_Buf(p) for p in pols], batch_size=128, repeat=2)
        for t in twins:
            t.process_fn(None, _Buf(t), None, batch_size=128)
        nus, nls = fg.calls[-1][0], fg.calls[-1][1]
        assert [(nu, nl) for nu, nl in zip(nus, nls)] == [t.engine.lib.set_nu[-1] for t in twins], rnd
        for p, t in zip(pols, twins):
            assert torch.equal(p._nu, t._nu)
    # the float32 tensor arithmetic of focops.py:155-158, clamp to [0, nu_max] included
    loss = 25.0 - 0.5
    assert fg.calls[0][0][2] == float(torch.clamp(torch.zeros(1) + 1.99 + (-0.01 * loss), 0, 2.0))
    assert fg.calls[0][1] == [10.0 - 3.7, 5.0 - 12.25, 25.0 - 0.5]
    assert fg.calls[0][2:4] == (128, 2) and fg.calls[0][4] is None and fg.calls[0][5] != fg.calls[1][5]


def test_keeps_focops_learn_bookkeeping():
    pols = [_focops(10.0, 1.0, 0.1, steps=3, sched=True), _focops(10.0, 1.0, 0.1, steps=0)]
    fg = _FakeGroup(steps=[8, 2], stopped=[-1, 0])
    grp = PolicyGroup(pols, engine_group=fg)
    perms = [[np.arange(4)], [np.arange(2)]]
    out = grp.update([_Buf(p) for p in pols], batch_size=64, repeat=4, perms=perms)
    assert fg.calls[0][4] is perms and fg.calls[0][5] == 0          # given permutations: no library shuffle seed
    assert out == [{"gradient_steps": 8, "early_stop_pass": -1}, {"gradient_steps": 2, "early_stop_pass": 0}]
    assert [p.gradient_steps for p in pols] == [11, 2]
    assert pols[0].lr_scheduler.n == 1 and all(p.stale == 1 and not p.updating for p in pols)
    assert pols[0].logger.printed == [] and pols[1].logger.printed == ["Early stop at step 0 due to reaching max kl."]
    for p, n in zip(pols, (8, 2)):
        rows = p.logger.rows
        assert len(rows) == 3 * n + 1                              # FOCOPS.learn's three stores per row, then gradient_steps
        assert set().union(*rows[:-1]) == set(FOCOPS_KEYS) and rows[-1] == {"gradient_steps": p.gradient_steps}


def test_refuses_mixed_classes_and_reference_rng():
    a = _focops(10.0, 1.0, 0.1)
    ppo = PPOLagrangian.__new__(PPOLagrangian)
    with pytest.raises(AssertionError, match="one algorithm"):
        PolicyGroup([a, ppo], engine_group=_FakeGroup())
    with pytest.raises(AssertionError, match="one algorithm"):
        PolicyGroup([ppo, a], engine_group=_FakeGroup())
    with pytest.raises(AssertionError, match="reference_rng"):
        PolicyGroup([a, _focops(10.0, 1.0, 0.1, reference_rng=True)], engine_group=_FakeGroup())


def test_a_failed_update_marks_mirrors_stale():
    pols = [_focops(10.0, 1.0, 0.1), _focops(10.0, 2.0, 0.2)]
    grp = PolicyGroup(pols, engine_group=_FakeGroup(fail=True))
    with pytest.raises(RuntimeError, match="device error"):
        grp.update([_Buf(p) for p in pols])
    assert all(p.stale == 1 and not p.updating and p.logger.rows == [] for p in pols)
