"""DDPGPolicyGroup on the host (no GPU): a fake engine group stands in for fsrl_sac_group_update.  Per member the group must pass
what DDPGLagrangian.learn would (lambda and rescaling of lagrangians_and_rescaling, n_i updates), run a fresh member's first update
on its own (it keys the Philox stream), keep the bookkeeping of n_i calls of policy.update (gradient_steps, pending rows, lr
scheduler steps, stale mirrors), and refuse what it cannot group."""
import pytest

from fsrl_amd.policy import DDPGPolicyGroup
from fsrl_amd.policy.ddpg_lag import DDPGLagrangian
from fsrl_amd.policy.sac_lag import SACLagrangian


class _FakeGroup:
    def __init__(self, fail=False):
        self.calls, self.fail = [], fail

    def update(self, batch_size, n_updates, lagrangians=None, rescalings=None):
        if self.fail:
            raise RuntimeError("device error")
        self.calls.append((batch_size, list(n_updates), lagrangians, list(rescalings)))

    def close(self):
        pass


class _Sched:
    def __init__(self):
        self.n = 0


def _policy(lam, steps=1, use_lag=True, sched=False, cls=DDPGLagrangian):
    p = cls.__new__(cls)
    p.engine = object()
    p.use_lagrangian = use_lag
    p._reference_rng, p._seed, p._pending = False, 0, 0
    p.gradient_steps = steps
    p.lr_scheduler = _Sched() if sched else None
    p._dirty = p._rest_dirty = False
    p.drained, p.own, p.stale = 0, [], 0
    p.lagrangians_and_rescaling = lambda: ([lam], 1.0 / (1.0 + lam))
    p._step_lr_scheduler = lambda: setattr(p.lr_scheduler, "n", p.lr_scheduler.n + 1) if p.lr_scheduler else None
    p._drain = lambda: (setattr(p, "drained", p.drained + p._pending), setattr(p, "_pending", 0))
    p._mark_stale = lambda: setattr(p, "stale", p.stale + 1)

    def own_update(B, buf):                      # what DDPGLagrangian.update leaves behind on the host
        p.own.append((B, buf))
        p.gradient_steps += 1
        p._pending += 1
        p._dirty = p._rest_dirty = True
        p._step_lr_scheduler()
        p.updating = False
        return {}
    p.update = own_update
    return p


class _Buf:
    def __init__(self, p):
        self.engine = p.engine


def test_is_exported_beside_the_sac_group():
    import fsrl_amd.policy as pol
    from fsrl_amd.policy.grouped_sac import ReplayPolicyGroup
    assert pol.DDPGPolicyGroup is DDPGPolicyGroup
    assert issubclass(DDPGPolicyGroup, ReplayPolicyGroup) and issubclass(pol.SACPolicyGroup, ReplayPolicyGroup)
    assert DDPGPolicyGroup.policy_cls is DDPGLagrangian and pol.SACPolicyGroup.policy_cls is SACLagrangian
    assert DDPGPolicyGroup.update is pol.SACPolicyGroup.update         # one loop, not a copy


def test_passes_each_members_lambda_rescaling_and_count():
    pols = [_policy(0.5), _policy(2.0), _policy(0.0)]
    fg = _FakeGroup()
    grp = DDPGPolicyGroup(pols, engine_group=fg)
    out = grp.update([_Buf(p) for p in pols], 128, [4, 0, 2])
    assert out == [{}, {}, {}]
    assert fg.calls == [(128, [4, 0, 2], [[0.5], [2.0], [0.0]], [1 / 1.5, 1 / 3.0, 1.0])]
    assert [p.gradient_steps for p in pols] == [5, 1, 3]
    assert [p._pending for p in pols] == [4, 0, 2]
    assert pols[0]._dirty and pols[0]._rest_dirty and not pols[1]._dirty and not pols[1]._rest_dirty
    assert not any(p.own for p in pols)
    assert not any(getattr(p, "updating", False) for p in pols)


def test_a_fresh_members_first_update_runs_on_its_own():
    pols = [_policy(0.5, steps=0), _policy(0.25, steps=7), _policy(0.1, steps=0)]
    bufs = [_Buf(p) for p in pols]
    fg = _FakeGroup()
    DDPGPolicyGroup(pols, engine_group=fg).update(bufs, 64, [3, 2, 1])
    assert pols[0].own == [(64, bufs[0])] and pols[1].own == [] and pols[2].own == [(64, bufs[2])]
    assert [c[1] for c in fg.calls] == [[2, 2, 0]]
    assert [p.gradient_steps for p in pols] == [3, 9, 1]
    assert [p._pending for p in pols] == [3, 2, 1]
    assert not any(p.updating for p in pols)
    # a fresh member with nothing to do is not keyed
    q = _policy(0.5, steps=0)
    fg = _FakeGroup()
    DDPGPolicyGroup([q], engine_group=fg).update([_Buf(q)], 64, [0])
    assert q.own == [] and fg.calls == [] and q.gradient_steps == 0


def test_lagrangian_off_and_scheduler_steps_one_update_per_call():
    pols = [_policy(0.5, use_lag=False, sched=True), _policy(0.5, use_lag=False)]
    fg = _FakeGroup()
    DDPGPolicyGroup(pols, engine_group=fg).update([_Buf(p) for p in pols], 64, [3, 1])
    assert [c[1] for c in fg.calls] == [[1, 1], [1, 0], [1, 0]]
    assert all(c[2] is None and c[3] == [1.0, 1.0] for c in fg.calls)
    assert pols[0].lr_scheduler.n == 3


def test_statistics_ring_is_drained_where_learn_drains_it():
    p = _policy(0.1)
    p._pending = 2000
    fg = _FakeGroup()
    DDPGPolicyGroup([p], engine_group=fg).update([_Buf(p)], 64, 100)
    assert [c[1] for c in fg.calls] == [[48], [52]]
    assert p.drained == 2048 and p._pending == 52


def test_rejects_what_cannot_be_grouped():
    p, q = _policy(0.1), _policy(0.1)
    q._reference_rng = True
    with pytest.raises(AssertionError, match="reference_rng"):
        DDPGPolicyGroup([p, q], engine_group=_FakeGroup())
    with pytest.raises(AssertionError, match="DDPGLagrangian"):
        DDPGPolicyGroup([p, _policy(0.1, cls=SACLagrangian)], engine_group=_FakeGroup())
    grp = DDPGPolicyGroup([p], engine_group=_FakeGroup())
    with pytest.raises(AssertionError, match="buffer"):
        grp.update([_Buf(_policy(0.1))], 64, [1])
    with pytest.raises(AssertionError, match="n_updates"):
        grp.update([_Buf(p)], 64, [-1])


def test_failure_marks_every_mirror_stale():
    pols = [_policy(0.1), _policy(0.2)]
    with pytest.raises(RuntimeError):
        DDPGPolicyGroup(pols, engine_group=_FakeGroup(fail=True)).update([_Buf(p) for p in pols], 64, [1, 1])
    assert all(p._dirty and p._rest_dirty and not p.updating and p.stale == 1 for p in pols)
