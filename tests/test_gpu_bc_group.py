"""Grouped behaviour cloning (fsrl_bc_update_group): per member (a) bit for bit the solo fsrl_bc_update on a twin engine holding the
same rows, and (b) the float64 autograd restatement of tests/test_gpu_bc.py within its bars (4 x the restatement's own float32
deviation).  Member i has its own actor and its own stored rows (make_case seed i); under shared_store its twin holds member 0's.
Library-drawn indices are not known to the test, so that case is held to (a) alone; the shared store meets (b) in the DDPG case."""
import numpy as np
import pytest
import torch

import test_gpu_bc as solo
from test_gpu_bc import BAR, N_UPD, make_case, make_engine, reference, rel
from fsrl_amd import _lib
from fsrl_amd.engine import Engine, EngineConfig, EngineSacGroup, bc_update_group

pytestmark = pytest.mark.gpu

# head, hidden, dims, unbounded, sigma scale, shared_store, drawn, members: (loss, batch, n_updates, max_action)
CASES = {
    "ragged-second-tile": ("onpolicy", (64, 64), (6, 2), False, 1.0, False, False, [("mse", 16, 3, 1.5), ("mse", 17, 3, 1.5)]),
    "sit-out-and-leave-early-JE6": ("onpolicy", (256, 256), (33, 8), True, 1.0, False, False,
                                    [("nll", 17, 3, 1.5), ("nll", 16, 0, 1.5), ("nll", 48, 1, 1.5)]),
    "per-member-loss-and-scalar": ("gauss", (64, 64), (6, 2), False, 40.0, False, False, [("mse", 48, 3, 1.5), ("nll", 17, 3, 0.75)]),
    "ddpg-padded-shared-store": ("ddpg", (48, 48), (6, 2), False, 1.0, True, False, [("mse", 17, 3, 1.5), ("mse", 16, 3, 1.5)]),
    "shared-store-drawn": ("onpolicy", (64, 64), (6, 2), False, 1.0, True, True, [("mse", 17, 3, 1.5), ("nll", 33, 3, 1.5)]),
    "k1-is-solo": ("gauss", (256, 256), (5, 1), True, 1.0, False, False, [("nll", 17, 3, 1.5)]),
}

def build(maxa, *args):
    solo.MAXA = maxa            # make_engine and reference read the module's max_action when they are called
    try:
        return make_engine(*args)
    finally:
        solo.MAXA = 1.5

@pytest.mark.parametrize("case", list(CASES))
def test_bc_update_group_is_the_solo_update_per_member(case):
    head, hidden, dims, unbounded, sig_scale, shared, drawn, members = CASES[case]
    k = len(members)
    data = [make_case(head, hidden, dims, b, sig_scale, seed=i) for i, (_, b, _, _) in enumerate(members)]
    rows = lambda i: data[0][1:3] if shared else data[i][1:3]
    group = [build(m[3], head, hidden, dims, unbounded, data[i][0], *data[i][1:3]) for i, m in enumerate(members)]
    twins = [build(m[3], head, hidden, dims, unbounded, data[i][0], *rows(i)) for i, m in enumerate(members)]
    loss, batch, n = [m[0] for m in members], [m[1] for m in members], np.array([m[2] for m in members])
    engines = [e for e, _ in group]
    try:
        # the first update of every member, the rest in a second call (who is done sits it out), then every member's updates again in
        # ONE call, where a member leaves while the others go on
        got = [dict() for _ in members]
        for phase, (lo, hi) in enumerate(((0, 1), (1, N_UPD), (0, N_UPD))):
            cnt = np.clip(n, lo, hi) - lo
            idx = None if drawn else [data[i][3][lo:lo + cnt[i]] for i in range(k)]
            ls = bc_update_group(engines, batch, cnt, loss=loss, indices=idx, seeds=[7 + i for i in range(k)], shared_store=shared)
            for i, (eng, get) in enumerate(group):
                twin, tget = twins[i]
                if cnt[i]:
                    lt = twin.bc_update(batch[i], int(cnt[i]), loss=loss[i], indices=None if drawn else idx[i], seed=7 + i)
                    assert np.array_equal(ls[i], lt), (case, phase, i)
                    assert np.array_equal(eng.get_grads(), twin.get_grads()) and np.array_equal(get(), tget()), (case, phase, i)
                else:
                    assert len(ls[i]) == 0          # sits out: its twin ran nothing, and the states below still agree
                assert eng.train_state(with_store=False) == twin.train_state(with_store=False), (case, phase, i)
                if phase == 0 and cnt[i]:
                    got[i] = {"loss": ls[i], "p1": get(), "grad": eng.get_grads()[:get().size]}
                elif phase == 1 and n[i]:
                    got[i].update(loss=np.concatenate([got[i]["loss"], ls[i]]), p3=get())
        for i, (l, b, ni, maxa) in enumerate(members):
            if drawn or not ni:
                continue
            solo.MAXA = maxa
            try:
                ref = reference(head, l, unbounded, data[i][0], *rows(i), data[i][3][:ni], torch.float64)
            finally:
                solo.MAXA = 1.5
            dev = {q: rel(v, ref[q]) for q, v in got[i].items()}
            print("grouped bc deviations", case, i, dev)
            assert all(d <= BAR[q] for q, d in dev.items()), (case, i, dev, BAR)
        if drawn:           # the members' seeds differ: so do their batches of the one store
            assert not np.array_equal(got[0]["loss"][:1], got[1]["loss"][:1])
    finally:
        for e, _ in group + twins:
            e.close()

def test_bc_update_group_refusals_name_the_member_and_change_nothing():
    actor, obs, act, idx = make_case("gauss", (64, 64), (6, 2), 16, 1.0)
    (a, _), (b, _) = [make_engine("gauss", (64, 64), (6, 2), False, actor, obs, act) for _ in range(2)]
    wide = Engine(EngineConfig(obs_dim=6, act_dim=2, hidden_sizes=(128, 128), env_num=1, buffer_size=64, algo=_lib.ALGO_SAC_LAG), device=0)
    wide.sac_init(actor_lr=1e-3)
    try:
        state = a.train_state(), b.train_state()
        for engines, reason in (([a, wide], "member 1: members must have one network shape"), ([a, b, a], "member 2: its context is listed twice"),
                                ([a] * 17, "k 17"), ([a, b], "member 1: .*member of a live group")):
            live = EngineSacGroup([b]) if "live group" in reason else None
            with pytest.raises(AssertionError, match=reason):
                bc_update_group(engines, 16, 1, indices=[idx[:1]] * len(engines))
            if live is not None:
                live.close()
        assert (a.train_state(), b.train_state()) == state
    finally:
        for e in [a, b, wide]:
            e.close()

def test_pretrain_group_from_pours_once_and_moves_the_actors_alone():
    from fsrl_amd.agent import PPOLagAgent, pretrain_group_from
    from fsrl_amd.env import SyntheticSafetyVectorEnv
    from test_gpu_store_fill import dataset
    env = SyntheticSafetyVectorEnv(env_num=2, obs_dim=6, act_dim=2, episode_len=20, seed=1)
    agents = [PPOLagAgent(env, None, cost_limit=10, device="cuda:0", seed=3 + i, hidden_sizes=(64, 64), training_num=2) for i in range(2)]
    engines = [ag.policy.engine for ag in agents]
    try:
        before = [e.get_params() for e in engines]
        losses = pretrain_group_from(agents, dataset(6, 2, [40, 25, 31], 9), batch_size=32, n_updates=4, loss="nll")
        assert [len(l) for l in losses] == [4, 4] and all(len(e) == 0 for e in engines)
        for e, p in zip(engines, before):
            n_a, after = e.n_actor_params, e.get_params()
            assert np.array_equal(after[n_a:], p[n_a:]) and not np.array_equal(after[:n_a], p[:n_a])
    finally:
        for e in engines:
            e.close()
