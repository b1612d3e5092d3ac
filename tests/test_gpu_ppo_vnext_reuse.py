"""process_fn with V(obs_next) taken from the V(obs) pass where batch row r's obs_next and row r + 1's obs are the same words
(batch_gather_flag_kernel flags and lists the rows, mlp_infer_kernel's value jobs store vnext[r] next to values[r + 1], its next jobs
walk only the listed rows) against a context created under FSRL_NO_VNEXT_REUSE, which evaluates every V(obs_next) row as before.
The change removes evaluations, not arithmetic: a row's value does not depend on the tile it sits in, and the same network on the
same words gives the same bits.  So everything is compared bit for bit: values, advs, rets, logp_old (and vnext) after ppo_begin, the
logged statistics, the parameters and the exported training state after a 2-pass update, without and with recompute_advantage
(whose value passes reuse the update's flags).  That the path ran is shown by the reuse counter: it equals the count of coinciding
rows computed here from the store's rows (compared as uint32: -0.0 != +0.0).

Shapes: hidden 64; obs 8 (W1 in LDS) and obs 17 (layer 1 on MFMA); 3 envs of 37-50 rows (one case: an env with one row), N % 16 != 0,
so the last tile of the batch and the last tile of the list are ragged; 1 and 2 critics.  Cases: contiguous episodes; an episode end
followed by a reset observation; a terminated row whose obs_next IS the next row's obs (vnext must be 0 there); a wrapped sub-buffer
(the ring's seam inside the batch); an env with one row; one observation word that differs only in the sign of zero; a store in which
no rows coincide, which must run the equal split of the launch."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H, DA, ENVS = 64, 2, 3
CASES = ("contiguous", "reset", "terminated_chain", "wrapped", "one_row", "sign_of_zero", "none_coincide")


def _engine(no_reuse, **kw):
    """A PPO-Lagrangian context; no_reuse: created under FSRL_NO_VNEXT_REUSE (fsrl_ctx_create reads it once)."""
    from fsrl_amd.engine import Engine, EngineConfig
    old = os.environ.get("FSRL_NO_VNEXT_REUSE")
    if no_reuse:
        os.environ["FSRL_NO_VNEXT_REUSE"] = "1"
    else:
        os.environ.pop("FSRL_NO_VNEXT_REUSE", None)
    try:
        return Engine(EngineConfig(env_num=ENVS, target_kl=None, max_grad_norm=0.5, hidden=H, act_dim=DA, **kw), device=0)
    finally:
        if old is None:
            os.environ.pop("FSRL_NO_VNEXT_REUSE", None)
        else:
            os.environ["FSRL_NO_VNEXT_REUSE"] = old


def _script(case, Do):
    """-> (buffer_size, rows): rows = [(env, obs, act, rew, cost, terminated, truncated, obs_next)] in push order, and the
    batch rows at which vnext must be exactly 0 although the row's obs_next coincides with the next row's obs"""
    rng = np.random.default_rng(11 + CASES.index(case) + 100 * Do)
    lens = {"one_row": (1, 50, 46), "wrapped": (63, 37, 42)}.get(case, (37, 50, 42))
    sub = 50
    rows, zero_rows, base = [], [], 0
    for e, T in enumerate(lens):
        obs = rng.standard_normal((T + 1, Do)).astype(np.float32)
        nxt = obs[1:].copy()
        term = np.zeros(T, bool); trunc = np.zeros(T, bool)
        kept = min(T, sub)                     # rows of this env in the batch (a wrapped sub-buffer keeps the last `sub`)
        first = T - kept
        if case == "reset" and T > 30:
            trunc[19] = True; term[30] = True   # the rows after them start from reset observations
            nxt[19] = rng.standard_normal(Do); nxt[30] = rng.standard_normal(Do)
        if case == "terminated_chain" and T > 20:
            term[20] = True                    # obs_next[20] stays obs[21]: a coinciding row whose vnext is masked
            zero_rows.append(base + 20 - first)
        if case == "sign_of_zero" and T > 25:
            obs[12, 3] = 0.0; nxt[11] = obs[12]; nxt[11, 3] = -0.0      # differs from obs[12] in one sign bit only
            obs[25, 0] = -0.0; nxt[24] = obs[25]                         # -0.0 on both sides: the same words
        if case == "none_coincide":
            nxt = rng.standard_normal((T, Do)).astype(np.float32)
        act = (0.3 * rng.standard_normal((T, DA))).astype(np.float32)
        rew = rng.normal(0.5, 0.5, T); cost = (rng.random(T) < 0.2).astype(np.float64)
        for t in range(T):
            rows.append((e, obs[t], act[t], rew[t], cost[t], term[t], trunc[t], nxt[t]))
        base += kept
    return sub * ENVS, rows, zero_rows


def _host_same(eng):
    """rows r of the batch whose obs_next is row r + 1's obs word for word, from the store's rows in sample(0) order"""
    got = eng.store_read(eng.sample0())
    a = np.ascontiguousarray(got["obs_next"]).view(np.uint32)[:-1]
    b = np.ascontiguousarray(got["obs"]).view(np.uint32)[1:]
    return (a == b).all(axis=1)


def _run(case, Do, C, recompute, no_reuse):
    size, rows, zero_rows = _script(case, Do)
    eng = _engine(no_reuse, obs_dim=Do, n_critics=C, buffer_size=size, recompute_adv=recompute)
    try:
        eng.set_params((0.1 * np.random.default_rng(3).standard_normal(eng.n_params)).astype(np.float32))
        for e, o, a, r, c, te, tr, nx in rows:
            eng.push([e], o[None], a[None], [r], [c], [te], [tr], nx[None])
        same = _host_same(eng)
        lag = np.array([0.5]) if C == 2 else np.zeros(0)
        n = eng.ppo_begin(lag, 1.0 / 1.5 if C == 2 else 1.0, 32)
        out = {k: eng.batch_get(k).copy() for k in ("values", "advs", "rets", "logp_old", "vnext")}
        out["process"] = eng.ppo_process_stats()
        rng = np.random.default_rng(5)
        for _ in range(2):
            assert eng.ppo_pass(rng.permutation(n)) is False
        out["stats"] = eng.ppo_end_stats(2 * max(1, n // 32)).copy()
        out["params"] = eng.get_params().copy()
        out["state"] = eng.train_state_array(with_store=True).copy()
        out["fuse"] = eng.ppo_clip_fuse_stats()
        out["n"], out["same"], out["zero_rows"] = n, same, zero_rows
        return out
    finally:
        eng.close()


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("Do", [8, 17])
@pytest.mark.parametrize("case", CASES)
def test_vnext_reuse_bit_identical_to_evaluating_every_row(case, Do, C):
    for recompute in (False, True):
        new = _run(case, Do, C, recompute, no_reuse=False)
        old = _run(case, Do, C, recompute, no_reuse=True)
        n, same = new["n"], new["same"]
        assert n == old["n"] and n % 16 != 0 and n > 16 * 5, n
        # the path ran, on exactly the rows the host finds
        ps = new["process"]
        print(case, Do, C, recompute, "N", n, "coinciding rows", int(same.sum()), ps)
        assert ps["reuse"] and not old["process"]["reuse"]
        assert ps["rows_reused"] == int(same.sum()) and ps["rows_evaluated"] == n - int(same.sum())
        assert old["process"]["rows_reused"] == 0 and old["process"]["rows_evaluated"] == n and old["process"]["equal_split"]
        if case == "none_coincide":
            assert ps["rows_reused"] == 0 and ps["equal_split"]
        else:
            assert ps["rows_reused"] >= n - 16 and not ps["equal_split"]       # at most one tile of listed rows
        if case == "sign_of_zero":
            assert ps["rows_reused"] == n - ENVS - ENVS          # per env: its last row and the row with the -0.0 / +0.0 word
        for r in new["zero_rows"]:
            assert same[r] and (new["vnext"][r] == 0).all() and (new["values"][r + 1] != 0).all()
        for k in ("values", "vnext", "advs", "rets", "logp_old", "stats", "params"):
            a, b = new[k], old[k]
            assert a.shape == b.shape and np.isfinite(a).all(), k
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (k, recompute, int((a != b).sum()))
        assert np.array_equal(new["state"], old["state"]), int((new["state"] != old["state"]).sum())
        assert new["fuse"]["fallbacks"] == 0 and old["fuse"]["fallbacks"] == 0
