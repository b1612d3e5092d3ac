"""The branch problems of tests/branch_problems.py prove their own populations (CPU, float64 oracle): every branch a case claims
holds at least 2 % of the compared rows and at least 3 rows, and no row is closer than 1e-3 (relative) to a branch boundary.  The
GPU tests (test_gpu_ppo_branches.py, test_gpu_replay_branches.py) build their inputs with the same constructors and repeat the
assertion.  Each test prints its case's census (pytest -s shows it)."""
import numpy as np
import pytest

import branch_problems as bp


@pytest.mark.parametrize("name", list(bp.PPO_CASES))
def test_ppo_case_populates_every_branch_it_claims(name):
    p = bp.ppo_problem(name)
    print(bp.census_line(name, p["census"], p["margin"]), f" chunk of {len(p['chunk'])} rows")
    claims = bp.ppo_claims(p["case"])
    if p["case"].get("dual_clip"):
        assert set(bp.POLICY_BRANCHES) <= {k for g in claims for k in g}
    if p["case"].get("value_clip"):
        assert len(claims) == 3
    bp.check_census(p["census"], p["margin"], claims, name)
    assert len(p["chunk"]) % 16 != 0 and p["n_steps"] >= 2
    # the fp32 oracle against its float64 run, in units of the project's bars: decides whether the project's bars stand
    gd, rd = bp.ppo_oracle_distance(p)
    print(f"    fp32 oracle vs float64: gradient {gd:.3f} x bar, logged row {rd:.3f} x bar")


def test_ppo_cases_cover_the_issues_list():
    """widths 64 / 128 / 256 and a layered context; act_dim 1, 6, 16; a case with both tile plans; dual clip on and off; value clip on
    and off; raw advantages; an unbounded head; no Lagrangian term"""
    cs = list(bp.PPO_CASES.values())
    assert {c["hidden"] for c in cs} >= {(64, 64), (128, 128), (256, 256)} and any(len(c["hidden"]) == 3 for c in cs)
    assert {c["Da"] for c in cs} >= {1, 6, 16}
    assert any(len(c.get("plans", ())) == 2 for c in cs)
    for key, vals in (("dual_clip", {None, 1.5}), ("value_clip", {None, True}), ("norm_adv", {None, False}), ("unbounded", {None, True}),
                      ("use_lag", {None, False})):
        assert {c.get(key) for c in cs} >= vals, key


@pytest.mark.parametrize("kind,name", [(k, n) for k in bp.REPLAY_CASES for n in bp.REPLAY_CASES[k]])
def test_replay_case_puts_its_columns_in_their_regimes(kind, name):
    p = bp.replay_problem_with_regimes(kind, name)
    for u, (census, margin) in enumerate(p["census"]):
        print(bp.census_line(f"{kind}/{name} update {u}", census, margin))
    bp.check_replay_census(p)
    ow, ovec, _ = bp.replay_distance(kind, p["rows"][0], p["final"][0], p["rows"][1], p["final"][1])
    print(f"    fp32 oracle vs float64: logged rows {ow:.3f} x bar, parameters max {max(v[0] for v in ovec.values()):.1e} "
          f"q99 {max(v[1] for v in ovec.values()):.1e}")
    if p["case"]["updates"] == 1:          # what the device is then held to bit for bit
        bp.check_frozen_rows(p, p["final"][0]["actor"], "fp32 oracle")


@pytest.mark.parametrize("kind,name", [(k, n) for k in bp.REPLAY_CASES for n, c in bp.REPLAY_CASES[k].items() if c["updates"] == 1])
def test_head_row_check_sees_one_row_stepping_the_wrong_way(kind, name):
    """the check the device is held to has teeth: the fp32 oracle's own final actor passes it; the same actor with ONE head row (each
    moved row in turn) stepped the other way fails it.  (The whole-vector bars do not notice such a row of a layered case -- 25 of
    3 528 entries -- and notice a 64-wide one only if over 80 % of its entries are wrong.)"""
    p = bp.replay_problem_with_regimes(kind, name)
    ref, before = p["final"][0]["actor"], p["tha"]
    bp.check_head_rows(p, ref, "fp32 oracle")
    tried = 0
    for d in range(p["case"]["Da"]):
        for rows in bp.head_rows(kind, p["aspec"], d):
            if rows is None or np.array_equal(ref[rows], before[rows]):
                continue
            wrong = ref.copy()
            wrong[rows] = before[rows] - (ref[rows] - before[rows])
            with pytest.raises(AssertionError):
                bp.check_head_rows(p, wrong, "wrong-way row")
            tried += 1
    assert tried >= 2
