"""The case table of the two-launch clipped step (tests/clip_fuse_problems.py) reaches what it claims: proved on the oracle alone, so it
runs anywhere.  These are conditions on the cases, not measurements of the library: a case whose data stops meeting them gets another
seed, the bars stay."""
import numpy as np
import pytest

import clip_fuse_problems as cf
from oracle.ppo_lag import split_chunks


@pytest.mark.parametrize("cid", list(cf.CASES))
def test_minibatch_sizes_are_what_the_table_says(cid):
    c = cf.CASES[cid]
    for perm in cf.problem(c)["perms"][:c.passes]:
        assert tuple(len(x) for x in split_chunks(c.n, c.batch, perm)) == c.minibatches
    assert len(cf.problem(c)["data"]) == c.n and len(set(c.rows)) > 1           # ragged environments


def test_the_table_covers_every_slot_of_the_dw1_role_and_both_sides_of_each_edge():
    obs = {c.obs for c in cf.FUSED.values()}
    assert {16, 17, 32, 33, 48, 49, 64} <= obs and max(obs) == 64              # CLIP_FUSE_MAX_OBS
    assert cf.SHAPES["o65"].refused and cf.SHAPES["o65"].obs == 65
    assert {c.H for c in cf.FUSED.values()} == {64, 128, 256}
    assert {c.critics for c in cf.FUSED.values()} == {1, 2} and {1, 16} <= {c.act for c in cf.FUSED.values()}
    pad = lambda m: -(-m // 16) * 16  # noqa: E731
    assert [pad(m) for m in cf.SHAPES["o33a16"].minibatches] == [512, 512] and 505 % 4
    assert [pad(m) <= 512 for m in cf.SHAPES["o64mix"].minibatches] == [True, False]
    assert cf.SHAPES["o64mix"].fused_steps == 2 and cf.SHAPES["o49tiny"].fused_steps == 10 and cf.SHAPES["o16"].fused_steps == 2


@pytest.mark.parametrize("cid", [*cf.SHAPES, *cf.OPTIONS])
def test_every_step_of_a_shape_case_clips(cid):
    """the coefficient is max_norm / (norm + 1e-6), well below 1: every float64 pre-clip norm is at least twice the threshold"""
    c = cf.CASES[cid]
    norms = cf.oracle_run(c, True)["norms"]
    assert len(norms) == c.steps and (norms >= 2 * c.max_grad_norm).all(), norms


@pytest.mark.parametrize("cid", ["o49tiny-loose", "o17-loose"])
def test_no_step_of_a_loose_case_clips(cid):
    c = cf.CASES[cid]
    norms = cf.oracle_run(c, True)["norms"]
    assert len(norms) == c.steps and (norms <= 0.5 * c.max_grad_norm).all(), norms


def test_the_straddle_case_has_steps_on_both_sides_of_its_threshold():
    """the fp32 oracle sits within 1e-6 relative of the float64 norm, so 2 % of clearance decides every step the same way in fp32"""
    c = cf.CASES["o49tiny-straddle"]
    for f64 in (True, False):
        norms = cf.oracle_run(c, f64)["norms"]
        assert (norms > c.max_grad_norm).any() and (norms < c.max_grad_norm).any(), norms
        assert (np.abs(norms / c.max_grad_norm - 1.0) >= 0.02).all(), norms
    a, b = cf.oracle_run(c, True)["norms"], cf.oracle_run(c, False)["norms"]
    assert np.array_equal(a > c.max_grad_norm, b > c.max_grad_norm) and (np.abs(a - b) <= 1e-6 * a).all()


@pytest.mark.parametrize("cid", list(cf.KL))
def test_the_kl_case_stops_in_the_same_pass_in_fp32_and_float64(cid):
    c = cf.CASES[cid]
    thr = 1.5 * c.target_kl
    assert 1 <= c.stop_pass < c.passes - 1              # the update goes on after the first verdict, and one pass is never run
    for f64 in (True, False):
        r = cf.oracle_run(c, f64)
        assert r["stopped"] == c.stop_pass and len(r["stats"]) == c.steps, (r["stopped"], len(r["stats"]))
        kl = cf.pass_kl(cf.oracle_run(c, f64, passes=c.stop_pass + 1, no_stop=True)["stats"], len(c.minibatches))
        assert kl[:c.stop_pass].max() <= 0.8 * thr and kl[c.stop_pass] >= 1.2 * thr, (kl, thr)
