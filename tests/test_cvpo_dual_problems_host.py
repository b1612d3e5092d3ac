"""The CVPO dual regimes of tests/cvpo_dual_problems.py prove themselves on the CPU: the float64 oracle AND the fp32 oracle show the
values each regime claims (the clamps exactly), and five one-defect copies of the fp32 oracle each break the bars the device is held
to.  tests/test_gpu_cvpo_duals.py builds its inputs with the same constructors and repeats the regime assertion on the device's own
log.  Each test prints its figures (pytest -s shows them)."""
import numpy as np
import pytest

import cvpo_dual_problems as dp


@pytest.fixture(scope="module")
def problems():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = dp.run_case(name)
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(dp.CASES))
def test_case_sits_in_its_regime(name, problems):
    p = problems(name)
    for run, who in ((1, "float64 oracle"), (0, "fp32 oracle")):
        tr = dp.trace(p["rows"][run])
        print(dp.trace_line(f"{name} ({who})", tr))
        dp.check_regime(name, tr, p["w64"] if run == 1 else None, who)
    if name == "eta_lo":          # at eta = 1.19e-6 a gap of 1e-3 is 800 eta: exp(-800) = 0 in either precision
        assert dp.row_gap(p) >= 1e-3, dp.row_gap(p)
    r, at, vr, vat, own = dp.distance(p, 0, against=1)
    print(f"    fp32 oracle vs float64: logged rows {own:.3f} x project bar, parameters {vr:.3f} x project bar ({vat})")
    assert own <= 0.5 and vr <= 0.5, (name, "the fp32 oracle is no yardstick here", own, vr)


def test_cases_cover_every_path_of_the_estep_kernel():
    """K a power of two <= 64 takes the lane path (1024 lanes per round), any other K the per-state loop (1024 states per round)"""
    lane, loop = [], []
    for name in dp.COSTLY_SWEEP:
        c = dp.case_of(name)
        (lane if c["K"] & (c["K"] - 1) == 0 else loop).append((c["K"], c["B"]))
    kb = [k * b for k, b in lane]
    assert any(n == 1024 for n in kb) and any(n > 1024 and n % 1024 for n in kb) and any(k == 64 for k, _ in lane)
    assert any(b > 1024 for _, b in loop) and any(b < 64 for _, b in loop) and len(loop) >= 3
    ctx = [dp.case_of(n) for n in dp.COSTLY_CONTEXTS]
    assert {c["double"] for c in ctx} == {False, True} and any(len(c["hidden"]) == 3 for c in ctx)
    assert any(c["hidden"] == (256, 256) and c["B"] > 1024 for c in ctx) and any(c["cycles"] == 2 for c in ctx)


MUTANTS = {"a": "costly_it3/h64_double", "b": "costly_it3/h64_single", "c": "costly_capped", "d": "mdual_hi", "e": "costly_it3/two_cycles"}


@pytest.mark.parametrize("letter", list(MUTANTS))
def test_mutant_breaks_the_bars(letter):
    """a one-defect fp32 oracle, held to the device's bars against the unmutated fp32 oracle, fails them -- by a wide margin (the
    module docstring of cvpo_dual_problems.py records the ratios; one near 1 would mean a case too weak to see the defect)"""
    name = MUTANTS[letter]
    p = dp.run_case(name, extra=lambda cfg: [dp.mutant(cfg, letter)])
    dp.check(p, 0, "fp32 oracle against itself")              # the check passes where nothing is wrong
    r, at, vr, vat, _ = dp.distance(p, 2)
    print(f"mutant ({letter}) on {name}: logged rows {r:.1f} x bar at update {at[0]} {at[1]}, parameters {vr:.1f} x bar ({vat})")
    assert r >= 5.0, (letter, name, r)
    with pytest.raises(AssertionError):
        dp.check(p, 2, f"mutant ({letter})")


def test_costly_fixtures_stay_small_and_keep_their_census():
    import os
    from helpers import GOLDEN
    for name in dp.COSTLY_FIXTURES:
        assert os.path.getsize(os.path.join(GOLDEN, f"cvpo_{name}.npz")) < 1 << 20, name
        dp.fixture_census(name)
