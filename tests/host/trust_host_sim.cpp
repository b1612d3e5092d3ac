// trust_host_sim.cpp -- host_decisions.hpp (what the update paths decide on the host between their launches) as a plain program:
// CPO's dual solve against rows recorded from the reference, the two line searches' schedules and acceptance rules, the minibatch
// split, the permutation check / shuffle and the tile-split simulation.  No GPU, no HIP; tests/test_trust_host.py builds it with the
// address / undefined-behaviour sanitizers and hands it the fixtures' rows as a text file (argv[1]):
//   dual  q r s c delta bb  case A B lam nu        one recorded dual solve
//   sched step_size coeff max_backtracks           one recorded CPO step size
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I fsrl_amd/csrc tests/host/trust_host_sim.cpp
#include "host_decisions.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>

#define REQUIRE(cond, ...) \
    do { if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s\n  ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static const double ULP2 = 2.0 * 1.1920928955078125e-07;       // two float32 ulps, 2 * 2^-23

// |got - want| / |want|; a recorded 0 (or NaN / infinity) must come back as itself
static double rel_err(float got, double want, const char* what, int row) {
    if (want == 0.0 || std::isinf(want)) { REQUIRE((double)got == want, "row %d %s: %g, recorded %g", row, what, got, want); return 0.0; }
    if (std::isnan(want)) { REQUIRE(std::isnan(got), "row %d %s: %g, recorded NaN", row, what, got); return 0.0; }
    return std::fabs((double)got - want) / std::fabs(want);
}

// ---------------------------------------------------------------------------------------------- the recorded rows
static void recorded_rows(const char* path) {
    FILE* f = fopen(path, "r");
    REQUIRE(f, "cannot open %s", path);
    char tag[16];
    int n_dual = 0, n_sched = 0, cases[5] = {0, 0, 0, 0, 0};
    double worst = 0.0;
    while (fscanf(f, "%15s", tag) == 1) {
        if (!strcmp(tag, "dual")) {
            double q, r, s, cv, delta, bb, A, B, lam, nu; int want_case;
            REQUIRE(fscanf(f, "%lf %lf %lf %lf %lf %lf %d %lf %lf %lf %lf", &q, &r, &s, &cv, &delta, &bb, &want_case, &A, &B, &lam, &nu) == 11, "bad dual row");
            const CpoDual d = cpo_dual_solve((float)q, (float)r, (float)s, (float)cv, (float)delta, (float)bb);
            REQUIRE(d.ocase == want_case, "dual row %d: case %d, recorded %d", n_dual, d.ocase, want_case);
            REQUIRE(cpo_cost_solve_skipped((float)bb, (float)cv) == (want_case == 4), "dual row %d: second solve", n_dual);
            const double e[4] = {rel_err(d.A, A, "A", n_dual), rel_err(d.B, B, "B", n_dual), rel_err(d.lam, lam, "lam", n_dual),
                                 rel_err(d.nu, nu, "nu", n_dual)};
            for (double x : e) { REQUIRE(x <= ULP2, "dual row %d: relative error %.3e > %.3e", n_dual, x, ULP2); worst = std::max(worst, x); }
            cases[d.ocase] += 1; n_dual += 1;
        } else if (!strcmp(tag, "sched")) {
            double step, coeff; int max_bt;
            REQUIRE(fscanf(f, "%lf %lf %d", &step, &coeff, &max_bt) == 3, "bad sched row");
            bool found = false;
            for (int j = 0; j <= max_bt && !found; ++j) {           // refused j times (j == max_bt: never accepted)
                int tries = 0;
                const CpoSearch ls = cpo_line_search(1.0f, coeff, max_bt, [&](double) { return tries++ == j; });
                found = (float)ls.beta == (float)step;
            }
            REQUIRE(found, "sched row %d: step size %.9g is no beta of the schedule (coeff %g, %d backtracks)", n_sched, step, coeff, max_bt);
            n_sched += 1;
        } else REQUIRE(false, "unknown row tag %s", tag);
    }
    fclose(f);
    printf("ok dual_recorded rows=%d cases=%d/%d/%d/%d/%d worst_rel=%.3e\n", n_dual, cases[0], cases[1], cases[2], cases[3], cases[4], worst);
    printf("ok sched_recorded rows=%d\n", n_sched);
}

// ---------------------------------------------------------------------------------------------- scripted rows
static void dual_scripted() {
    // no cost gradient (bb <= 1e-8) but AT or OVER the limit: not case 4, the second solve runs
    REQUIRE(!cpo_cost_solve_skipped(0.0f, 0.0f) && !cpo_cost_solve_skipped(0.0f, 0.2f) && !cpo_cost_solve_skipped(1e-9f, 0.05f), "skip");
    REQUIRE(cpo_dual_solve(1.0f, 0.1f, 0.5f, 0.2f, 0.01f, 0.0f).ocase == 0, "bb = 0, c = 0.2: B = 0.02 - 0.08 < 0 -> case 0");
    REQUIRE(cpo_dual_solve(1.0f, 0.1f, 0.5f, 0.05f, 0.01f, 0.0f).ocase == 1, "bb = 0, c = 0.05: B = 0.02 - 0.005 >= 0 -> case 1");
    // the threshold itself: bb == 1e-8f inside the limit is case 4, the next float above it is not
    REQUIRE(cpo_cost_solve_skipped(1e-8f, -0.1f) && !cpo_cost_solve_skipped(std::nextafter(1e-8f, 1.0f), -0.1f), "bb threshold");
    const CpoDual d4 = cpo_dual_solve(0.32f, 0.0f, 0.0f, -0.1f, 0.01f, 1e-8f);
    REQUIRE(d4.ocase == 4 && d4.A == 0.0f && d4.B == 0.0f && d4.nu == 0.0f && d4.lam == std::sqrt(0.32f / (2.0f * 0.01f)), "case 4 row");
    // B == 0 exactly (2 delta = c^2 / s = 1): B >= 0 on both sides of the limit
    const CpoDual b0n = cpo_dual_solve(2.0f, 0.5f, 1.0f, -1.0f, 0.5f, 1.0f), b0p = cpo_dual_solve(2.0f, 0.5f, 1.0f, 1.0f, 0.5f, 1.0f);
    REQUIRE(b0n.B == 0.0f && b0n.ocase == 2 && b0p.B == 0.0f && b0p.ocase == 1, "B == 0: cases %d %d", b0n.ocase, b0p.ocase);
    REQUIRE(cpo_dual_solve(2.0f, 0.5f, 1.0f, -1.5f, 0.5f, 1.0f).ocase == 3 && cpo_dual_solve(2.0f, 0.5f, 1.0f, 1.5f, 0.5f, 1.0f).ocase == 0, "B < 0");
    // c_value == 0 counts as at the limit (c >= 0): B = 2 delta > 0 -> case 1
    const CpoDual c0 = cpo_dual_solve(2.0f, 0.5f, 1.0f, 0.0f, 0.01f, 1.0f);
    REQUIRE(c0.ocase == 1 && c0.B == 0.02f, "c == 0: case %d", c0.ocase);
    printf("ok dual_scripted\n");
}

static void schedules_scripted() {
    const float coeff = 0.8f;
    const int max_bt = 10;
    for (int j = 0; j <= max_bt; ++j) {                             // accepted at try j; j == max_bt: never
        std::vector<double> seen_d; std::vector<float> seen_f;
        const CpoSearch c = cpo_line_search(0.5f, coeff, max_bt, [&](double b) { seen_d.push_back(b); return (int)seen_d.size() == j + 1; });
        const TrpoSearch t = trpo_line_search(0.25f, coeff, max_bt, [&](float s) { seen_f.push_back(s); return (int)seen_f.size() == j + 1; });
        double beta = 1.0; float step = 0.25f;
        for (int i = 0; i < std::min(j, max_bt); ++i) {             // the steps each try was given: the schedule so far
            REQUIRE(seen_d[(size_t)i] == beta && seen_f[(size_t)i] == step, "try %d of %d", i, j);
            beta *= (double)coeff; step *= coeff;
        }
        const int evals = std::min(j + 1, max_bt);
        REQUIRE(c.evals == evals && t.evals == evals && (int)seen_d.size() == evals && (int)seen_f.size() == evals, "evaluations at j = %d", j);
        // CPO logs coeff^j, after a total failure coeff^max_backtracks; TRPO-Lag logs the accepted step, after a total failure 0
        REQUIRE(c.beta == beta, "CPO beta at j = %d: %.17g, want %.17g", j, c.beta, beta);
        REQUIRE(t.step == (j < max_bt ? step : 0.0f), "TRPO step at j = %d: %g", j, t.step);
    }
    int calls = 0;
    const CpoSearch nan_lam = cpo_line_search(NAN, coeff, max_bt, [&](double) { ++calls; return true; });
    REQUIRE(nan_lam.evals == 0 && nan_lam.beta == 1.0 && calls == 0, "NaN multiplier: no evaluation, beta 1");
    const CpoSearch none = cpo_line_search(0.5f, coeff, 0, [&](double) { return true; });
    const TrpoSearch nonet = trpo_line_search(0.25f, coeff, 0, [&](float) { return true; });
    REQUIRE(none.evals == 0 && none.beta == 1.0 && nonet.evals == 0 && nonet.step == 0.25f, "no backtracks allowed");
    printf("ok schedules_scripted\n");
}

static void predicates() {
    const float delta = 0.01f, above = std::nextafter(delta, 1.0f), below = std::nextafter(delta, 0.0f);
    // cpo_accepts(new_kl, new_obj, new_cs, delta, case, objective, cost_sur, c_value)
    REQUIRE(cpo_accepts(delta, 1.1f, 5.0f, delta, 3, 1.0f, 5.0f, -1.0f), "CPO: kl == delta is accepted (<=)");
    REQUIRE(!cpo_accepts(above, 1.1f, 5.0f, delta, 3, 1.0f, 5.0f, -1.0f), "CPO: kl just above delta");
    REQUIRE(!trpo_accepts(delta, delta, 0.9f, 1.0f) && trpo_accepts(below, delta, 0.9f, 1.0f), "TRPO-Lag: kl == delta is refused (<)");
    REQUIRE(!trpo_accepts(below, delta, 1.0f, 1.0f) && !trpo_accepts(NAN, delta, 0.9f, 1.0f), "TRPO-Lag: the loss must fall; NaN kl");
    for (int oc = 0; oc <= 4; ++oc) {                               // cases 0 and 1 ignore the objective, 2 .. 4 need it to RISE
        REQUIRE(cpo_accepts(0.0f, 0.5f, 5.0f, delta, oc, 1.0f, 5.0f, -1.0f) == (oc <= 1), "objective fell, case %d", oc);
        REQUIRE(cpo_accepts(0.0f, 1.0f, 5.0f, delta, oc, 1.0f, 5.0f, -1.0f) == (oc <= 1), "objective equal, case %d", oc);
        REQUIRE(cpo_accepts(0.0f, 1.5f, 5.0f, delta, oc, 1.0f, 5.0f, -1.0f), "objective rose, case %d", oc);
    }
    // the cost surrogate may rise by max(-c_value, 0): the room under the limit, none at or over it
    REQUIRE(cpo_accepts(0.0f, 2.0f, 5.5f, delta, 3, 1.0f, 5.0f, -0.5f) && !cpo_accepts(0.0f, 2.0f, 5.75f, delta, 3, 1.0f, 5.0f, -0.5f), "room 0.5");
    REQUIRE(cpo_accepts(0.0f, 2.0f, 5.0f, delta, 1, 1.0f, 5.0f, 0.5f) && !cpo_accepts(0.0f, 2.0f, 5.25f, delta, 1, 1.0f, 5.0f, 0.5f), "over: no room");
    REQUIRE(cpo_accepts(0.0f, 2.0f, 4.0f, delta, 0, 1.0f, 5.0f, 2.0f) && !cpo_accepts(0.0f, 2.0f, 5.25f, delta, 0, 1.0f, 5.0f, 0.0f), "c = 0");
    REQUIRE(!cpo_accepts(NAN, 2.0f, 5.0f, delta, 3, 1.0f, 5.0f, -1.0f) && !cpo_accepts(0.0f, 2.0f, NAN, delta, 3, 1.0f, 5.0f, -1.0f), "NaN refuses");
    printf("ok predicates\n");
}

static void splits() {
    const int B = 150;
    for (int n : {1, 149, 150, 151, 299, 300, 560}) {
        std::vector<int> st, sz;
        split_plan(n, B, st, sz);
        const int k = std::max(1, n / B);                           // merge_last: k chunks of B rows, the remainder in the last
        REQUIRE((int)st.size() == k && (int)sz.size() == k, "n = %d: %zu chunks, want %d", n, st.size(), k);
        for (int i = 0; i < k; ++i)
            REQUIRE(st[(size_t)i] == i * B && sz[(size_t)i] == (i < k - 1 ? B : n - (k - 1) * B), "n = %d chunk %d: %d + %d", n, i, st[(size_t)i], sz[(size_t)i]);
    }
    std::vector<int> st, sz;
    split_plan(560, B, st, sz);
    REQUIRE(sz == (std::vector<int>{150, 150, 260}), "560 -> 150 / 150 / 260");
    printf("ok split_plan\n");
}

static void permutations() {
    const int n = 16;
    std::vector<int> out((size_t)n, -1);
    uint64_t rng[4] = {1, 2, 3, 4};
    std::vector<int64_t> p((size_t)n);
    for (int i = 0; i < n; ++i) p[(size_t)i] = (i * 5 + 3) % n;
    PermFill r = perm_fill(out.data(), n, p.data(), rng, 9);
    REQUIRE(r.code == PERM_OK && rng[0] == 1 && rng[1] == 2, "a caller's permutation leaves the generator alone");
    for (int i = 0; i < n; ++i) REQUIRE(out[(size_t)i] == (int)p[(size_t)i], "copied");
    for (long long bad : {-1LL, (long long)n, 1LL << 40}) {
        std::vector<int64_t> q = p; q[5] = bad;
        r = perm_fill(out.data(), n, q.data(), rng, 0);
        REQUIRE(r.code == PERM_RANGE && r.index == 5 && r.value == bad, "out of range: code %d index %d", r.code, r.index);
    }
    { std::vector<int64_t> q = p; q[11] = q[2];
      r = perm_fill(out.data(), n, q.data(), rng, 0);
      REQUIRE(r.code == PERM_TWICE && r.index == 11 && r.value == q[2], "repeated: code %d index %d", r.code, r.index); }
    // the library's own shuffle: literals from the loop as it stood before it moved here (state {1, 2, 3, 4}, n = 16)
    const std::vector<int> want0 = {3, 6, 10, 4, 12, 2, 9, 1, 7, 5, 13, 14, 11, 8, 15, 0};
    const std::vector<int> want7 = {7, 4, 13, 14, 9, 8, 10, 5, 15, 1, 6, 2, 3, 12, 11, 0};
    std::vector<int> a((size_t)n), b((size_t)n), c7((size_t)n);
    uint64_t r0[4] = {1, 2, 3, 4}, r1[4] = {1, 2, 3, 4}, r7[4] = {1, 2, 3, 4};
    REQUIRE(perm_fill(a.data(), n, nullptr, r0, 0).code == PERM_OK && perm_fill(b.data(), n, nullptr, r1, 0).code == PERM_OK, "shuffle");
    REQUIRE(perm_fill(c7.data(), n, nullptr, r7, 7).code == PERM_OK, "shuffle");
    REQUIRE(a == b && !memcmp(r0, r1, sizeof(r0)), "equal state and seed: equal output and equal state after");
    REQUIRE(a == want0 && c7 == want7 && a != c7, "the recorded shuffles");
    for (int big : {1, 2, 1000}) {                                  // a permutation at every size, the stream continuing
        std::vector<int> o((size_t)big);
        REQUIRE(perm_fill(o.data(), big, nullptr, r0, 3).code == PERM_OK, "shuffle");
        REQUIRE((int)std::set<int>(o.begin(), o.end()).size() == big && *std::min_element(o.begin(), o.end()) == 0 &&
                *std::max_element(o.begin(), o.end()) == big - 1, "n = %d: not a permutation", big);
    }
    REQUIRE(perm_fill(out.data(), 0, nullptr, r0, 0).code == PERM_OK && perm_fill(out.data(), 0, p.data(), r0, 0).code == PERM_OK, "n = 0");
    printf("ok perm_fill\n");
}

// the dispatch, simulated independently: every block in launch order onto the CU that is free first (a linear scan)
static double span_of(int n32, int n16, int ny, int n_cus, double rho) {
    std::vector<double> cu((size_t)n_cus, 0.0);
    double span = 0.0;
    for (int b = 0; b < ny * (n32 + n16); ++b) {
        size_t first = 0;
        for (size_t i = 1; i < cu.size(); ++i) if (cu[i] < cu[first]) first = i;
        cu[first] += b < ny * n32 ? 1.0 : rho;
        span = std::max(span, cu[first]);
    }
    return span;
}
static void tile_splits() {
    int checked = 0;
    for (int64_t N : {1, 16, 17, 32, 33, 500, 4097}) for (int ny : {1, 2}) for (int n_cus : {1, 4, 256}) for (double rho : {0.60, 0.62}) {
        const TileSplit sp = mixed_split(N, ny, n_cus, rho);
        const int max32 = (int)((N + 31) / 32);
        const int64_t covered = 32 * (int64_t)sp.n32 + 16 * (int64_t)sp.n16;
        REQUIRE(sp.n32 >= 0 && sp.n16 >= 0 && covered >= N, "N = %lld: %d + %d tiles do not cover it", (long long)N, sp.n32, sp.n16);
        // 16-row tiles end within one tile of N; 32-row tiles alone may stand one 16-row group past the last 16-row boundary
        // (what TrState::rows_pad leaves room for), never a whole 32-row tile
        REQUIRE(covered - N < (sp.n16 > 0 ? 16 : 32), "N = %lld: %d + %d tiles, %lld spare rows", (long long)N, sp.n32, sp.n16, (long long)(covered - N));
        REQUIRE(sp.n32 < max32 || sp.n16 == 0, "N = %lld: 16-row tiles beside a full count of 32-row tiles", (long long)N);
        double best = 1e300; int best32 = -1;
        for (int n32 = 0; n32 <= max32; ++n32) {                    // every candidate; ties go to the larger n32
            const int64_t rem = N - 32 * (int64_t)n32;
            const double s = span_of(n32, rem > 0 ? (int)((rem + 15) / 16) : 0, ny, n_cus, rho);
            if (s < best - 1e-9 || std::fabs(s - best) <= 1e-9) { best = std::min(best, s); best32 = n32; }
        }
        REQUIRE(std::fabs(span_of(sp.n32, sp.n16, ny, n_cus, rho) - best) <= 1e-9 && sp.n32 == best32,
                "N = %lld ny %d cus %d rho %.2f: %d + %d, the scan says n32 = %d (span %g)", (long long)N, ny, n_cus, rho, sp.n32, sp.n16, best32, best);
        checked += 1;
    }
    // full size, literals from the function as it stood before it moved here (either rho)
    const int lit[4][4] = {{1, 256, 512, 226}, {3, 256, 597, 56}, {1, 512, 512, 226}, {3, 512, 625, 0}};
    for (const auto& l : lit) for (double rho : {0.60, 0.62}) {
        const TileSplit sp = mixed_split(20000, l[0], l[1], rho);
        REQUIRE(sp.n32 == l[2] && sp.n16 == l[3], "N = 20000 ny %d cus %d: %d + %d", l[0], l[1], sp.n32, sp.n16);
    }
    // the two plans that do not simulate
    int a = -1, b = -1;
    co_plan(20000, 512, &a, &b);   REQUIRE(a == 497 && b == 256 && 32 * a + 16 * b >= 20000, "co_plan: %d + %d", a, b);
    co_plan(100, 512, &a, &b);     REQUIRE(a == 0 && b == 7, "co_plan below one tail: %d + %d", a, b);
    forced_split(100, 2, &a, &b);  REQUIRE(a == 2 && b == 3, "forced_split: %d + %d", a, b);
    forced_split(100, 99, &a, &b); REQUIRE(a == 3 && b == 1, "forced_split keeps whole 32-row tiles: %d + %d", a, b);
    printf("ok mixed_split shapes=%d\n", checked);
}

int main(int argc, char** argv) {
    REQUIRE(argc == 2, "usage: trust_host_sim ROWS.txt");
    recorded_rows(argv[1]);
    dual_scripted();
    schedules_scripted();
    predicates();
    splits();
    permutations();
    tile_splits();
    return 0;
}
