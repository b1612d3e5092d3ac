// host_decisions.hpp -- what the update paths DECIDE on the host between their launches: CPO's dual solve, the two line searches'
// acceptance rules and step schedules, the minibatch split, the permutation check / shuffle, the tile-split dispatch simulation.
// Standard library only (no HIP), so tests/host/trust_host_sim.cpp drives it as a plain program (tests/test_trust_host.py).
#pragma once
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include <functional>
#include <queue>
#include <vector>

// ---- CPO's dual problem (cpo.py:256-304), float32 like the reference.  q = g.H^-1 g, r = g.H^-1 b, s = b.H^-1 b, bb = b.b.
static constexpr float CPO_EPS = 1e-8f;
// case 4: no cost gradient and inside the limit -- the caller skips the second conjugate-gradient solve (H^-1 b := 0, r = s = 0)
static inline bool cpo_cost_solve_skipped(float bb, float c_value) { return bb <= CPO_EPS && c_value < 0; }
struct CpoDual { int ocase; float A, B, lam, nu; };
static inline CpoDual cpo_dual_solve(float s_q, float s_r, float s_s, float c_value, float delta, float bb) {
    const float EPS = CPO_EPS;
    float A = 0.f, B = 0.f, lam, nu;
    int ocase = 4;
    if (!cpo_cost_solve_skipped(bb, c_value)) {
        A = s_q - s_r * s_r / s_s;
        B = 2.0f * delta - c_value * c_value / s_s;
        if (c_value < 0 && B < 0) ocase = 3;
        else if (c_value < 0 && B >= 0) ocase = 2;
        else if (c_value >= 0 && B >= 0) ocase = 1;
        else ocase = 0;
    }
    if (ocase == 3 || ocase == 4) {
        lam = std::sqrt(s_q / (2.0f * delta));
        nu = 0.0f;
    } else if (ocase == 1 || ocase == 2) {
        const float rc_ = s_r / c_value, inf = INFINITY;
        float LA[2] = {0.0f, rc_}, LB[2] = {rc_, inf};
        if (!(c_value < 0)) { std::swap(LA[0], LB[0]); std::swap(LA[1], LB[1]); }
        auto proj = [](float x, const float* L) { return std::max(L[0], std::min(L[1], x)); };
        const float lam_a = proj(std::sqrt(A / B), LA), lam_b = proj(std::sqrt(s_q / (2.0f * delta)), LB);
        auto f_a = [&](float l) { return -0.5f * (A / (l + EPS) + B * l) - s_r * c_value / (s_s + EPS); };
        auto f_b = [&](float l) { return -0.5f * (s_q / (l + EPS) + 2.0f * delta * l); };
        lam = (f_a(lam_a) >= f_b(lam_b)) ? lam_a : lam_b;
        nu = std::max(0.0f, lam * c_value - s_r) / (s_s + EPS);
    } else {
        nu = std::sqrt(2.0f * delta / (s_s + EPS));
        lam = 0.0f;
    }
    return {ocase, A, B, lam, nu};
}

// ---- line searches.  `try_step(step)` moves theta to theta0 + step * dir, evaluates and says whether the step is accepted.
// CPO (cpo.py:306-333): cases 0 and 1 (recovery) ignore the objective; the cost may rise by the room left under the limit.
// TRPO-Lagrangian (trpo_lag.py:211-227): inside the trust region, strictly, and the loss must fall.
static inline bool cpo_accepts(float new_kl, float new_obj, float new_cs, float delta, int ocase, float objective, float cost_sur,
                               float c_value) {
    return ((double)new_kl <= (double)delta) && (ocase > 1 ? new_obj > objective : true) &&
           ((double)(new_cs - cost_sur) <= std::max(-(double)c_value, 0.0));
}
static inline bool trpo_accepts(float kl, float delta, float loss_new, float loss_actor) {
    return (double)kl < (double)delta && loss_new < loss_actor;
}
// CPO's schedule, in float64 like the reference's: beta shrinks after EVERY refusal (a total failure logs coeff^max_backtracks);
// a NaN multiplier tries nothing
struct CpoSearch { double beta; int evals; };
template <class Try>
static CpoSearch cpo_line_search(float lam, double coeff, int max_backtracks, Try&& try_step) {
    CpoSearch r{1.0, 0};
    if (std::isnan(lam)) return r;
    for (int bt = 0; bt < max_backtracks; ++bt) {
        ++r.evals;
        if (try_step(r.beta)) break;
        r.beta *= coeff;
    }
    return r;
}
// TRPO-Lagrangian's: the step shrinks after a refusal except the last, where it is logged as 0 (the last tried theta stays)
struct TrpoSearch { float step; int evals; };
template <class Try>
static TrpoSearch trpo_line_search(float step, float coeff, int max_backtracks, Try&& try_step) {
    TrpoSearch r{step, 0};
    for (int i = 0; i < max_backtracks; ++i) {
        ++r.evals;
        if (try_step(r.step)) break;
        else if (i < max_backtracks - 1) r.step *= coeff;
        else r.step = 0.0f;
    }
    return r;
}

// ---- minibatches: tianshou Batch.split(size, merge_last=True): the remainder is merged into the last chunk
static inline void split_plan(int n, int B, std::vector<int>& st, std::vector<int>& sz) {
    st.clear(); sz.clear();
    const bool merge = (n % B) > 0;
    for (int i = 0; i < n; i += B) {
        if (merge && i + 2 * B >= n) { st.push_back(i); sz.push_back(n - i); break; }
        st.push_back(i); sz.push_back(std::min(B, n - i));
    }
}

// ---- xoshiro256**: the library's random streams (action noise, its own minibatch shuffles)
static inline uint64_t rotl64(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
static inline uint64_t xoshiro_next(uint64_t* s) {
    const uint64_t result = rotl64(s[1] * 5, 7) * 9, t = s[1] << 17;
    s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3]; s[2] ^= t; s[3] = rotl64(s[3], 45);
    return result;
}
// out[0 .. n) := the caller's permutation after checking it, or (perm == NULL) a Fisher-Yates shuffle from `rng`, which a
// non-zero seed perturbs first.  A refusal names the entry: perm[index] == value.
enum { PERM_OK = 0, PERM_RANGE, PERM_TWICE };
struct PermFill { int code, index; long long value; };
static inline PermFill perm_fill(int* out, int n, const int64_t* perm, uint64_t* rng, uint64_t seed) {
    if (perm) {
        std::vector<uint8_t> seen((size_t)n, 0);
        for (int i = 0; i < n; ++i) {
            if (!(perm[i] >= 0 && perm[i] < n)) return {PERM_RANGE, i, (long long)perm[i]};
            if (seen[(size_t)perm[i]]) return {PERM_TWICE, i, (long long)perm[i]};
            seen[(size_t)perm[i]] = 1;
            out[i] = (int)perm[i];
        }
        return {PERM_OK, 0, 0};
    }
    if (seed) { rng[0] ^= seed; rng[1] += seed * 0x9E3779B97F4A7C15ull; }
    for (int i = 0; i < n; ++i) out[i] = i;
    for (int i = n - 1; i > 0; --i) std::swap(out[i], out[(int)(xoshiro_next(rng) % (uint64_t)(i + 1))]);
    return {PERM_OK, 0, 0};
}

// ---- Tile heights of one full-batch launch over N rows of ny networks on n_cus CUs (one workgroup per CU): n32 32-row tiles
// first, n16 16-row tiles for the remaining rows.  A 32-row tile moves half the weight-fragment bytes per row but a partly filled
// LAST round of them idles most of the chip for a whole tile time, so the split is chosen by simulating the dispatch (blocks in
// launch order onto the earliest free CU) with rho = duration of a 16-row tile / a 32-row tile.  Ties go to the larger n32.
struct TileSplit { int n32, n16; };
static inline TileSplit mixed_split(int64_t N, int ny, int n_cus, double rho) {
    const int max32 = (int)((N + 31) / 32);
    double best = 1e300; int best32 = 0, best16 = (int)((N + 15) / 16);
    std::vector<double> cu((size_t)std::max(n_cus, 1));
    for (int n32 = 0; n32 <= max32; ++n32) {
        const int64_t rem = N - 32 * (int64_t)n32;
        const int n16 = rem > 0 ? (int)((rem + 15) / 16) : 0;
        if (n16 > 0 && n32 == max32) continue;
        std::fill(cu.begin(), cu.end(), 0.0);
        std::priority_queue<double, std::vector<double>, std::greater<double>> pq(cu.begin(), cu.end());
        double span = 0.0;
        for (int b = 0; b < ny * n32; ++b) { const double e = pq.top() + 1.0; pq.pop(); pq.push(e); span = std::max(span, e); }
        for (int b = 0; b < ny * n16; ++b) { const double e = pq.top() + rho; pq.pop(); pq.push(e); span = std::max(span, e); }
        if (span < best - 1e-9 || (std::fabs(span - best) <= 1e-9 && n32 > best32)) { best = span; best32 = n32; best16 = n16; }
    }
    return {best32, best16};
}
// the persistent launches' tile mix: 32-row tiles while a whole round of workgroup pairs is left, then 16-row tiles so that the
// CUs run dry together (the dispatch is dynamic: no simulation needed, only the size of the fine-grained tail)
static inline void co_plan(int64_t N, int n_wgs, int* n32_out, int* n16_out) {
    const int64_t tail_rows = std::min<int64_t>(N, 16 * (int64_t)(n_wgs / 2));      // half a round of 16-row tiles
    const int n32 = (int)((N - tail_rows) / 32);
    const int64_t rem = N - 32 * (int64_t)n32;
    *n32_out = n32; *n16_out = (int)((rem + 15) / 16);
}
static inline void forced_split(int64_t N, int want32, int* n32_out, int* n16_out) {
    const int n32 = (int)std::min<int64_t>(want32, N / 32);             // whole 32-row tiles only
    const int64_t rem = N - 32 * (int64_t)n32;
    *n32_out = n32; *n16_out = (int)((rem + 15) / 16);
}

// ---- The clipped PPO-Lagrangian step in two launches: the weight-gradient launch exchanges its blocks' squared-norm partials inside
// the launch and applies clip + Adam itself (kernels_mlp.hpp: clip_exchange).  Its blocks wait for each other, so (a) all of them must
// fit the chip at once, (b) the wait is bounded, and (c) an update in which a wait ran out is replayed from a snapshot with three
// launches per step -- which reproduces the update only where nothing but P, M, V and the step counters carries over from it.
// The bound: an exchange takes 1.7 us on an idle chip (profiles/clip_exchange_ubench.txt) and the blocks of one weight-gradient launch
// finish within about 6 us of each other, so 50 us = 5 000 ticks of the 100 MHz wall clock is some 30 exchanges -- far above
// anything a launch that has the chip to itself needs, far below anything a person would call a hang.
static constexpr int CLIP_FUSE_DEFAULT_TICKS = 5000;
static constexpr int CLIP_FUSE_MAX_OBS = 64;       // the dW1 role holds back one gradient element per 16 observation columns, 4 at most
struct ClipFuseFacts {
    int mode;                 // fsrl_ppo_set_clip_fuse: -1 automatic, 0 off, 1 on
    bool env_off;             // FSRL_NO_CLIP_FUSE
    bool dead;                // a wait ran out earlier in this context's life
    bool ppo_lag, layered, grouped;
    bool recompute_adv, rew_norm;
    float max_grad_norm;
    int nparts, n_cus;        // blocks of the weight-gradient launch | CUs
    int obs_dim;
    int live_contexts;        // contexts alive on this device in this process, this one included
};
// may THIS UPDATE take the two-launch step?  mode 1 forces nothing the kernel or the replay cannot do.  The automatic rule has one
// condition more: the context is alone on its device in this process.  Contexts that update side by side (one host thread each:
// bench.py's multi_seed leg) take CUs from each other's weight-gradient launches, the waits run out, and every context pays one
// replayed update before it settles on three launches (measured: each of three contexts fell back in its first concurrent update,
// the six-update leg 181 -> 149 updates/s aggregate); other PROCESSES on the GPU cannot be seen from here, the bounded wait covers them.
static inline bool clip_fuse_update_ok(const ClipFuseFacts& f) {
    if (f.mode == 0 || f.env_off || f.dead) return false;
    if (f.mode < 0 && f.live_contexts > 1) return false;
    if (!f.ppo_lag || f.layered || f.grouped) return false;                 // solo fused PPO-Lagrangian contexts only
    if (!(f.max_grad_norm > 0.0f)) return false;                            // no clip: the fuse_adam form needs no exchange
    if (f.recompute_adv || f.rew_norm) return false;                        // a replay would not reproduce the update
    if (f.nparts > f.n_cus || f.nparts > 1024) return false;                // every block resident at once, one poller thread per block
    return f.obs_dim <= CLIP_FUSE_MAX_OBS;
}
// may this STEP?  padded rows of the minibatch: above 512 the weight gradients take the split-K route and its own Adam launch
static inline bool clip_fuse_step_ok(bool update_ok, int rows_pad) { return update_ok && rows_pad <= 512; }
// after a read of the control block: replay?  (only an update that ran two-launch steps can have been poisoned)
static inline bool clip_fuse_must_replay(bool active, int poisoned) { return active && poisoned != 0; }
// what a replay starts from
struct ClipFuseReplay { long long adam_t, n_steps; int pass_index, passes; };
static inline ClipFuseReplay clip_fuse_replay_plan(long long snap_adam_t, int passes_enqueued) {
    return {snap_adam_t, 0, 0, passes_enqueued};
}

// ---- process_fn: V(obs_next) from V(obs).  In an on-policy store obs_next[t] is obs[t + 1] unless the episode ended or the ring wrapped,
// so the value job of row r + 1 also gives vnext[r] where the two rows' words are bitwise equal (next_same[r], written next to the gather);
// the "next" jobs of mlp_infer_kernel walk only the compacted list of the other rows ("misses").  The split of the launch's workgroups over
// its jobs is decided IN the kernel from the device-side miss count (no host synchronisation); the host calls the same function for its
// counters and the tests.  gx x jobs_y: the launch grid (jobs_y = 2 C + 1 with the actor job, 2 C without), C next jobs, jobs_y - C full
// jobs of n_tiles 16-row tiles, miss_tiles tiles of listed rows per next job.
//   bn workgroups per next job, bf per full job, C * bn + (jobs_y - C) * bf <= gx * jobs_y; the workgroups left over exit at once.
//   The workgroups are shared out in proportion to the tiles: bn = ceil(T * m / (F * n + C * m)), at most gx and at most m.  A store whose
//   rows never coincide (m = n) gives bn = bf = gx, the equal split of a launch without reuse.
#if defined(__HIPCC__)
#define FSRL_HD __host__ __device__
#else
#define FSRL_HD
#endif
// persistent over tiles: about one workgroup per CU in total (their LDS footprint allows no more), gx per job
static inline int infer_grid_x(int tiles, int n_cus, int jobs_y) { return std::min(tiles, std::max(1, n_cus / jobs_y)); }
struct InferSplit { int bn, bf, equal; };
FSRL_HD static inline InferSplit infer_split(int gx, int jobs_y, int C, int n_tiles, int miss_tiles) {
    const int F = jobs_y - C, T = gx * jobs_y;
    InferSplit s{0, 0, 0};
    if (miss_tiles > 0) {
        const long long den = (long long)F * n_tiles + (long long)C * miss_tiles;
        long long bn = ((long long)T * miss_tiles + den - 1) / den;
        if (bn > gx) bn = gx;
        if (bn > miss_tiles) bn = miss_tiles;
        if (bn < 1) bn = 1;
        s.bn = (int)bn;
    }
    if (s.bn == gx) { s.bf = gx; s.equal = 1; return s; }
    s.bf = (T - C * s.bn) / F;
    if (s.bf > n_tiles) s.bf = n_tiles;
    return s;
}
// the host's count of the rows whose obs_next is the next batch row's obs, word for word (tests; the device flags the same rows)
static inline int next_same_count(const uint32_t* obs, const uint32_t* obs_next, int n, int Do) {
    int same = 0;
    for (int r = 0; r + 1 < n; ++r) {
        bool eq = true;
        for (int k = 0; k < Do && eq; ++k) eq = obs_next[(size_t)r * Do + k] == obs[(size_t)(r + 1) * Do + k];
        same += eq ? 1 : 0;
    }
    return same;
}

// ---- fsrl_ppo_begin's one upload: everything the device needs from the host for an update in one pinned block, one device block of
// the same layout and one copy.  Byte offsets; every array starts on 64 bytes.  The control block leads (its device address never
// moves), the miss counter of the V(obs_next) reuse follows it (uploaded as 0), then the sample(0) indices -- written in place by the
// sampler, before n is known to anybody else, which is why they come first -- the end flags, the GAE segment starts and the minibatch plan.
struct UploadLayout { size_t ctrl, miss_count, indices, end, seg, mb_start, mb_size, total; };
static constexpr size_t UPLOAD_HEAD = 128;            // control block (<= 64 bytes) | miss counter
static inline size_t upload_align(size_t x) { return (x + 63) / 64 * 64; }
static inline UploadLayout upload_layout(size_t n, size_t n_seg, size_t n_mb) {
    UploadLayout u{};
    u.ctrl = 0; u.miss_count = 64; u.indices = UPLOAD_HEAD;
    u.end = u.indices + upload_align(n * 4);
    u.seg = u.end + upload_align(n);
    u.mb_start = u.seg + upload_align((n_seg + 1) * 4);
    u.mb_size = u.mb_start + upload_align(n_mb * 4);
    u.total = u.mb_size + upload_align(n_mb * 4);
    return u;
}
// capacity of the two blocks for a store of `rows` rows: at most `rows` segments and `rows` minibatches
static inline size_t upload_capacity(size_t rows) { return upload_layout(rows, rows, rows).total; }
