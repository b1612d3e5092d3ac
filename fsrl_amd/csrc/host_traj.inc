// host_traj.inc -- the trajectory archive: fsrl_traj_* (part of fsrl_hip.hip; include/fsrl_hip.h has the contract).
//
// A tap on a context's store ingest.  fsrl_store_push hands every row it stages to tap_row (host: the env's float64 returns, the
// row's place in the open-episode area, the action the env received); flush_stage hands every window it flushes to tap_flush, which
// on the context's SIDE stream, behind the window's own copy and scatter, issues
//     one H2D copy      the tap's records of the window (+ the job table of the episodes that ended in it)
//     traj_stage_kernel the window's rows -> the open-episode area
//     traj_move_kernel  the episodes that ended in the window -> the tail of the archive     (only when one ended)
// so a row is in HBM once and comes back to the host only in fsrl_traj_export.  The bookkeeping -- episode table, room, the job tables, the
// two halves of the archive -- is traj_plan.hpp (HIP-free, driven by tests/host/traj_plan_sim.cpp).
//
// Ordering.  Everything a context feeds is ordered by that context's side stream.  Several contexts may feed one archive: their
// commits go to disjoint rows the host assigned, so their side streams need no order among each other.  A compaction reads what all
// of them wrote: it waits for every feeding context's side stream, runs on the archive's own stream and is waited for.  The calls
// of one archive, and the pushes of the contexts that feed it, come from one thread.
//
// Datasets in.  fsrl_traj_import commits host columns in the export layout as tapped episodes are committed: the accepted rows go to
// the tail of the current half in one copy per column and run of neighbouring accepted episodes, on the archive's own stream, and
// are waited for.  fsrl_store_fill pours archived episodes into a context's store: one H2D copy of a job table (store_fill_plan.hpp)
// and ONE launch of store_fill_kernel on that context's side stream.  The kernel reads the current half; a compaction (which makes
// the other half current, so that the one after it would write what the kernel reads) waits for the last fill first.
#include "traj_plan.hpp"
#include "store_fill_plan.hpp"
#include "kernels_traj.hpp"

static_assert(sizeof(TrajJob) == sizeof(trajp::Job), "TrajJob mirrors trajp::Job");

struct fsrl_traj {
    int device = 0, Do = 0, Da = 0;
    int32_t bound_method = 0;
    bool bounds = false;
    std::vector<float> low, high;
    trajp::Book book;
    TrajCols half[2] = {};
    hipStream_t stream = nullptr;
    DevTable<TrajJob> jobs;             // compaction's job table
    std::vector<fsrl_tap*> taps;
    int32_t next_source = 0;
    int64_t launches = 0, h2d_bytes = 0;
    // fsrl_store_fill: [job table | low[Da] | scale[Da]] in one pinned buffer and its device copy; fill_done is recorded behind the
    // last fill's launch on the side stream it ran on
    DevTable<uint8_t> fill;
    Mem mem;                            // the two halves' columns
    hipEvent_t fill_done = nullptr;
    bool fill_pending = false;
    int64_t fill_launches = 0, fill_copies = 0;
};
static int traj_fill_wait(fsrl_traj* t) {
    if (!t->fill_pending) return 0;
    HIPCHK(hipEventSynchronize(t->fill_done));
    t->fill_pending = false;
    return 0;
}

struct fsrl_tap {
    fsrl_traj* t = nullptr;
    fsrl_ctx* c = nullptr;
    Mem mem;                            // the open-episode columns and the two windows
    int32_t source = 0;
    int L = 0;                          // rows per env of the open-episode area = max_episode_len
    std::vector<trajp::OpenEpisode> env;
    std::vector<trajp::Pending> pending;
    TrajCols open = {};                 // [2 cfg.env_num x L] rows: two slots per env (trajp::OpenEpisode)
    uint8_t* h[2] = {nullptr, nullptr};     // pinned, one per staging window: STAGE_CAP records, then the window's job table
    uint8_t* d[2] = {nullptr, nullptr};
    size_t rec = 0, max_jobs = 0;
};

static int traj_cols_alloc(Mem& m, TrajCols& c, size_t rows, int Do, int Da) {
    HIPCHK(m.dev(&c.obs, rows * Do * 4)); HIPCHK(m.dev(&c.obs_next, rows * Do * 4));
    HIPCHK(m.dev(&c.act, rows * Da * 4)); HIPCHK(m.dev(&c.rew, rows * 8)); HIPCHK(m.dev(&c.cost, rows * 8));
    HIPCHK(m.dev(&c.terminals, rows)); HIPCHK(m.dev(&c.timeouts, rows));
    return 0;
}

static inline bool tap_closed(const fsrl_ctx* c, int e) { return c->tap->env[(size_t)e].ends >= 2; }

// one staged row: record i of the current window, env e
static void tap_row(fsrl_ctx* c, int e, int i, const float* act, double rew, double cost, uint8_t fl) {
    fsrl_tap* tp = c->tap;
    fsrl_traj* t = tp->t;
    trajp::OpenEpisode& oe = tp->env[(size_t)e];
    uint8_t* r = tp->h[c->cur_stage] + (size_t)i * tp->rec;
    const int32_t slot = 2 * e + oe.parity;
    const int32_t dst = oe.rows < tp->L ? (int32_t)((int64_t)slot * tp->L + oe.rows) : -1;
    memcpy(r, &dst, 4);
    map_env_action(t->Da, 1, t->bound_method, t->bounds ? t->low.data() : nullptr, t->bounds ? t->high.data() : nullptr, act,
                   reinterpret_cast<float*>(r + 4));
    oe.rows += 1; oe.rew += rew; oe.cost += cost;       // current_rew += ... .item() (traj_buf.py:66-69): float64, push order
    if (!fl) return;
    if (oe.rows > tp->L) t->book.n.dropped_long += 1;
    else if (!t->book.in_window(oe.rew, oe.cost)) t->book.n.rejected_window += 1;
    else tp->pending.push_back(trajp::Pending{slot, oe.rows, oe.rew, oe.cost, fl});
    oe.next();              // its rows are in this window, in this slot: the env's next episode takes the other one
}

static int traj_compact(fsrl_traj* t) {
    int frc = traj_fill_wait(t);
    if (frc) return frc;
    for (fsrl_tap* tp : t->taps) HIPCHK(hipStreamSynchronize(tp->c->side));
    std::vector<trajp::Job> jobs;
    const int from = t->book.cur;
    t->book.compact(jobs);
    if (jobs.empty()) return 0;
    int rc = table_ensure(t->jobs, jobs.size(), jobs.size() + jobs.size() / 2 + 64, t->stream);
    if (rc) return rc;
    memcpy(t->jobs.h, jobs.data(), jobs.size() * sizeof(TrajJob));
    HIPCHK(hipMemcpyAsync(t->jobs.d, t->jobs.h, jobs.size() * sizeof(TrajJob), hipMemcpyHostToDevice, t->stream));
    hipLaunchKernelGGL(traj_move_kernel, dim3((unsigned)std::min<size_t>(jobs.size(), 4096)), dim3(256), 0, t->stream, t->half[from],
                       t->half[from ^ 1], t->jobs.d, (int)jobs.size(), t->Do, t->Da);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(t->stream));
    return 0;
}

// the window of k records that flush_stage just sent (staging buffer `w`, device copy recs_d), on c->side
static int tap_flush(fsrl_ctx* c, int w, const uint8_t* recs_d, int stage_rec, int k) {
    fsrl_tap* tp = c->tap;
    fsrl_traj* t = tp->t;
    int rc = 0;
    std::vector<trajp::Job> jobs;
    if (!tp->pending.empty()) {
        if (trajp::batch_wants_compaction(t->book, tp->pending)) {
            rc = traj_compact(t);
            if (rc) return rc;
        }
        if (trajp::commit_batch(t->book, tp->pending, tp->L, tp->source, jobs)) rc = fail(FSRL_ENOMEM, "%s", t->book.err.c_str());
        tp->pending.clear();
    }
    for (trajp::OpenEpisode& oe : tp->env) oe.ends = 0;
    const size_t recs_bytes = ((size_t)k * tp->rec + 7) / 8 * 8;
    if (jobs.size() > tp->max_jobs) return fail(FSRL_ESTATE, "trajectory tap: %zu jobs in one window (table of %zu)", jobs.size(), tp->max_jobs);
    if (!jobs.empty()) memcpy(tp->h[w] + recs_bytes, jobs.data(), jobs.size() * sizeof(TrajJob));
    const size_t bytes = recs_bytes + jobs.size() * sizeof(TrajJob);
    HIPCHK(hipMemcpyAsync(tp->d[w], tp->h[w], bytes, hipMemcpyHostToDevice, c->side));
    const int per = 2 * t->Do + t->Da + 1;
    hipLaunchKernelGGL(traj_stage_kernel, dim3(std::min(1024, (k * per + 255) / 256)), dim3(256), 0, c->side, tp->open, recs_d,
                       stage_rec, tp->d[w], (int)tp->rec, k, t->Do, t->Da);
    HIPCHK(hipGetLastError());
    t->launches += 1; t->h2d_bytes += (int64_t)bytes;
    if (!jobs.empty()) {
        hipLaunchKernelGGL(traj_move_kernel, dim3((unsigned)std::min<size_t>(jobs.size(), 4096)), dim3(256), 0, c->side, tp->open,
                           t->half[t->book.cur], reinterpret_cast<const TrajJob*>(tp->d[w] + recs_bytes), (int)jobs.size(), t->Do, t->Da);
        HIPCHK(hipGetLastError());
        t->launches += 1;
    }
    return rc;
}

// take the tap off its context.  commit: flush the context's staging window first, so that episodes that have ended are archived
static void tap_free(fsrl_tap* tp, bool commit) {
    fsrl_ctx* c = tp->c;
    (void)hipSetDevice(c->device);
    if (commit) (void)flush_stage(c);
    (void)hipStreamSynchronize(c->side);
    c->tap = nullptr;
    fsrl_traj* t = tp->t;
    t->taps.erase(std::remove(t->taps.begin(), t->taps.end(), tp), t->taps.end());
    tp->mem.release_all();
    delete tp;
}
static void tap_ctx_gone(fsrl_ctx* c) { if (c->tap) tap_free(c->tap, true); }

extern "C" int fsrl_traj_destroy(fsrl_traj* t) {
    if (!t) return 0;
    (void)hipSetDevice(t->device);
    while (!t->taps.empty()) tap_free(t->taps.back(), false);
    (void)traj_fill_wait(t);
    if (t->fill_done) (void)hipEventDestroy(t->fill_done);
    table_free(t->fill);
    if (t->stream) { (void)hipStreamSynchronize(t->stream); (void)hipStreamDestroy(t->stream); }
    t->mem.release_all();
    table_free(t->jobs);
    delete t;
    return 0;
}

extern "C" int fsrl_traj_create(fsrl_ctx* c, int64_t max_rows, int32_t max_episodes, int32_t max_episode_len, int32_t bound_method,
                                const float* act_low, const float* act_high, fsrl_traj** out) {
    CHECK_ARG(c && out, "null argument");
    CHECK_ARG(max_episode_len >= 1, "max_episode_len must be at least 1");
    CHECK_ARG(max_episodes >= 1, "max_episodes must be at least 1");
    CHECK_ARG(max_rows >= max_episode_len && max_rows < (int64_t)INT_MAX, "max_rows must be in [max_episode_len, 2^31)");
    CHECK_ARG(2 * (int64_t)c->cfg.env_num * max_episode_len < (int64_t)INT_MAX, "2 x env_num x max_episode_len must stay below 2^31");
    CHECK_ARG(bound_method >= 0 && bound_method <= 2, "bound_method: 0 none, 1 clip, 2 tanh");
    CHECK_ARG((act_low == nullptr) == (act_high == nullptr), "act_low and act_high are given together");
    HIPCHK(hipSetDevice(c->device));
    fsrl_traj* t = new fsrl_traj();
    t->device = c->device; t->Do = c->cfg.obs_dim; t->Da = c->cfg.act_dim;
    t->bound_method = bound_method;
    if (act_low) { t->bounds = true; t->low.assign(act_low, act_low + t->Da); t->high.assign(act_high, act_high + t->Da); }
    t->book.max_rows = max_rows; t->book.max_episodes = max_episodes; t->book.max_len = max_episode_len;
    int rc = 0;
    { hipError_t e = hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking); if (e != hipSuccess) rc = fail(FSRL_EHIP, "hipStreamCreate failed: %s", hipGetErrorString(e)); }
    if (!rc && hipEventCreateWithFlags(&t->fill_done, hipEventDisableTiming) != hipSuccess) rc = fail(FSRL_EHIP, "hipEventCreate failed");
    if (!rc) rc = traj_cols_alloc(t->mem, t->half[0], (size_t)max_rows, t->Do, t->Da);
    if (!rc) rc = traj_cols_alloc(t->mem, t->half[1], (size_t)max_rows, t->Do, t->Da);
    if (rc) { const std::string keep = g_err; fsrl_traj_destroy(t); g_err = keep; return rc; }
    *out = t;
    return 0;
}

extern "C" int fsrl_traj_attach(fsrl_traj* t, fsrl_ctx* c, int32_t* source_out) {
    CHECK_ARG(t && c, "null argument");
    CHECK_ARG(!c->tap, "the context already has a trajectory tap (a context has at most one)");
    CHECK_ARG(c->cfg.obs_dim == t->Do, "obs_dim: the context has %d, the trajectory archive %d", c->cfg.obs_dim, t->Do);
    CHECK_ARG(c->cfg.act_dim == t->Da, "act_dim: the context has %d, the trajectory archive %d", c->cfg.act_dim, t->Da);
    CHECK_ARG(c->device == t->device, "device: the context is on %d, the trajectory archive on %d", c->device, t->device);
    HIPCHK(hipSetDevice(c->device));
    int rc = flush_stage(c);        // rows staged before the tap existed carry no tap records
    if (rc) return rc;
    fsrl_tap* tp = new fsrl_tap();
    tp->t = t; tp->c = c; tp->source = t->next_source; tp->L = t->book.max_len;
    tp->env.resize((size_t)c->cfg.env_num);
    tp->rec = 4 + 4 * (size_t)t->Da;
    tp->max_jobs = 2 * (size_t)c->cfg.env_num * (((size_t)tp->L + trajp::JOB_ROWS - 1) / trajp::JOB_ROWS);
    const size_t bytes = ((size_t)fsrl_ctx::STAGE_CAP * tp->rec + 7) / 8 * 8 + tp->max_jobs * sizeof(TrajJob);
    rc = traj_cols_alloc(tp->mem, tp->open, 2 * (size_t)c->cfg.env_num * tp->L, t->Do, t->Da);
    for (int i = 0; i < 2 && !rc; ++i) {
        if (tp->mem.pinned(&tp->h[i], bytes) != hipSuccess || tp->mem.dev(&tp->d[i], bytes) != hipSuccess)
            rc = fail(FSRL_EHIP, "trajectory tap: allocating %zu bytes failed", bytes);
    }
    t->taps.push_back(tp);
    c->tap = tp;
    if (rc) { const std::string keep = g_err; tap_free(tp, false); g_err = keep; return rc; }
    t->next_source += 1;
    if (source_out) *source_out = tp->source;
    return 0;
}

extern "C" int fsrl_traj_detach(fsrl_traj* t, fsrl_ctx* c) {
    CHECK_ARG(t && c, "null argument");
    CHECK_ARG(c->tap && c->tap->t == t, "the context does not feed this trajectory archive");
    tap_free(c->tap, true);
    return 0;
}

// the env of `c` were reset in mid-episode (a collector's reset_env): what their open episodes hold is no trajectory
extern "C" int fsrl_traj_abandon(fsrl_traj* t, fsrl_ctx* c) {
    CHECK_ARG(t && c, "null argument");
    CHECK_ARG(c->tap && c->tap->t == t, "the context does not feed this trajectory archive");
    for (trajp::OpenEpisode& oe : c->tap->env) {
        if (oe.rows == 0) continue;
        oe.next();              // rows of it may be in the current window: the env's next episode takes the other slot
        t->book.n.abandoned += 1;
    }
    return 0;
}

extern "C" int fsrl_traj_set_window(fsrl_traj* t, double rmin, double rmax, double cmin, double cmax) {
    CHECK_ARG(t, "null argument");
    t->book.set_window(rmin, rmax, cmin, cmax);
    return 0;
}

extern "C" int fsrl_traj_flush(fsrl_traj* t) {
    CHECK_ARG(t, "null argument");
    HIPCHK(hipSetDevice(t->device));
    int rc = 0;
    std::string first;
    for (fsrl_tap* tp : t->taps) {
        const int r = flush_stage(tp->c);
        if (r && !rc) { rc = r; first = g_err; }
    }
    for (fsrl_tap* tp : t->taps) HIPCHK(hipStreamSynchronize(tp->c->side));
    if (rc) g_err = first;
    return rc;
}

extern "C" int fsrl_traj_episodes(fsrl_traj* t, int64_t cap, int32_t* ids_out, int32_t* rows_out, double* rew_out, double* cost_out,
                                  int32_t* source_out, int64_t* n_out) {
    CHECK_ARG(t && n_out, "null argument");
    const int64_t n = (int64_t)t->book.table.size();
    *n_out = n;
    if (!ids_out && !rows_out && !rew_out && !cost_out && !source_out) return 0;
    CHECK_ARG(cap >= n, "episode table: room for %lld, %lld alive", (long long)cap, (long long)n);
    for (int64_t i = 0; i < n; ++i) {
        const trajp::Episode& e = t->book.table[(size_t)i];
        if (ids_out) ids_out[i] = e.id;
        if (rows_out) rows_out[i] = e.rows;
        if (rew_out) rew_out[i] = e.rew;
        if (cost_out) cost_out[i] = e.cost;
        if (source_out) source_out[i] = e.source;
    }
    return 0;
}

extern "C" int fsrl_traj_keep(fsrl_traj* t, const int32_t* episode_ids, int64_t n) {
    CHECK_ARG(t && (episode_ids || n == 0) && n >= 0, "bad argument");
    HIPCHK(hipSetDevice(t->device));
    int rc = fsrl_traj_flush(t);
    if (rc) return rc;
    if (!t->book.keep(episode_ids, n)) return fail(FSRL_EINVAL, "%s", t->book.err.c_str());
    return traj_compact(t);
}

extern "C" int fsrl_traj_replace(fsrl_traj* t, int32_t victim_id) {
    CHECK_ARG(t, "null argument");
    int rc = fsrl_traj_flush(t);
    if (rc) return rc;
    if (!t->book.replace(victim_id)) return fail(FSRL_EINVAL, "%s", t->book.err.c_str());
    return 0;
}

extern "C" int fsrl_traj_export(fsrl_traj* t, float* obs, float* next_obs, float* act, double* rew, double* cost, uint8_t* terminals,
                                uint8_t* timeouts, int64_t rows_cap, int64_t* rows_out) {
    CHECK_ARG(t && rows_out, "null argument");
    int rc = fsrl_traj_flush(t);
    if (rc) return rc;
    const size_t n = (size_t)t->book.alive_rows;
    *rows_out = (int64_t)n;
    if (!obs && !next_obs && !act && !rew && !cost && !terminals && !timeouts) return 0;
    CHECK_ARG(rows_cap >= (int64_t)n, "export: room for %lld rows, %lld alive", (long long)rows_cap, (long long)n);
    if (!t->book.packed) { rc = traj_compact(t); if (rc) return rc; }
    if (n == 0) return 0;
    const TrajCols& a = t->half[t->book.cur];
    const size_t Do = (size_t)t->Do, Da = (size_t)t->Da;
    if (obs) HIPCHK(hipMemcpy(obs, a.obs, n * Do * 4, hipMemcpyDeviceToHost));
    if (next_obs) HIPCHK(hipMemcpy(next_obs, a.obs_next, n * Do * 4, hipMemcpyDeviceToHost));
    if (act) HIPCHK(hipMemcpy(act, a.act, n * Da * 4, hipMemcpyDeviceToHost));
    if (rew) HIPCHK(hipMemcpy(rew, a.rew, n * 8, hipMemcpyDeviceToHost));
    if (cost) HIPCHK(hipMemcpy(cost, a.cost, n * 8, hipMemcpyDeviceToHost));
    if (terminals) HIPCHK(hipMemcpy(terminals, a.terminals, n, hipMemcpyDeviceToHost));
    if (timeouts) HIPCHK(hipMemcpy(timeouts, a.timeouts, n, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int fsrl_traj_clear(fsrl_traj* t) {
    CHECK_ARG(t, "null argument");
    int rc = fsrl_traj_flush(t);
    t->book.clear();
    return rc;
}

extern "C" int fsrl_traj_counters(fsrl_traj* t, int64_t* out, int32_t n) {
    CHECK_ARG(t && out && n >= 0, "bad argument");
    const trajp::Counters& k = t->book.n;
    const int64_t v[13] = {k.committed, k.rejected_window, k.dropped_long, k.compactions, k.rows, k.refused_full,
                           (int64_t)t->book.table.size(), t->launches, t->h2d_bytes, k.abandoned, k.import_open, t->fill_launches,
                           t->fill_copies};
    for (int i = 0; i < n && i < 13; ++i) out[i] = v[i];
    return 0;
}

// ------------------------------------------------------------------------------ datasets in
// the accepted runs so far: one copy per column, host rows -> the tail of the current half, on the archive's stream
static int import_send(fsrl_traj* t, std::vector<trajp::ImportRun>& runs, const float* obs, const float* next_obs, const float* act,
                       const double* rew, const double* cost, const uint8_t* terminals, const uint8_t* timeouts) {
    const TrajCols& a = t->half[t->book.cur];
    const size_t Do = (size_t)t->Do, Da = (size_t)t->Da;
    for (const trajp::ImportRun& r : runs) {
        const size_t s = (size_t)r.src, d = (size_t)r.dst, n = (size_t)r.rows;
        HIPCHK(hipMemcpyAsync(a.obs + d * Do, obs + s * Do, n * Do * 4, hipMemcpyHostToDevice, t->stream));
        HIPCHK(hipMemcpyAsync(a.obs_next + d * Do, next_obs + s * Do, n * Do * 4, hipMemcpyHostToDevice, t->stream));
        HIPCHK(hipMemcpyAsync(a.act + d * Da, act + s * Da, n * Da * 4, hipMemcpyHostToDevice, t->stream));
        HIPCHK(hipMemcpyAsync(a.rew + d, rew + s, n * 8, hipMemcpyHostToDevice, t->stream));
        if (cost) HIPCHK(hipMemcpyAsync(a.cost + d, cost + s, n * 8, hipMemcpyHostToDevice, t->stream));
        else HIPCHK(hipMemsetAsync(a.cost + d, 0, n * 8, t->stream));
        if (terminals) HIPCHK(hipMemcpyAsync(a.terminals + d, terminals + s, n, hipMemcpyHostToDevice, t->stream));
        else HIPCHK(hipMemsetAsync(a.terminals + d, 0, n, t->stream));
        if (timeouts) HIPCHK(hipMemcpyAsync(a.timeouts + d, timeouts + s, n, hipMemcpyHostToDevice, t->stream));
        else HIPCHK(hipMemsetAsync(a.timeouts + d, 0, n, t->stream));
    }
    runs.clear();
    HIPCHK(hipStreamSynchronize(t->stream));
    return 0;
}

extern "C" int fsrl_traj_import(fsrl_traj* t, int64_t rows, const float* obs, const float* next_obs, const float* act,
                                const double* rew, const double* cost, const uint8_t* terminals, const uint8_t* timeouts,
                                int32_t source, int64_t* episodes_out, int64_t* rows_out) {
    CHECK_ARG(t && rows >= 0, "bad argument");
    CHECK_ARG(rows == 0 || (obs && next_obs && act && rew), "null column (observations, next_observations, actions and rewards are required)");
    CHECK_ARG(terminals || timeouts || rows == 0, "terminals and timeouts are both null: no episode ever ends");
    HIPCHK(hipSetDevice(t->device));
    if (episodes_out) *episodes_out = 0;
    if (rows_out) *rows_out = 0;
    std::vector<trajp::ImportEpisode> eps;
    trajp::import_scan(t->book, rows, rew, cost, terminals, timeouts, eps);
    // the flag columns hold 0 / 1 in the archive whatever non-zero value the caller's have
    std::vector<uint8_t> term01, time01;
    if (terminals) { term01.resize((size_t)rows); for (int64_t i = 0; i < rows; ++i) term01[(size_t)i] = terminals[i] ? 1 : 0; }
    if (timeouts) { time01.resize((size_t)rows); for (int64_t i = 0; i < rows; ++i) time01[(size_t)i] = timeouts[i] ? 1 : 0; }
    const uint8_t* tm = terminals ? term01.data() : nullptr;
    const uint8_t* to = timeouts ? time01.data() : nullptr;
    std::vector<trajp::ImportRun> runs;
    int64_t n_eps = 0, n_rows = 0;
    int rc = 0, refused = 0;
    std::string why;
    for (const trajp::ImportEpisode& e : eps) {
        int r = trajp::import_commit(t->book, e, source, runs);
        if (r == 1) {       // rows accepted so far must be in the archive before a compaction copies them
            rc = import_send(t, runs, obs, next_obs, act, rew, cost, tm, to);
            if (!rc) rc = traj_compact(t);
            if (rc) return rc;
            r = trajp::import_commit(t->book, e, source, runs);
        }
        if (r == 0) { n_eps += 1; n_rows += e.rows; }
        else if (r == -1 || r == 1) { if (!refused++) why = t->book.err; }
    }
    rc = import_send(t, runs, obs, next_obs, act, rew, cost, tm, to);
    if (rc) return rc;
    if (episodes_out) *episodes_out = n_eps;
    if (rows_out) *rows_out = n_rows;
    if (refused) return fail(FSRL_ENOMEM, "%s", why.c_str());
    return 0;
}

extern "C" int fsrl_store_fill(fsrl_ctx* c, fsrl_traj* t, const int32_t* episode_ids, int64_t n, int32_t first_env,
                               int32_t bound_method, const float* act_low, const float* act_high, int64_t* rows_out) {
    CHECK_ARG(c && t, "null argument");
    CHECK_ARG(c->cfg.obs_dim == t->Do, "obs_dim: the context has %d, the trajectory archive %d", c->cfg.obs_dim, t->Do);
    CHECK_ARG(c->cfg.act_dim == t->Da, "act_dim: the context has %d, the trajectory archive %d", c->cfg.act_dim, t->Da);
    CHECK_ARG(c->device == t->device, "device: the context is on %d, the trajectory archive on %d", c->device, t->device);
    CHECK_ARG(bound_method >= 0 && bound_method <= 2, "bound_method %d: 0 none, 1 clip, 2 tanh", bound_method);
    CHECK_ARG((act_low == nullptr) == (act_high == nullptr), "act_low and act_high are given together");
    if (c->in_update || c->verdict_pending)
        return fail(FSRL_ESTATE, "update: fsrl_store_fill inside an update (between fsrl_ppo_begin and fsrl_ppo_end)");
    if (rows_out) *rows_out = 0;
    ENTER_DEV(c);
    // the archive's rows are final: every feeding context's window is flushed and its side stream has finished (this context's
    // own window among them when it feeds `t`; an archive without room reports it here, before anything is written)
    int rc = fsrl_traj_flush(t);
    if (rc) return rc;
    fillp::Plan p;
    std::vector<fillp::SubBook> books((size_t)c->active_envs);
    for (int e = 0; e < c->active_envs; ++e) {
        const EnvBook& b = c->env[(size_t)e];
        fillp::SubBook& s = books[(size_t)e];
        s.index = b.index; s.size = b.size; s.last_index = b.last_index; s.ep_rew = b.ep_rew; s.ep_len = b.ep_len; s.ep_idx = b.ep_idx;
    }
    if (!fillp::plan(t->book.table, episode_ids, n, first_env, c->sub_size, c->active_envs, books, p))
        return fail(p.code == fillp::REFUSE_STATE ? FSRL_ESTATE : FSRL_EINVAL, "%s", p.err.c_str());
    if (rows_out) *rows_out = p.rows;
    if (p.rows == 0) return 0;      // the loop of no pushes
    // what the kernel relies on, once more, against the allocations themselves
    for (const trajp::Job& j : p.jobs)
        if (j.rows < 1 || j.src < 0 || j.src + j.rows > t->book.max_rows || j.dst < 0 || j.dst + j.rows > c->maxsize ||
            c->maxsize > c->alloc_rows)
            return fail(FSRL_ESTATE, "fsrl_store_fill: a job leaves its buffers (src %lld, dst %lld, rows %d)", (long long)j.src,
                        (long long)j.dst, j.rows);
    rc = flush_stage(c);            // rows already in the staging window land first
    if (rc) return rc;
    rc = traj_fill_wait(t);         // the last fill may still read the table
    if (rc) return rc;
    const size_t nj = p.jobs.size(), Da = (size_t)t->Da;
    const size_t map_off = nj * sizeof(TrajJob), bytes = map_off + (act_low ? 2 * Da * 4 : 0);
    rc = table_ensure(t->fill, bytes, bytes + bytes / 2 + 4096);
    if (rc) return rc;
    memcpy(t->fill.h, p.jobs.data(), map_off);
    if (act_low) {
        float* m = reinterpret_cast<float*>(t->fill.h + map_off);
        const float eps = 1.1920928955078125e-07f;      // np.finfo(np.float32).eps
        for (size_t d = 0; d < Da; ++d) {
            float scale = act_high[d] - act_low[d];
            if (scale < eps) scale += eps;              // scale[scale < eps] += eps (base_policy.py:279)
            m[d] = act_low[d]; m[Da + d] = scale;
        }
    }
    HIPCHK(hipMemcpyAsync(t->fill.d, t->fill.h, bytes, hipMemcpyHostToDevice, c->side));
    hipLaunchKernelGGL(store_fill_kernel, dim3((unsigned)std::min<size_t>(nj, 4096)), dim3(256), 0, c->side, t->half[t->book.cur],
                       c->st, reinterpret_cast<const TrajJob*>(t->fill.d), (int)nj, t->Do, t->Da, (int)bound_method,
                       act_low ? reinterpret_cast<const float*>(t->fill.d + map_off) : nullptr);
    HIPCHK(hipGetLastError());
    if (c->per) {                   // the poured rows' leaves (the pushes of the model: max_prio ** alpha each), read from the same job table
        rc = per_fill(c, reinterpret_cast<const TrajJob*>(t->fill.d), (int)nj);
        if (rc) return rc;
    }
    HIPCHK(hipEventRecord(t->fill_done, c->side));
    t->fill_pending = true;
    t->fill_launches += 1; t->fill_copies += 1;
    // the host's side of the pushes: the flag mirror, the books, and a store that has changed
    fillp::apply_flags(p, c->h_flags.data());
    for (int e = 0; e < c->active_envs; ++e) {
        EnvBook& b = c->env[(size_t)e];
        const fillp::SubBook& s = p.books[(size_t)e];
        b.index = s.index; b.size = s.size; b.last_index = s.last_index; b.ep_rew = s.ep_rew; b.ep_len = s.ep_len; b.ep_idx = s.ep_idx;
    }
    c->store_version += 1;
    return 0;
}
