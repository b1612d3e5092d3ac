// host_per.inc -- prioritised experience replay for SAC-Lag / DDPG-Lag contexts: fsrl_per_* (part of fsrl_hip.hip, included by
// host_sac.inc behind SacState; a group of prioritised members: host_sac_group.inc).  The sum tree lives in HBM next to the store (kernels_per.hpp); nothing of a sample, a weight or a
// TD error crosses the bus inside an update.
//   who writes the tree          on which stream
//   rows reaching the store      side    (flush_stage, fsrl_store_fill: per_ingest / per_fill behind the row copies)
//   fsrl_store_reset / configure side    (per_store_reset)
//   an update's new priorities   compute (per_update_launch behind the critics' Q_TRAIN launch), fsrl_per_update_weight
//   a grouped call's priorities  the group's stream, which the member's compute and side streams wait for (rgroup_end)
// The side stream's writers wait for upd_done first -- the last update's priorities are in and max_prio is the value after it --
// and the compute stream picks the side stream's work up through join_store, as it does the rows themselves.
#include "kernels_per.hpp"

struct PerState {
    Mem mem;
    double alpha = 0.6, beta = 0.4;
    int weight_norm = 1;
    int bound = 1, slots = 0;
    int64_t cap_nodes = 0;                      // doubles in `tree`: 2 * the bound of the rows allocated at fsrl_ctx_create
    double* tree = nullptr; double* sc = nullptr; int* stamp = nullptr;
    float* w = nullptr; double* wd = nullptr; float* td = nullptr; int cap_B = 0;      // the batch's weights and TD averages
    int* u_idx = nullptr; double* u_w = nullptr; int64_t cap_u = 0;                    // fsrl_per_update_weight's operands
    hipEvent_t upd_done = nullptr; bool upd_recorded = false;
};

static int per_pow2_at_least(int64_t n) { int b = 1; while (b < n) b *= 2; return b; }
static PerDev per_dev(const PerState* p) {
    PerDev d{};
    d.tree = p->tree; d.sc = p->sc; d.stamp = p->stamp; d.bound = p->bound; d.slots = p->slots; d.alpha = p->alpha;
    return d;
}
static void per_free(fsrl_ctx* c) {
    PerState* p = c->per;
    if (!p) return;
    p->mem.release_all();
    if (p->upd_done) (void)hipEventDestroy(p->upd_done);
    delete p;
    c->per = nullptr;
}
// the side stream's next tree write goes behind the last update's priorities
static int per_side_enter(fsrl_ctx* c) {
    if (c->per->upd_recorded) HIPCHK(hipStreamWaitEvent(c->side, c->per->upd_done, 0));
    return 0;
}
static int per_mark_update(fsrl_ctx* c) {
    HIPCHK(hipEventRecord(c->per->upd_done, c->compute));
    c->per->upd_recorded = true;
    return 0;
}

// flush_stage: the window's k records are on the device (recs_d) and store_scatter_kernel is enqueued on the side stream
static int per_ingest(fsrl_ctx* c, const uint8_t* recs_d, int rec, int k) {
    int rc = per_side_enter(c);
    if (rc) return rc;
    hipLaunchKernelGGL(per_ingest_kernel, dim3(1), dim3(PER_THREADS), 0, c->side, per_dev(c->per), recs_d, rec, k);
    HIPCHK(hipGetLastError());
    return 0;
}
// A device collect: collect_device_group_kernel has written the member's rows' slots (slots_d) and their number (n_rows_d) itself, and
// the member's COMPUTE stream is behind that launch (host_devcollect_group.inc).  Ordering: the compute stream is behind the last update's priorities by stream order (max_prio is the value
// after it, as per_side_enter gives the side stream's writers) and behind the side stream's tree writers through the collect's
// join_store; the side stream's NEXT writer waits for upd_done, which is recorded again behind this launch.
static int per_devcollect(fsrl_ctx* c, const int32_t* slots_d, const int32_t* n_rows_d, int cap) {
    hipLaunchKernelGGL(per_slots_kernel, dim3(1), dim3(PER_THREADS), 0, c->compute, per_dev(c->per), slots_d, n_rows_d, cap);
    HIPCHK(hipGetLastError());
    return per_mark_update(c);
}
// fsrl_store_fill: the job table is on the device and store_fill_kernel is enqueued on the side stream
static int per_fill(fsrl_ctx* c, const TrajJob* jobs_d, int n_jobs) {
    int rc = per_side_enter(c);
    if (rc) return rc;
    const PerDev d = per_dev(c->per);
    hipLaunchKernelGGL(per_fill_kernel, dim3((unsigned)std::min(n_jobs, 1024)), dim3(256), 0, c->side, d, jobs_d, n_jobs);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(per_rebuild_kernel, dim3(1), dim3(PER_THREADS), 0, c->side, d);
    HIPCHK(hipGetLastError());
    return 0;
}
// fsrl_store_reset, fsrl_store_configure: the tree of the store's geometry as it is now, empty, both scalars back at 1
static int per_store_reset(fsrl_ctx* c) {
    PerState* p = c->per;
    int rc = per_side_enter(c);
    if (rc) return rc;
    p->slots = (int)c->maxsize;
    p->bound = per_pow2_at_least(c->maxsize);
    if (2 * (int64_t)p->bound > p->cap_nodes) return fail(FSRL_ESTATE, "prioritised replay: the store outgrew its sum tree");
    const PerDev d = per_dev(p);
    hipLaunchKernelGGL(per_reset_kernel, dim3((unsigned)std::min(1024, (2 * p->bound + 255) / 256)), dim3(256), 0, c->side, d);
    HIPCHK(hipGetLastError());
    return 0;
}

// leaves (one per slot of the store as it is cut now) and the two scalars from the host, the rest of the tree rebuilt; waits
static int per_load(fsrl_ctx* c, const double* leaves, double max_prio, double min_prio) {
    PerState* p = c->per;
    HIPCHK(hipStreamSynchronize(c->side));
    HIPCHK(hipStreamSynchronize(c->compute));
    p->slots = (int)c->maxsize;
    p->bound = per_pow2_at_least(c->maxsize);
    HIPCHK(hipMemset(p->tree, 0, (size_t)2 * p->bound * 8));
    HIPCHK(hipMemcpy(p->tree + p->bound, leaves, (size_t)p->slots * 8, hipMemcpyHostToDevice));
    const double sc[3] = {max_prio, min_prio, 0.0};
    HIPCHK(hipMemcpy(p->sc, sc, sizeof(sc), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(per_rebuild_kernel, dim3(1), dim3(PER_THREADS), 0, c->compute, per_dev(p));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->compute));
    return 0;
}

extern "C" int fsrl_per_enable(fsrl_ctx* c, double alpha, double beta, int32_t weight_norm) {
    CHECK_ARG(c, "null ctx");
    SacState* s = sac_of(c);
    if (!s) return fail(FSRL_ESTATE, "prioritised replay: fsrl_sac_init first (SAC-Lagrangian and DDPG-Lagrangian contexts)");
    CHECK_ARG(!s->cvpo, "prioritised replay is not built for CVPO contexts: its update has no per-row TD error to hand back");
    CHECK_ARG(!c->sac_group && !c->cvpo_group,
              "this context is already in a group of grouped updates, whose members all have prioritised replay on or all off: "
              "fsrl_per_enable before the group is made");
    CHECK_ARG(std::isfinite(alpha) && alpha >= 0.0 && std::isfinite(beta) && beta >= 0.0, "alpha and beta must be finite and >= 0");
    CHECK_ARG(!c->in_update, "fsrl_per_enable inside an update");
    ENTER_DEV(c);
    int rc = flush_stage(c);                    // staged rows land first: they are stored rows, and get a leaf below
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->side));
    HIPCHK(hipStreamSynchronize(c->compute));
    per_free(c);
    PerState* p = new PerState();
    c->per = p;
    p->alpha = alpha; p->beta = beta; p->weight_norm = weight_norm ? 1 : 0;
    p->cap_nodes = 2 * (int64_t)per_pow2_at_least(std::max<int64_t>(c->alloc_rows, c->maxsize));
    HIPCHK(p->mem.dev(&p->tree, (size_t)p->cap_nodes * 8));
    HIPCHK(p->mem.dev(&p->sc, 3 * 8));
    HIPCHK(p->mem.dev(&p->stamp, (size_t)(p->cap_nodes / 2) * 4));
    HIPCHK(hipMemset(p->stamp, 0xff, (size_t)(p->cap_nodes / 2) * 4));
    HIPCHK(hipEventCreateWithFlags(&p->upd_done, hipEventDisableTiming));
    // rows already stored: PrioritizedReplayBuffer.add's max_prio ** alpha with max_prio at its initial 1
    std::vector<double> leaves((size_t)c->maxsize, 0.0);
    for (int e = 0; e < c->active_envs; ++e)
        for (int64_t i = 0; i < c->env[(size_t)e].size; ++i) leaves[(size_t)(e * c->sub_size + i)] = 1.0;
    s->pre_valid = false;                       // a uniform sample drawn ahead is not this context's next one any more
    return per_load(c, leaves.data(), 1.0, 1.0);
}

extern "C" int fsrl_per_set_beta(fsrl_ctx* c, double beta) {
    CHECK_ARG(c, "null ctx");
    if (!c->per) return fail(FSRL_ESTATE, "fsrl_per_enable first");
    CHECK_ARG(std::isfinite(beta) && beta >= 0.0, "beta must be finite and >= 0");
    c->per->beta = beta;                        // a kernel argument of the next sample
    return 0;
}

static int per_alloc_batch(fsrl_ctx* c, int B) {
    PerState* p = c->per;
    if (B <= p->cap_B) return 0;
    HIPCHK(hipStreamSynchronize(c->compute));
    HIPCHK(p->mem.regrow(p->cap_B, B, B, {Mem::D(&p->w, (size_t)B * 4), Mem::D(&p->wd, (size_t)B * 8), Mem::D(&p->td, (size_t)B * 4)}));
    HIPCHK(hipMemsetAsync(p->td, 0, (size_t)B * 4, c->compute));
    return 0;
}
// the weights' side of a sample of B rows, and the priorities' side of the update behind it (the solo launches below; a
// prioritised group's member table, host_sac_group.inc)
static PerBatch per_batch_args(const PerState* p, int B) {
    PerBatch pb{};
    pb.w = p->w; pb.wd = p->wd; pb.B = B; pb.weight_norm = p->weight_norm; pb.beta = p->beta;
    return pb;
}
static PerUpd per_upd_args(const PerState* p, const SacState* s, int B) {
    PerUpd u{};
    u.idx = s->d_idx; u.q = s->QP; u.y = s->Y; u.ext = nullptr; u.td_out = p->td; u.B = B; u.n_q = s->n_q; u.pair_shift = s->n_q == 2 ? 0 : 1;
    return u;
}
// the update's sample (draw: library RNG; otherwise the caller's indices are already in s->d_idx) and its importance weights
static int per_sample_launch(fsrl_ctx* c, SacState* s, int B, bool draw, int64_t stored) {
    PerState* p = c->per;
    int rc = per_alloc_batch(c, B);
    if (rc) return rc;
    const SacSampleArgs sa = sac_sample_args(c, s, B, s->cfg.n_step, stored, s->n_updates);
    hipLaunchKernelGGL(per_sample_kernel, dim3(1), dim3(PER_THREADS), 0, c->compute, sa, per_dev(p), per_batch_args(p, B), draw ? 1 : 0);
    HIPCHK(hipGetLastError());
    return 0;
}
// behind the critics' Q_TRAIN launch: the sampled rows' new priorities from the TD errors that launch used
static int per_update_launch(fsrl_ctx* c, SacState* s, int B) {
    PerState* p = c->per;
    const PerUpd u = per_upd_args(p, s, B);
    hipLaunchKernelGGL(per_update_kernel, dim3(1), dim3(PER_THREADS), 0, c->compute, per_dev(p), u);
    HIPCHK(hipGetLastError());
    return per_mark_update(c);
}

extern "C" int fsrl_per_update_weight(fsrl_ctx* c, const int64_t* indices, const double* weights, int64_t n) {
    CHECK_ARG(c && indices && weights, "null argument");
    PerState* p = c->per;
    if (!p) return fail(FSRL_ESTATE, "fsrl_per_enable first");
    CHECK_ARG(n >= 0 && n <= INT32_MAX, "n out of range");
    if (n == 0) return 0;
    std::vector<int> idx((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        CHECK_ARG(indices[i] >= 0 && indices[i] < c->maxsize, "index %lld out of range", (long long)indices[i]);
        idx[(size_t)i] = (int)indices[i];
    }
    ENTER_DEV(c);
    int rc = join_store(c);
    if (rc) return rc;
    if (n > p->cap_u) {
        HIPCHK(hipStreamSynchronize(c->compute));
        HIPCHK(p->mem.regrow(p->cap_u, n, n, {Mem::D(&p->u_idx, (size_t)n * 4), Mem::D(&p->u_w, (size_t)n * 8)}));
    }
    HIPCHK(hipMemcpyAsync(p->u_idx, idx.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->compute));
    HIPCHK(hipMemcpyAsync(p->u_w, weights, (size_t)n * 8, hipMemcpyHostToDevice, c->compute));
    PerUpd u{};
    u.idx = p->u_idx; u.ext = p->u_w; u.B = (int)n; u.n_q = 0;
    hipLaunchKernelGGL(per_update_kernel, dim3(1), dim3(PER_THREADS), 0, c->compute, per_dev(p), u);
    HIPCHK(hipGetLastError());
    rc = per_mark_update(c);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->compute));   // idx and the caller's weights were the copies' sources
    return 0;
}

// every pending tree write of either stream is done
static int per_settle(fsrl_ctx* c) {
    ENTER_DEV(c);
    int rc = flush_stage(c);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->compute));   // an update's priorities first: the side stream's writers wait for them
    HIPCHK(hipStreamSynchronize(c->side));
    return 0;
}

extern "C" int fsrl_per_state(fsrl_ctx* c, double* leaves_out, int64_t n, double* max_prio, double* min_prio, double* total) {
    CHECK_ARG(c, "null ctx");
    PerState* p = c->per;
    if (!p) return fail(FSRL_ESTATE, "fsrl_per_enable first");
    CHECK_ARG(!leaves_out || n == p->slots, "the store has %d slots (buffer_num * sub_size), n is %lld", p->slots, (long long)n);
    int rc = per_settle(c);
    if (rc) return rc;
    if (leaves_out) HIPCHK(hipMemcpy(leaves_out, p->tree + p->bound, (size_t)p->slots * 8, hipMemcpyDeviceToHost));
    double sc[3];
    HIPCHK(hipMemcpy(sc, p->sc, sizeof(sc), hipMemcpyDeviceToHost));
    if (max_prio) *max_prio = sc[0];
    if (min_prio) *min_prio = sc[1];
    if (total) *total = sc[2];
    return 0;
}

static int per_last_check(fsrl_ctx* c, int32_t B) {
    if (!c->per) return fail(FSRL_ESTATE, "fsrl_per_enable first");
    SacState* s = sac_of(c);
    CHECK_ARG(s && B == s->last_B && B > 0 && B <= c->per->cap_B, "the last prioritised update used batch_size %d", s ? s->last_B : 0);
    return 0;
}
// The importance weights the last fsrl_sac_update's critic loss used (float32, after weight_norm).
extern "C" int fsrl_per_last_weights(fsrl_ctx* c, float* w_out, int32_t B) {
    CHECK_ARG(c && w_out, "null argument");
    int rc = per_last_check(c, B);
    if (rc) return rc;
    ENTER_DEV(c);
    HIPCHK(hipMemcpyAsync(w_out, c->per->w, (size_t)B * 4, hipMemcpyDeviceToHost, c->compute));
    HIPCHK(hipStreamSynchronize(c->compute));
    return 0;
}
// The per-row TD average the last fsrl_sac_update turned into priorities.
extern "C" int fsrl_per_last_td(fsrl_ctx* c, float* td_out, int32_t B) {
    CHECK_ARG(c && td_out, "null argument");
    int rc = per_last_check(c, B);
    if (rc) return rc;
    ENTER_DEV(c);
    HIPCHK(hipMemcpyAsync(td_out, c->per->td, (size_t)B * 4, hipMemcpyDeviceToHost, c->compute));
    HIPCHK(hipStreamSynchronize(c->compute));
    return 0;
}
// The n-step chains [n_step][B] and end bits of the last fsrl_sac_update's sample (either RNG mode, PER or not).
extern "C" int fsrl_sac_last_chain(fsrl_ctx* c, int64_t* chain_out, uint8_t* end_out, int32_t B) {
    CHECK_ARG(c && chain_out && end_out, "null argument");
    SacState* s = sac_of(c);
    if (!s) return fail(FSRL_ESTATE, "fsrl_sac_init first");
    CHECK_ARG(B == s->last_B && B > 0, "last update used batch_size %d", s->last_B);
    ENTER_DEV(c);
    const size_t n = (size_t)B * s->cfg.n_step;
    std::vector<int> ch(n);
    HIPCHK(hipMemcpyAsync(ch.data(), s->d_chain, n * 4, hipMemcpyDeviceToHost, c->compute));
    HIPCHK(hipMemcpyAsync(end_out, s->d_end, n, hipMemcpyDeviceToHost, c->compute));
    HIPCHK(hipStreamSynchronize(c->compute));
    for (size_t i = 0; i < n; ++i) chain_out[i] = ch[i];
    return 0;
}
