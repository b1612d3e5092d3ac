// host_actor_ring.inc -- the pinned ring of a resident actor kernel that serves SEVERAL contexts from one launch and one doorbell
// (part of fsrl_hip.hip, before host_group.inc).  Two owners embed a GaRing: fsrl_group (host_group_collect.inc: on-policy members,
// actor_group_resident_kernel<H, false>) and fsrl_collect_group (host_collect_group.inc: replay members,
// actor_group_resident_kernel<H, true>; on-policy members that keep their own streams, <H, false>).  The owner supplies the stream the kernel runs on and the launch itself; the protocol --
// request / wait / release, generation and sequence numbers, the bounded wait -- is resident_ring.hpp's, the one a context's own
// kernel runs, with 1 in the command word and a per-member row count k_m next to the doorbell.  Here: the layout, the request's rows
// and the lock-step collect step both owners' entry points run (ga_collect_step).
static_assert(RR_MAX_MEMBERS == GACTOR_MAX_MEMBERS && RR_EXIT == PACTOR_EXIT, "resident_ring.hpp and kernels_mlp.hpp disagree");

// pinned ring: [bell 8 B | pad | k_m[16] at 64 | done[64] at 128 | state[64] at 384 | pad | obs [64 * 16][Do] at 1024 |
//               out [64 * 16][cols] | sigma_param [16][FSRL_MAX_ACT]]
// cols = floats per output row: act_dim for the on-policy head, raw_cols for the replay actors.  Workgroup b owns rows 16 b .. 16 b + 15
// of obs and out, so a member's rows start on a tile boundary.
struct GaLayout { unsigned long long* bell; unsigned* k_m; unsigned* done; unsigned* state; float* obs; float* mu; float* sp; };
static constexpr int GA_ROWS = GACTOR_MAX_WG * 16;

struct GaRing : ResidentRing {                  // ResidentRing::owner is the GaRing itself (ga_bind)
    int Do = 0, cols = 0;                       // observation width / floats per output row of the ring
    void* h = nullptr;                          // pinned ring (GaLayout)
    Mem mem;                                    // owns it, and a layered group's collect buffers (LayGroup::ch / cd: that struct is reset by assignment)
    hipStream_t stream = nullptr;               // the stream the kernel is launched on (the group's)
    void* group = nullptr;                      // the fsrl_group / fsrl_collect_group, for its launch hook
};

static GaLayout ga_layout(const GaRing& r) {
    char* b = (char*)r.h;
    GaLayout l;
    l.bell = (unsigned long long*)b; l.k_m = (unsigned*)(b + 64); l.done = (unsigned*)(b + 128); l.state = (unsigned*)(b + 384);
    l.obs = (float*)(b + 1024);
    l.mu = l.obs + (size_t)GA_ROWS * r.Do;
    l.sp = l.mu + (size_t)GA_ROWS * r.cols;
    return l;
}
static size_t ga_bytes(int Do, int cols) {
    return 1024 + ((size_t)GA_ROWS * (Do + cols) + (size_t)GACTOR_MAX_MEMBERS * FSRL_MAX_ACT) * 4;
}

// the group's stream, its launch hook (none: a group of layered contexts, which only waits through the ring) and the stream query
static void ga_bind(GaRing& r, hipStream_t stream, int (*launch)(void*, ResidentRing&, unsigned), void* group) {
    r.stream = stream; r.launch = launch; r.group = group; r.owner = &r;
    r.query = [](void* ring) { return stream_state(((GaRing*)ring)->stream); };
}

// the ring and the workgroup layout: member m gets min(PACTOR_BLOCKS, ceil(env_num / 16)) tiles, as its own resident actor would
static int gactor_ensure(GaRing& r, fsrl_ctx* const* m, int n, int cols) {
    if (r.h) return 0;
    const size_t bytes = ga_bytes(m[0]->cfg.obs_dim, cols);
    HIPCHK(r.mem.pinned(&r.h, bytes));
    memset(r.h, 0, bytes);
    r.n = n; r.Do = m[0]->cfg.obs_dim; r.cols = cols;
    int base = 0;
    for (int i = 0; i < n; ++i) {
        r.base[i] = base;
        r.tiles[i] = std::min(PACTOR_BLOCKS, std::max(1, (m[i]->cfg.env_num + 15) / 16));
        base += r.tiles[i];
    }
    r.blocks = base;
    const GaLayout l = ga_layout(r);
    r.bell = l.bell; r.done = l.done; r.state = l.state;
    return 0;
}

// the common part of a launch's arguments: the ring's areas, the workgroup -> (member, tile) table, generation and timeout
static void gactor_fill_args(const GaRing& r, GActorArgs& a, unsigned last_seq) {
    const GaLayout l = ga_layout(r);
    for (int i = 0; i < r.n; ++i)
        for (int t = 0; t < r.tiles[i]; ++t) {
            a.wg_member[r.base[i] + t] = (unsigned char)i;
            a.wg_tile[r.base[i] + t] = (unsigned char)t;
        }
    a.obs = l.obs; a.mu_out = l.mu; a.sigma_param_out = l.sp; a.bell = l.bell; a.k_m = l.k_m; a.done = l.done; a.state = l.state;
    a.gen = r.gen; a.last_seq = last_seq;
    a.timeout_ticks = (unsigned long long)(r.idle_us * 100.0);               // wall_clock64: 100 MHz
}

// one request for every member: k_act[m] rows of obs_act (concatenated over members)
static int gactor_post(GaRing& r, const int32_t* k_act, const float* obs_act) {
    const int Do = r.Do;
    const GaLayout l = ga_layout(r);
    size_t off = 0;
    for (int i = 0; i < r.n; ++i) {
        const int k = k_act[i];
        if (k > 0) memcpy(l.obs + (size_t)r.base[i] * 16 * Do, obs_act + off * Do, (size_t)k * Do * 4);
        l.k_m[i] = (unsigned)k;
        r.k[i] = k;
        off += (size_t)k;
    }
    return rr_code(rr_request(r, 1u), "the group's resident actor");
}
static int gactor_wait(GaRing& r) { return rr_code(rr_wait(r), "the group's resident actor"); }

// a member's row cap on the resident path: what its own resident actor serves
static inline int gactor_member_rows(const fsrl_ctx* c) {
    return 16 * std::min(PACTOR_BLOCKS, std::max(1, (c->cfg.env_num + 15) / 16));
}

// ---- one lock-step collect step: fsrl_collect_step on every member, in member order, with one request to the ring's kernel.  Row
//      arrays are concatenated over members; k[m] / k_act[m] may be 0; act_low / act_high: NULL or [members][act_dim].
struct GaStepArgs {
    const int32_t* k; const int32_t* env_ids; const float* obs; const float* act; const double* rew; const double* cost;
    const uint8_t* terminated; const uint8_t* truncated; const float* obs_next; int64_t* ptr_out; double* ep_rew_out;
    int32_t* ep_len_out; int64_t* ep_idx_out; const int32_t* k_act; const float* obs_act; int32_t deterministic; int32_t bound_method;
    const float* act_low; const float* act_high; float* act_out; float* env_act_out;
};
// The owners differ in three callables: ensure() makes the ring before a request (0 or an error); finish(i, c, ka, l) turns member
// i's ka ring rows into c->act_mu / c->act_sg (sized [ka][act_dim] already); drain() leaves no evaluation in flight when a push
// fails off the resident path.
// ga_collect_step_via is the step itself with the shared request as three more callables, so that an owner without a resident
// kernel (a group of layered contexts, host_layered_group.inc: one launch sequence per step for all members) runs the same
// step: fits(i) -- member i's rows can go through the shared request; post() -- place and start it (0 or an error); wait() --
// its answer is in host memory (0 or an error); abandon() -- a push failed behind a posted request: leave nothing in flight.
template <class Fits, class Post, class Wait, class Abandon, class Finish, class Drain>
static int ga_collect_step_via(GaRing& ga, fsrl_ctx* const* m, int n, int device, const GaStepArgs& a, Fits&& fits, Post&& post,
                               Wait&& wait, Abandon&& abandon, Finish&& finish, Drain&& drain) {
    const int32_t *k = a.k, *k_act = a.k_act;
    const int Do = m[0]->cfg.obs_dim, Da = m[0]->cfg.act_dim;
    int64_t rows = 0, rows_act = 0;
    bool resident = ga.on;
    for (int i = 0; i < n; ++i) {
        CHECK_ARG(k[i] >= 0 && k_act[i] >= 0, "negative row count (member %d)", i);
        rows += k[i]; rows_act += k_act[i];
        resident = resident && !m[i]->no_spin && fits(i);
    }
    CHECK_ARG(rows_act == 0 || (a.obs_act && a.act_out), "obs_act / act_out missing");
    CHECK_ARG(rows == 0 || a.env_ids, "env_ids missing");
    CHECK_ARG(a.bound_method >= 0 && a.bound_method <= 2, "bound_method: 0 none, 1 clip, 2 tanh");
    CHECK_ARG((a.act_low == nullptr) == (a.act_high == nullptr), "act_low and act_high are given together");
    HIPCHK(hipSetDevice(device));               // keeps the group's resident actor alive
    // 1. one request for every member (or, off the resident path, every member's own actor call)
    int rc = 0;
    if (rows_act > 0) {
        if (resident) {
            rc = post();
            if (rc) return rc;
        } else {
            rr_release(ga);
            size_t off = 0;
            for (int i = 0; i < n; ++i) {
                if (k_act[i] > 0) {
                    rc = actor_eval_launch(m[i], a.obs_act + off * Do, k_act[i], true);
                    if (rc) return rc;
                }
                off += (size_t)k_act[i];
            }
        }
    }
    // 2. every member's finished transitions into its own store (flushes on the member's side stream)
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
        if (k[i] > 0) {
            const size_t o = off;
            rc = fsrl_store_push(m[i], a.env_ids + o, k[i], a.obs + o * Do, a.act + o * Da, a.rew + o, a.cost ? a.cost + o : nullptr,
                                 a.terminated + o, a.truncated + o, a.obs_next + o * Do, a.ptr_out ? a.ptr_out + o : nullptr,
                                 a.ep_rew_out ? a.ep_rew_out + o : nullptr, a.ep_len_out ? a.ep_len_out + o : nullptr,
                                 a.ep_idx_out ? a.ep_idx_out + o : nullptr);
            if (rc) {                           // leave no evaluation in flight behind the error
                if (rows_act > 0) { if (resident) abandon(); else drain(); }
                return rc;
            }
        }
        off += (size_t)k[i];
    }
    if (rows_act == 0) return 0;
    // 3. wait; 4. per member in order: mean / std from its ring rows, its noise from its own stream, then map_action
    if (resident) {
        rc = wait();
        if (rc) return rc;
    }
    const GaLayout l = (resident && ga.h) ? ga_layout(ga) : GaLayout{};
    off = 0;
    for (int i = 0; i < n; ++i) {
        const int ka = k_act[i];
        fsrl_ctx* c = m[i];
        if (ka > 0) {
            float* ao = a.act_out + off * Da;
            if (resident) {
                c->actor_k = ka;
                c->act_mu.resize((size_t)ka * Da); c->act_sg.resize((size_t)ka * Da);
                finish(i, c, ka, l);
                actor_draw(c, a.deterministic, ao);
            } else {
                rc = actor_sample_finish(c, a.deterministic, ao);
                if (rc) return rc;
            }
            if (a.env_act_out)
                map_env_action(Da, ka, a.bound_method, a.act_low ? a.act_low + (size_t)i * Da : nullptr,
                               a.act_high ? a.act_high + (size_t)i * Da : nullptr, ao, a.env_act_out + off * Da);
        }
        off += (size_t)ka;
    }
    return 0;
}
template <class Ensure, class Finish, class Drain>
static int ga_collect_step(GaRing& ga, fsrl_ctx* const* m, int n, int device, const GaStepArgs& a, Ensure&& ensure, Finish&& finish,
                           Drain&& drain) {
    return ga_collect_step_via(
        ga, m, n, device, a, [&](int i) { return a.k_act[i] <= gactor_member_rows(m[i]); },
        [&]() { const int rc = ensure(); return rc ? rc : gactor_post(ga, a.k_act, a.obs_act); }, [&]() { return gactor_wait(ga); },
        [&]() { (void)gactor_wait(ga); }, finish, drain);
}
