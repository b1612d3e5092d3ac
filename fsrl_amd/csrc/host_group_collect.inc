// host_group_collect.inc -- lock-step collection of a group: fsrl_collect_step on every member in ONE call with ONE actor request for
// all of them (part of fsrl_hip.hip, after host_group.inc).  The request goes to actor_group_resident_kernel (kernels_mlp.hpp): the
// resident actor of DESIGN 3.4 with a workgroup per (member, 16-row tile), on the group's stream.  Protocol as pactor_* (post / ring /
// wait / release, generation and sequence numbers), with one doorbell for the group and a per-member row count k_m next to it.
// The kernel is told to end (EXIT) before anything else is enqueued on the group's stream: fsrl_group_ppo_update, fsrl_group_destroy,
// group_detach and every member entry point that goes through pactor_release (ENTER_DEV, a member's own actor calls).

// pinned ring: [bell 8 B | pad | k_m[16] at 64 | done[64] at 128 | state[64] at 384 | pad | obs [64 * 16][Do] at 1024 |
//               mu [64 * 16][Da] | sigma_param [16][FSRL_MAX_ACT]]
struct GaLayout { unsigned long long* bell; unsigned* k_m; unsigned* done; unsigned* state; float* obs; float* mu; float* sp; };
static constexpr int GA_ROWS = GACTOR_MAX_WG * 16;
static GaLayout ga_layout(const fsrl_group* g) {
    char* b = (char*)g->h_ga;
    GaLayout l;
    l.bell = (unsigned long long*)b; l.k_m = (unsigned*)(b + 64); l.done = (unsigned*)(b + 128); l.state = (unsigned*)(b + 384);
    l.obs = (float*)(b + 1024);
    l.mu = l.obs + (size_t)GA_ROWS * g->ga_do;
    l.sp = l.mu + (size_t)GA_ROWS * g->ga_da;
    return l;
}
static size_t ga_bytes(const fsrl_config& cfg) {
    return 1024 + ((size_t)GA_ROWS * (cfg.obs_dim + cfg.act_dim) + (size_t)GACTOR_MAX_MEMBERS * FSRL_MAX_ACT) * 4;
}

static void group_actor_release(fsrl_group* g) {
    if (!g->ga_live) return;
    g->ga_seq += 1;
    __atomic_store_n(ga_layout(g).bell, ((unsigned long long)PACTOR_EXIT << 32) | g->ga_seq, __ATOMIC_RELEASE);
    g->ga_live = false;
}

// how many workgroups of generation ga_gen have ended
static int gactor_ended_count(const fsrl_group* g) {
    const GaLayout l = ga_layout(g);
    int n = 0;
    for (int b = 0; b < g->ga_blocks; ++b) n += __atomic_load_n(l.state + b, __ATOMIC_ACQUIRE) == g->ga_gen;
    return n;
}

static double ga_now_us() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec * 1e6 + (double)ts.tv_nsec * 1e-3;
}

// Bounded wait: `ready()` polled; every 2 ms without it the group's stream is asked.  A HIP error there -> FSRL_EHIP; an idle stream
// (every workgroup has ended, nothing else queued) -> 1; 20 s -> FSRL_EHIP.  0 once `ready()` holds.
template <typename F>
static int ga_poll(fsrl_group* g, F&& ready, const char* what) {
    const double t0 = ga_now_us();
    double next_query = t0 + 2000.0;
    for (long spins = 0;; ++spins) {
        if (ready()) return 0;
        if ((spins & 255) == 255) {
            const double t = ga_now_us();
            if (t >= next_query) {
                next_query = t + 2000.0;
                const hipError_t e = hipStreamQuery(g->stream);
                if (e == hipSuccess) return ready() ? 0 : 1;
                if (e != hipErrorNotReady) return fail(FSRL_EHIP, "%s: %s", what, hipGetErrorString(e));
            }
            if (t - t0 > 20.0e6) return fail(FSRL_EHIP, "%s: no answer for 20 s", what);
        }
        __builtin_ia32_pause();
    }
}

// generation ga_gen has ended (at once if none was launched); it was told to end, so this waits for a kernel on its way out
static int gactor_wait_ended(fsrl_group* g) {
    if (g->ga_gen == 0) return 0;
    const int rc = ga_poll(g, [&]() { return gactor_ended_count(g) == g->ga_blocks; }, "the group's resident actor did not end");
    return rc == 1 ? 0 : rc;                    // an idle stream: the kernel is gone
}

static int gactor_launch(fsrl_group* g, unsigned last_seq) {
    const fsrl_ctx* c0 = g->m[0];
    const GaLayout l = ga_layout(g);
    GActorArgs a{};
    for (size_t i = 0; i < g->m.size(); ++i) {
        a.P[i] = g->m[i]->P;
        for (int t = 0; t < g->ga_tiles[i]; ++t) {
            a.wg_member[g->ga_base[i] + t] = (unsigned char)i;
            a.wg_tile[g->ga_base[i] + t] = (unsigned char)t;
        }
    }
    a.obs = l.obs; a.mu_out = l.mu; a.sigma_param_out = l.sp; a.bell = l.bell; a.k_m = l.k_m; a.done = l.done; a.state = l.state;
    g->ga_gen += 1;
    if (g->ga_gen == 0) g->ga_gen = 1;
    a.gen = g->ga_gen; a.last_seq = last_seq; a.max_action = c0->cfg.max_action;
    a.timeout_ticks = (unsigned long long)(g->ga_idle_us * 100.0);            // wall_clock64: 100 MHz
    const ModelDesc md = c0->md;
    const int rc = dispatch_H(c0->cfg.hidden, [&](auto hc) {
        constexpr int H = decltype(hc)::value;
        hipLaunchKernelGGL((actor_group_resident_kernel<H>), dim3(g->ga_blocks), dim3(4 * H), 0, g->stream, md, a);
        HIPCHK(hipGetLastError());
        return 0;
    });
    if (rc) return rc;
    g->ga_live = true; g->ga_launches += 1;
    return 0;
}

// ring the doorbell for the request already in place (launching a kernel first if none can hear it)
static int gactor_ring(fsrl_group* g) {
    const GaLayout l = ga_layout(g);
    if (g->ga_live && gactor_ended_count(g) > 0) group_actor_release(g);      // (some of) it ended by its idle timeout: the rest follows
    g->ga_seq += 1;
    if (!g->ga_live) {
        int rc = gactor_wait_ended(g);
        if (rc) return rc;
        rc = gactor_launch(g, g->ga_seq - 1);
        if (rc) return rc;
    }
    __atomic_store_n(l.bell, ((unsigned long long)1 << 32) | g->ga_seq, __ATOMIC_RELEASE);
    return 0;
}

// the ring and the workgroup layout: member m gets min(PACTOR_BLOCKS, ceil(env_num / 16)) tiles, as its own resident actor would
static int gactor_ensure(fsrl_group* g) {
    if (g->h_ga) return 0;
    const size_t bytes = ga_bytes(g->m[0]->cfg);
    HIPCHK(hipHostMalloc(&g->h_ga, bytes));
    memset(g->h_ga, 0, bytes);
    g->ga_do = g->m[0]->cfg.obs_dim; g->ga_da = g->m[0]->cfg.act_dim;
    int base = 0;
    for (size_t i = 0; i < g->m.size(); ++i) {
        g->ga_base[i] = base;
        g->ga_tiles[i] = std::min(PACTOR_BLOCKS, std::max(1, (g->m[i]->cfg.env_num + 15) / 16));
        base += g->ga_tiles[i];
    }
    g->ga_blocks = base;
    return 0;
}

// one request for every member: k_act[m] rows of obs_act (concatenated over members)
static int gactor_post(fsrl_group* g, const int32_t* k_act, const float* obs_act) {
    const int Do = g->m[0]->cfg.obs_dim;
    const GaLayout l = ga_layout(g);
    size_t off = 0;
    for (size_t i = 0; i < g->m.size(); ++i) {
        const int k = k_act[i];
        if (k > 0) memcpy(l.obs + (size_t)g->ga_base[i] * 16 * Do, obs_act + off * Do, (size_t)k * Do * 4);
        l.k_m[i] = (unsigned)k;
        g->ga_k[i] = k;
        off += (size_t)k;
    }
    const int rc = gactor_ring(g);
    if (rc) return rc;
    g->ga_requests += 1;
    return 0;
}

static int gactor_wait(fsrl_group* g) {
    const GaLayout l = ga_layout(g);
    auto served = [&]() {
        for (size_t i = 0; i < g->m.size(); ++i) {
            const int tiles = (g->ga_k[i] + 15) / 16;
            for (int t = 0; t < tiles; ++t)
                if (__atomic_load_n(l.done + g->ga_base[i] + t, __ATOMIC_ACQUIRE) != g->ga_seq) return false;
        }
        return true;
    };
    for (;;) {
        // a workgroup gone before it served the request (idle timeout just before the doorbell): end the rest, relaunch, ring again
        const int rc = ga_poll(g, [&]() { return served() || gactor_ended_count(g) > 0; }, "the group's resident actor");
        if (rc < 0 || rc > 1) return rc;
        if (served()) return 0;
        if (rc == 1) g->ga_live = false;        // the stream is idle: every workgroup has ended
        const int rr = gactor_ring(g);
        if (rr) return rr;
    }
}

extern "C" int fsrl_group_collect_step(fsrl_group* g, const int32_t* k, const int32_t* env_ids, const float* obs, const float* act,
                                       const double* rew, const double* cost, const uint8_t* terminated, const uint8_t* truncated,
                                       const float* obs_next, int64_t* ptr_out, double* ep_rew_out, int32_t* ep_len_out,
                                       int64_t* ep_idx_out, const int32_t* k_act, const float* obs_act, int32_t deterministic,
                                       int32_t bound_method, const float* act_low, const float* act_high, float* act_out,
                                       float* env_act_out) {
    CHECK_ARG(g && k && k_act, "null argument");
    if (g->broken) return fail(FSRL_ESTATE, "a member of this group has been destroyed");
    const int n = (int)g->m.size();
    fsrl_ctx* c0 = g->m[0];
    const int Do = c0->cfg.obs_dim, Da = c0->cfg.act_dim;
    int64_t rows = 0, rows_act = 0;
    bool resident = g->ga_on;
    for (int i = 0; i < n; ++i) {
        CHECK_ARG(k[i] >= 0 && k_act[i] >= 0, "negative row count (member %d)", i);
        rows += k[i]; rows_act += k_act[i];
        const fsrl_ctx* c = g->m[i];
        resident = resident && !c->no_spin && k_act[i] <= 16 * std::min(PACTOR_BLOCKS, std::max(1, (c->cfg.env_num + 15) / 16));
    }
    CHECK_ARG(rows_act == 0 || (obs_act && act_out), "obs_act / act_out missing");
    CHECK_ARG(rows == 0 || env_ids, "env_ids missing");
    CHECK_ARG(bound_method >= 0 && bound_method <= 2, "bound_method: 0 none, 1 clip, 2 tanh");
    CHECK_ARG((act_low == nullptr) == (act_high == nullptr), "act_low and act_high are given together");
    HIPCHK(hipSetDevice(c0->device));           // keeps the group's resident actor alive
    // 1. one request for every member (or, off the resident path, one launch per member on the group's stream)
    int rc = 0;
    if (rows_act > 0) {
        if (resident) {
            rc = gactor_ensure(g);
            if (!rc) rc = gactor_post(g, k_act, obs_act);
            if (rc) return rc;
        } else {
            group_actor_release(g);
            size_t off = 0;
            for (int i = 0; i < n; ++i) {
                if (k_act[i] > 0) {
                    rc = actor_eval_launch(g->m[i], obs_act + off * Do, k_act[i], true);
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
            rc = fsrl_store_push(g->m[i], env_ids + o, k[i], obs + o * Do, act + o * Da, rew + o, cost ? cost + o : nullptr,
                                 terminated + o, truncated + o, obs_next + o * Do, ptr_out ? ptr_out + o : nullptr,
                                 ep_rew_out ? ep_rew_out + o : nullptr, ep_len_out ? ep_len_out + o : nullptr,
                                 ep_idx_out ? ep_idx_out + o : nullptr);
            if (rc) {
                if (rows_act > 0) { if (resident) (void)gactor_wait(g); else (void)hipStreamSynchronize(g->stream); }
                return rc;
            }
        }
        off += (size_t)k[i];
    }
    if (rows_act == 0) return 0;
    // 3. wait; 4. per member in order: its noise from its own stream, then map_action
    if (resident) {
        rc = gactor_wait(g);
        if (rc) return rc;
    }
    const GaLayout l = resident ? ga_layout(g) : GaLayout{};
    off = 0;
    for (int i = 0; i < n; ++i) {
        const int ka = k_act[i];
        fsrl_ctx* c = g->m[i];
        if (ka > 0) {
            float* ao = act_out + off * Da;
            if (resident) {
                c->actor_k = ka;
                c->act_mu.resize((size_t)ka * Da); c->act_sg.resize((size_t)ka * Da);
                memcpy(c->act_mu.data(), l.mu + (size_t)g->ga_base[i] * 16 * Da, (size_t)ka * Da * 4);
                const float* sp = l.sp + (size_t)i * FSRL_MAX_ACT;
                for (int r = 0; r < ka; ++r)
                    for (int d = 0; d < Da; ++d) c->act_sg[(size_t)r * Da + d] = expf(sp[d]);
                actor_draw(c, deterministic, ao);
            } else {
                rc = actor_sample_finish(c, deterministic, ao);
                if (rc) return rc;
            }
            if (env_act_out)
                map_env_action(Da, ka, bound_method, act_low ? act_low + (size_t)i * Da : nullptr,
                               act_high ? act_high + (size_t)i * Da : nullptr, ao, env_act_out + off * Da);
        }
        off += (size_t)ka;
    }
    return 0;
}

extern "C" int fsrl_group_actor_set_resident(fsrl_group* g, int32_t on, double idle_timeout_us) {
    CHECK_ARG(g, "null group");
    CHECK_ARG(idle_timeout_us <= 1.0e6, "idle_timeout_us above one second");
    group_actor_release(g);
    g->ga_on = on != 0;
    if (idle_timeout_us > 0.0) g->ga_idle_us = idle_timeout_us;
    return 0;
}

// out3 = {kernel launches, requests served through the doorbell, 1 if the group's resident kernel is live now}
extern "C" int fsrl_group_actor_resident_stats(fsrl_group* g, int64_t* out3) {
    CHECK_ARG(g && out3, "null argument");
    out3[0] = g->ga_launches; out3[1] = g->ga_requests; out3[2] = g->ga_live ? 1 : 0;
    return 0;
}

extern "C" int fsrl_group_actor_release(fsrl_group* g) {
    CHECK_ARG(g, "null group");
    group_actor_release(g);
    return 0;
}
