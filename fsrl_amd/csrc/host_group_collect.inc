// host_group_collect.inc -- lock-step collection of a group: fsrl_collect_step on every member in ONE call with ONE actor request for
// all of them (part of fsrl_hip.hip, after host_group.inc).  The request goes to actor_group_resident_kernel (kernels_mlp.hpp): the
// resident actor of DESIGN 3.4 with a workgroup per (member, 16-row tile), on the group's stream.  Protocol as pactor_* (post / ring /
// wait / release, generation and sequence numbers), with one doorbell for the group and a per-member row count k_m next to it.
// The kernel is told to end (EXIT) before anything else is enqueued on the group's stream: fsrl_group_ppo_update, fsrl_group_destroy,
// group_detach and every member entry point that goes through pactor_release (ENTER_DEV, a member's own actor calls).

// The ring and the protocol live in host_actor_ring.inc (GaRing), shared with the replay agents' collect group.

static void group_actor_release(fsrl_group* g) { ga_release(g->ga); }

// GaRing::launch of an on-policy group: the members' parameter vectors, the on-policy head
static int group_actor_launch(void* owner, GaRing& r, unsigned last_seq) {
    fsrl_group* g = (fsrl_group*)owner;
    const fsrl_ctx* c0 = g->m[0];
    GActorArgs a{};
    for (size_t i = 0; i < g->m.size(); ++i) a.P[i] = g->m[i]->P;
    gactor_fill_args(r, a, last_seq);
    a.max_action = c0->cfg.max_action;
    const ModelDesc md = c0->md;
    return dispatch_H(c0->cfg.hidden, [&](auto hc) {
        constexpr int H = decltype(hc)::value;
        hipLaunchKernelGGL((actor_group_resident_kernel<H>), dim3(r.blocks), dim3(4 * H), 0, r.stream, md, a);
        HIPCHK(hipGetLastError());
        return 0;
    });
}

static int group_actor_ensure(fsrl_group* g) {
    g->ga.stream = g->stream; g->ga.launch = group_actor_launch; g->ga.owner = g;
    return gactor_ensure(g->ga, g->m.data(), (int)g->m.size(), g->m[0]->cfg.act_dim);
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
    bool resident = g->ga.on;
    for (int i = 0; i < n; ++i) {
        CHECK_ARG(k[i] >= 0 && k_act[i] >= 0, "negative row count (member %d)", i);
        rows += k[i]; rows_act += k_act[i];
        const fsrl_ctx* c = g->m[i];
        resident = resident && !c->no_spin && k_act[i] <= gactor_member_rows(c);
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
            rc = group_actor_ensure(g);
            if (!rc) rc = gactor_post(g->ga, k_act, obs_act);
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
                if (rows_act > 0) { if (resident) (void)gactor_wait(g->ga); else (void)hipStreamSynchronize(g->stream); }
                return rc;
            }
        }
        off += (size_t)k[i];
    }
    if (rows_act == 0) return 0;
    // 3. wait; 4. per member in order: its noise from its own stream, then map_action
    if (resident) {
        rc = gactor_wait(g->ga);
        if (rc) return rc;
    }
    const GaLayout l = resident ? ga_layout(g->ga) : GaLayout{};
    off = 0;
    for (int i = 0; i < n; ++i) {
        const int ka = k_act[i];
        fsrl_ctx* c = g->m[i];
        if (ka > 0) {
            float* ao = act_out + off * Da;
            if (resident) {
                c->actor_k = ka;
                c->act_mu.resize((size_t)ka * Da); c->act_sg.resize((size_t)ka * Da);
                memcpy(c->act_mu.data(), l.mu + (size_t)g->ga.base[i] * 16 * Da, (size_t)ka * Da * 4);
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
    g->ga.on = on != 0;
    if (idle_timeout_us > 0.0) g->ga.idle_us = idle_timeout_us;
    return 0;
}

// out3 = {kernel launches, requests served through the doorbell, 1 if the group's resident kernel is live now}
extern "C" int fsrl_group_actor_resident_stats(fsrl_group* g, int64_t* out3) {
    CHECK_ARG(g && out3, "null argument");
    out3[0] = g->ga.launches; out3[1] = g->ga.requests; out3[2] = g->ga.live ? 1 : 0;
    return 0;
}

extern "C" int fsrl_group_actor_release(fsrl_group* g) {
    CHECK_ARG(g, "null group");
    group_actor_release(g);
    return 0;
}
