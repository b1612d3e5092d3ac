// host_group_collect.inc -- lock-step collection of a group: fsrl_collect_step on every member in ONE call with ONE actor request for
// all of them (part of fsrl_hip.hip, after host_group.inc).  The request goes to actor_group_resident_kernel (kernels_mlp.hpp): the
// resident actor of DESIGN 3.4 with a workgroup per (member, 16-row tile), on the group's stream.  Protocol: resident_ring.hpp
// (request / wait / release, generation and sequence numbers), with one doorbell for the group and a per-member row count k_m next to it.
// A group of LAYERED contexts has no resident kernel: its request is one launch sequence for all members (host_layered_group.inc);
// fsrl_group_actor_resident_stats then reports {shared launch sequences, requests served by them, 0}, fsrl_group_actor_release
// has nothing to end.
// The kernel is told to end (EXIT) before anything else is enqueued on the group's stream: fsrl_group_ppo_update, fsrl_group_destroy,
// group_detach and every member entry point that goes through pactor_release (ENTER_DEV, a member's own actor calls).

// The ring lives in host_actor_ring.inc (GaRing), shared with the replay agents' collect group.

static void group_actor_release(fsrl_group* g) { rr_release(g->ga); }

// GaRing::launch of an on-policy group: the members' parameter vectors, the on-policy head
static int group_actor_launch(void* ring, ResidentRing&, unsigned last_seq) {
    GaRing& r = *(GaRing*)ring;
    fsrl_group* g = (fsrl_group*)r.group;
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
    ga_bind(g->ga, g->stream, group_actor_launch, g);
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
    const GaStepArgs a{k, env_ids, obs, act, rew, cost, terminated, truncated, obs_next, ptr_out, ep_rew_out, ep_len_out, ep_idx_out,
                       k_act, obs_act, deterministic, bound_method, act_low, act_high, act_out, env_act_out};
    const int Da = g->m[0]->cfg.act_dim;
    if (g->m[0]->lay) {
        // a group of layered contexts: no resident kernel, ONE launch sequence per step for all members (host_layered_group.inc);
        // any row count per member goes through it.  fsrl_group_actor_set_resident(g, 0, ...) selects the member-by-member calls.
        const int n = (int)g->m.size(), Do = g->m[0]->cfg.obs_dim;
        ga_bind(g->ga, g->stream, nullptr, g);
        return ga_collect_step_via(
            g->ga, g->m.data(), n, g->m[0]->device, a, [](int) { return true; },
            [&]() { return lay_group_collect_post(g->lay, g->ga, g->m.data(), n, k_act, obs_act); },
            [&]() { return lay_group_collect_wait(g->lay, g->ga, n, Do, Da); },
            [&]() { (void)hipStreamSynchronize(g->stream); },       // a push failed behind the request: drain the stream
            [&](int i, fsrl_ctx* c, int ka, const GaLayout&) {
                const LayGroupPinned pin = lay_group_pinned(g->lay, Do, Da);
                memcpy(c->act_mu.data(), pin.mu + (size_t)i * g->lay.ccap * Da, (size_t)ka * Da * 4);
                const float* sp = pin.sp + (size_t)i * FSRL_MAX_ACT;
                for (int r = 0; r < ka; ++r)
                    for (int d = 0; d < Da; ++d) c->act_sg[(size_t)r * Da + d] = expf(sp[d]);
            },
            [&]() { (void)hipStreamSynchronize(g->stream); });
    }
    return ga_collect_step(
        g->ga, g->m.data(), (int)g->m.size(), g->m[0]->device, a, [&]() { return group_actor_ensure(g); },
        // the ring holds the means and each member's log-sigma parameter row
        [&](int i, fsrl_ctx* c, int ka, const GaLayout& l) {
            memcpy(c->act_mu.data(), l.mu + (size_t)g->ga.base[i] * 16 * Da, (size_t)ka * Da * 4);
            const float* sp = l.sp + (size_t)i * FSRL_MAX_ACT;
            for (int r = 0; r < ka; ++r)
                for (int d = 0; d < Da; ++d) c->act_sg[(size_t)r * Da + d] = expf(sp[d]);
        },
        [&]() { (void)hipStreamSynchronize(g->stream); });     // the members' launches went to the group's stream
}

extern "C" int fsrl_group_actor_set_resident(fsrl_group* g, int32_t on, double idle_timeout_us) {
    CHECK_ARG(g, "null group");
    return rr_code(rr_set_resident(g->ga, on, idle_timeout_us), "");
}

extern "C" int fsrl_group_actor_resident_stats(fsrl_group* g, int64_t* out3) {
    CHECK_ARG(g && out3, "null argument");
    rr_stats(g->ga, out3);
    return 0;
}

extern "C" int fsrl_group_actor_release(fsrl_group* g) {
    CHECK_ARG(g, "null group");
    group_actor_release(g);
    return 0;
}
