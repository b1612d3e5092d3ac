// host_collect_group.inc -- lock-step collection for seeds that keep their own streams: fsrl_collect_group_* (part of fsrl_hip.hip,
// after the SAC / CVPO code).  Two families of members, never mixed: replay contexts (below) and ON-POLICY contexts (CPO, TRPO-Lag,
// PPO-Lag or FOCOPS contexts outside an fsrl_group; "on-policy members" further down).
// Replay members: k SAC-Lag, DDPG-Lag or CVPO contexts of one network shape collect with ONE library call and ONE request per vector
// step to actor_group_resident_kernel<H, true> (kernels_mlp.hpp): a workgroup per (member, 16-row tile) running the member's ACTOR
// network (SacState::PA, mda) and writing the raw head rows [rows][raw_cols] to the pinned ring; the host then finishes each member
// as its own fsrl_collect_step would (sac_actor_finish, actor_draw from ITS xoshiro stream, map_env_action with its bounds).  The
// ring is host_actor_ring.inc's (GaRing), the protocol resident_ring.hpp's, shared with the on-policy group (host_group_collect.inc).
// The object is independent of the update groups: a member may at the same time be in an fsrl_sac_group / fsrl_cvpo_group, keeps its
// own streams, store and resident actor, and is not owned.
//
// Ordering.  The kernel runs on a stream of the collect group's own and holds every member's actor weights in registers / LDS from
// its prologue on, so:
//   * launch: a request must be answered with the parameters the member's own actor call would have used at that point of the host
//     program.  Before a generation is launched, an event is recorded on EACH member's compute stream and the group's stream waits
//     on it: the kernel's prologue reads the parameters behind everything the members have enqueued (grouped updates make the
//     members' streams wait on the update group's `done` event, so they are covered).  The members' own resident actors are told to
//     end first -- an event behind a live one would only complete at its idle timeout.
//   * release: the kernel is told to end (EXIT) before anything can change a member's actor.  pactor_release carries the hook
//     (c->cgroup), so every ENTER_DEV entry point does it -- a member's own updates, fsrl_sac_put_params, fsrl_sac_group_update and
//     fsrl_cvpo_group_update (ENTER_DEV for every active member) -- and so does a member's own actor call (actor_eval_launch).
//     fsrl_store_push keeps it alive (plain hipSetDevice), as it keeps the solo resident actor.
//   * after EXIT nothing is waited for.  Requests are synchronous, so none is in flight at release: every workgroup that had rows in
//     a request is past its prologue.  A workgroup that never had rows may still be in its prologue when a member's stream overwrites
//     the parameters; what it reads then it never uses -- the next doorbell it sees is EXIT.  The NEXT generation is only launched
//     once every workgroup of this one has stored its `state` word (rr_ring), behind the events above.
//   * fsrl_ctx_destroy of a member breaks the group (collect_group_detach: later steps fail with FSRL_ESTATE, destroy still works).
//   * the wait is resident_ring.hpp's (rr_poll): hipStreamQuery every 2 ms, a HIP error fails the call, an idle stream relaunches, 20 s fails.
// The step path allocates nothing: ring, stream and events are made at create.
//
// On-policy members.  Only the actor matters here, and the actor of every on-policy context is the Gaussian actor in c->P under
// c->md (sigma_param row included), the one actor_group_resident_kernel<H> serves for an fsrl_group: CPO and TRPO-Lag members may
// share a group.  Launch: group_actor_launch's arguments (a.P[i] = m[i]->P, member 0's md and max_action) with the ordering above;
// finish: fsrl_group_collect_step's (means and exp(sigma_param row) from the ring).  Layered members: lay_group_collect_post / _wait
// of host_layered_group.inc, with the `reorder` rule of the layered replay group.  Nothing is grouped on the update side: members run
// their own fsrl_tr_begin / fsrl_cpo_learn / fsrl_trpo_learn, and may do so on host threads of their own, all at once.  Every one of
// those calls runs the release hook below on THIS ring, so the hook takes the group's mutex (rr_release_guarded); a step of the
// group holds it from its request to the answer.  A member's entry point that runs while a step of its group is in progress
// remains a caller error (the step would answer with parameters in the middle of a change); the mutex only keeps the ring's words whole.
// ====================================================================================== the collect group
struct fsrl_collect_group {
    std::vector<fsrl_ctx*> m;                  // members (not owned; all nullptr once one was destroyed)
    int device = 0;
    hipStream_t stream = nullptr;              // the kernel's stream
    std::vector<hipEvent_t> ready;             // per member: its compute stream's work before a launch
    bool broken = false;
    int raw_cols = 0;
    GaRing ga;
    // a group of layered members (host_sac_group_layered.inc): no resident kernel, one launch sequence per request
    bool layered = false;
    bool reorder = true;                       // a release since the last request: the next one goes behind the members' streams first
    LayGroup lay;
    bool onpolicy = false;                     // on-policy members (c->P under c->md); else replay members (SacState::PA under mda)
    std::mutex mu;                             // the ring's host state and `reorder`: the release hook runs on any number of threads
};
static int lay_collect_group_step(fsrl_collect_group* g, const GaStepArgs& a);

// The hook of pactor_release / actor_eval_launch: something may change a member's actor, or runs it.  A fused group's kernel ends;
// a layered group has no kernel to end, so the hook marks it and its next request orders the group's stream behind the members'
// streams (a fused group never reads the mark).  Only this hook re-orders: the public fsrl_collect_group_actor_release changes
// nothing of a member and leaves the mark alone.
static void collect_group_actor_release(fsrl_collect_group* g) { rr_release_guarded(g->ga, g->mu, [g]() { g->reorder = true; }); }
// the other releases (destroy, detach, the public calls): the same lock, no mark
static void collect_group_end_kernel(fsrl_collect_group* g) { rr_release_guarded(g->ga, g->mu, []() {}); }

static void collect_group_detach(fsrl_ctx* c) {
    fsrl_collect_group* g = c->cgroup;
    if (!g) return;
    collect_group_end_kernel(g);
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    for (auto& x : g->m) if (x) { x->cgroup = nullptr; x = nullptr; }
    g->broken = true;
}

// GaRing::launch: order the group's stream behind every member's compute stream, then the RAW kernel over the members' actor networks
// (on-policy members: the on-policy head over the members' parameter vectors, as group_actor_launch)
static int collect_group_launch(void* ring, ResidentRing&, unsigned last_seq) {
    GaRing& r = *(GaRing*)ring;
    fsrl_collect_group* g = (fsrl_collect_group*)r.group;
    GActorArgs a{};
    const ModelDesc* md0 = nullptr;
    for (size_t i = 0; i < g->m.size(); ++i) {
        fsrl_ctx* c = g->m[i];
        const float* P = c->P; const ModelDesc* md = &c->md;
        if (!g->onpolicy && !sac_actor_resident_args(c, &P, &md)) return fail(FSRL_ESTATE, "member %d has no fused actor network", (int)i);
        a.P[i] = P;
        if (i == 0) md0 = md;
        rr_release(c->pa);                      // its own resident actor: the event below would wait for its idle timeout
        HIPCHK(hipEventRecord(g->ready[i], c->compute));
        HIPCHK(hipStreamWaitEvent(g->stream, g->ready[i], 0));
    }
    gactor_fill_args(r, a, last_seq);
    a.max_action = g->onpolicy ? g->m[0]->cfg.max_action : 1.0f; a.raw_cols = g->onpolicy ? 0 : g->raw_cols;
    const ModelDesc mdv = *md0;
    return dispatch_H(g->m[0]->cfg.hidden, [&](auto hc) {
        constexpr int H = decltype(hc)::value;
        if (g->onpolicy) hipLaunchKernelGGL((actor_group_resident_kernel<H>), dim3(r.blocks), dim3(4 * H), 0, r.stream, mdv, a);
        else hipLaunchKernelGGL((actor_group_resident_kernel<H, true>), dim3(r.blocks), dim3(4 * H), 0, r.stream, mdv, a);
        HIPCHK(hipGetLastError());
        return 0;
    });
}

extern "C" int fsrl_collect_group_destroy(fsrl_collect_group* g) {
    if (!g) return 0;
    (void)hipSetDevice(g->device);
    collect_group_end_kernel(g);
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    for (fsrl_ctx* c : g->m) if (c) c->cgroup = nullptr;
    for (hipEvent_t e : g->ready) if (e) (void)hipEventDestroy(e);
    lay_group_free(g->lay, g->ga.mem);
    if (g->stream) (void)hipStreamDestroy(g->stream);
    g->ga.mem.release_all();
    delete g;
    return 0;
}

static int collect_group_kind(const SacState* s) { return s->ddpg ? 1 : s->cvpo ? 2 : 0; }

// create's checks of member i against member 0, both on-policy contexts
static int collect_group_check_onpolicy(const fsrl_ctx* c, const fsrl_ctx* c0, int i) {
    CHECK_ARG(!c->group, "member %d is in an fsrl_group: it shares that group's stream and collects through fsrl_group_collect_step", i);
    CHECK_ARG((c->lay != nullptr) == (c0->lay != nullptr), "member %d is a %s context and member 0 a %s one: a collect group is all fused "
              "(the resident kernel) or all layered contexts", i, c->lay ? "layered" : "fused", c0->lay ? "layered" : "fused");
    CHECK_ARG(c->device == c0->device, "member %d: members live on one device", i);
    // one actor layout: the kernel reads every member's parameters through member 0's description of the actor network (the
    // fused layout keeps the W2 mirrors behind ALL networks, so the number of critics moves the actor's)
    CHECK_ARG(c->cfg.obs_dim == c0->cfg.obs_dim && c->cfg.act_dim == c0->cfg.act_dim && c->cfg.hidden == c0->cfg.hidden &&
              (!c->lay || lay_same_shape(c->cfg, c0->cfg)) && c->cfg.n_critics == c0->cfg.n_critics,
              "member %d: members must have one network shape (obs_dim, act_dim, hidden, n_critics; layered: every hidden_sizes[l] and "
              "force_layered)", i);
    CHECK_ARG(c->cfg.max_action == c0->cfg.max_action, "member %d: members must share max_action (%g, member 0's %g)", i,
              (double)c->cfg.max_action, (double)c0->cfg.max_action);
    CHECK_ARG((c->cfg.unbounded != 0) == (c0->cfg.unbounded != 0), "member %d: members must share unbounded (the actor's mean is %s, "
              "member 0's %s)", i, c->cfg.unbounded ? "the head itself" : "max_action * tanh(head)",
              c0->cfg.unbounded ? "the head itself" : "max_action * tanh(head)");
    return 0;
}

extern "C" int fsrl_collect_group_create(fsrl_ctx** ctxs, int32_t k, fsrl_collect_group** out) {
    CHECK_ARG(ctxs && out, "null argument");
    CHECK_ARG(k >= 1 && k <= GACTOR_MAX_MEMBERS, "a collect group has 1..%d members", GACTOR_MAX_MEMBERS);
    static const char* const kinds[] = {"SAC-Lagrangian", "DDPG-Lagrangian", "CVPO"};
    fsrl_ctx* c0 = ctxs[0];
    CHECK_ARG(c0, "null member");
    const bool onpolicy = !ctx_is_replay(c0);
    for (int i = 0; i < k; ++i) {
        fsrl_ctx* c = ctxs[i];
        CHECK_ARG(c, "null member");
        CHECK_ARG(ctx_is_replay(c) != onpolicy,
                  "member %d is %s context and member 0 %s one: a collect group is all replay contexts (SAC-Lag, DDPG-Lag, CVPO) or all "
                  "on-policy contexts (CPO, TRPO-Lag; PPO-Lag and FOCOPS seeds with grouped updates collect through fsrl_group_create / "
                  "fsrl_group_collect_step)", i, onpolicy ? "a replay" : "an on-policy", onpolicy ? "an on-policy" : "a replay");
        if (onpolicy) {
            const int rc = collect_group_check_onpolicy(c, c0, i);
            if (rc) return rc;
        } else {
            const SacState* s = sac_of(c);
            CHECK_ARG(s, "member %d is not initialised: fsrl_sac_init / fsrl_cvpo_init first", i);
            const SacState* s0 = sac_of(c0);
            CHECK_ARG(!s0 || s->layered == s0->layered, "member %d is a %s context and member 0 a %s one: a collect group is all fused (the "
                      "resident kernel) or all layered contexts", i, s->layered ? "layered" : "fused", s0->layered ? "layered" : "fused");
            CHECK_ARG(!s0 || collect_group_kind(s) == collect_group_kind(s0),
                      "member %d is a %s context, member 0 a %s one: a collect group has one kind of member", i, kinds[collect_group_kind(s)],
                      kinds[collect_group_kind(s0)]);
            CHECK_ARG(c->device == c0->device, "member %d: members live on one device", i);
            CHECK_ARG(!s0 || s->mean_tanh == s0->mean_tanh, "member %d: members must share actor_mean (the actor's mean is %s, member 0's %s)", i,
                      s->mean_tanh ? "max_action * tanh(head)" : "unbounded", s0->mean_tanh ? "max_action * tanh(head)" : "unbounded");
            CHECK_ARG(c->cfg.obs_dim == c0->cfg.obs_dim && c->cfg.act_dim == c0->cfg.act_dim && c->cfg.hidden == c0->cfg.hidden &&
                      (!s->layered || lay_same_shape(c->cfg, c0->cfg)),
                      "member %d: members must have one network shape (obs_dim, act_dim, hidden; layered: every hidden_sizes[l] and force_layered)", i);
        }
        for (int j = 0; j < i; ++j) CHECK_ARG(ctxs[j] != c, "member %d is listed twice", i);
        CHECK_ARG(!c->cgroup, "member %d is already in a collect group", i);
    }
    HIPCHK(hipSetDevice(c0->device));
    for (int i = 0; i < k; ++i) pactor_release(ctxs[i]);       // the allocations below would wait for a live resident actor's idle timeout
    fsrl_collect_group* g = new fsrl_collect_group();
    g->device = c0->device;
    g->onpolicy = onpolicy;
    g->raw_cols = onpolicy ? c0->cfg.act_dim : sac_raw_cols(c0);           // floats per answered row (on-policy: the means)
    g->layered = onpolicy ? c0->lay != nullptr : sac_of(c0)->layered;
    g->ready.assign((size_t)k, nullptr);
    for (int i = 0; i < k; ++i) g->m.push_back(ctxs[i]);
    hipError_t e = hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking);
    for (int i = 0; i < k && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&g->ready[(size_t)i], hipEventDisableTiming);
    if (e != hipSuccess) {
        fail(FSRL_EHIP, "collect group allocation failed: %s", hipGetErrorString(e));
        g->m.clear();
        (void)fsrl_collect_group_destroy(g);
        return FSRL_EHIP;
    }
    ga_bind(g->ga, g->stream, collect_group_launch, g);
    const int rc = g->layered ? 0 : gactor_ensure(g->ga, g->m.data(), k, g->raw_cols);      // a layered group has no ring
    if (rc) { g->m.clear(); (void)fsrl_collect_group_destroy(g); return rc; }
    for (int i = 0; i < k; ++i) ctxs[i]->cgroup = g;
    *out = g;
    return 0;
}

// a member's mean / std from its answered rows: replay members from the raw head rows, on-policy members the means as they are and
// exp of the member's sigma_param row (fsrl_group_collect_step's finish)
static void collect_group_finish(const fsrl_collect_group* g, fsrl_ctx* c, const float* rows, const float* sp, int ka) {
    if (!g->onpolicy) { sac_actor_finish(c, rows, ka, c->act_mu.data(), c->act_sg.data()); return; }
    const int Da = c->cfg.act_dim;
    memcpy(c->act_mu.data(), rows, (size_t)ka * Da * 4);
    for (int r = 0; r < ka; ++r)
        for (int d = 0; d < Da; ++d) c->act_sg[(size_t)r * Da + d] = expf(sp[d]);
}
// off the resident path a push failed behind the members' own actor calls: leave none in flight
static void collect_group_drain(fsrl_collect_group* g, const int32_t* k_act) {
    const int Da = g->m[0]->cfg.act_dim;
    for (size_t j = 0; j < g->m.size(); ++j) {
        fsrl_ctx* c = g->m[j];
        if (k_act[j] <= 0) continue;
        c->act_mu.resize((size_t)k_act[j] * Da); c->act_sg.resize((size_t)k_act[j] * Da);
        (void)actor_eval_finish(c, c->act_mu.data(), c->act_sg.data());
    }
}

// the first request after a release goes behind the members' compute streams (a layered group; under the group's mutex)
static int collect_group_reorder(fsrl_collect_group* g) {
    if (!g->reorder) return 0;
    for (size_t i = 0; i < g->m.size(); ++i) {
        HIPCHK(hipEventRecord(g->ready[i], g->m[i]->compute));
        HIPCHK(hipStreamWaitEvent(g->stream, g->ready[i], 0));
    }
    g->reorder = false;
    return 0;
}

// fsrl_collect_group_step for a group of layered ON-POLICY members: the shared request of a layered fsrl_group
// (lay_group_collect_post: L + 1 forward launches over the members' c->P, then lay_infer_out_group_kernel), ordered as the layered
// replay group's (lay_collect_group_step, host_sac_group_layered.inc)
static int lay_collect_group_step_onpolicy(fsrl_collect_group* g, const GaStepArgs& a) {
    const int n = (int)g->m.size(), Do = g->m[0]->cfg.obs_dim, Da = g->m[0]->cfg.act_dim;
    return ga_collect_step_via(
        g->ga, g->m.data(), n, g->device, a, [](int) { return true; },
        [&]() -> int {
            std::lock_guard<std::mutex> lock(g->mu);                // `reorder` is the release hook's, on any thread
            const int rc = collect_group_reorder(g);
            return rc ? rc : lay_group_collect_post(g->lay, g->ga, g->m.data(), n, a.k_act, a.obs_act);
        },
        [&]() { return lay_group_collect_wait(g->lay, g->ga, n, Do, Da); },
        [&]() { (void)hipStreamSynchronize(g->stream); },           // a push failed behind the request: drain the stream
        [&](int i, fsrl_ctx* c, int ka, const GaLayout&) {
            const LayGroupPinned pin = lay_group_pinned(g->lay, Do, Da);
            collect_group_finish(g, c, pin.mu + (size_t)i * g->lay.ccap * Da, pin.sp + (size_t)i * FSRL_MAX_ACT, ka);
        },
        [&]() { collect_group_drain(g, a.k_act); });
}

// ga_collect_step (host_actor_ring.inc) with this owner's differences: the ring exists since create, the group's mutex is held from
// the request to its answer (the release hook may run on other threads), a member's mean / std come from its answered rows
// (collect_group_finish), and off the resident path every member's own evaluation is drained
extern "C" int fsrl_collect_group_step(fsrl_collect_group* g, const int32_t* k, const int32_t* env_ids, const float* obs, const float* act,
                                       const double* rew, const double* cost, const uint8_t* terminated, const uint8_t* truncated,
                                       const float* obs_next, int64_t* ptr_out, double* ep_rew_out, int32_t* ep_len_out,
                                       int64_t* ep_idx_out, const int32_t* k_act, const float* obs_act, int32_t deterministic,
                                       int32_t bound_method, const float* act_low, const float* act_high, float* act_out,
                                       float* env_act_out) {
    CHECK_ARG(g && k && k_act, "null argument");
    if (g->broken) return fail(FSRL_ESTATE, "a member of this collect group has been destroyed");
    const GaStepArgs a{k, env_ids, obs, act, rew, cost, terminated, truncated, obs_next, ptr_out, ep_rew_out, ep_len_out, ep_idx_out,
                       k_act, obs_act, deterministic, bound_method, act_low, act_high, act_out, env_act_out};
    if (g->layered) return g->onpolicy ? lay_collect_group_step_onpolicy(g, a) : lay_collect_group_step(g, a);
    const int n = (int)g->m.size(), cols = g->raw_cols;
    // held from the request to its answer: a release hook that comes in between (a caller error, see the top) waits for the answer
    // instead of ending the kernel under the request; on every other way out the destructor lets go
    std::unique_lock<std::mutex> held(g->mu, std::defer_lock);
    return ga_collect_step_via(
        g->ga, g->m.data(), n, g->device, a, [&](int i) { return k_act[i] <= gactor_member_rows(g->m[i]); },
        [&]() { held.lock(); const int rc = gactor_post(g->ga, k_act, obs_act); if (rc) held.unlock(); return rc; },
        [&]() { const int rc = gactor_wait(g->ga); held.unlock(); return rc; },
        [&]() { (void)gactor_wait(g->ga); held.unlock(); },
        [&](int i, fsrl_ctx* c, int ka, const GaLayout& l) {
            collect_group_finish(g, c, l.mu + (size_t)g->ga.base[i] * 16 * cols, l.sp + (size_t)i * FSRL_MAX_ACT, ka);
        },
        [&]() { collect_group_drain(g, k_act); });
}

extern "C" int fsrl_collect_group_actor_set_resident(fsrl_collect_group* g, int32_t on, double idle_timeout_us) {
    CHECK_ARG(g, "null group");
    if (g->layered) return 0;                  // no resident kernel to switch: accepted, no effect
    std::lock_guard<std::mutex> lock(g->mu);
    return rr_code(rr_set_resident(g->ga, on, idle_timeout_us), "");
}

extern "C" int fsrl_collect_group_actor_resident_stats(fsrl_collect_group* g, int64_t* out3) {
    CHECK_ARG(g && out3, "null argument");
    std::lock_guard<std::mutex> lock(g->mu);
    rr_stats(g->ga, out3);
    return 0;
}

extern "C" int fsrl_collect_group_actor_release(fsrl_collect_group* g) {
    CHECK_ARG(g, "null group");
    collect_group_end_kernel(g);               // (a layered group: nothing is live)
    return 0;
}
