// host_devcollect_group.inc -- the launch loop of every device collect and evaluation, and their four entry points: fsrl_collect_device,
// fsrl_collect_device_group, fsrl_evaluate_device, fsrl_evaluate_device_group (part of fsrl_hip.hip, behind every kind of group;
// include/fsrl_hip.h "Device environments").
//
// A device collect is ONE workgroup (kernels_devcollect.hpp), and k seeds' collects share nothing: collect_device_group_kernel runs
// them as the k workgroups of one launch, workgroup b the loop on member b's store, env arrays, DcState and log.  There is one loop
// on the host (devcollect_group_run) over what host_devcollect.inc does per member: devcollect_check, devcollect_begin,
// devcollect_replay.  It is a free function over contexts because there are four kinds of group: a member may be ungrouped or sit
// in an fsrl_group, an fsrl_collect_group, an fsrl_sac_group or an fsrl_cvpo_group, and is not owned here.
// The solo calls are the one-member launch (`named = false`): fsrl_collect_device keeps its refusal of grouped contexts, and their
// failures name no member and no group.
//
// Ordering.  The launches go on member 0's compute stream.  devcollect_begin leaves every member's uploads on ITS compute stream, behind
// whatever that member has enqueued (updates, parameter uploads; grouped updates make the members' streams wait for the update
// group's `done`); an event per member then puts member 0's stream behind all of them -- once per collect, not per launch.  Every
// launch is waited for on the host before its logs are replayed, so whatever a member enqueues after the call is behind the collect.
// Prioritised members: per_devcollect on the member's OWN compute stream, which re-records upd_done.  Where that is the launch stream
// (always, for one member) it is directly behind the launch by stream order; elsewhere behind an event recorded after the launch,
// and waited for before the next launch overwrites the slots.
// The member table and the events are made by an env's first call in the role that needs them, and kept (fsrl_devenv).
// Evaluations are the same call with `store = false`: evaluate_device_group_kernel in the launch, no tree launches, the logs replayed
// through the envs' accumulators.  The members' stores, books, samplers and random streams are not touched.
static int devcollect_group_ensure(fsrl_devenv* v0, bool layered) {       // member 0's env: the table and the event behind the launch
    if (!v0->g_done) HIPCHK(hipEventCreateWithFlags(&v0->g_done, hipEventDisableTiming));
    if (layered) {
        if (!v0->d_ltab) HIPCHK(v0->mem.dev(&v0->d_ltab, sizeof(LayCollectTable)));
        if (!v0->h_ltab) HIPCHK(v0->mem.pinned(&v0->h_ltab, sizeof(LayCollectTable)));
        return 0;
    }
    if (!v0->d_tab) HIPCHK(v0->mem.dev(&v0->d_tab, sizeof(DevCollectGroupTable)));
    if (!v0->h_tab) HIPCHK(v0->mem.pinned(&v0->h_tab, sizeof(DevCollectGroupTable)));
    return 0;
}

// the actor of a layered context as lay_collect_kernel takes it: the on-policy context's own first network, or a replay context's
// actor (SacState::ka, PA).  false: not a layered context, or a replay context nothing was initialised on
static bool devcollect_lay_actor(fsrl_ctx* c, const float** P, const LayNet** net, int* hmax) {
    if (!c->lay) return false;
    *hmax = c->lay->hmax;
    if (!ctx_is_replay(c)) { *P = c->P; *net = &c->lay->lm.net[0]; return true; }
    SacState* s = sac_of(c);
    if (!s || !s->layered) return false;
    *P = s->PA; *net = &s->ka.lm.net[0];
    return true;
}

static int devcollect_head_kind(const fsrl_ctx* c) {
    if (!ctx_is_replay(c)) return DC_HEAD_ONPOLICY;
    const SacState* s = sac_of(const_cast<fsrl_ctx*>(c));
    return s && s->ddpg ? DC_HEAD_DDPG : DC_HEAD_GAUSS;
}

// member i against member 0: everything the ONE instantiation and the shared ModelDesc stand for.  What travels in each member's own
// DevCollectArgs may differ: env_num, n_episode, the env seed, the bounds, max_action, squash, exploration_sigma, prioritised replay.
static int devcollect_group_agree(const fsrl_ctx* c, const fsrl_devenv* v, const fsrl_ctx* c0, const fsrl_devenv* v0, int i, bool layered) {
    static const char* const heads[] = {"an on-policy", "a Gaussian replay (SAC-Lag, CVPO)", "a DDPG-Lag"};
    CHECK_ARG(c->device == c0->device, "member %d: members live on one device", i);
    CHECK_ARG(devcollect_head_kind(c) == devcollect_head_kind(c0), "member %d is %s context and member 0 %s one: a grouped device collect "
              "has one head kind (on-policy, Gaussian or DDPG)", i, heads[devcollect_head_kind(c)], heads[devcollect_head_kind(c0)]);
    CHECK_ARG(c->cfg.obs_dim == c0->cfg.obs_dim && c->cfg.act_dim == c0->cfg.act_dim && c->cfg.hidden == c0->cfg.hidden &&
              c->cfg.n_critics == c0->cfg.n_critics,
              "member %d: members must have one network shape (obs_dim, act_dim, hidden, n_critics): (%d, %d, %d, %d), member 0's "
              "(%d, %d, %d, %d)", i, c->cfg.obs_dim, c->cfg.act_dim, c->cfg.hidden, c->cfg.n_critics, c0->cfg.obs_dim, c0->cfg.act_dim,
              c0->cfg.hidden, c0->cfg.n_critics);
    if (layered)        // every member brings its own LayNet, but the groups ask one shape of layered members and so does this call
        CHECK_ARG(lay_same_shape(c->cfg, c0->cfg), "member %d: members of a layered device collect must have one hidden_sizes and "
                  "force_layered (it has %d hidden layers, member 0 %d)", i, c->cfg.n_hidden, c0->cfg.n_hidden);
    CHECK_ARG(v->cfg.kind == v0->cfg.kind, "member %d: its device env is of kind %d, member 0's of kind %d: one env kind per grouped collect "
              "(the kernel is instantiated once)", i, v->cfg.kind, v0->cfg.kind);
    CHECK_ARG(v->cfg.max_episode_steps == v0->cfg.max_episode_steps, "member %d: members must share max_episode_steps (%d, member 0's %d)", i,
              v->cfg.max_episode_steps, v0->cfg.max_episode_steps);
    if (!ctx_is_replay(c)) {
        CHECK_ARG((c->cfg.unbounded != 0) == (c0->cfg.unbounded != 0), "member %d: members must share unbounded (the actor's mean is %s, "
                  "member 0's %s)", i, c->cfg.unbounded ? "the head itself" : "max_action * tanh(head)",
                  c0->cfg.unbounded ? "the head itself" : "max_action * tanh(head)");
    } else {
        const SacState* s = sac_of(const_cast<fsrl_ctx*>(c)); const SacState* s0 = sac_of(const_cast<fsrl_ctx*>(c0));
        CHECK_ARG(s->mean_tanh == s0->mean_tanh, "member %d: members must share actor_mean (the actor's mean is %s, member 0's %s)", i,
                  s->mean_tanh ? "max_action * tanh(head)" : "unbounded", s0->mean_tanh ? "max_action * tanh(head)" : "unbounded");
    }
    return 0;
}

struct DcGroupOut {
    int64_t* steps; double* total_cost; int32_t* terms; int32_t* truncs; double* ep_rew; int32_t* ep_len; int32_t* episodes; int32_t* launches;
};
// everything behind the checks; the caller waits for the launch stream when this fails half-way
static int devcollect_group_run(fsrl_ctx** ctxs, fsrl_devenv** envs, int k, const int32_t* n_episode, int32_t deterministic,
                                int32_t bound_method, const float* act_low, const float* act_high, int max_steps, const DcGroupOut& o,
                                bool store, bool named, bool layered) {
    const char* const what = !store ? "device evaluation" : named ? "grouped device collect" : "device collect";
    // how a failure names member i: `grouped` with its number in place of the %d, `solo` for the one member of an unnamed call
    const auto who = [&](int i, const char* solo, const char* grouped) {
        char b[64];
        snprintf(b, sizeof(b), grouped, i);
        return named ? std::string(b) : std::string(solo);
    };
    fsrl_devenv* v0 = envs[0];
    const int Da = v0->cfg.act_dim;
    DcActor actor0{};
    for (int i = 0; i < k; ++i) {
        DcActor actor{};
        const int rc = devcollect_begin(ctxs[i], envs[i], n_episode[i], deterministic, bound_method, act_low ? act_low + (size_t)i * Da : nullptr,
                                        act_high ? act_high + (size_t)i * Da : nullptr, max_steps, &actor, store, layered);
        if (rc) return rc;
        if (i == 0) actor0 = actor;
        if (actor.head != actor0.head) return fail(FSRL_ESTATE, "member %d: its actor's head kind changed under the call", i);
        if (layered) {
            LayCollectMember& m = v0->h_ltab->m[i];
            m.P = actor.P; m.a = envs[i]->d_args; m.ws = envs[i]->d_ws; m.ld = envs[i]->ws_ld;
            m.unbounded = ctxs[i]->cfg.unbounded ? 1 : 0; m.net = *actor.net;
        } else {
            v0->h_tab->P[i] = actor.P; v0->h_tab->a[i] = envs[i]->d_args;
        }
    }
    hipStream_t s = ctxs[0]->compute;
    for (int i = 1; i < k; ++i) {
        if (ctxs[i]->compute == s) continue;           // members of one fsrl_group share a stream
        // the members' resident kernels are on their way out (ENTER_DEV above): making the event does not wait for an idle timeout
        if (!envs[i]->g_ready) HIPCHK(hipEventCreateWithFlags(&envs[i]->g_ready, hipEventDisableTiming));
        HIPCHK(hipEventRecord(envs[i]->g_ready, ctxs[i]->compute));
        HIPCHK(hipStreamWaitEvent(s, envs[i]->g_ready, 0));
    }
    if (layered) HIPCHK(hipMemcpyAsync(v0->d_ltab, v0->h_ltab, sizeof(LayCollectTable), hipMemcpyHostToDevice, s));
    else HIPCHK(hipMemcpyAsync(v0->d_tab, v0->h_tab, sizeof(DevCollectGroupTable), hipMemcpyHostToDevice, s));
    const ModelDesc mdv = layered ? ModelDesc{} : *actor0.md;
    const int head = actor0.head;
    DcTotals t[FSRL_MAX_GROUP];
    uint8_t finished[FSRL_MAX_GROUP] = {}, was_finished[FSRL_MAX_GROUP] = {};
    int32_t steps[FSRL_MAX_GROUP] = {}, mes[FSRL_MAX_GROUP] = {};
    int64_t off[FSRL_MAX_GROUP + 1];
    dc_group_offsets(n_episode, k, off);
    for (int i = 0; i < k; ++i) mes[i] = envs[i]->cfg.max_episode_steps;
    const int64_t launch_cap = dc_group_launch_cap(n_episode, mes, k, max_steps);
    int32_t launches = 0;
    for (;;) {
        if (launches >= launch_cap)
            return fail(FSRL_ESTATE, "%s: %d launches did not finish %s", what, launches,
                        named ? "every member" : (std::to_string(n_episode[0]) + " episodes").c_str());
        // layered members: the one looping kernel of kernels_devcollect_layered.hpp, whatever the widths
        const auto lay_go = [&]() {
            devenv_dispatch(v0->cfg.kind, [&](auto env) {
                using Env = decltype(env);
                const LayCollectTable* tab = v0->d_ltab;
#define LAYC_GO(HEAD_, STORE_) hipLaunchKernelGGL((lay_collect_kernel<Env, HEAD_, STORE_>), dim3(k), dim3(LAYC_NT), 0, s, tab)
                if (store) { if (head == DC_HEAD_GAUSS) LAYC_GO(DC_HEAD_GAUSS, true); else if (head == DC_HEAD_DDPG) LAYC_GO(DC_HEAD_DDPG, true); else LAYC_GO(DC_HEAD_ONPOLICY, true); }
                else { if (head == DC_HEAD_GAUSS) LAYC_GO(DC_HEAD_GAUSS, false); else if (head == DC_HEAD_DDPG) LAYC_GO(DC_HEAD_DDPG, false); else LAYC_GO(DC_HEAD_ONPOLICY, false); }
#undef LAYC_GO
            });
            HIPCHK(hipGetLastError());
            return 0;
        };
        int rc = layered ? lay_go() : dispatch_H(ctxs[0]->cfg.hidden, [&](auto hc) {
            constexpr int H = decltype(hc)::value;
            devenv_dispatch(v0->cfg.kind, [&](auto env) {
                using Env = decltype(env);
                const DevCollectGroupTable* tab = v0->d_tab;
                if (!store) {
                    if (head == DC_HEAD_GAUSS) hipLaunchKernelGGL((evaluate_device_group_kernel<H, Env, DC_HEAD_GAUSS>), dim3(k), dim3(4 * H), 0, s, mdv, tab);
                    else if (head == DC_HEAD_DDPG) hipLaunchKernelGGL((evaluate_device_group_kernel<H, Env, DC_HEAD_DDPG>), dim3(k), dim3(4 * H), 0, s, mdv, tab);
                    else hipLaunchKernelGGL((evaluate_device_group_kernel<H, Env>), dim3(k), dim3(4 * H), 0, s, mdv, tab);
                } else if (head == DC_HEAD_GAUSS) hipLaunchKernelGGL((collect_device_group_kernel<H, Env, DC_HEAD_GAUSS>), dim3(k), dim3(4 * H), 0, s, mdv, tab);
                else if (head == DC_HEAD_DDPG) hipLaunchKernelGGL((collect_device_group_kernel<H, Env, DC_HEAD_DDPG>), dim3(k), dim3(4 * H), 0, s, mdv, tab);
                else hipLaunchKernelGGL((collect_device_group_kernel<H, Env>), dim3(k), dim3(4 * H), 0, s, mdv, tab);
            });
            HIPCHK(hipGetLastError());
            return 0;
        });
        if (rc) return rc;
        // PrioritizedReplayBuffer.add for the rows of every prioritised member that went in unfinished: its own small launch, on its
        // own compute stream, behind this launch -- by stream order where that is the launch stream, else through g_done
        bool per_other = false;
        for (int i = 0; i < k; ++i) per_other = per_other || (envs[i]->h_args->slots && !finished[i] && ctxs[i]->compute != s);
        if (per_other) HIPCHK(hipEventRecord(v0->g_done, s));
        for (int i = 0; i < k; ++i) {
            if (!envs[i]->h_args->slots || finished[i]) continue;
            if (ctxs[i]->compute != s) HIPCHK(hipStreamWaitEvent(ctxs[i]->compute, v0->g_done, 0));
            rc = per_devcollect(ctxs[i], envs[i]->d_slot, &envs[i]->d_state->log_rows, max_steps * envs[i]->cfg.env_num);
            if (rc) return rc;
        }
        ++launches;
        for (int i = 0; i < k; ++i) HIPCHK(hipMemcpyAsync(envs[i]->h_state, envs[i]->d_state, sizeof(DcState), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (int i = 0; i < k; ++i)         // the tree launches read the slots and log_rows the next launch overwrites
            if (envs[i]->h_args->slots && !finished[i] && ctxs[i]->compute != s) HIPCHK(hipStreamSynchronize(ctxs[i]->compute));
        bool any_rows = false;
        for (int i = 0; i < k; ++i) {
            const DcState& hs = *envs[i]->h_state;
            if (!devcollect_state_sane(hs, max_steps, envs[i]->cfg.env_num))
                return fail(FSRL_ESTATE, "%s: %s reported %d rows in %d steps", what, who(i, "the kernel", "member %d's workgroup").c_str(),
                            hs.log_rows, hs.steps);
            if (finished[i] && (hs.steps != 0 || hs.log_rows != 0))
                return fail(FSRL_ESTATE, "%s: member %d was finished and its workgroup reported %d rows in %d steps", what, i,
                            hs.log_rows, hs.steps);
            if (hs.log_rows > 0) {
                HIPCHK(hipMemcpyAsync(envs[i]->h_log, envs[i]->d_log, (size_t)hs.log_rows * sizeof(DcLogRow), hipMemcpyDeviceToHost, s));
                any_rows = true;
            }
        }
        if (any_rows) HIPCHK(hipStreamSynchronize(s));
        for (int i = 0; i < k; ++i) {
            const DcState& hs = *envs[i]->h_state;
            rc = devcollect_replay(ctxs[i], envs[i], hs, n_episode[i], t[i], o.ep_rew + off[i], o.ep_len + off[i], store);
            if (rc) { if (named) g_err = "member " + std::to_string(i) + ": " + g_err; return rc; }
            was_finished[i] = finished[i]; steps[i] = hs.steps; finished[i] = hs.finished ? 1 : 0;
        }
        if (dc_group_complete(finished, k)) break;
        const int stalled = dc_group_stalled(was_finished, steps, k);
        if (stalled >= 0) return fail(FSRL_ESTATE, "%s: a launch made no step%s", what, who(stalled, "", " for member %d").c_str());
    }
    for (int i = 0; i < k; ++i)
        if (t[i].episodes != envs[i]->h_state->episodes)
            return fail(FSRL_ESTATE, "%s: %s holds %d episodes, the kernel counted %d", what, who(i, "the log", "member %d's log").c_str(),
                        t[i].episodes, envs[i]->h_state->episodes);
    // FastCollector.reset_env at the end of every collect: ALL envs of ALL members, then one wait
    for (int i = 0; i < k; ++i) {
        DevEnvIo io{};
        io.n = envs[i]->cfg.env_num;
        const int rc = devenv_reset_launch(envs[i], io, s);
        if (rc) return rc;
    }
    HIPCHK(hipStreamSynchronize(s));
    for (int i = 0; i < k; ++i) {
        o.steps[i] = t[i].rows; o.total_cost[i] = t[i].total_cost; o.terms[i] = t[i].terms; o.truncs[i] = t[i].truncs;
        o.episodes[i] = std::min(t[i].episodes, n_episode[i]);
    }
    if (o.launches) *o.launches = launches;
    return 0;
}

// the call behind the four entry points, storing or not.  named: the _group calls, whose refusals and failures say which member.
// named = false: a solo call -- one member, made of the caller's own non-null arguments -- whose refusals are devcollect_check's, in
// its order, and then the outputs'
static int devcollect_group_call(fsrl_ctx** ctxs, fsrl_devenv** envs, int32_t k, const int32_t* n_episode, int32_t deterministic,
                                 int32_t bound_method, const float* act_low, const float* act_high, int32_t max_steps_per_launch,
                                 const DcGroupOut& o, bool store, bool named, bool layered = false) {
    // ---- every refusal before anything is touched
    const bool outputs = o.steps && o.total_cost && o.terms && o.truncs && o.ep_rew && o.ep_len && o.episodes;
    if (named) {        // the lists' own
        CHECK_ARG(k >= 1 && k <= FSRL_MAX_GROUP, "k %d: a grouped device %s has 1..%d members", k, store ? "collect" : "evaluation", FSRL_MAX_GROUP);
        CHECK_ARG(ctxs && envs && n_episode, "null argument");
        CHECK_ARG(outputs, "null output");
        CHECK_ARG((act_low == nullptr) == (act_high == nullptr), "act_low and act_high are given together");
        for (int i = 0; i < k; ++i) {
            CHECK_ARG(ctxs[i] && envs[i], "member %d: null context / env", i);
            for (int j = 0; j < i; ++j) {
                CHECK_ARG(ctxs[j] != ctxs[i], "member %d: its context is listed twice (member %d)", i, j);
                CHECK_ARG(envs[j] != envs[i], "member %d: its device env is listed twice (member %d)", i, j);
            }
        }
    }
    const int Da0 = ctxs[0]->cfg.act_dim;
    for (int i = 0; i < k; ++i) {
        const int rc = devcollect_check(ctxs[i], envs[i], n_episode[i], bound_method, act_low ? act_low + (size_t)i * Da0 : nullptr,
                                        act_high ? act_high + (size_t)i * Da0 : nullptr, max_steps_per_launch, named, store, layered);
        if (rc) { if (named) g_err = "member " + std::to_string(i) + ": " + g_err; return rc; }
    }
    for (int i = 1; i < k; ++i) {
        const int rc = devcollect_group_agree(ctxs[i], envs[i], ctxs[0], envs[0], i, layered);
        if (rc) return rc;
    }
    CHECK_ARG(outputs, "null output");
    const int max_steps = max_steps_per_launch > 0 ? max_steps_per_launch : DC_DEFAULT_STEPS;
    HIPCHK(hipSetDevice(ctxs[0]->device));
    for (int i = 0; i < k; ++i) pactor_release(ctxs[i]);       // the table's first allocation would wait for a live resident actor's idle timeout
    int rc = devcollect_group_ensure(envs[0], layered);
    if (rc) return rc;
    rc = devcollect_group_run(ctxs, envs, k, n_episode, deterministic, bound_method, act_low, act_high, max_steps, o, store, named, layered);
    if (rc) {       // leave nothing of the call in flight: the kernel reads every member's env arrays from member 0's stream
        const std::string why = g_err;
        (void)hipStreamSynchronize(ctxs[0]->compute);
        g_err = why;
    }
    return rc;
}

extern "C" int fsrl_collect_device_group(fsrl_ctx** ctxs, fsrl_devenv** envs, int32_t k, const int32_t* n_episode, int32_t deterministic,
                                         int32_t bound_method, const float* act_low, const float* act_high, int32_t max_steps_per_launch,
                                         int64_t* steps_out, double* total_cost_out, int32_t* term_count_out, int32_t* trunc_count_out,
                                         double* ep_rew_out, int32_t* ep_len_out, int32_t* episodes_out, int32_t* launches_out) {
    const DcGroupOut o{steps_out, total_cost_out, term_count_out, trunc_count_out, ep_rew_out, ep_len_out, episodes_out, launches_out};
    return devcollect_group_call(ctxs, envs, k, n_episode, deterministic, bound_method, act_low, act_high, max_steps_per_launch, o, true, true);
}

extern "C" int fsrl_evaluate_device_group(fsrl_ctx** ctxs, fsrl_devenv** envs, int32_t k, const int32_t* n_episode, int32_t deterministic,
                                          int32_t bound_method, const float* act_low, const float* act_high, int32_t max_steps_per_launch,
                                          int64_t* steps_out, double* total_cost_out, int32_t* term_count_out, int32_t* trunc_count_out,
                                          double* ep_rew_out, int32_t* ep_len_out, int32_t* episodes_out, int32_t* launches_out) {
    const DcGroupOut o{steps_out, total_cost_out, term_count_out, trunc_count_out, ep_rew_out, ep_len_out, episodes_out, launches_out};
    return devcollect_group_call(ctxs, envs, k, n_episode, deterministic, bound_method, act_low, act_high, max_steps_per_launch, o, false, true);
}

// ---- the solo calls: the one-member launch over the caller's own arguments
extern "C" int fsrl_collect_device(fsrl_ctx* c, fsrl_devenv* v, int32_t n_episode, int32_t deterministic, int32_t bound_method,
                                   const float* act_low, const float* act_high, int32_t max_steps_per_launch, int64_t* steps_out,
                                   double* total_cost_out, int32_t* term_count_out, int32_t* trunc_count_out, double* ep_rew_out,
                                   int32_t* ep_len_out, int32_t* episodes_out, int32_t* launches_out) {
    CHECK_ARG(c && v, "null context / env");
    const DcGroupOut o{steps_out, total_cost_out, term_count_out, trunc_count_out, ep_rew_out, ep_len_out, episodes_out, launches_out};
    return devcollect_group_call(&c, &v, 1, &n_episode, deterministic, bound_method, act_low, act_high, max_steps_per_launch, o, true, false);
}

extern "C" int fsrl_evaluate_device(fsrl_ctx* c, fsrl_devenv* v, int32_t n_episode, int32_t deterministic, int32_t bound_method,
                                    const float* act_low, const float* act_high, int32_t max_steps_per_launch, int64_t* steps_out,
                                    double* total_cost_out, int32_t* term_count_out, int32_t* trunc_count_out, double* ep_rew_out,
                                    int32_t* ep_len_out, int32_t* episodes_out, int32_t* launches_out) {
    CHECK_ARG(c && v, "null context / env");
    const DcGroupOut o{steps_out, total_cost_out, term_count_out, trunc_count_out, ep_rew_out, ep_len_out, episodes_out, launches_out};
    return devcollect_group_call(&c, &v, 1, &n_episode, deterministic, bound_method, act_low, act_high, max_steps_per_launch, o, false, false);
}

// ---- layered contexts: the _group calls' arguments, the same loop, lay_collect_kernel in the launch.  k = 1 is the solo collect, and
// its failures name no member; members may sit in any kind of group or in none.
extern "C" int fsrl_collect_device_layered(fsrl_ctx** ctxs, fsrl_devenv** envs, int32_t k, const int32_t* n_episode, int32_t deterministic,
                                           int32_t bound_method, const float* act_low, const float* act_high, int32_t max_steps_per_launch,
                                           int64_t* steps_out, double* total_cost_out, int32_t* term_count_out, int32_t* trunc_count_out,
                                           double* ep_rew_out, int32_t* ep_len_out, int32_t* episodes_out, int32_t* launches_out) {
    const DcGroupOut o{steps_out, total_cost_out, term_count_out, trunc_count_out, ep_rew_out, ep_len_out, episodes_out, launches_out};
    if (k == 1) CHECK_ARG(ctxs && envs && n_episode && ctxs[0] && envs[0], "null context / env");
    return devcollect_group_call(ctxs, envs, k, n_episode, deterministic, bound_method, act_low, act_high, max_steps_per_launch, o, true, k != 1, true);
}

extern "C" int fsrl_evaluate_device_layered(fsrl_ctx** ctxs, fsrl_devenv** envs, int32_t k, const int32_t* n_episode, int32_t deterministic,
                                            int32_t bound_method, const float* act_low, const float* act_high, int32_t max_steps_per_launch,
                                            int64_t* steps_out, double* total_cost_out, int32_t* term_count_out, int32_t* trunc_count_out,
                                            double* ep_rew_out, int32_t* ep_len_out, int32_t* episodes_out, int32_t* launches_out) {
    const DcGroupOut o{steps_out, total_cost_out, term_count_out, trunc_count_out, ep_rew_out, ep_len_out, episodes_out, launches_out};
    if (k == 1) CHECK_ARG(ctxs && envs && n_episode && ctxs[0] && envs[0], "null context / env");
    return devcollect_group_call(ctxs, envs, k, n_episode, deterministic, bound_method, act_low, act_high, max_steps_per_launch, o, false, k != 1, true);
}
