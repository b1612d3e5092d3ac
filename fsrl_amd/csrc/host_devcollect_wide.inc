// host_devcollect_wide.inc -- fsrl_collect_device_wide: the device collect over a wide env, 1 .. DCW_MAX_ENVS envs (part of
// fsrl_hip.hip, behind host_devcollect_group.inc; kernels_devcollect_wide.hpp; include/fsrl_hip.h "Device environments").
//
// One launch of wide_collect_step_kernel is one vector step, a workgroup per 16-row tile.  The host enqueues a BATCH of S step
// launches and one one-workgroup settle launch without waiting, reads the settled scalars and the batch's log back once, and replays
// the rows through the store's bookkeeping exactly as the looping collect does: the checks, the entry and the replay are
// devcollect_check / devcollect_begin / devcollect_replay of host_devcollect.inc with `wide = true`, the launch cap and the "made
// no step" rule are those of devcollect_plan.hpp with a batch in the place of a launch.  The launches of a batch behind the step that
// finished the collect exit at their first test.  The launch ordinal runs on across batches and collects (fsrl_devenv::wide_t): its
// parity names the side of DcwState a launch reads.
// Layered contexts come in through fsrl_collect_device_wide_layered: the same checks, entry, batch loop and replay with
// `layered = true` and wide_layered_step_kernel (kernels_devcollect_wide_layered.hpp) in the launch -- the loop takes the launch as a
// function.  A tile's activations are dynamic LDS sized to the shape, or (a layer beyond DCWL_LDS_WIDTH) the env's workspace.
// k members' wide collects in one launch per step are fsrl_collect_device_wide_group (host_devcollect_wide_group.inc, behind this file):
// the same batch loop, devcollect_wide_run, with the grouped kernels in the launch.
// Evaluations over wide envs have kernels and a batch loop of their own (host_deveval_wide.inc: no log, no replay).
// Not here: prioritised contexts -- refused by name.
#include <chrono>
static int devcollect_wide_launch(fsrl_ctx* c, fsrl_devenv* v, const DcActor& actor, int grid, bool first, bool settle) {
    hipStream_t s = c->compute;
    const ModelDesc mdv = *actor.md;
    const int head = actor.head, t = (int)(v->wide_t & 0x7FFFFFFFu), fi = first ? 1 : 0, se = settle ? 1 : 0;
    const float* P = actor.P;
    const WideCollectArgs* wa = v->d_wargs;
    const dim3 g((unsigned)(settle ? 1 : grid));
    const int rc = dispatch_H(c->cfg.hidden, [&](auto hc) {
        constexpr int H = decltype(hc)::value;
        devenv_dispatch(v->cfg.kind, [&](auto env) {
            using Env = decltype(env);
            if (head == DC_HEAD_GAUSS) hipLaunchKernelGGL((wide_collect_step_kernel<H, Env, DC_HEAD_GAUSS>), g, dim3(4 * H), 0, s, mdv, P, wa, t, fi, se);
            else if (head == DC_HEAD_DDPG) hipLaunchKernelGGL((wide_collect_step_kernel<H, Env, DC_HEAD_DDPG>), g, dim3(4 * H), 0, s, mdv, P, wa, t, fi, se);
            else hipLaunchKernelGGL((wide_collect_step_kernel<H, Env, DC_HEAD_ONPOLICY>), g, dim3(4 * H), 0, s, mdv, P, wa, t, fi, se);
        });
        HIPCHK(hipGetLastError());
        return 0;
    });
    ++v->wide_t;
    return rc;
}

// the layered launches: one kernel per (env kind, head, form) for every shape; above 64 KB of dynamic LDS the function's limit is raised,
// once per instantiation (KERNEL: wide_layered_step_kernel or wide_layered_group_step_kernel) and device
template <auto KERNEL, class... Args>
static int devcollect_wide_layered_go(int device, const dim3 g, size_t lds, hipStream_t s, Args... args) {
    static std::atomic<uint64_t> raised{0};         // a bit per device (the attribute belongs to the function on the current device)
    if (lds > 64 * 1024 && !(raised.load() >> (device & 63) & 1ull)) {
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dc_wl_lds_bytes(DCWL_LDS_WIDTH)));
        raised.fetch_or(1ull << (device & 63));
    }
    hipLaunchKernelGGL(KERNEL, g, dim3(WL_NT), lds, s, args...);
    HIPCHK(hipGetLastError());
    return 0;
}
static int devcollect_wide_layered_launch(fsrl_ctx* c, fsrl_devenv* v, const DcActor& actor, int grid, bool first, bool settle) {
    hipStream_t s = c->compute;
    const int head = actor.head, t = (int)(v->wide_t & 0x7FFFFFFFu), fi = first ? 1 : 0, se = settle ? 1 : 0;
    const WideCollectArgs* wa = v->d_wargs;
    const WideLayActor* la = v->d_wlact;
    const bool devws = v->h_wlact->ws != nullptr;
    const size_t lds = settle ? 0 : (size_t)dc_wl_lds_bytes(v->h_wlact->ld);       // the settle launch touches no activation
    const dim3 g((unsigned)(settle ? 1 : grid));
    int rc = 0;
    devenv_dispatch(v->cfg.kind, [&](auto env) {
        using Env = decltype(env);
#define WL_GO(HEAD_) (devws ? devcollect_wide_layered_go<&wide_layered_step_kernel<Env, HEAD_, true>>(c->device, g, lds, s, wa, la, t, fi, se) \
                            : devcollect_wide_layered_go<&wide_layered_step_kernel<Env, HEAD_, false>>(c->device, g, lds, s, wa, la, t, fi, se))
        rc = head == DC_HEAD_GAUSS ? WL_GO(DC_HEAD_GAUSS) : head == DC_HEAD_DDPG ? WL_GO(DC_HEAD_DDPG) : WL_GO(DC_HEAD_ONPOLICY);
#undef WL_GO
    });
    ++v->wide_t;
    return rc;
}

// One wide call: k members (the solo calls: one, unnamed), and how a launch of a batch goes out for all of them -- the solo kernels on
// the one member, or the grouped kernels over the member table (host_devcollect_wide_group.inc).  `prepare` runs once, behind every
// member's devcollect_begin, on the launch stream.
struct DcwCall {
    fsrl_ctx** ctxs; fsrl_devenv** envs; int k; const int32_t* n_episode;
    bool layered, grouped;
    int (*prepare)(DcwCall& w, hipStream_t s);
    int (*launch)(DcwCall& w, bool first, bool settle);      // every member's wide_t moves on by one
    DcActor actor[FSRL_MAX_GROUP];
    int grid, j;                // workgroups of a step launch; launches of this call so far
};
static int devcollect_wide_solo_launch(DcwCall& w, bool first, bool settle) {
    ++w.j;
    return (w.layered ? devcollect_wide_layered_launch : devcollect_wide_launch)(w.ctxs[0], w.envs[0], w.actor[0], w.grid, first, settle);
}

// The batch loop of every wide collect.  A batch is S step launches and one settle launch, enqueued without waiting on member 0's
// compute stream (the members' uploads are put in front of it as in devcollect_group_run); then every member's settled scalars come
// back -- the one member's from its DcwState, a group's in one copy of the block the settle launch gathered them in -- each member's
// log rows follow, and each member is replayed with devcollect_replay.  The loop ends when every member has finished.
static int devcollect_wide_run(DcwCall& w, int32_t deterministic, int32_t bound_method, const float* act_low, const float* act_high, int S,
                               const DcGroupOut& o) {
    const int k = w.k, Da = w.envs[0]->cfg.act_dim;
    fsrl_ctx** ctxs = w.ctxs; fsrl_devenv** envs = w.envs; const int32_t* n_episode = w.n_episode;
    const char* const what = w.grouped ? "grouped wide device collect" : "wide device collect";
    const auto who = [&](int i) { return w.grouped ? " (member " + std::to_string(i) + ")" : std::string(); };
    // a failure at member i leaves members 0 .. i - 1 entered (resident actors ended, windows landed, state uploaded), as in
    // devcollect_group_run: entering is what every collect does first and moves no store, env or ordinal
    for (int i = 0; i < k; ++i) {
        const int rc = devcollect_begin(ctxs[i], envs[i], n_episode[i], deterministic, bound_method, act_low ? act_low + (size_t)i * Da : nullptr,
                                        act_high ? act_high + (size_t)i * Da : nullptr, S, &w.actor[i], true, w.layered, true);
        if (rc) return rc;
        if (w.actor[i].head != w.actor[0].head) return fail(FSRL_ESTATE, "member %d: its actor's head kind changed under the call", i);
    }
    hipStream_t s = ctxs[0]->compute;
    for (int i = 1; i < k; ++i) {
        if (ctxs[i]->compute == s) continue;           // members of one fsrl_group share a stream
        if (!envs[i]->g_ready) HIPCHK(hipEventCreateWithFlags(&envs[i]->g_ready, hipEventDisableTiming));
        HIPCHK(hipEventRecord(envs[i]->g_ready, ctxs[i]->compute));
        HIPCHK(hipStreamWaitEvent(s, envs[i]->g_ready, 0));
    }
    w.grid = (dc_first_live(envs[0]->cfg.env_num, n_episode[0]) + 15) / 16;       // fixed for the collect: the live set only shrinks
    w.j = 0;
    int rc = w.prepare ? w.prepare(w, s) : 0;
    if (rc) return rc;
    int32_t mes[FSRL_MAX_GROUP] = {}, steps[FSRL_MAX_GROUP] = {};
    for (int i = 0; i < k; ++i) mes[i] = envs[i]->cfg.max_episode_steps;
    const int64_t batch_cap = dc_group_launch_cap(n_episode, mes, k, S);
    int64_t off[FSRL_MAX_GROUP + 1];
    dc_group_offsets(n_episode, k, off);
    DcTotals t[FSRL_MAX_GROUP];
    DcwScalars hs[FSRL_MAX_GROUP] = {};
    uint8_t finished[FSRL_MAX_GROUP] = {}, was_finished[FSRL_MAX_GROUP] = {};
    int32_t launches = 0, batches = 0;
    const auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_begin = now();
    double t_replay[FSRL_MAX_GROUP] = {};
    for (;;) {
        if (batches >= batch_cap) {
            int i = 0;
            while (i + 1 < k && finished[i]) ++i;
            return fail(FSRL_ESTATE, "%s: %d batches of %d launches did not finish %d episodes%s", what, batches, S, n_episode[i], who(i).c_str());
        }
        for (int j = 0; j < S; ++j) {
            rc = w.launch(w, j == 0, false);
            if (rc) return rc;
        }
        rc = w.launch(w, false, true);
        if (rc) return rc;
        launches += S + 1; ++batches;
        if (w.grouped) {
            HIPCHK(hipMemcpyAsync(envs[0]->h_wgs, envs[0]->d_wgs, (size_t)k * sizeof(DcwScalars), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            for (int i = 0; i < k; ++i) hs[i] = envs[0]->h_wgs[i];
        } else {
            HIPCHK(hipMemcpyAsync(&envs[0]->h_wstate->s[0], &envs[0]->d_wstate->s[envs[0]->wide_t & 1], sizeof(DcwScalars), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            hs[0] = envs[0]->h_wstate->s[0];
        }
        bool any_rows = false;
        for (int i = 0; i < k; ++i) {
            const int n = envs[i]->cfg.env_num;
            DcState rs{};
            rs.log_rows = hs[i].log_rows; rs.steps = hs[i].steps;
            if (!devcollect_state_sane(rs, S, n) || hs[i].pending || hs[i].n_live < 0 || hs[i].n_live > n)
                return fail(FSRL_ESTATE, "%s: the kernels reported %d rows in %d steps, %d live%s", what, hs[i].log_rows, hs[i].steps, hs[i].n_live,
                            who(i).c_str());
            if (finished[i] && (hs[i].steps != 0 || hs[i].log_rows != 0))
                return fail(FSRL_ESTATE, "%s: member %d was finished and its tiles reported %d rows in %d steps", what, i, hs[i].log_rows, hs[i].steps);
            if (hs[i].log_rows > 0) {
                HIPCHK(hipMemcpyAsync(envs[i]->h_log, envs[i]->d_log, (size_t)hs[i].log_rows * sizeof(DcLogRow), hipMemcpyDeviceToHost, s));
                any_rows = true;
            }
        }
        if (any_rows) HIPCHK(hipStreamSynchronize(s));
        for (int i = 0; i < k; ++i) {
            const double t_r = now();
            DcState rs{};           // what devcollect_replay reads of a launch's state
            rs.log_rows = hs[i].log_rows; rs.steps = hs[i].steps;
            rc = devcollect_replay(ctxs[i], envs[i], rs, n_episode[i], t[i], o.ep_rew + off[i], o.ep_len + off[i], true);
            t_replay[i] += now() - t_r;
            if (rc) { if (w.grouped) g_err = "member " + std::to_string(i) + ": " + g_err; return rc; }
            was_finished[i] = finished[i]; steps[i] = hs[i].steps; finished[i] = hs[i].finished ? 1 : 0;
        }
        if (dc_group_complete(finished, k)) break;
        for (int i = 0; i < k; ++i)         // unfinished going in, no step, and still unfinished: the next batch would do the same
            if (!was_finished[i] && steps[i] == 0 && !finished[i])
                return fail(FSRL_ESTATE, "%s: a batch of launches made no step%s", what, who(i).c_str());
    }
    for (int i = 0; i < k; ++i)
        if (t[i].episodes != hs[i].episodes)
            return fail(FSRL_ESTATE, "%s: the log holds %d episodes, the kernels counted %d%s", what, t[i].episodes, hs[i].episodes, who(i).c_str());
    // FastCollector.reset_env at the end of every collect: ALL envs of ALL members, then one wait
    for (int i = 0; i < k; ++i) {
        DevEnvIo io{};
        io.n = envs[i]->cfg.env_num;
        rc = devenv_reset_launch(envs[i], io, s);
        if (rc) return rc;
    }
    HIPCHK(hipStreamSynchronize(s));
    const double t_all = now() - t_begin;
    for (int i = 0; i < k; ++i) {
        o.steps[i] = t[i].rows; o.total_cost[i] = t[i].total_cost; o.terms[i] = t[i].terms; o.truncs[i] = t[i].truncs;
        o.episodes[i] = std::min(t[i].episodes, n_episode[i]);
        envs[i]->wide_seconds[0] = t_all; envs[i]->wide_seconds[1] = t_replay[i];
    }
    if (o.launches) *o.launches = launches;
    return 0;
}

// the last wide collect of `v` on the host's clock: out[0] seconds from the first launch to the end, out[1] of them in the log replay
extern "C" int fsrl_collect_device_wide_timing(fsrl_devenv* v, double* out) {
    CHECK_ARG(v && out, "null argument");
    out[0] = v->wide_seconds[0]; out[1] = v->wide_seconds[1];
    return 0;
}

static int devcollect_wide_call(fsrl_ctx* c, fsrl_devenv* v, int32_t n_episode, int32_t deterministic, int32_t bound_method, const float* act_low,
                                const float* act_high, int32_t max_steps_per_launch, const DcGroupOut& o, bool layered) {
    // ---- every refusal before anything is touched
    CHECK_ARG(c && v, "null context / env");
    int rc = devcollect_check(c, v, n_episode, bound_method, act_low, act_high, max_steps_per_launch, false, true, layered, true);
    if (rc) return rc;
    CHECK_ARG(o.steps && o.total_cost && o.terms && o.truncs && o.ep_rew && o.ep_len && o.episodes, "null output");
    const int S = dc_wide_batch_steps(v->cfg.env_num, max_steps_per_launch);
    HIPCHK(hipSetDevice(c->device));
    pactor_release(c);
    DcwCall w{};
    w.ctxs = &c; w.envs = &v; w.k = 1; w.n_episode = &n_episode; w.layered = layered; w.launch = devcollect_wide_solo_launch;
    rc = devcollect_wide_run(w, deterministic, bound_method, act_low, act_high, S, o);
    if (rc) {       // leave nothing of the call in flight
        const std::string why = g_err;
        (void)hipStreamSynchronize(c->compute);
        g_err = why;
    }
    return rc;
}
extern "C" int fsrl_collect_device_wide(fsrl_ctx* c, fsrl_devenv* v, int32_t n_episode, int32_t deterministic, int32_t bound_method,
                                        const float* act_low, const float* act_high, int32_t max_steps_per_launch, int64_t* steps_out,
                                        double* total_cost_out, int32_t* term_count_out, int32_t* trunc_count_out, double* ep_rew_out,
                                        int32_t* ep_len_out, int32_t* episodes_out, int32_t* launches_out) {
    const DcGroupOut o{steps_out, total_cost_out, term_count_out, trunc_count_out, ep_rew_out, ep_len_out, episodes_out, launches_out};
    return devcollect_wide_call(c, v, n_episode, deterministic, bound_method, act_low, act_high, max_steps_per_launch, o, false);
}
// the wide collect of a LAYERED context: the same call around wide_layered_step_kernel
extern "C" int fsrl_collect_device_wide_layered(fsrl_ctx* c, fsrl_devenv* v, int32_t n_episode, int32_t deterministic, int32_t bound_method,
                                                const float* act_low, const float* act_high, int32_t max_steps_per_launch, int64_t* steps_out,
                                                double* total_cost_out, int32_t* term_count_out, int32_t* trunc_count_out, double* ep_rew_out,
                                                int32_t* ep_len_out, int32_t* episodes_out, int32_t* launches_out) {
    const DcGroupOut o{steps_out, total_cost_out, term_count_out, trunc_count_out, ep_rew_out, ep_len_out, episodes_out, launches_out};
    return devcollect_wide_call(c, v, n_episode, deterministic, bound_method, act_low, act_high, max_steps_per_launch, o, true);
}
