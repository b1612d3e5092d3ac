// host_deveval_wide.inc -- fsrl_evaluate_device_wide / fsrl_evaluate_device_wide_layered: the device evaluation over a wide env,
// 1 .. DCW_MAX_ENVS envs (part of fsrl_hip.hip, behind host_devcollect_wide.inc; kernels_deveval_wide.hpp; include/fsrl_hip.h
// "Device environments").
//
// The launch scheme is the wide collect's: a BATCH is S step launches (wide_eval_step_kernel, or wide_eval_layered_step_kernel on a
// layered context) and one one-workgroup settle launch, enqueued without waiting.  What comes back is not: an evaluation stores
// nothing, so there is no log of step rows to read and replay.  The kernels accumulate every env's running episode on the device and
// leave the finished episodes as rows of an episode log in the collector's order; per batch the host reads the settled DcwScalars
// (32 bytes) and nothing else, and behind the last batch n_episode rows of 24 bytes, once.
// The checks and the entry are devcollect_check / devcollect_begin with store = false, wide = true: valid on a member of any group,
// with a trajectory tap attached, with more envs than the store has sub-buffers and on a prioritised context; the staging window,
// the books, the sampler and the engine's random streams do not move.  The env's state, steps and reset ordinals move as under a
// collect.  S is max_steps_per_launch (default DC_DEFAULT_STEPS, at most DC_MAX_STEPS): without a log, no log cap cuts it.
// "finished", "a batch made no step" and the batch cap are the wide collect's rules.
// k members' evaluations in one launch per step are fsrl_evaluate_device_wide_group (host_deveval_wide_group.inc, behind this file): the
// same batch loop, deveval_wide_run, with the grouped kernels in the launch and one copy of k x 32 bytes per batch.
static int deveval_wide_launch(fsrl_ctx* c, fsrl_devenv* v, const DcActor& actor, int grid, bool layered, bool first, bool settle) {
    hipStream_t s = c->compute;
    const int head = actor.head, t = (int)(v->wide_t & 0x7FFFFFFFu), fi = first ? 1 : 0, se = settle ? 1 : 0;
    const WideEvalArgs* wa = v->d_weargs;
    const dim3 g((unsigned)(settle ? 1 : grid));
    int rc = 0;
    if (layered) {
        const WideLayActor* la = v->d_wlact;
        const bool devws = v->h_wlact->ws != nullptr;
        const size_t lds = settle ? 0 : (size_t)dc_wl_lds_bytes(v->h_wlact->ld);       // the settle launch touches no activation
        devenv_dispatch(v->cfg.kind, [&](auto env) {
            using Env = decltype(env);
#define WE_GO(HEAD_) (devws ? devcollect_wide_layered_go<&wide_eval_layered_step_kernel<Env, HEAD_, true>>(c->device, g, lds, s, wa, la, t, fi, se) \
                            : devcollect_wide_layered_go<&wide_eval_layered_step_kernel<Env, HEAD_, false>>(c->device, g, lds, s, wa, la, t, fi, se))
            rc = head == DC_HEAD_GAUSS ? WE_GO(DC_HEAD_GAUSS) : head == DC_HEAD_DDPG ? WE_GO(DC_HEAD_DDPG) : WE_GO(DC_HEAD_ONPOLICY);
#undef WE_GO
        });
    } else {
        const ModelDesc mdv = *actor.md;
        const float* P = actor.P;
        rc = dispatch_H(c->cfg.hidden, [&](auto hc) {
            constexpr int H = decltype(hc)::value;
            devenv_dispatch(v->cfg.kind, [&](auto env) {
                using Env = decltype(env);
                if (head == DC_HEAD_GAUSS) hipLaunchKernelGGL((wide_eval_step_kernel<H, Env, DC_HEAD_GAUSS>), g, dim3(4 * H), 0, s, mdv, P, wa, t, fi, se);
                else if (head == DC_HEAD_DDPG) hipLaunchKernelGGL((wide_eval_step_kernel<H, Env, DC_HEAD_DDPG>), g, dim3(4 * H), 0, s, mdv, P, wa, t, fi, se);
                else hipLaunchKernelGGL((wide_eval_step_kernel<H, Env, DC_HEAD_ONPOLICY>), g, dim3(4 * H), 0, s, mdv, P, wa, t, fi, se);
            });
            HIPCHK(hipGetLastError());
            return 0;
        });
    }
    ++v->wide_t;
    return rc;
}

// One wide evaluation call is a DcwCall (host_devcollect_wide.inc): k members (the solo calls: one, unnamed) and how a launch of a
// batch goes out for all of them -- the solo kernels on the one member, or the grouped kernels over the evaluations' member table
// (host_deveval_wide_group.inc).
static int deveval_wide_solo_launch(DcwCall& w, bool first, bool settle) {
    ++w.j;
    return deveval_wide_launch(w.ctxs[0], w.envs[0], w.actor[0], w.grid, w.layered, first, settle);
}

// The batch loop of every wide evaluation.  Per member: devcollect_begin on its own compute stream, and behind it the zeroing of its
// running episodes, park and episode log and the upload of its WideEvalArgs.  The launches go on member 0's compute stream, behind
// every other member's stream by one event per member, once per call.  A batch is S step launches and one settle launch, enqueued
// without waiting; then every member's settled scalars come back -- the one member's from its DcwState, a group's in one copy of the
// block the settle launch gathered them in -- and nothing else.  The loop ends when every member has finished; then each member's
// n_episode rows come back, every env of every member is reset, and one wait ends the call.
static int deveval_wide_run(DcwCall& w, int32_t deterministic, int32_t bound_method, const float* act_low, const float* act_high, int S,
                            const DcGroupOut& o) {
    const int k = w.k, Da = w.envs[0]->cfg.act_dim;
    fsrl_ctx** ctxs = w.ctxs; fsrl_devenv** envs = w.envs; const int32_t* n_episode = w.n_episode;
    const char* const what = w.grouped ? "grouped wide device evaluation" : "wide device evaluation";
    const auto who = [&](int i) { return w.grouped ? " (member " + std::to_string(i) + ")" : std::string(); };
    // a failure at member i leaves members 0 .. i - 1 entered, as in devcollect_wide_run: entering moves no env and no ordinal
    for (int i = 0; i < k; ++i) {
        fsrl_devenv* v = envs[i];
        const int rc = devcollect_begin(ctxs[i], v, n_episode[i], deterministic, bound_method, act_low ? act_low + (size_t)i * Da : nullptr,
                                        act_high ? act_high + (size_t)i * Da : nullptr, S, &w.actor[i], false, w.layered, true);
        if (rc) return rc;
        if (w.actor[i].head != w.actor[0].head) return fail(FSRL_ESTATE, "member %d: its actor's head kind changed under the call", i);
        // the running episodes, the park and the episode log belong to the env; zeroed on entry, behind the last call's launches
        hipStream_t si = ctxs[i]->compute;
        if (!v->d_weval) HIPCHK(v->mem.dev(&v->d_weval, sizeof(DcwEval)));
        if (!v->d_weargs) HIPCHK(v->mem.dev(&v->d_weargs, sizeof(WideEvalArgs)));
        if (!v->h_weargs) HIPCHK(v->mem.pinned(&v->h_weargs, sizeof(WideEvalArgs)));
        HIPCHK(v->mem.regrow(v->eplog_rows, n_episode[i], n_episode[i], {Mem::D(&v->d_eplog, (size_t)n_episode[i] * sizeof(DcEpisodeRow)),
                             Mem::H(&v->h_eplog, (size_t)n_episode[i] * sizeof(DcEpisodeRow))}));
        HIPCHK(hipMemsetAsync(v->d_weval, 0, sizeof(DcwEval), si));
        HIPCHK(hipMemsetAsync(v->d_eplog, 0, (size_t)n_episode[i] * sizeof(DcEpisodeRow), si));
        WideEvalArgs& wa = *v->h_weargs;
        wa.a = v->h_wargs->a; wa.ws = v->d_wstate; wa.ev = v->d_weval; wa.ep_log = v->d_eplog;
        HIPCHK(hipMemcpyAsync(v->d_weargs, v->h_weargs, sizeof(WideEvalArgs), hipMemcpyHostToDevice, si));
    }
    hipStream_t s = ctxs[0]->compute;
    for (int i = 1; i < k; ++i) {
        if (ctxs[i]->compute == s) continue;           // members of one fsrl_group share a stream
        if (!envs[i]->g_ready) HIPCHK(hipEventCreateWithFlags(&envs[i]->g_ready, hipEventDisableTiming));
        HIPCHK(hipEventRecord(envs[i]->g_ready, ctxs[i]->compute));
        HIPCHK(hipStreamWaitEvent(s, envs[i]->g_ready, 0));
    }
    w.grid = dc_wide_tiles(envs[0]->cfg.env_num, n_episode[0]);       // fixed for the call: the live set only shrinks
    w.j = 0;
    int rc = w.prepare ? w.prepare(w, s) : 0;
    if (rc) return rc;
    int32_t mes[FSRL_MAX_GROUP] = {}, steps[FSRL_MAX_GROUP] = {};
    for (int i = 0; i < k; ++i) mes[i] = envs[i]->cfg.max_episode_steps;
    const int64_t batch_cap = dc_group_launch_cap(n_episode, mes, k, S);       // the largest member's dc_launch_cap
    int64_t off[FSRL_MAX_GROUP + 1];
    dc_group_offsets(n_episode, k, off);
    DcwScalars hs[FSRL_MAX_GROUP] = {};
    int64_t rows[FSRL_MAX_GROUP] = {};
    uint8_t finished[FSRL_MAX_GROUP] = {}, was_finished[FSRL_MAX_GROUP] = {};
    int32_t launches = 0, batches = 0;
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
        for (int i = 0; i < k; ++i) {
            const int n = envs[i]->cfg.env_num;
            const DcwScalars& h = hs[i];
            if (h.steps < 0 || h.steps > S || h.log_rows < 0 || (int64_t)h.log_rows > (int64_t)S * n || h.pending || h.n_live < 0 || h.n_live > n ||
                h.episodes < 0 || h.episodes > n_episode[i])
                return fail(FSRL_ESTATE, "%s: the kernels reported %d rows in %d steps, %d live, %d episodes%s", what, h.log_rows, h.steps, h.n_live,
                            h.episodes, who(i).c_str());
            if (finished[i] && (h.steps != 0 || h.log_rows != 0))
                return fail(FSRL_ESTATE, "%s: member %d was finished and its tiles reported %d rows in %d steps", what, i, h.log_rows, h.steps);
            rows[i] += h.log_rows;
            was_finished[i] = finished[i]; steps[i] = h.steps; finished[i] = h.finished ? 1 : 0;
        }
        if (dc_group_complete(finished, k)) break;
        // unfinished going in and no step: the next batch would do the same (every batch ends settled, so an unfinished member's
        // first launch has nothing pending and steps)
        const int stalled = dc_group_stalled(was_finished, steps, k);
        if (stalled >= 0) return fail(FSRL_ESTATE, "%s: a batch of launches made no step%s", what, who(stalled).c_str());
    }
    // the episodes, once; every env of every member is reset behind them (FastCollector.reset_env at the end of every collect)
    for (int i = 0; i < k; ++i) {
        HIPCHK(hipMemcpyAsync(envs[i]->h_eplog, envs[i]->d_eplog, (size_t)n_episode[i] * sizeof(DcEpisodeRow), hipMemcpyDeviceToHost, s));
        DevEnvIo io{};
        io.n = envs[i]->cfg.env_num;
        rc = devenv_reset_launch(envs[i], io, s);
        if (rc) return rc;
    }
    HIPCHK(hipStreamSynchronize(s));
    for (int i = 0; i < k; ++i) {
        if (hs[i].episodes != n_episode[i])
            return fail(FSRL_ESTATE, "%s: the episode log holds %d episodes, the kernels counted %d%s", what, n_episode[i], hs[i].episodes, who(i).c_str());
        DcTotals t;
        for (int e = 0; e < n_episode[i]; ++e) {
            const DcEpisodeRow& r = envs[i]->h_eplog[e];
            if (r.len < 1 || r.flags == 0u || r.flags > 3u)
                return fail(FSRL_ESTATE, "%s: episode row %d has length %d and flags %u%s", what, e, r.len, r.flags, who(i).c_str());
            o.ep_rew[off[i] + e] = r.rew; o.ep_len[off[i] + e] = r.len;
            t.rows += r.len; t.total_cost += r.cost;
            t.terms += (int32_t)(r.flags & 1u); t.truncs += (int32_t)((r.flags >> 1) & 1u);
        }
        if (t.rows != rows[i])
            return fail(FSRL_ESTATE, "%s: the episode log holds %lld steps, the kernels counted %lld%s", what, (long long)t.rows, (long long)rows[i],
                        who(i).c_str());
        o.steps[i] = rows[i]; o.total_cost[i] = t.total_cost; o.terms[i] = t.terms; o.truncs[i] = t.truncs; o.episodes[i] = n_episode[i];
    }
    if (o.launches) *o.launches = launches;
    return 0;
}

static int deveval_wide_call(fsrl_ctx* c, fsrl_devenv* v, int32_t n_episode, int32_t deterministic, int32_t bound_method, const float* act_low,
                             const float* act_high, int32_t max_steps_per_launch, const DcGroupOut& o, bool layered) {
    // ---- every refusal before anything is touched
    CHECK_ARG(c && v, "null context / env");
    int rc = devcollect_check(c, v, n_episode, bound_method, act_low, act_high, max_steps_per_launch, false, false, layered, true);
    if (rc) return rc;
    CHECK_ARG(o.steps && o.total_cost && o.terms && o.truncs && o.ep_rew && o.ep_len && o.episodes, "null output");
    const int S = max_steps_per_launch > 0 ? max_steps_per_launch : DC_DEFAULT_STEPS;
    HIPCHK(hipSetDevice(c->device));
    pactor_release(c);
    DcwCall w{};
    w.ctxs = &c; w.envs = &v; w.k = 1; w.n_episode = &n_episode; w.layered = layered; w.launch = deveval_wide_solo_launch;
    rc = deveval_wide_run(w, deterministic, bound_method, act_low, act_high, S, o);
    if (rc) {       // leave nothing of the call in flight
        const std::string why = g_err;
        (void)hipStreamSynchronize(c->compute);
        g_err = why;
    }
    return rc;
}
extern "C" int fsrl_evaluate_device_wide(fsrl_ctx* c, fsrl_devenv* v, int32_t n_episode, int32_t deterministic, int32_t bound_method,
                                         const float* act_low, const float* act_high, int32_t max_steps_per_launch, int64_t* steps_out,
                                         double* total_cost_out, int32_t* term_count_out, int32_t* trunc_count_out, double* ep_rew_out,
                                         int32_t* ep_len_out, int32_t* episodes_out, int32_t* launches_out) {
    const DcGroupOut o{steps_out, total_cost_out, term_count_out, trunc_count_out, ep_rew_out, ep_len_out, episodes_out, launches_out};
    return deveval_wide_call(c, v, n_episode, deterministic, bound_method, act_low, act_high, max_steps_per_launch, o, false);
}
extern "C" int fsrl_evaluate_device_wide_layered(fsrl_ctx* c, fsrl_devenv* v, int32_t n_episode, int32_t deterministic, int32_t bound_method,
                                                 const float* act_low, const float* act_high, int32_t max_steps_per_launch, int64_t* steps_out,
                                                 double* total_cost_out, int32_t* term_count_out, int32_t* trunc_count_out, double* ep_rew_out,
                                                 int32_t* ep_len_out, int32_t* episodes_out, int32_t* launches_out) {
    const DcGroupOut o{steps_out, total_cost_out, term_count_out, trunc_count_out, ep_rew_out, ep_len_out, episodes_out, launches_out};
    return deveval_wide_call(c, v, n_episode, deterministic, bound_method, act_low, act_high, max_steps_per_launch, o, true);
}
