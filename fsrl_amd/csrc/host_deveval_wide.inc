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

// The batch loop.  Entered: devcollect_begin has uploaded the state and the arguments on the compute stream.
static int deveval_wide_run(fsrl_ctx* c, fsrl_devenv* v, int32_t n_episode, int32_t deterministic, int32_t bound_method, const float* act_low,
                            const float* act_high, int S, bool layered, const DcGroupOut& o) {
    const char* const what = "wide device evaluation";
    const int n = v->cfg.env_num;
    DcActor actor{};
    int rc = devcollect_begin(c, v, n_episode, deterministic, bound_method, act_low, act_high, S, &actor, false, layered, true);
    if (rc) return rc;
    // the running episodes, the park and the episode log belong to the env; zeroed on entry, behind the last call's launches
    hipStream_t s = c->compute;
    if (!v->d_weval) HIPCHK(v->mem.dev(&v->d_weval, sizeof(DcwEval)));
    if (!v->d_weargs) HIPCHK(v->mem.dev(&v->d_weargs, sizeof(WideEvalArgs)));
    if (!v->h_weargs) HIPCHK(v->mem.pinned(&v->h_weargs, sizeof(WideEvalArgs)));
    HIPCHK(v->mem.regrow(v->eplog_rows, n_episode, n_episode, {Mem::D(&v->d_eplog, (size_t)n_episode * sizeof(DcEpisodeRow)),
                         Mem::H(&v->h_eplog, (size_t)n_episode * sizeof(DcEpisodeRow))}));
    HIPCHK(hipMemsetAsync(v->d_weval, 0, sizeof(DcwEval), s));
    HIPCHK(hipMemsetAsync(v->d_eplog, 0, (size_t)n_episode * sizeof(DcEpisodeRow), s));
    WideEvalArgs& w = *v->h_weargs;
    w.a = v->h_wargs->a; w.ws = v->d_wstate; w.ev = v->d_weval; w.ep_log = v->d_eplog;
    HIPCHK(hipMemcpyAsync(v->d_weargs, v->h_weargs, sizeof(WideEvalArgs), hipMemcpyHostToDevice, s));
    const int grid = (dc_first_live(n, n_episode) + 15) / 16;       // fixed for the call: the live set only shrinks
    const int64_t batch_cap = dc_launch_cap(n_episode, v->cfg.max_episode_steps, S);
    DcwScalars hs{};
    int64_t rows = 0;
    int32_t launches = 0, batches = 0;
    for (;;) {
        if (batches >= batch_cap) return fail(FSRL_ESTATE, "%s: %d batches of %d launches did not finish %d episodes", what, batches, S, n_episode);
        for (int j = 0; j < S; ++j) {
            rc = deveval_wide_launch(c, v, actor, grid, layered, j == 0, false);
            if (rc) return rc;
        }
        rc = deveval_wide_launch(c, v, actor, grid, layered, false, true);
        if (rc) return rc;
        launches += S + 1; ++batches;
        HIPCHK(hipMemcpyAsync(&v->h_wstate->s[0], &v->d_wstate->s[v->wide_t & 1], sizeof(DcwScalars), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        hs = v->h_wstate->s[0];
        if (hs.steps < 0 || hs.steps > S || hs.log_rows < 0 || (int64_t)hs.log_rows > (int64_t)S * n || hs.pending || hs.n_live < 0 || hs.n_live > n ||
            hs.episodes < 0 || hs.episodes > n_episode)
            return fail(FSRL_ESTATE, "%s: the kernels reported %d rows in %d steps, %d live, %d episodes", what, hs.log_rows, hs.steps, hs.n_live, hs.episodes);
        rows += hs.log_rows;
        if (hs.finished) break;
        if (hs.steps == 0) return fail(FSRL_ESTATE, "%s: a batch of launches made no step", what);
    }
    // the episodes, once; every env is reset behind them (FastCollector.reset_env at the end of every collect)
    HIPCHK(hipMemcpyAsync(v->h_eplog, v->d_eplog, (size_t)n_episode * sizeof(DcEpisodeRow), hipMemcpyDeviceToHost, s));
    DevEnvIo io{};
    io.n = n;
    rc = devenv_reset_launch(v, io, s);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(s));
    if (hs.episodes != n_episode)
        return fail(FSRL_ESTATE, "%s: the episode log holds %d episodes, the kernels counted %d", what, n_episode, hs.episodes);
    DcTotals t;
    for (int i = 0; i < n_episode; ++i) {
        const DcEpisodeRow& r = v->h_eplog[i];
        if (r.len < 1 || r.flags == 0u || r.flags > 3u) return fail(FSRL_ESTATE, "%s: episode row %d has length %d and flags %u", what, i, r.len, r.flags);
        o.ep_rew[i] = r.rew; o.ep_len[i] = r.len;
        t.rows += r.len; t.total_cost += r.cost;
        t.terms += (int32_t)(r.flags & 1u); t.truncs += (int32_t)((r.flags >> 1) & 1u);
    }
    if (t.rows != rows)
        return fail(FSRL_ESTATE, "%s: the episode log holds %lld steps, the kernels counted %lld", what, (long long)t.rows, (long long)rows);
    *o.steps = rows; *o.total_cost = t.total_cost; *o.terms = t.terms; *o.truncs = t.truncs; *o.episodes = n_episode;
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
    rc = deveval_wide_run(c, v, n_episode, deterministic, bound_method, act_low, act_high, S, layered, o);
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
