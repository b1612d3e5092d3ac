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
// Not here: evaluations over wide envs, prioritised contexts, grouped wide collects -- refused by name.
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

// the layered launch: one kernel per (env kind, head, form) for every shape; above 64 KB of dynamic LDS the function's limit is raised,
// once per instantiation
template <class Env, int HEAD, bool DEVWS>
static int devcollect_wide_layered_go(int device, const dim3 g, size_t lds, hipStream_t s, const WideCollectArgs* wa, const WideLayActor* la, int t, int fi,
                                      int se) {
    static std::atomic<uint64_t> raised{0};         // a bit per device (the attribute belongs to the function on the current device)
    if (lds > 64 * 1024 && !(raised.load() >> (device & 63) & 1ull)) {
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&wide_layered_step_kernel<Env, HEAD, DEVWS>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)dc_wl_lds_bytes(DCWL_LDS_WIDTH)));
        raised.fetch_or(1ull << (device & 63));
    }
    hipLaunchKernelGGL((wide_layered_step_kernel<Env, HEAD, DEVWS>), g, dim3(WL_NT), lds, s, wa, la, t, fi, se);
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
#define WL_GO(HEAD_) (devws ? devcollect_wide_layered_go<Env, HEAD_, true>(c->device, g, lds, s, wa, la, t, fi, se) \
                            : devcollect_wide_layered_go<Env, HEAD_, false>(c->device, g, lds, s, wa, la, t, fi, se))
        rc = head == DC_HEAD_GAUSS ? WL_GO(DC_HEAD_GAUSS) : head == DC_HEAD_DDPG ? WL_GO(DC_HEAD_DDPG) : WL_GO(DC_HEAD_ONPOLICY);
#undef WL_GO
    });
    ++v->wide_t;
    return rc;
}

// one launch of a batch: devcollect_wide_launch, or the layered one
typedef int (*DcwLaunch)(fsrl_ctx* c, fsrl_devenv* v, const DcActor& actor, int grid, bool first, bool settle);
static int devcollect_wide_run(fsrl_ctx* c, fsrl_devenv* v, int32_t n_episode, int32_t deterministic, int32_t bound_method, const float* act_low,
                               const float* act_high, int S, const DcGroupOut& o, bool layered, DcwLaunch launch) {
    const int n = v->cfg.env_num;
    DcActor actor{};
    int rc = devcollect_begin(c, v, n_episode, deterministic, bound_method, act_low, act_high, S, &actor, true, layered, true);
    if (rc) return rc;
    hipStream_t s = c->compute;
    const int grid = (dc_first_live(n, n_episode) + 15) / 16;       // fixed for the collect: the live set only shrinks
    const int64_t batch_cap = dc_launch_cap(n_episode, v->cfg.max_episode_steps, S);
    DcTotals t;
    int32_t launches = 0, batches = 0;
    DcwScalars hs{};
    const auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_begin = now();
    double t_replay = 0.0;
    for (;;) {
        if (batches >= batch_cap) return fail(FSRL_ESTATE, "wide device collect: %d batches of %d launches did not finish %d episodes", batches, S, n_episode);
        for (int j = 0; j < S; ++j) {
            rc = launch(c, v, actor, grid, j == 0, false);
            if (rc) return rc;
        }
        rc = launch(c, v, actor, grid, false, true);
        if (rc) return rc;
        launches += S + 1; ++batches;
        HIPCHK(hipMemcpyAsync(&v->h_wstate->s[0], &v->d_wstate->s[v->wide_t & 1], sizeof(DcwScalars), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        hs = v->h_wstate->s[0];
        DcState rs{};           // what devcollect_replay reads of a launch's state
        rs.log_rows = hs.log_rows; rs.steps = hs.steps;
        if (!devcollect_state_sane(rs, S, n) || hs.pending || hs.n_live < 0 || hs.n_live > n)
            return fail(FSRL_ESTATE, "wide device collect: the kernels reported %d rows in %d steps, %d live", hs.log_rows, hs.steps, hs.n_live);
        if (hs.log_rows > 0) {
            HIPCHK(hipMemcpyAsync(v->h_log, v->d_log, (size_t)hs.log_rows * sizeof(DcLogRow), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        }
        const double t_r = now();
        rc = devcollect_replay(c, v, rs, n_episode, t, o.ep_rew, o.ep_len, true);
        t_replay += now() - t_r;
        if (rc) return rc;
        if (hs.finished) break;
        if (hs.steps == 0) return fail(FSRL_ESTATE, "wide device collect: a batch of launches made no step");
    }
    if (t.episodes != hs.episodes)
        return fail(FSRL_ESTATE, "wide device collect: the log holds %d episodes, the kernels counted %d", t.episodes, hs.episodes);
    // FastCollector.reset_env at the end of every collect
    DevEnvIo io{};
    io.n = n;
    rc = devenv_reset_launch(v, io, s);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(s));
    o.steps[0] = t.rows; o.total_cost[0] = t.total_cost; o.terms[0] = t.terms; o.truncs[0] = t.truncs;
    o.episodes[0] = std::min(t.episodes, n_episode);
    if (o.launches) *o.launches = launches;
    v->wide_seconds[0] = now() - t_begin; v->wide_seconds[1] = t_replay;
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
    rc = devcollect_wide_run(c, v, n_episode, deterministic, bound_method, act_low, act_high, S, o, layered,
                             layered ? devcollect_wide_layered_launch : devcollect_wide_launch);
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
