// host_deveval_wide_group.inc -- fsrl_evaluate_device_wide_group: k members' wide device evaluations, ONE launch per vector step for
// all of them (part of fsrl_hip.hip, behind host_deveval_wide.inc; kernels_deveval_wide_group.hpp; include/fsrl_hip.h "Device
// environments").
//
// A solo wide evaluation occupies ceil(env_num / 16) compute units for a dependent chain of launches; k of them one after the other
// pay that chain k times.  Here the members' tiles are the workgroups of one grid, laid end to end (wide_eval_group_step_kernel /
// wide_eval_layered_group_step_kernel; WideEvalGroupTable: tile prefix, each member's WideEvalArgs, parameters or actor row, launch
// ordinal parity).  The checks per member are the solo wide evaluation's (devcollect_check, store = false, wide = true), what the
// members must agree on is what fsrl_collect_device_group asks (devcollect_group_agree), and the batch loop and the read-back are
// deveval_wide_run with the grouped launch: S = max_steps_per_launch step launches (no log caps it) and one settle launch of k
// workgroups that gathers the members' settled scalars in one block.  Members may sit in any kind of group or in none, with a tap,
// prioritised replay or more envs than sub-buffers; the launches go on member 0's compute stream, behind every member's own stream
// as the call found it.  All members are fused or all layered.
static int deveval_wide_group_prepare(DcwCall& w, hipStream_t s) {
    fsrl_devenv* v0 = w.envs[0];
    if (!v0->d_wegtab) HIPCHK(v0->mem.dev(&v0->d_wegtab, sizeof(WideEvalGroupTable)));
    if (!v0->h_wegtab) HIPCHK(v0->mem.pinned(&v0->h_wegtab, sizeof(WideEvalGroupTable)));
    if (!v0->d_wgs) HIPCHK(v0->mem.dev(&v0->d_wgs, FSRL_MAX_GROUP * sizeof(DcwScalars)));
    if (!v0->h_wgs) HIPCHK(v0->mem.pinned(&v0->h_wgs, FSRL_MAX_GROUP * sizeof(DcwScalars)));
    WideEvalGroupTable& tb = *v0->h_wegtab;
    tb = WideEvalGroupTable{};
    int32_t env_num[FSRL_MAX_GROUP];
    for (int i = 0; i < w.k; ++i) {
        env_num[i] = w.envs[i]->cfg.env_num;
        tb.par0[i] = (int32_t)(w.envs[i]->wide_t & 1u);           // a launch reads its ordinal's parity alone
        tb.wa[i] = w.envs[i]->d_weargs;
        tb.P[i] = w.actor[i].P;
        tb.la[i] = w.layered ? w.envs[i]->d_wlact : nullptr;
    }
    w.grid = dc_wgroup_prefix(env_num, w.n_episode, w.k, tb.prefix);
    HIPCHK(hipMemcpyAsync(v0->d_wegtab, v0->h_wegtab, sizeof(WideEvalGroupTable), hipMemcpyHostToDevice, s));
    return 0;
}

static int deveval_wide_group_launch(DcwCall& w, bool first, bool settle) {
    fsrl_ctx* c0 = w.ctxs[0]; fsrl_devenv* v0 = w.envs[0];
    hipStream_t s = c0->compute;
    const int head = w.actor[0].head, j = w.j, fi = first ? 1 : 0, se = settle ? 1 : 0;
    const WideEvalGroupTable* tab = v0->d_wegtab;
    DcwScalars* gs = v0->d_wgs;
    const dim3 g((unsigned)(settle ? w.k : w.grid));
    int rc = 0;
    if (w.layered) {
        const bool devws = v0->h_wlact->ws != nullptr;          // one hidden_sizes: one form and one LDS size for the launch
        const size_t lds = settle ? 0 : (size_t)dc_wl_lds_bytes(v0->h_wlact->ld);
        devenv_dispatch(v0->cfg.kind, [&](auto env) {
            using Env = decltype(env);
#define WEG_GO(HEAD_) (devws ? devcollect_wide_layered_go<&wide_eval_layered_group_step_kernel<Env, HEAD_, true>>(c0->device, g, lds, s, tab, gs, j, fi, se) \
                             : devcollect_wide_layered_go<&wide_eval_layered_group_step_kernel<Env, HEAD_, false>>(c0->device, g, lds, s, tab, gs, j, fi, se))
            rc = head == DC_HEAD_GAUSS ? WEG_GO(DC_HEAD_GAUSS) : head == DC_HEAD_DDPG ? WEG_GO(DC_HEAD_DDPG) : WEG_GO(DC_HEAD_ONPOLICY);
#undef WEG_GO
        });
    } else {
        const ModelDesc mdv = *w.actor[0].md;
        rc = dispatch_H(c0->cfg.hidden, [&](auto hc) {
            constexpr int H = decltype(hc)::value;
            devenv_dispatch(v0->cfg.kind, [&](auto env) {
                using Env = decltype(env);
                if (head == DC_HEAD_GAUSS) hipLaunchKernelGGL((wide_eval_group_step_kernel<H, Env, DC_HEAD_GAUSS>), g, dim3(4 * H), 0, s, mdv, tab, gs, j, fi, se);
                else if (head == DC_HEAD_DDPG) hipLaunchKernelGGL((wide_eval_group_step_kernel<H, Env, DC_HEAD_DDPG>), g, dim3(4 * H), 0, s, mdv, tab, gs, j, fi, se);
                else hipLaunchKernelGGL((wide_eval_group_step_kernel<H, Env, DC_HEAD_ONPOLICY>), g, dim3(4 * H), 0, s, mdv, tab, gs, j, fi, se);
            });
            HIPCHK(hipGetLastError());
            return 0;
        });
    }
    ++w.j;
    for (int i = 0; i < w.k; ++i) ++w.envs[i]->wide_t;         // launches behind a member's finished evaluation count too: they hand its state on
    return rc;
}

extern "C" int fsrl_evaluate_device_wide_group(fsrl_ctx** ctxs, fsrl_devenv** envs, int32_t k, const int32_t* n_episode, int32_t deterministic,
                                               int32_t bound_method, const float* act_low, const float* act_high, int32_t max_steps_per_launch,
                                               int64_t* steps_out, double* total_cost_out, int32_t* term_count_out, int32_t* trunc_count_out,
                                               double* ep_rew_out, int32_t* ep_len_out, int32_t* episodes_out, int32_t* launches_out) {
    const DcGroupOut o{steps_out, total_cost_out, term_count_out, trunc_count_out, ep_rew_out, ep_len_out, episodes_out, launches_out};
    // ---- every refusal before anything is touched
    CHECK_ARG(k >= 1 && k <= FSRL_MAX_GROUP, "k %d: a grouped wide device evaluation has 1..%d members", k, FSRL_MAX_GROUP);
    CHECK_ARG(ctxs && envs && n_episode, "null argument");
    CHECK_ARG(o.steps && o.total_cost && o.terms && o.truncs && o.ep_rew && o.ep_len && o.episodes, "null output");
    CHECK_ARG((act_low == nullptr) == (act_high == nullptr), "act_low and act_high are given together");
    for (int i = 0; i < k; ++i) {
        CHECK_ARG(ctxs[i] && envs[i], "member %d: null context / env", i);
        for (int j = 0; j < i; ++j) {
            CHECK_ARG(ctxs[j] != ctxs[i], "member %d: its context is listed twice (member %d)", i, j);
            CHECK_ARG(envs[j] != envs[i], "member %d: its device env is listed twice (member %d)", i, j);
        }
    }
    const bool layered = ctxs[0]->lay != nullptr;
    for (int i = 1; i < k; ++i)
        CHECK_ARG((ctxs[i]->lay != nullptr) == layered, "member %d is a %s context and member 0 a %s one: a grouped wide device evaluation runs one "
                  "kernel family, its members are all fused or all layered (hidden_sizes)", i, layered ? "fused" : "layered",
                  layered ? "layered" : "fused");
    const int Da0 = ctxs[0]->cfg.act_dim;
    for (int i = 0; i < k; ++i) {
        const int rc = devcollect_check(ctxs[i], envs[i], n_episode[i], bound_method, act_low ? act_low + (size_t)i * Da0 : nullptr,
                                        act_high ? act_high + (size_t)i * Da0 : nullptr, max_steps_per_launch, true, false, layered, true);
        if (rc) { g_err = "member " + std::to_string(i) + ": " + g_err; return rc; }
    }
    for (int i = 1; i < k; ++i) {
        const int rc = devcollect_group_agree(ctxs[i], envs[i], ctxs[0], envs[0], i, layered);
        if (rc) return rc;
    }
    const int S = max_steps_per_launch > 0 ? max_steps_per_launch : DC_DEFAULT_STEPS;
    HIPCHK(hipSetDevice(ctxs[0]->device));
    for (int i = 0; i < k; ++i) pactor_release(ctxs[i]);       // the table's first allocation would wait for a live resident actor's idle timeout
    DcwCall w{};
    w.ctxs = ctxs; w.envs = envs; w.k = k; w.n_episode = n_episode; w.layered = layered; w.grouped = true;
    w.prepare = deveval_wide_group_prepare; w.launch = deveval_wide_group_launch;
    const int rc = deveval_wide_run(w, deterministic, bound_method, act_low, act_high, S, o);
    if (rc) {       // leave nothing of the call in flight: the kernels read every member's arrays from member 0's stream
        const std::string why = g_err;
        (void)hipStreamSynchronize(ctxs[0]->compute);
        g_err = why;
    }
    return rc;
}
