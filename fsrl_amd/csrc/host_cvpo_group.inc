// host_cvpo_group.inc -- grouped CVPO updates: fsrl_cvpo_group_* (part of fsrl_hip.hip, kernels: kernels_cvpo_group.hpp and the
// shared ones of kernels_sac_group.hpp).
// k CVPO contexts of one launch structure, each stepped n_i times per call in lock step: every launch of an update carries all
// members that still have updates to run (9 + 4 * mstep_iter_num launches per update, whatever k is).  The structure is
// host_sac_group.inc's, and so is the frame of a call (rgroup_begin / rgroup_enter / rgroup_end): members keep their own streams,
// stores, parameters, targets, actor_old, Adam state, duals, Philox key and statistics ring; the group's stream waits on each
// active member's stream before the call and each member's streams wait on the group's completion event after it, so
// fsrl_cvpo_pre_update / _post_update / _set_thres and the member's own updates order against grouped calls like any other work on
// the member's stream.
// A member's arguments are formed by the helpers fsrl_cvpo_update uses (host_cvpo.inc), its arithmetic is the single path's bodies
// with the single path's split-K plan, and the tile height of a launch is the single-context rule applied to the whole group's
// launch: a group of one is bit-identical to its solo run, a group that runs sixteen-row tiles in every launch is bit-identical to
// solo runs created under FSRL_TILE16 (tests/test_gpu_cvpo_group.py).
// A group is all fused or all layered contexts (hidden_sizes of any depth / width).  A layered group runs the launch sequence of the
// member's own layered update, 6 L + 15 + mstep_iter_num (2 L + 6) launches per update for L hidden layers, and is bit-identical
// to it at every k and batch size: host_cvpo_group_layered.inc.
// ====================================================================================== grouped CVPO
struct LayCvpoGroup;
static void lay_cvpo_group_free(LayCvpoGroup* lg);
static int lay_cvpo_group_update(fsrl_cvpo_group* g, int32_t B, const int32_t* n_updates);

struct fsrl_cvpo_group {
    ReplayGroupCore core;                      // members, stream, events (host_sac_group.inc)
    DevTable<SacGroupMember> tab;              // [k]: what the SAC group's kernels read
    DevTable<CvpoGroupMember> ctab;            // [k]: CVPO's own launches
    DevTable<SacGroupStep> steps;              // [updates][k]
    DevTable<CvpoGroupIter> iters;             // [updates][mstep_iter_num][k]
    LayCvpoGroup* lay = nullptr;               // job and head tables of a layered group, made by its first update
};

static void cvpo_group_detach(fsrl_ctx* c) {
    if (!c->cvpo_group) return;
    rgroup_detach(c->cvpo_group->core, c);
    c->cvpo_group = nullptr;
}

extern "C" int fsrl_cvpo_group_destroy(fsrl_cvpo_group* g) {
    if (!g) return 0;
    for (fsrl_ctx* c : g->core.m) if (c) c->cvpo_group = nullptr;
    rgroup_destroy(g->core);
    table_free(g->tab); table_free(g->ctab); table_free(g->steps); table_free(g->iters);
    lay_cvpo_group_free(g->lay);
    delete g;
    return 0;
}

// what decides the launch structure must agree (checked at create and again at every update); `own`: the group the members may
// already belong to (nullptr at create)
static int cvpo_group_check(fsrl_ctx* const* ctxs, int k, const fsrl_cvpo_group* own) {
    const fsrl_ctx* c0 = ctxs[0];
    CHECK_ARG(c0, "null member");
    for (int i = 0; i < k; ++i) {
        const fsrl_ctx* c = ctxs[i];
        CHECK_ARG(c, "null member");
        for (int j = 0; j < i; ++j) CHECK_ARG(ctxs[j] != c, "member %d is listed twice", i);
        const SacState* s = reinterpret_cast<const SacState*>(c->sac);
        CHECK_ARG(c->cfg.algo == FSRL_ALGO_SAC_LAG && s, "member %d: grouped CVPO updates take CVPO contexts (fsrl_cvpo_init)", i);
        CHECK_ARG(!c->per, "member %d has prioritised replay on (fsrl_per_enable): it covers solo SAC-Lagrangian and DDPG-Lagrangian "
                  "contexts only", i);
        CHECK_ARG(!s->ddpg, "member %d is a DDPG-Lagrangian context: grouped CVPO updates take CVPO contexts (fsrl_cvpo_init)", i);
        CHECK_ARG(s->cvpo, "member %d is a SAC-Lagrangian context: grouped CVPO updates take CVPO contexts (fsrl_cvpo_init)", i);
        const SacState* s0 = reinterpret_cast<const SacState*>(c0->sac);
        CHECK_ARG(s->layered == s0->layered, "member %d is a %s context and member 0 a %s one: a group is all fused (two hidden layers of at "
                  "most 256 units) or all layered contexts", i, s->layered ? "layered" : "fused", s0->layered ? "layered" : "fused");
        CHECK_ARG(c->device == c0->device, "member %d: members live on one device", i);
        CHECK_ARG(!c->sac_group, "member %d is already in a SAC group", i);
        CHECK_ARG(c->cvpo_group == own, "member %d is already in a CVPO group", i);
        CHECK_ARG(c->cfg.obs_dim == c0->cfg.obs_dim && c->cfg.act_dim == c0->cfg.act_dim && c->cfg.hidden == c0->cfg.hidden &&
                  (s->layered ? lay_same_shape(c->cfg, c0->cfg) : (c->h1 == c0->h1 && c->h2 == c0->h2)),
                  "member %d: members must have one network shape (obs_dim, act_dim, hidden layer widths; layered: every hidden_sizes[l] "
                  "and force_layered)", i);
        CHECK_ARG(s->ccfg.n_step == s0->ccfg.n_step, "member %d: members must share n_step", i);
        CHECK_ARG((s->ccfg.double_critic != 0) == (s0->ccfg.double_critic != 0), "member %d: members must share double_critic", i);
        CHECK_ARG(s->ccfg.sample_act_num == s0->ccfg.sample_act_num, "member %d: members must share sample_act_num", i);
        CHECK_ARG(s->ccfg.estep_iter_num == s0->ccfg.estep_iter_num, "member %d: members must share estep_iter_num", i);
        CHECK_ARG(s->ccfg.mstep_iter_num == s0->ccfg.mstep_iter_num, "member %d: members must share mstep_iter_num", i);
        CHECK_ARG(s->mean_tanh == s0->mean_tanh, "member %d: members must share actor_mean (the actor's mean is %s, member 0's %s)", i,
                  s->mean_tanh ? "max_action * tanh(head)" : "unbounded", s0->mean_tanh ? "max_action * tanh(head)" : "unbounded");
        // a layered update has one weight-side plan
        CHECK_ARG(s->layered || s->wgrad_splitk == s0->wgrad_splitk,
                  "member %d: members must agree on fsrl_sac_set_plan bit 0 (split-K weight gradients)", i);
    }
    return 0;
}

extern "C" int fsrl_cvpo_group_create(fsrl_ctx** ctxs, int32_t k, fsrl_cvpo_group** out) {
    CHECK_ARG(ctxs && out, "null argument");
    CHECK_ARG(k >= 1 && k <= FSRL_MAX_GROUP, "a CVPO group has 1..%d members", FSRL_MAX_GROUP);
    int rc = cvpo_group_check(ctxs, k, nullptr);
    if (rc) return rc;
    const fsrl_ctx* c0 = ctxs[0];
    HIPCHK(hipSetDevice(c0->device));
    fsrl_cvpo_group* g = new fsrl_cvpo_group();
    hipError_t e = rgroup_create(g->core, c0->device, k);
    if (e != hipSuccess) fail(FSRL_EHIP, "CVPO group allocation failed: %s", hipGetErrorString(e));
    if (e != hipSuccess || table_ensure(g->tab, (size_t)k, (size_t)k) || table_ensure(g->ctab, (size_t)k, (size_t)k)) {
        (void)fsrl_cvpo_group_destroy(g);
        return FSRL_EHIP;
    }
    for (int i = 0; i < k; ++i) { g->core.m.push_back(ctxs[i]); ctxs[i]->cvpo_group = g; }
    *out = g;
    return 0;
}

// the member's entries in both tables: every argument of the update's launches as fsrl_cvpo_update forms it (library RNG, fused
// sample + gather, n-step targets folded into the critics' launch)
struct CvpoGroupTiles { bool q_r4, a_r4, f_r4, k_r4; };
static int cvpo_group_member(fsrl_ctx* c, SacState* s, SacGroupMember& t, CvpoGroupMember& v, int B, const CvpoGroupTiles& th,
                             bool small_wgrad, int* nsplit_q, int* nsplit_a) {
    const int nt = s->n_tiles, K = s->ccfg.sample_act_num;
    const int rc = group_member_base(c, s, t, B, cvpo_nstep_args(c, s, B), s->ccfg.tau, small_wgrad, nsplit_q, nsplit_a);
    if (rc) return rc;
    v = CvpoGroupMember{};
    v.PA = s->PA; v.MA = s->MA; v.VA = s->VA; v.GA = t.GA;
    member_adam_consts(v, c);
    v.ga = sac_gather_args(c, s, B, s->ccfg.n_step);
    v.at = cvpo_actor_args(c, s, B, CVPO_A_TARGET, s->OBSN, s->eps_t, s->XN, true, th.f_r4 ? 4 * nt : nt);
    v.am = cvpo_actor_args(c, s, B, CVPO_A_MFWD, s->OBS, nullptr, nullptr, false, 0);
    v.ab = cvpo_actor_args(c, s, B, CVPO_A_MBWD, s->OBS, nullptr, nullptr, false, 0);
    t.qd = sac_q_args(c, s, s->PQ, s->XK, FB_MODE_Q_FWD, 0.f, 0.f, s->stqk, K * B, s->QK, s->n_tiles_k, nullptr);   // the K * B particles
    v.es = cvpo_estep_args(c, s, B);
    v.md = cvpo_mdual_args(c, s, B, th.a_r4 ? 4 * nt : nt, 0);
    v.fin = cvpo_final_args(c, s, B, th.q_r4 ? 4 * nt : nt, nullptr);
    v.stats = s->d_stats; v.nstats = s->nstats;
    return 0;
}

// the actor's M Adam steps of update u of member i (t_actor advances once per M iteration); zero where the member sits it out
// (s == nullptr).  The fused and the layered update fill their CvpoGroupIter rows here.
static void cvpo_group_iter_rows(fsrl_cvpo_group* g, int u, int i, int k, int M, const fsrl_ctx* c, const SacState* s) {
    for (int it = 0; it < M; ++it) {
        CvpoGroupIter& gi = g->iters.h[((size_t)u * M + it) * k + i];
        gi = CvpoGroupIter{};
        if (!s) continue;
        const AdamStep as = adam_step(s->cfg.actor_lr, c->cfg.beta1, c->cfg.beta2, s->t_actor + (int64_t)u * M + it + 1);
        gi.a_step = as.step_size; gi.a_bc2 = as.bc2_sqrt;
    }
}

extern "C" int fsrl_cvpo_group_update(fsrl_cvpo_group* g, int32_t B, const int32_t* n_updates) {
    CHECK_ARG(g && n_updates, "null argument");
    ReplayGroupCore& gc = g->core;
    if (gc.broken) return fail(FSRL_ESTATE, "a member of this CVPO group was destroyed: destroy the group");
    CHECK_ARG(B >= 1, "batch_size must be >= 1");
    const int k = (int)gc.m.size();
    int rc = cvpo_group_check(gc.m.data(), k, g);
    if (rc) return rc;
    fsrl_ctx* c0 = gc.m[0];
    SacState* s0 = sac_of(c0);
    if (s0->layered) return lay_cvpo_group_update(g, B, n_updates);
    ReplayGroupCall call;
    rc = rgroup_begin(gc, true, n_updates, call, [&](int i, const fsrl_ctx* c, const SacState*) { return rgroup_no_stream_wgrad(i, c, B); });
    if (rc) return rc;
    const int n_max = call.n_max;
    if (n_max == 0) return 0;
    const int H = c0->cfg.hidden, nt = (B + 15) / 16, rp = nt * 16, n_q = s0->n_q;
    const int K = s0->ccfg.sample_act_num, M = s0->ccfg.mstep_iter_num, ntk = (B * K + 15) / 16;
    // tile heights: the single-context rule applied to the group's whole launch (4-row tiles while it fits one round)
    const bool t16 = c0->probe_tile16;
    CvpoGroupTiles th;
    th.q_r4 = (size_t)4 * nt * n_q * k <= (size_t)c0->n_cus && !t16;
    th.a_r4 = (size_t)4 * nt * k <= (size_t)c0->n_cus && !t16;
    th.f_r4 = th.a_r4 && (size_t)8 * nt * k <= (size_t)c0->n_cus;
    // the particle launch has K times the rows of any other launch, so under the whole-launch rule it was the first to leave
    // four-row tiles as k grows and alone decided where a small-batch group stops being bit-identical to fsrl_cvpo_update (B 32, K 8:
    // k = 2, while the B-row launches fit one round up to k = 16).  It keeps the height a member's own update gives it
    // (sac_alloc_batch: k_rows4, four-row tiles up to 4 n_tiles_k n_q <= CUs, i.e. K * B <= 512 rows with single critics).  The
    // benchmarked shapes (K * B = 4096 and up) run sixteen-row tiles under either rule.
    th.k_r4 = (size_t)4 * ntk * n_q <= (size_t)c0->n_cus && !t16;
    const bool small_wgrad = rp <= 512 && !s0->wgrad_splitk;
    const size_t n_steps = (size_t)n_max * k, n_iters = n_steps * M;
    HIPCHK(hipSetDevice(gc.device));
    rc = table_ensure(g->iters, n_iters, std::max<size_t>(n_iters, 64), gc.stream);    // before any member is touched
    if (rc) return rc;
    int nsq = 1, nsa = 1, rq_total = 0, ra_total = 0;
    rc = rgroup_enter(gc, g->steps, call, B, [&]() {
        for (int i = 0; i < k; ++i) {
            if (!call.work[i]) continue;
            fsrl_ctx* c = gc.m[i];
            SacGroupMember& t = g->tab.h[i];
            const int rc = cvpo_group_member(c, sac_of(c), t, g->ctab.h[i], B, th, small_wgrad, &nsq, &nsa);
            if (rc) return rc;                         // nsq, nsa, remap totals: one shape, one plan -- the same for every member
            rq_total = t.fq.remap_total; ra_total = t.fa.remap_total;
        }
        return 0;
    }, [&](int u, int i, SacGroupStep&, const fsrl_ctx* c, const SacState* s) { cvpo_group_iter_rows(g, u, i, k, M, c, s); });
    if (rc) return rc;
    hipStream_t gs = gc.stream;
    HIPCHK(hipMemcpyAsync(g->tab.d, g->tab.h, (size_t)k * sizeof(SacGroupMember), hipMemcpyHostToDevice, gs));
    HIPCHK(hipMemcpyAsync(g->ctab.d, g->ctab.h, (size_t)k * sizeof(CvpoGroupMember), hipMemcpyHostToDevice, gs));
    HIPCHK(hipMemcpyAsync(g->steps.d, g->steps.h, n_steps * sizeof(SacGroupStep), hipMemcpyHostToDevice, gs));
    HIPCHK(hipMemcpyAsync(g->iters.d, g->iters.h, n_iters * sizeof(CvpoGroupIter), hipMemcpyHostToDevice, gs));
    const ModelDesc mda = s0->mda;
    ModelDesc mdq = s0->mdq, mdq_w = s0->mdq, mda_w = s0->mda;
    mdq_w.n_nets = n_q; mda_w.n_nets = 1;              // sac_wgrad: the launch covers the first ny networks
    const int na_dev = s0->na_dev;
    const SacGroupMember* tab = g->tab.d;
    const CvpoGroupMember* ctab = g->ctab.d;
    const int sg_blocks = (B + SG_ROWS - 1) / SG_ROWS + (B * K + 255) / 256;
    rc = dispatch_H(H, [&](auto hc) {
        constexpr int HH = decltype(hc)::value;
        const int ft = th.f_r4 ? 4 * nt : nt, qt = th.q_r4 ? 4 * nt : nt, at = th.a_r4 ? 4 * nt : nt, kt = th.k_r4 ? 4 * ntk : ntk;
        const int ga = round_up(ra_total, 8);
        const ReplayGroupCritic cr{k, n_q, qt, rp, round_up(rq_total, 8), s0->nq_dev, nsq, th.q_r4, small_wgrad};
        for (int u = 0; u < n_max; ++u) {
            const SacGroupStep* st = g->steps.d + (size_t)u * k;
            // 1. sample + gather + the particles' noise; 2. a' ~ actor(s_{t+n}) and the K particles of actor_old at s_t
            hipLaunchKernelGGL(cvpo_sample_gather_group_kernel, dim3(sg_blocks, k), dim3(256), 0, gs, ctab, st);
            if (th.f_r4) hipLaunchKernelGGL((cvpo_actor_group_kernel<HH, 4, 0>), dim3(2 * ft, k), dim3(4 * HH), 0, gs, mda, ctab, st);
            else hipLaunchKernelGGL((cvpo_actor_group_kernel<HH, 16, 0>), dim3(2 * ft, k), dim3(4 * HH), 0, gs, mda, ctab, st);
            // 3. - 6. the critic half
            rgroup_critic_half<HH>(gs, cr, mdq, mdq_w, tab, st);
            // 7. the K * B particles through the updated critics; 8. the E-step, one workgroup per member
            if (th.k_r4) hipLaunchKernelGGL((sac_q_group_kernel<HH, 4, 2>), dim3(kt, n_q, k), dim3(4 * HH), 0, gs, mdq, tab, st);
            else hipLaunchKernelGGL((sac_q_group_kernel<HH, 16, 2>), dim3(kt, n_q, k), dim3(4 * HH), 0, gs, mdq, tab, st);
            hipLaunchKernelGGL(cvpo_estep_group_kernel, dim3(k), dim3(1024), 0, gs, ctab, st);
            // ---- M-step: statistics, dual step (one wave per member), backward, weight gradients, Adam
            for (int it = 0; it < M; ++it) {
                const CvpoGroupIter* gi = g->iters.d + ((size_t)u * M + it) * k;
                if (th.a_r4) hipLaunchKernelGGL((cvpo_actor_group_kernel<HH, 4, 1>), dim3(at, k), dim3(4 * HH), 0, gs, mda, ctab, st);
                else hipLaunchKernelGGL((cvpo_actor_group_kernel<HH, 16, 1>), dim3(at, k), dim3(4 * HH), 0, gs, mda, ctab, st);
                hipLaunchKernelGGL(cvpo_mdual_group_kernel, dim3(k), dim3(64), 0, gs, ctab, st, it == 0 ? 1 : 0);
                if (th.a_r4) hipLaunchKernelGGL((cvpo_actor_group_kernel<HH, 4, 2>), dim3(at, k), dim3(4 * HH), 0, gs, mda, ctab, st);
                else hipLaunchKernelGGL((cvpo_actor_group_kernel<HH, 16, 2>), dim3(at, k), dim3(4 * HH), 0, gs, mda, ctab, st);
                if (small_wgrad) hipLaunchKernelGGL((sac_wgrad_group_kernel<HH, 1>), dim3(wg_grid(HH, 1), k), dim3(1024), 0, gs, mda_w, tab, st, rp);
                else hipLaunchKernelGGL((sac_wgrad_split_group_kernel<HH, 1>), dim3(ga, k), dim3(1024), 0, gs, mda, tab, st);
                // the last actor Adam carries the logged-row block
                if (it < M - 1) hipLaunchKernelGGL(cvpo_adam_group_kernel<0>, dim3((na_dev + 255) / 256, k), dim3(256), 0, gs, mda, ctab, st, gi, na_dev, nsa, na_dev);
                else hipLaunchKernelGGL(cvpo_adam_group_kernel<1>, dim3((na_dev + 255) / 256 + 1, k), dim3(256), 0, gs, mda, ctab, st, gi, na_dev, nsa, na_dev);
            }
            HIPCHK(hipGetLastError());
        }
        return 0;
    });
    if (rc) return rc;
    return rgroup_end(gc, call, B, M);
}
