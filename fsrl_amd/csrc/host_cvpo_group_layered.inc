// host_cvpo_group_layered.inc -- a group of LAYERED CVPO contexts of one shape (part of fsrl_hip.hip, after host_cvpo_group.inc and
// host_sac_group_layered.inc): the layered branch of fsrl_cvpo_group_update.
// The launch sequence of fsrl_cvpo_update's layered branches, each launch carrying every member that still has updates to run:
//   1. sample + gather + the particles' noise;
//   2. the actor on OBSN and the TARGET head;  3. actor_old on OBS and the PARTICLES head;
//   4. the target Q-networks on XN and their head;  5. the n-step targets;
//   6. the critics on XQ, the Q_TRAIN head, backward, weight side, Adam + Polyak;
//   7. the critics on the K * B particle rows XK and their head into QK;  8. the E-step;
//   9. mstep_iter_num times: the actor on OBS, the MFWD head, the M dual step, the MBWD head, backward, weight side, the actor's
//      Adam (the last one with the logged row).
// The member's own update runs the actor's forward on OBS a second time in front of the MBWD head.  That forward recomputes what
// the MFWD head's forward left in ka.act / ka.out from the same parameters and rows, and nothing in between writes them (the dual
// step touches CvpoScalars only), so the grouped program LEAVES IT OUT: 6 L + 15 + M (2 L + 6) launches per update for L hidden
// layers and M = mstep_iter_num, whatever k is, against the member's own 6 L + 15 + M (3 L + 7).
// The linear jobs are LayReplayProg's (host_sac_group_layered.inc), the heads' arguments sit in device tables, and every per-member
// argument comes from the builder the member's own update uses (host_cvpo.inc).  The tables are built once per grouped call after
// every member has joined (a join may regrow a member's working set and move its buffers).  Step rows and CvpoGroupIter rows are
// the fused group's.  Bit-identical to the member's own fsrl_cvpo_update at every k and batch size: lin_body accumulates every
// output element in one ascending chain whatever the launch shape, and a layered launch has no tile-height plan.
enum { LCG_TARGET, LCG_PARTICLES, LCG_MFWD, LCG_MBWD, LCG_NHEADS };        // rows of LayCvpoGroup::ah
enum { LCG_Q_TARGET, LCG_Q_TRAIN, LCG_Q_PARTICLES, LCG_NQHEADS };          // rows of LayCvpoGroup::qh
struct LayCvpoGroup {
    DevTable<LinGroupJob> jobs;
    DevTable<LayCvpoActorArgs> ah;             // [LCG_NHEADS][k]
    DevTable<LaySacQArgs> qh;                  // [LCG_NQHEADS][k]
    DevTable<SacNstepArgs> na;                 // [k]
    std::vector<LinGroupJob> hjobs;            // the jobs while the tables are built
    std::vector<LaySacOp> prog;                // one update: [0, m_begin) once, [m_begin, end) per M iteration
    size_t m_begin = 0;
};
static void lay_cvpo_group_free(LayCvpoGroup* lg) {
    if (!lg) return;
    table_free(lg->jobs); table_free(lg->ah); table_free(lg->qh); table_free(lg->na);
    delete lg;
}

// The tables and the launch list of one grouped call.  work[i] == 0: member i sits the whole call out (its working set may not
// exist yet); its jobs stay empty and its step rows inactive.
static int lay_cvpo_group_tables(fsrl_cvpo_group* g, LayCvpoGroup& lg, int B, const char* work) {
    ReplayGroupCore& gc = g->core;
    const int k = (int)gc.m.size();
    fsrl_ctx* c0 = gc.m[0];
    const SacState* s0 = sac_of(c0);
    const int K = s0->ccfg.sample_act_num;
    const int tiles = (B + 15) / 16, tiles_k = (K * B + 15) / 16;
    int rc = table_ensure(lg.ah, (size_t)LCG_NHEADS * k, (size_t)LCG_NHEADS * k);
    if (!rc) rc = table_ensure(lg.qh, (size_t)LCG_NQHEADS * k, (size_t)LCG_NQHEADS * k);
    if (!rc) rc = table_ensure(lg.na, (size_t)k, (size_t)k);
    if (rc) return rc;
    memset(lg.ah.h, 0, (size_t)LCG_NHEADS * k * sizeof(LayCvpoActorArgs)); memset(lg.qh.h, 0, (size_t)LCG_NQHEADS * k * sizeof(LaySacQArgs));
    memset(lg.na.h, 0, (size_t)k * sizeof(SacNstepArgs));
    LayReplayProg pg(gc, work, lg.hjobs, lg.prog);
    auto S = [&](int i) { return sac_of(gc.m[i]); };
    auto PA = [&](int i) { return S(i)->PA; };
    auto PQ = [&](int i) { return S(i)->PQ; };
    auto OBS = [&](int i) { return S(i)->OBS; };
    // ---- the update, launch by launch (fsrl_cvpo_update, layered branches)
    pg.op(LSG_CVPO_SAMPLE);
    pg.fwd(true, B, PA, [&](int i) { return S(i)->OBSN; });
    pg.op(LSG_CVPO_AHEAD, LCG_TARGET, tiles);
    pg.fwd(true, B, [&](int i) { return S(i)->PAT; }, OBS);
    pg.op(LSG_CVPO_AHEAD, LCG_PARTICLES, tiles);
    pg.fwd(false, B, [&](int i) { return S(i)->PQT; }, [&](int i) { return S(i)->XN; });
    pg.op(LSG_QHEAD, LCG_Q_TARGET, tiles);
    pg.op(LSG_NSTEP);
    pg.fwd(false, B, PQ, [&](int i) { return S(i)->XQ; });
    pg.op(LSG_QHEAD, LCG_Q_TRAIN, tiles);
    pg.bwd(false, B, PQ, false);
    pg.wgrad(false, B, [&](int i) { return S(i)->XQ; });
    pg.op(LSG_ADAM_Q);
    pg.fwd(false, K * B, PQ, [&](int i) { return S(i)->XK; });
    pg.op(LSG_QHEAD, LCG_Q_PARTICLES, tiles_k);
    pg.op(LSG_CVPO_ESTEP);
    lg.m_begin = lg.prog.size();
    pg.fwd(true, B, PA, OBS);
    pg.op(LSG_CVPO_AHEAD, LCG_MFWD, tiles);
    pg.op(LSG_CVPO_MDUAL);
    pg.op(LSG_CVPO_AHEAD, LCG_MBWD, tiles);        // on the activations and head outputs the MFWD head's forward left
    pg.bwd(true, B, PA, false);
    pg.wgrad(true, B, OBS);
    pg.op(LSG_CVPO_ADAM_A);
    // ---- per member: heads, n-step targets, the two member tables
    for (int i = 0; i < k; ++i) {
        SacGroupMember& t = g->tab.h[i];
        CvpoGroupMember& v = g->ctab.h[i];
        t = SacGroupMember{};
        v = CvpoGroupMember{};
        if (!work[i]) continue;
        fsrl_ctx* c = gc.m[i];
        const SacState* s = sac_of(c);
        // the heads of fsrl_cvpo_update's actor passes (lay_cvpo_actor_pass) and Q-network passes (sac_q_launch), as it forms them
        auto ah = [&](int w) -> LayCvpoActorArgs& { return lg.ah.h[(size_t)w * k + i]; };
        ah(LCG_TARGET) = lay_cvpo_actor_head_args(c, s, B, CVPO_A_TARGET, s->OBSN, s->eps_t, s->XN);
        ah(LCG_PARTICLES) = lay_cvpo_actor_head_args(c, s, B, CVPO_A_PARTICLES, s->OBS, s->eps_k, s->XK);
        ah(LCG_MFWD) = lay_cvpo_actor_head_args(c, s, B, CVPO_A_MFWD, s->OBS, nullptr, nullptr);
        ah(LCG_MBWD) = lay_cvpo_actor_head_args(c, s, B, CVPO_A_MBWD, s->OBS, nullptr, nullptr);
        auto qh = [&](int w) -> LaySacQArgs& { return lg.qh.h[(size_t)w * k + i]; };
        qh(LCG_Q_TARGET) = lay_sac_q_head_args(c, s, FB_MODE_Q_FWD, s->stq, B, nullptr, s->PQT);
        qh(LCG_Q_TRAIN) = lay_sac_q_head_args(c, s, FB_MODE_Q_TRAIN, s->stq, B, nullptr, s->PQ);
        qh(LCG_Q_PARTICLES) = lay_sac_q_head_args(c, s, FB_MODE_Q_FWD, s->stqk, K * B, s->QK, s->PQ);
        lg.na.h[i] = cvpo_nstep_args(c, s, B);
        t.PQ = s->PQ; t.PQT = s->PQT; t.MQ = s->MQ; t.VQ = s->VQ;
        t.GQ = s->GQ;                           // the weight-side launches leave the finished gradients there: one partial
        v.PA = s->PA; v.MA = s->MA; v.VA = s->VA; v.GA = s->GA;
        v.ga = sac_gather_args(c, s, B, s->ccfg.n_step);
        v.es = cvpo_estep_args(c, s, B);
        v.md = cvpo_mdual_args(c, s, B, s->n_tiles, 0);
        v.fin = cvpo_final_args(c, s, B, s->n_tiles, nullptr);
        v.stats = s->d_stats; v.nstats = s->nstats;
        member_adam_consts(t, c, s->ccfg.tau);
        member_adam_consts(v, c);
    }
    rc = pg.upload(lg.jobs);
    if (rc) return rc;
    hipStream_t gs = gc.stream;
    HIPCHK(hipMemcpyAsync(lg.ah.d, lg.ah.h, (size_t)LCG_NHEADS * k * sizeof(LayCvpoActorArgs), hipMemcpyHostToDevice, gs));
    HIPCHK(hipMemcpyAsync(lg.qh.d, lg.qh.h, (size_t)LCG_NQHEADS * k * sizeof(LaySacQArgs), hipMemcpyHostToDevice, gs));
    HIPCHK(hipMemcpyAsync(lg.na.d, lg.na.h, (size_t)k * sizeof(SacNstepArgs), hipMemcpyHostToDevice, gs));
    HIPCHK(hipMemcpyAsync(g->tab.d, g->tab.h, (size_t)k * sizeof(SacGroupMember), hipMemcpyHostToDevice, gs));
    HIPCHK(hipMemcpyAsync(g->ctab.d, g->ctab.h, (size_t)k * sizeof(CvpoGroupMember), hipMemcpyHostToDevice, gs));
    return 0;
}

// fsrl_cvpo_group_update for a group of layered members (the caller has checked the group and B)
static int lay_cvpo_group_update(fsrl_cvpo_group* g, int32_t B, const int32_t* n_updates) {
    ReplayGroupCore& gc = g->core;
    const int k = (int)gc.m.size();
    const SacState* s0 = sac_of(gc.m[0]);
    ReplayGroupCall call;
    int rc = rgroup_begin(gc, true, n_updates, call, [](int, const fsrl_ctx*, const SacState*) { return 0; });
    if (rc) return rc;
    const int n_max = call.n_max;
    if (n_max == 0) return 0;
    const int K = s0->ccfg.sample_act_num, M = s0->ccfg.mstep_iter_num;
    const size_t n_steps = (size_t)n_max * k, n_iters = n_steps * M;
    HIPCHK(hipSetDevice(gc.device));
    rc = table_ensure(g->iters, n_iters, std::max<size_t>(n_iters, 64), gc.stream);    // before any member is touched
    if (rc) return rc;
    if (!g->lay) g->lay = new LayCvpoGroup();
    LayCvpoGroup& lg = *g->lay;
    rc = rgroup_enter(gc, g->steps, call, B, [&]() { return lay_cvpo_group_tables(g, lg, B, call.work); },
                      [&](int u, int i, SacGroupStep&, const fsrl_ctx* c, const SacState* s) { cvpo_group_iter_rows(g, u, i, k, M, c, s); });
    if (rc) return rc;
    hipStream_t gs = gc.stream;
    HIPCHK(hipMemcpyAsync(g->steps.d, g->steps.h, n_steps * sizeof(SacGroupStep), hipMemcpyHostToDevice, gs));
    HIPCHK(hipMemcpyAsync(g->iters.d, g->iters.h, n_iters * sizeof(CvpoGroupIter), hipMemcpyHostToDevice, gs));
    const ModelDesc mda = s0->mda;
    const int na_dev = s0->na_dev;
    const int sg_blocks = (B + SG_ROWS - 1) / SG_ROWS + (B * K + 255) / 256;
    const SacGroupMember* tab = g->tab.d;
    const CvpoGroupMember* ctab = g->ctab.d;
    // one launch of the program; it: the M iteration (0 in front of the M-step)
    auto launch = [&](const LaySacOp& op, const SacGroupStep* st, int u, int it) {
        if (lay_replay_group_launch(op, gs, s0, B, k, lg.jobs.d, lg.qh.d, lg.na.d, tab, st)) return;
        switch (op.kind) {
        case LSG_CVPO_SAMPLE:
            hipLaunchKernelGGL(cvpo_sample_gather_group_kernel, dim3(sg_blocks, k), dim3(256), 0, gs, ctab, st);
            break;
        case LSG_CVPO_AHEAD:
            hipLaunchKernelGGL(lay_cvpo_actor_head_group_kernel, dim3(op.gx, k), dim3(256), 0, gs, lg.ah.d + (size_t)op.which * k, st);
            break;
        case LSG_CVPO_ESTEP:
            hipLaunchKernelGGL(cvpo_estep_group_kernel, dim3(k), dim3(1024), 0, gs, ctab, st);
            break;
        case LSG_CVPO_MDUAL:
            hipLaunchKernelGGL(cvpo_mdual_group_kernel, dim3(k), dim3(64), 0, gs, ctab, st, it == 0 ? 1 : 0);
            break;
        case LSG_CVPO_ADAM_A: {
            const CvpoGroupIter* gi = g->iters.d + ((size_t)u * M + it) * k;
            // the last actor Adam carries the logged-row block
            if (it < M - 1) hipLaunchKernelGGL(cvpo_adam_group_kernel<0>, dim3((na_dev + 255) / 256, k), dim3(256), 0, gs, mda, ctab, st, gi, na_dev, 1, na_dev);
            else hipLaunchKernelGGL(cvpo_adam_group_kernel<1>, dim3((na_dev + 255) / 256 + 1, k), dim3(256), 0, gs, mda, ctab, st, gi, na_dev, 1, na_dev);
            break;
        }
        }
    };
    for (int u = 0; u < n_max; ++u) {
        const SacGroupStep* st = g->steps.d + (size_t)u * k;
        for (size_t p = 0; p < lg.m_begin; ++p) launch(lg.prog[p], st, u, 0);
        for (int it = 0; it < M; ++it)
            for (size_t p = lg.m_begin; p < lg.prog.size(); ++p) launch(lg.prog[p], st, u, it);
        HIPCHK(hipGetLastError());
    }
    return rgroup_end(gc, call, B, M);
}
