// host_sac_group_layered.inc -- a group of LAYERED SAC-Lagrangian or DDPG-Lagrangian contexts of one shape (part of fsrl_hip.hip,
// after host_sac_group.inc; kernels_layered_sac_group.hpp has the kernels): the layered branch of fsrl_sac_group_update and the
// shared actor request of a layered fsrl_collect_group.
//   update:  the launch sequence of fsrl_sac_update's layered branches -- sample + gather, both actors' forward and heads, the
//            target Q-networks, the n-step targets, the critics' forward / head / backward / weight side / Adam + Polyak, Q and
//            dQ / da at a ~ pi, the actor's forward / head / backward / weight side / Adam + alpha step + logged row -- each launch
//            carrying every member that still has updates to run: 9 L + 19 launches per update whatever k is.  The linear jobs
//            and the heads' arguments sit in device tables, built once per grouped call after every member has joined (a join may
//            regrow a member's working set and move its buffers); the list of launches (`prog`) is built with them.
//            Bit-identical to the member's own fsrl_sac_update: see kernels_layered_sac_group.hpp.
//            A group of prioritised members (host_sac_group.inc): per_sample_group + gather in place of sample + gather, and
//            per_update_group behind the training Q head, whose rows carry the members' weights: 9 L + 21 launches.
//   collect: no resident kernel -- lay_group_collect_post's staging (host_layered_group.inc) with the members' actor parameters
//            SacState::PA and lay_raw_out_group_kernel as the last launch: L + 2 launches per vector step instead of k (L + 2).
enum { LSG_LIN, LSG_SAMPLE, LSG_NSTEP, LSG_AHEAD, LSG_QHEAD, LSG_ADAM_Q, LSG_ADAM_A,
       LSG_CVPO_SAMPLE, LSG_CVPO_AHEAD, LSG_CVPO_ESTEP, LSG_CVPO_MDUAL, LSG_CVPO_ADAM_A,      // host_cvpo_group_layered.inc
       LSG_PER_UPDATE };                       // a group of prioritised members: the new priorities behind the training Q head
struct LaySacOp {
    int kind;
    int form = 0, nw = 4, gx = 1, gy = 1, n = 0, which = 0;     // LSG_LIN: the launch; heads: which of the three argument rows
    bool vec = true;
    size_t off = 0;                                              // LSG_LIN: first job of the launch in `jobs`
};
struct LaySacGroup {
    DevTable<LinGroupJob> jobs;
    DevTable<LaySacActorArgs> ah;              // [target a' | a ~ pi | backward][k]
    DevTable<LaySacQArgs> qh;                  // [target Q | training | input gradients][k]
    DevTable<SacGatherArgs> ga;                // [k]
    DevTable<SacNstepArgs> na;                 // [k]
    std::vector<LinGroupJob> hjobs;            // the jobs while the tables are built
    std::vector<LaySacOp> prog;                // one update
};
static void lay_sac_group_free(LaySacGroup* lg) {
    if (!lg) return;
    table_free(lg->jobs); table_free(lg->ah); table_free(lg->qh); table_free(lg->ga); table_free(lg->na);
    delete lg;
}

template <int FORM>
static void lay_sac_group_launch(const LaySacOp& op, hipStream_t s, const LinGroupJob* jobs, const SacGroupStep* st) {
    const dim3 grid(op.gx, op.gy, op.n);
#define LSG_GO(V, NW_) hipLaunchKernelGGL((lin_sac_group_kernel<FORM, V, NW_>), grid, dim3(256 * NW_), 0, s, jobs + op.off, st)
    if (op.vec) { if (op.nw == 4) LSG_GO(true, 4); else if (op.nw == 2) LSG_GO(true, 2); else LSG_GO(true, 1); }
    else { if (op.nw == 4) LSG_GO(false, 4); else if (op.nw == 2) LSG_GO(false, 2); else LSG_GO(false, 1); }
#undef LSG_GO
}
// the launches the layered SAC / DDPG program and the layered CVPO program (host_cvpo_group_layered.inc) have in common: the linear
// jobs, the n-step targets, a Q head (op.gx row tiles) and the critics' Adam + Polyak.  false: the kind is the caller's own
static bool lay_replay_group_launch(const LaySacOp& op, hipStream_t gs, const SacState* s0, int B, int k, const LinGroupJob* jobs,
                                    const LaySacQArgs* qh, const SacNstepArgs* na, const SacGroupMember* tab, const SacGroupStep* st) {
    switch (op.kind) {
    case LSG_LIN:
        if (op.form == LIN_F) lay_sac_group_launch<LIN_F>(op, gs, jobs, st);
        else if (op.form == LIN_X) lay_sac_group_launch<LIN_X>(op, gs, jobs, st);
        else lay_sac_group_launch<LIN_W>(op, gs, jobs, st);
        return true;
    case LSG_NSTEP:
        hipLaunchKernelGGL(sac_nstep_group_kernel, dim3((B + 255) / 256, k), dim3(256), 0, gs, na, st);
        return true;
    case LSG_QHEAD:
        hipLaunchKernelGGL(lay_sac_q_head_group_kernel, dim3(op.gx, s0->n_q, k), dim3(64), 0, gs, qh + (size_t)op.which * k, st);
        return true;
    case LSG_ADAM_Q:
        hipLaunchKernelGGL(sac_adam_group_kernel, dim3((s0->nq_dev + 255) / 256, k), dim3(256), 0, gs, s0->mdq, tab, st, s0->nq_dev, 1, s0->nq_dev);
        return true;
    }
    return false;
}

// ---- the launch list of one grouped layered replay update while it is built: the Linear jobs of lay_fwd_k / lay_bwd_dz_k /
//      lay_wgrad_k for every member in one launch each, and the other launches by kind.  The layered SAC / DDPG program below and
//      the layered CVPO program (host_cvpo_group_layered.inc) are both written with it.  work[i] == 0: member i sits the whole call
//      out (its working set may not exist yet); its jobs stay empty.
struct LayReplayProg {
    const ReplayGroupCore& gc;
    const char* work;
    std::vector<LinGroupJob>& hjobs;
    std::vector<LaySacOp>& prog;
    int k, L, n_q, Din, n_cus;
    LayReplayProg(const ReplayGroupCore& gc_, const char* work_, std::vector<LinGroupJob>& hjobs_, std::vector<LaySacOp>& prog_)
        : gc(gc_), work(work_), hjobs(hjobs_), prog(prog_) {
        const fsrl_ctx* c0 = gc.m[0];
        const SacState* s0 = sac_of(gc.m[0]);
        k = (int)gc.m.size(); L = s0->ka.L; n_q = s0->n_q; Din = c0->cfg.obs_dim + c0->cfg.act_dim; n_cus = c0->n_cus;
        hjobs.clear(); prog.clear();
    }
    // one linear launch: `per` jobs per member, fill(i, y, job) forms job y of member i as the member's own launch would
    template <class Fill>
    void lin(int form, int per, Fill&& fill) {
        LaySacOp op{LSG_LIN};
        op.form = form; op.off = hjobs.size(); op.n = k * per;
        long wgs = 0;
        for (int i = 0; i < k; ++i)
            for (int y = 0; y < per; ++y) {
                LinGroupJob gj{};
                gj.member = i;
                if (work[i]) {
                    LinJob& jb = gj.j;
                    fill(i, y, jb);
                    op.gx = std::max(op.gx, (jb.N + 63) / 64); op.gy = std::max(op.gy, (jb.M + 63) / 64);
                    op.vec = op.vec && lay_vec_ok(jb.A, jb.lda, jb.a_len ? jb.a_len : (form == LIN_W ? jb.M : jb.K)) &&
                             lay_vec_ok(jb.N > 0 ? jb.B : nullptr, jb.ldb, form == LIN_F ? jb.K : jb.N);
                    wgs += (long)std::max(1, (jb.N + 63) / 64) * ((jb.M + 63) / 64);
                }
                hjobs.push_back(gj);
            }
        op.nw = wgs <= 2 * n_cus ? 4 : (wgs <= 4 * n_cus ? 2 : 1);       // lay_launch's rule on the whole launch (any NW: the same bits)
        prog.push_back(op);
    }
    const LayWork& work_of(int i, bool actor) const { const SacState* s = sac_of(gc.m[i]); return actor ? s->ka : s->kq; }
    // lay_fwd_k over `rows` rows: P(i) the parameters, X(i) the input rows
    template <class Par, class In>
    void fwd(bool actor, int rows, Par&& P, In&& X) {
        const int nn = actor ? 1 : n_q;
        for (int l = 0; l <= L; ++l)
            lin(LIN_F, nn, [&](int i, int net, LinJob& jb) {
                const LayWork& w = work_of(i, actor);
                const LayLayer& ll = w.lm.net[net].l[l];
                jb.A = (l == 0) ? X(i) : w.act[net][l - 1]; jb.lda = ll.in;
                jb.B = P(i) + ll.W; jb.ldb = ll.in;
                jb.aux = P(i) + ll.b;
                jb.M = rows; jb.N = ll.out; jb.K = ll.in;
                if (l < L) { jb.C = w.act[net][l]; jb.ldc = ll.out; jb.relu = 1; }
                else { jb.C = w.out + (size_t)net * w.mbp * FSRL_MAX_ACT; jb.ldc = FSRL_MAX_ACT; jb.relu = 0; }
            });
    }
    // lay_bwd_dz_k; to_input: down to the network's input (the Q-networks' dQ / d[obs | act] into DXQ)
    template <class Par>
    void bwd(bool actor, int rows, Par&& P, bool to_input) {
        const int nn = actor ? 1 : n_q;
        for (int l = L - 1; l >= (to_input ? -1 : 0); --l)
            lin(LIN_X, nn, [&](int i, int net, LinJob& jb) {
                const LayWork& w = work_of(i, actor);
                const LayLayer& up = w.lm.net[net].l[l + 1];
                if (l == L - 1) { jb.A = w.dout + (size_t)net * w.mbp * FSRL_DOW; jb.lda = FSRL_DOW; jb.a_len = 16; }
                else { jb.A = w.dz[net][l + 1]; jb.lda = up.out; }
                jb.B = P(i) + up.W; jb.ldb = up.in;
                if (l >= 0) { jb.C = w.dz[net][l]; jb.ldc = up.in; jb.aux = w.act[net][l]; jb.ldaux = up.in; }
                else { jb.C = sac_of(gc.m[i])->DXQ + (size_t)net * w.mbp * Din; jb.ldc = up.in; }
                jb.M = rows; jb.N = up.in; jb.K = up.out;
            });
    }
    // lay_wgrad_k: every Linear of every network of the family in one launch, into the member's GA / GQ
    template <class In>
    void wgrad(bool actor, int rows, In&& X) {
        const int nn = actor ? 1 : n_q;
        lin(LIN_W, nn * (L + 1), [&](int i, int y, LinJob& jb) {
            const SacState* s = sac_of(gc.m[i]);
            const LayWork& w = actor ? s->ka : s->kq;
            float* G = actor ? s->GA : s->GQ;
            const int net = y / (L + 1), l = y % (L + 1);
            const LayLayer& ll = w.lm.net[net].l[l];
            jb.A = (l < L) ? w.dz[net][l] : w.dout + (size_t)net * w.mbp * FSRL_DOW;
            jb.lda = (l < L) ? ll.out : FSRL_DOW; jb.a_len = (l < L) ? 0 : 16;
            jb.B = (l == 0) ? X(i) : w.act[net][l - 1]; jb.ldb = ll.in;
            jb.C = G + ll.W; jb.ldc = ll.in;
            jb.bias_out = G + ll.b;
            jb.M = ll.out; jb.N = ll.in; jb.K = rows;
        });
    }
    // any other launch; which: the argument row of a head (the M-iteration's first flag of a dual step); tiles: a head's row tiles
    void op(int kind, int which = 0, int tiles = 0) { LaySacOp o{kind}; o.which = which; o.gx = std::max(1, tiles); prog.push_back(o); }
    // the finished job list into the device table, on the group's stream
    int upload(DevTable<LinGroupJob>& jobs) {
        const size_t nj = hjobs.size();
        const int rc = table_ensure(jobs, nj, nj);
        if (rc) return rc;
        memcpy(jobs.h, hjobs.data(), nj * sizeof(LinGroupJob));
        HIPCHK(hipMemcpyAsync(jobs.d, jobs.h, nj * sizeof(LinGroupJob), hipMemcpyHostToDevice, gc.stream));
        return 0;
    }
};

// The tables and the launch list of one grouped call.  work[i] == 0: member i sits the whole call out (its working set may not
// exist yet); its jobs stay empty and its step rows inactive.
static int lay_sac_group_tables(fsrl_sac_group* g, LaySacGroup& lg, int B, const char* work, const double* lagrangians,
                                const double* rescaling) {
    ReplayGroupCore& gc = g->core;
    const int k = (int)gc.m.size();
    fsrl_ctx* c0 = gc.m[0];
    const size_t lag_stride = (size_t)std::max(1, c0->cfg.n_critics - 1);
    int rc = table_ensure(lg.ah, (size_t)3 * k, (size_t)3 * k);
    if (!rc) rc = table_ensure(lg.qh, (size_t)3 * k, (size_t)3 * k);
    if (!rc) rc = table_ensure(lg.ga, (size_t)k, (size_t)k);
    if (!rc) rc = table_ensure(lg.na, (size_t)k, (size_t)k);
    if (rc) return rc;
    memset(lg.ah.h, 0, (size_t)3 * k * sizeof(LaySacActorArgs)); memset(lg.qh.h, 0, (size_t)3 * k * sizeof(LaySacQArgs));
    memset(lg.ga.h, 0, (size_t)k * sizeof(SacGatherArgs)); memset(lg.na.h, 0, (size_t)k * sizeof(SacNstepArgs));
    LayReplayProg pg(gc, work, lg.hjobs, lg.prog);
    const int tiles = (B + 15) / 16;                   // row tiles of a head launch
    auto S = [&](int i) { return sac_of(gc.m[i]); };
    // ---- the update, launch by launch (fsrl_sac_update, layered branches)
    pg.op(LSG_SAMPLE);
    pg.fwd(true, B, [&](int i) { return S(i)->ddpg ? S(i)->PAT : S(i)->PA; }, [&](int i) { return S(i)->OBSN; });
    pg.op(LSG_AHEAD, 0, tiles);
    pg.fwd(true, B, [&](int i) { return S(i)->PA; }, [&](int i) { return S(i)->OBS; });
    pg.op(LSG_AHEAD, 1, tiles);
    pg.fwd(false, B, [&](int i) { return S(i)->PQT; }, [&](int i) { return S(i)->XN; });
    pg.op(LSG_QHEAD, 0, tiles);
    pg.op(LSG_NSTEP);
    pg.fwd(false, B, [&](int i) { return S(i)->PQ; }, [&](int i) { return S(i)->XQ; });
    pg.op(LSG_QHEAD, 1, tiles);
    if (sac_group_per(g)) pg.op(LSG_PER_UPDATE);       // reads the Q values and targets that head just used
    pg.bwd(false, B, [&](int i) { return S(i)->PQ; }, false);
    pg.wgrad(false, B, [&](int i) { return S(i)->XQ; });
    pg.op(LSG_ADAM_Q);
    pg.fwd(false, B, [&](int i) { return S(i)->PQ; }, [&](int i) { return S(i)->XP; });
    pg.op(LSG_QHEAD, 2, tiles);
    pg.bwd(false, B, [&](int i) { return S(i)->PQ; }, true);
    pg.fwd(true, B, [&](int i) { return S(i)->PA; }, [&](int i) { return S(i)->OBS; });
    pg.op(LSG_AHEAD, 2, tiles);
    pg.bwd(true, B, [&](int i) { return S(i)->PA; }, false);
    pg.wgrad(true, B, [&](int i) { return S(i)->OBS; });
    pg.op(LSG_ADAM_A);
    // ---- per member: heads, sample, n-step targets, the Adam passes' member row
    for (int i = 0; i < k; ++i) {
        SacGroupMember& t = g->tab.h[i];
        t = SacGroupMember{};
        if (!work[i]) continue;
        fsrl_ctx* c = gc.m[i];
        const SacState* s = sac_of(c);
        const float lam = s->cfg.use_lagrangian ? (float)lagrangians[(size_t)i * lag_stride] : 0.0f;
        const float resc = (float)rescaling[i];
        // the heads of fsrl_sac_update's three actor passes and three Q-network passes, in its order
        lg.ah.h[(size_t)0 * k + i] = lay_sac_actor_head_args(c, s, B, SAC_A_FWD, s->eps_t, s->XN, s->LPN, resc, lam);
        lg.ah.h[(size_t)1 * k + i] = lay_sac_actor_head_args(c, s, B, SAC_A_FWD, s->eps_p, s->XP, s->LP, resc, lam);
        lg.ah.h[(size_t)2 * k + i] = lay_sac_actor_head_args(c, s, B, SAC_A_BWD, s->eps_p, s->XP, s->LP, resc, lam);
        lg.qh.h[(size_t)0 * k + i] = lay_sac_q_head_args(c, s, FB_MODE_Q_FWD, s->stq, B, nullptr, s->PQT);
        lg.qh.h[(size_t)1 * k + i] = lay_sac_q_head_args(c, s, FB_MODE_Q_TRAIN, s->stq, B, nullptr, s->PQ);
        lg.qh.h[(size_t)2 * k + i] = lay_sac_q_head_args(c, s, FB_MODE_Q_DIN, s->stdin_, B, nullptr, s->PQ);
        lg.ga.h[i] = sac_gather_args(c, s, B, s->cfg.n_step);
        lg.na.h[i] = sac_nstep_args(c, s, B);
        t.PA = s->PA; t.MA = s->MA; t.VA = s->VA; t.PQ = s->PQ; t.PQT = s->PQT; t.MQ = s->MQ; t.VQ = s->VQ;
        t.PAT = s->ddpg ? s->PAT : nullptr;
        t.GA = s->GA; t.GQ = s->GQ;             // the weight-side launches leave the finished gradients there: one partial
        t.fin = sac_final_args(c, s, B, resc, lam, s->n_tiles, s->n_tiles, nullptr);
        t.stats = s->d_stats; t.nstats = s->nstats;
        member_adam_consts(t, c, s->cfg.tau);
    }
    rc = pg.upload(lg.jobs);
    if (rc) return rc;
    hipStream_t gs = gc.stream;
    HIPCHK(hipMemcpyAsync(lg.ah.d, lg.ah.h, (size_t)3 * k * sizeof(LaySacActorArgs), hipMemcpyHostToDevice, gs));
    HIPCHK(hipMemcpyAsync(lg.qh.d, lg.qh.h, (size_t)3 * k * sizeof(LaySacQArgs), hipMemcpyHostToDevice, gs));
    HIPCHK(hipMemcpyAsync(lg.ga.d, lg.ga.h, (size_t)k * sizeof(SacGatherArgs), hipMemcpyHostToDevice, gs));
    HIPCHK(hipMemcpyAsync(lg.na.d, lg.na.h, (size_t)k * sizeof(SacNstepArgs), hipMemcpyHostToDevice, gs));
    HIPCHK(hipMemcpyAsync(g->tab.d, g->tab.h, (size_t)k * sizeof(SacGroupMember), hipMemcpyHostToDevice, gs));
    return 0;
}

// fsrl_sac_group_update for a group of layered members (the caller has checked the group and B)
static int lay_sac_group_update(fsrl_sac_group* g, int32_t B, const int32_t* n_updates, const double* lagrangians,
                                const double* rescaling) {
    ReplayGroupCore& gc = g->core;
    const int k = (int)gc.m.size();
    const SacState* s0 = sac_of(gc.m[0]);
    ReplayGroupCall call;
    int rc = rgroup_begin(gc, false, n_updates, call, [](int, const fsrl_ctx*, const SacState*) { return 0; });
    if (rc) return rc;
    CHECK_ARG(!s0->cfg.use_lagrangian || lagrangians, "lagrangians: [k][n_critics - 1] when use_lagrangian is on");
    const int n_max = call.n_max;
    if (n_max == 0) return 0;
    if (!g->lay) g->lay = new LaySacGroup();
    LaySacGroup& lg = *g->lay;
    const bool per_on = sac_group_per(g);
    rc = rgroup_enter(gc, g->steps, call, B, [&]() {
        const int rc = per_on ? per_group_table(g, call, B) : 0;
        return rc ? rc : lay_sac_group_tables(g, lg, B, call.work, lagrangians, rescaling);
    },
                      [](int u, int, SacGroupStep& st, const fsrl_ctx* c, const SacState* s) { sac_group_step_row(u, st, c, s); });
    if (rc) return rc;
    hipStream_t gs = gc.stream;
    HIPCHK(hipMemcpyAsync(g->steps.d, g->steps.h, (size_t)n_max * k * sizeof(SacGroupStep), hipMemcpyHostToDevice, gs));
    const ModelDesc mda = s0->mda;
    const int na_dev = s0->na_dev;
    const int gather_blocks = std::min(1024, (B * (gc.m[0]->cfg.obs_dim + gc.m[0]->cfg.act_dim) + 255) / 256);
    const SacGroupMember* tab = g->tab.d;
    for (int u = 0; u < n_max; ++u) {
        const SacGroupStep* st = g->steps.d + (size_t)u * k;
        for (const LaySacOp& op : lg.prog) {
            if (lay_replay_group_launch(op, gs, s0, B, k, lg.jobs.d, lg.qh.d, lg.na.d, tab, st)) continue;
            switch (op.kind) {
            case LSG_SAMPLE:
                if (per_on) {       // the descent of each member's sum tree with its weights, then the plain gather
                    hipLaunchKernelGGL(per_sample_group_kernel, dim3(k), dim3(PER_THREADS), 0, gs, g->per.d, st);
                    hipLaunchKernelGGL(sac_gather_group_kernel, dim3(gather_blocks, k), dim3(256), 0, gs, lg.ga.d, sizeof(SacGatherArgs), st);
                } else hipLaunchKernelGGL(sac_sample_gather_group_kernel, dim3((B + SG_ROWS - 1) / SG_ROWS, k), dim3(256), 0, gs, lg.ga.d, st);
                break;
            case LSG_PER_UPDATE:
                hipLaunchKernelGGL(per_update_group_kernel, dim3(k), dim3(PER_THREADS), 0, gs, g->per.d, st);
                break;
            case LSG_AHEAD:
                hipLaunchKernelGGL(lay_sac_actor_head_group_kernel, dim3(op.gx, k), dim3(256), 0, gs, lg.ah.d + (size_t)op.which * k, st);
                break;
            case LSG_ADAM_A:
                hipLaunchKernelGGL(sac_adam_final_group_kernel, dim3((na_dev + 255) / 256 + 1, k), dim3(256), 0, gs, mda, tab, st, na_dev, 1, na_dev);
                break;
            }
        }
        HIPCHK(hipGetLastError());
    }
    return rgroup_end(gc, call, B, 1);
}

// ---------------------------------------------------------------- lock-step collection
// fsrl_collect_group_step for a group of layered members: ga_collect_step_via with the shared request as lay_group_collect_stage's
// L + 1 forward launches over the members' actor parameters SacState::PA and lay_raw_out_group_kernel; the host then finishes each
// member as its own fsrl_collect_step does.  Ordering: after a release (a member's parameters may have changed: its own update or
// actor call, fsrl_sac_put_params, a grouped update) the next request first puts the group's stream behind every member's compute
// stream; requests between two releases are ordered by the group's stream alone.  Requests are synchronous, so nothing of the
// group reads a member's parameters once the step has returned.
static int lay_collect_group_step(fsrl_collect_group* g, const GaStepArgs& a) {
    const int n = (int)g->m.size(), Do = g->m[0]->cfg.obs_dim, Da = g->m[0]->cfg.act_dim, cols = g->raw_cols;
    auto post = [&]() -> int {
        std::lock_guard<std::mutex> lock(g->mu);                    // `reorder` is the release hook's, on any thread
        const int ro = collect_group_reorder(g);
        if (ro) return ro;
        fsrl_ctx* c0 = g->m[0];
        const SacState* s0 = sac_of(c0);
        return lay_group_collect_stage(
            g->lay, g->ga, c0, s0->ka.lm.net[0], Do, s0->ka.hmax, n, cols, a.k_act, a.obs_act, [&](int i) { return sac_of(g->m[i])->PA; },
            [&](float* outb, const LayGroupPinned& pin, int maxk) {
                LayRawGroupArgs ra{};
                for (int i = 0; i < n; ++i) ra.rows[i] = a.k_act[i];
                ra.out = outb; ra.raw = pin.mu; ra.done = pin.done; ra.cap = g->lay.ccap; ra.tiles_cap = g->lay.ccap / 16; ra.cols = cols;
                ra.seq = g->lay.cseq;
                hipLaunchKernelGGL(lay_raw_out_group_kernel, dim3((maxk + 15) / 16, n), dim3(64), 0, g->stream, ra);
            });
    };
    return ga_collect_step_via(
        g->ga, g->m.data(), n, g->device, a, [](int) { return true; }, post,
        [&]() { return lay_group_collect_wait(g->lay, g->ga, n, Do, cols); },
        [&]() { (void)hipStreamSynchronize(g->stream); },           // a push failed behind the request: drain the stream
        [&](int i, fsrl_ctx* c, int ka, const GaLayout&) {
            const LayGroupPinned pin = lay_group_pinned(g->lay, Do, cols);
            sac_actor_finish(c, pin.mu + (size_t)i * g->lay.ccap * cols, ka, c->act_mu.data(), c->act_sg.data());
        },
        [&]() {
            for (int j = 0; j < n; ++j) {
                fsrl_ctx* c = g->m[j];
                if (a.k_act[j] <= 0) continue;
                c->act_mu.resize((size_t)a.k_act[j] * Da); c->act_sg.resize((size_t)a.k_act[j] * Da);
                (void)actor_eval_finish(c, c->act_mu.data(), c->act_sg.data());
            }
        });
}
