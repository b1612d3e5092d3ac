// host_sac_group.inc -- grouped SAC-Lagrangian updates: fsrl_sac_group_* (part of fsrl_hip.hip, kernels: kernels_sac_group.hpp).
// k SAC-Lag contexts of one network shape, each stepped n_i times per call in lock step: every launch of an update carries all
// members that still have updates to run (nine launches per update, whatever k is).  Members keep their own streams, stores,
// parameters, targets, Adam state, alpha, Philox key and statistics ring; the group has a stream of its own that waits on each
// member's stream before the call and that each member's streams wait on after it.  Between grouped calls a member is an ordinary
// context (its resident actor included: a grouped call ends it, the member's next collect launches it again).
// Bit-identity with fsrl_sac_update: the member's arithmetic is the single path's body with the single path's split-K plan; the
// tile height of a launch is the single-context rule applied to the whole group's launch (4-row tiles while the group still fits
// one round of workgroups), so a group of one is bit-identical to its solo run, and larger groups are wherever the tile height
// does not change a row's result (tests/test_gpu_sac_group.py).
// ====================================================================================== grouped SAC-Lagrangian
struct fsrl_sac_group {
    std::vector<fsrl_ctx*> m;                  // members (not owned; nullptr once destroyed)
    int device = 0;
    hipStream_t stream = nullptr;              // the group's own stream
    hipEvent_t done = nullptr;                 // end of the last grouped call on `stream`
    std::vector<hipEvent_t> ready;             // per member: its stream's work before the call
    SacGroupMember *d_tab = nullptr, *h_tab = nullptr;       // device / pinned, [k]
    SacGroupStep *d_steps = nullptr, *h_steps = nullptr;     // device / pinned, [updates][k]
    size_t cap_steps = 0;
    bool broken = false;                       // a member was destroyed first: no more updates
};

// a member destroyed before its group (fsrl_ctx_destroy): the group stops updating, its destroy still works
static void sac_group_detach(fsrl_ctx* c) {
    fsrl_sac_group* g = c->sac_group;
    if (!g) return;
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    for (auto& x : g->m) if (x == c) x = nullptr;
    c->sac_group = nullptr;
    g->broken = true;
}

extern "C" int fsrl_sac_group_destroy(fsrl_sac_group* g) {
    if (!g) return 0;
    (void)hipSetDevice(g->device);
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    for (fsrl_ctx* c : g->m) if (c) c->sac_group = nullptr;
    for (hipEvent_t e : g->ready) if (e) (void)hipEventDestroy(e);
    if (g->done) (void)hipEventDestroy(g->done);
    if (g->stream) (void)hipStreamDestroy(g->stream);
    if (g->d_tab) (void)hipFree(g->d_tab);
    if (g->h_tab) (void)hipHostFree(g->h_tab);
    if (g->d_steps) (void)hipFree(g->d_steps);
    if (g->h_steps) (void)hipHostFree(g->h_steps);
    delete g;
    return 0;
}

extern "C" int fsrl_sac_group_create(fsrl_ctx** ctxs, int32_t k, fsrl_sac_group** out) {
    CHECK_ARG(ctxs && out, "null argument");
    CHECK_ARG(k >= 1 && k <= FSRL_MAX_GROUP, "a SAC group has 1..%d members", FSRL_MAX_GROUP);
    const fsrl_ctx* c0 = ctxs[0];
    CHECK_ARG(c0, "null member");
    for (int i = 0; i < k; ++i) {
        const fsrl_ctx* c = ctxs[i];
        CHECK_ARG(c, "null member");
        const SacState* s = reinterpret_cast<const SacState*>(c->sac);
        CHECK_ARG(c->cfg.algo == FSRL_ALGO_SAC_LAG && s, "member %d: grouped SAC updates take SAC-Lagrangian contexts (fsrl_sac_init)", i);
        CHECK_ARG(!s->cvpo, "member %d runs CVPO: grouped SAC updates take SAC-Lagrangian contexts only", i);
        CHECK_ARG(!s->ddpg, "member %d is a DDPG-Lagrangian context (deterministic actor): grouped SAC updates need the stochastic actor", i);
        CHECK_ARG(!s->layered && !c->lay, "member %d is a layered context: grouped SAC updates run the fused kernels (two hidden layers)", i);
        CHECK_ARG(c->device == c0->device, "member %d: members live on one device", i);
        CHECK_ARG(!c->sac_group, "member %d is already in a SAC group", i);
        const SacState* s0 = reinterpret_cast<const SacState*>(c0->sac);
        CHECK_ARG(c->cfg.obs_dim == c0->cfg.obs_dim && c->cfg.act_dim == c0->cfg.act_dim && c->cfg.hidden == c0->cfg.hidden,
                  "member %d: members must have one network shape (obs_dim, act_dim, hidden)", i);
        CHECK_ARG(s->cfg.n_step == s0->cfg.n_step && (s->cfg.auto_alpha != 0) == (s0->cfg.auto_alpha != 0) &&
                  (s->cfg.use_lagrangian != 0) == (s0->cfg.use_lagrangian != 0),
                  "member %d: members must share n_step, auto_alpha and use_lagrangian (learning rates, tau, seeds and data may differ)", i);
        CHECK_ARG(c->cfg.n_critics == c0->cfg.n_critics, "member %d: members must share n_critics (the lagrangians' row length)", i);
        for (int j = 0; j < i; ++j) CHECK_ARG(ctxs[j] != c, "member %d is listed twice", i);
    }
    HIPCHK(hipSetDevice(c0->device));
    fsrl_sac_group* g = new fsrl_sac_group();
    g->device = c0->device;
    g->ready.assign((size_t)k, nullptr);
    hipError_t e = hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&g->done, hipEventDisableTiming);
    for (int i = 0; i < k && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&g->ready[(size_t)i], hipEventDisableTiming);
    if (e == hipSuccess) e = hipMalloc(&g->d_tab, (size_t)k * sizeof(SacGroupMember));
    if (e == hipSuccess) e = hipHostMalloc(&g->h_tab, (size_t)k * sizeof(SacGroupMember));
    if (e != hipSuccess) {
        fail(FSRL_EHIP, "SAC group allocation failed: %s", hipGetErrorString(e));
        (void)fsrl_sac_group_destroy(g);
        return FSRL_EHIP;
    }
    for (int i = 0; i < k; ++i) { g->m.push_back(ctxs[i]); ctxs[i]->sac_group = g; }
    *out = g;
    return 0;
}

// a member's weight-gradient arguments (the grouped CVPO update, host_cvpo_group.inc, forms its members' here too).
// Batches of up to 512 padded rows: ppo_wgrad_body writes the final gradient into G.
static WgradPtrs group_wgrad_small(const SacState* s, int rp, const float* X, float* G) {
    WgradPtrs w{};
    w.A1 = s->A1; w.A2 = s->A2; w.D1 = s->D1; w.D2 = s->D2; w.DO = s->DO; w.X = X; w.grad = G;
    w.gsq_part = s->gsq_scratch; w.mbp_max = rp;
    return w;
}
// larger batches: sac_wgrad's split-K plan of `ny` networks for this member alone, its partials in the member's own buffer *G
static int group_wgrad_split(fsrl_ctx* c, const SacState* s, FbWgradArgs& wa, const ModelDesc& md, int ny, const float* X, int stride,
                             int B, const float** G, int* nsplit) {
    const int H = c->cfg.hidden, rp = s->n_tiles * 16;
    wa = FbWgradArgs{};
    for (int y = 0; y < ny; ++y) {
        FbWgradNet& wn = wa.nets[y];
        const size_t nb = (size_t)y * rp;
        wn.w2_ya = s->D2 + nb * H; wn.w2_xa = s->A1 + nb * H; wn.w2_yb = nullptr; wn.w2_xb = nullptr;
        wn.w1_y = s->D1 + nb * H; wn.w3_xa = s->A2 + nb * H; wn.w3_ya = s->DO + nb * FSRL_DOW;
        wn.w3_xb = nullptr; wn.w3_yb = nullptr; wn.b1_src = s->D1 + nb * H; wn.b2_src = s->D2 + nb * H;
        wn.do_src = s->DO + nb * FSRL_DOW; wn.net = y;
    }
    wa.obs = X; wa.rows = rp; wa.N = B;
    // wgrad_launch's fb_wgrad_kernel plan
    const int passes = 1 + std::max(0, (md.Do - 16 * 2 + 63) / 64);
    const int NB = (H / 64) * (H / 64) + (H / FB_AUX_COLS) * passes + 1;
    const WgradPlan pl = wgrad_plan(rp, NB * ny, c->n_cus);
    int rc = ensure_parts(c, stride, pl.nsplit);
    if (rc) return rc;
    wa.out = c->wg_parts; wa.ks_per_split = pl.ks_per_split; wa.split_stride = stride; wa.dbg_skip = 0;
    wa.aux_passes = passes; wa.remap_total = NB * ny * pl.nsplit; wa.remap_ny = ny;
    *G = c->wg_parts; *nsplit = pl.nsplit;
    return 0;
}

// the member's table entry: every argument of the nine launches as fsrl_sac_update forms it (library RNG, fold path)
static int sac_group_member(fsrl_ctx* c, SacState* s, SacGroupMember& t, int B, int64_t stored, const double* lags, double rescaling,
                            bool q_r4, bool a_r4, bool f_r4, bool small_wgrad, int* nsplit_q, int* nsplit_a) {
    const int Do = c->cfg.obs_dim, Da = c->cfg.act_dim, ns = s->cfg.n_step, H = c->cfg.hidden;
    const int nt = s->n_tiles, rp = nt * 16;
    const float lam = (s->cfg.use_lagrangian && lags) ? (float)lags[0] : 0.0f;
    const float resc = (float)rescaling;
    t = SacGroupMember{};
    t.PA = s->PA; t.MA = s->MA; t.VA = s->VA; t.PQ = s->PQ; t.PQT = s->PQT; t.MQ = s->MQ; t.VQ = s->VQ;
    // ---- the sample (sa.counter per step) and gather
    SacSampleArgs sa{}; SacGatherArgs ga{};
    sa.book = s->d_book; sa.flags = c->st.flags; sa.idx = s->d_idx; sa.chain = s->d_chain; sa.endbits = s->d_end;
    sa.eps_t = s->eps_t; sa.eps_p = s->eps_p; sa.env_num = c->cfg.env_num; sa.sub_size = (int)c->sub_size; sa.B = B;
    sa.n_step = ns; sa.Da = Da; sa.stored = (unsigned long long)stored; sa.key = s->key; sa.counter = 0;
    ga.st = c->st; ga.idx = s->d_idx; ga.term = s->d_chain + (size_t)(ns - 1) * B; ga.XQ = s->XQ; ga.OBS = s->OBS;
    ga.OBSN = s->OBSN; ga.XN = s->XN; ga.XP = s->XP; ga.B = B; ga.Do = Do; ga.Da = Da;
    // ---- actors
    auto actor = [&](SacActorArgs& aa, const float* obs, const float* eps, float* X, float* lp, int mode) {
        aa = SacActorArgs{};
        aa.deterministic = 0; aa.max_action = c->cfg.max_action;
        aa.obs = obs; aa.eps = eps; aa.X = X; aa.lp_out = lp; aa.DA = s->DA; aa.QP = s->QP; aa.sc = s->sc; aa.A1 = s->A1; aa.A2 = s->A2;
        aa.cr = -resc; aa.cc = s->cfg.use_lagrangian ? resc * lam : 0.0f;
        aa.D1 = s->D1; aa.D2 = s->D2; aa.DO = s->DO; aa.statp = s->stpi; aa.B = B; aa.mode = mode; aa.rescale = resc;
        aa.auto_alpha = s->cfg.auto_alpha; aa.alpha_fixed = s->cfg.alpha;
        aa.probe = 0;
    };
    actor(t.af, s->OBSN, s->eps_t, s->XN, s->LPN, SAC_A_FWD);
    t.af.P2 = s->PA; t.af.obs2 = s->OBS; t.af.eps2 = s->eps_p; t.af.X2 = s->XP; t.af.lp2 = s->LP; t.af.tiles_half = f_r4 ? 4 * nt : nt;
    t.af.sg_on = 1; t.af.sa = sa; t.af.ga = ga;
    actor(t.ab, s->OBS, s->eps_p, s->XP, s->LP, SAC_A_BWD);
    // ---- Q-network tile launches
    SacNstepArgs na{};
    na.QT = s->QT; na.lpn = s->LPN; na.chain = s->d_chain; na.endbits = s->d_end; na.rew = c->st.rew; na.cost = c->st.cost;
    na.flags = c->st.flags; na.sc = s->sc; na.Y = s->Y; na.B = B; na.n_step = ns; na.gamma = c->cfg.gamma;
    na.auto_alpha = s->cfg.auto_alpha; na.alpha_fixed = s->cfg.alpha; na.single = 0;
    auto q = [&](FbArgs& a, const float* X, int mode, float* statp, float* qout, const SacNstepArgs* nsa) {
        a = FbArgs{};
        a.obs = X; a.rd = nullptr; a.A1 = s->A1; a.A2 = s->A2; a.D1 = s->D1; a.D2 = s->D2; a.DO = s->DO; a.statp = statp;
        a.N = B; a.rows_pad = rp; a.mode = mode; a.net0 = 0; a.cr = 0.f; a.cc = 0.f; a.max_action = 1.0f;
        a.tgt = s->Y; a.qout = qout; a.qin = s->QP; a.da_out = s->DA;
        a.act_cols = Da; a.pair_shift = 1;
        if (nsa) { a.ns_on = 1; a.ns = *nsa; }
    };
    q(t.qf, s->XN, FB_MODE_Q_FWD, s->stq, s->QT, nullptr);
    q(t.qt, s->XQ, FB_MODE_Q_TRAIN, s->stq, s->QP, &na);
    q(t.qd, s->XP, FB_MODE_Q_DIN, s->stdin_, s->QP, nullptr);
    // ---- weight gradients: sac_wgrad's plan for this member alone
    if (small_wgrad) {
        int rc = ensure_parts(c, s->nq_dev, 1);
        if (rc) return rc;
        t.GQ = c->wg_parts;
        rc = ensure_parts(c, s->na_dev, 1);
        if (rc) return rc;
        t.GA = c->wg_parts;
        if (!s->gsq_scratch) HIPCHK(hipMalloc(&s->gsq_scratch, (size_t)wg_grid(256, FSRL_MAX_NETS) * 4));
        t.wq = group_wgrad_small(s, rp, s->XQ, const_cast<float*>(t.GQ));
        t.wa = group_wgrad_small(s, rp, s->OBS, const_cast<float*>(t.GA));
        *nsplit_q = *nsplit_a = 1;
    } else {
        int rc = group_wgrad_split(c, s, t.fq, s->mdq, 4, s->XQ, s->nq_dev, B, &t.GQ, nsplit_q);
        if (rc) return rc;
        rc = group_wgrad_split(c, s, t.fa, s->mda, 1, s->OBS, s->na_dev, B, &t.GA, nsplit_a);
        if (rc) return rc;
    }
    // ---- the logged row (fin.stats per step) and Adam's constants
    SacFinalArgs& fa = t.fin;
    fa.statp_q = s->stq; fa.statp_pi = s->stpi; fa.sc = s->sc; fa.stats = nullptr;
    fa.n_tiles_q = q_r4 ? 4 * nt : nt; fa.n_tiles_pi = a_r4 ? 4 * nt : nt; fa.B = B; fa.rescale = resc; fa.lam = lam;
    fa.target_entropy = s->cfg.target_entropy;
    fa.alpha_lr = s->cfg.alpha_lr; fa.beta1 = c->cfg.beta1; fa.beta2 = c->cfg.beta2; fa.adam_eps = c->cfg.adam_eps;
    fa.alpha_fixed = s->cfg.alpha; fa.auto_alpha = s->cfg.auto_alpha; fa.use_lagrangian = s->cfg.use_lagrangian; fa.n_q = 4;
    t.stats = s->d_stats; t.nstats = s->nstats;
    const double b1 = c->cfg.beta1, b2 = c->cfg.beta2;
    t.one_minus_b1 = (float)(1.0 - b1); t.beta2 = c->cfg.beta2; t.one_minus_b2 = (float)(1.0 - b2); t.adam_eps = c->cfg.adam_eps;
    t.tau = s->cfg.tau; t.one_minus_tau = (float)(1.0 - (double)s->cfg.tau);
    return 0;
}

extern "C" int fsrl_sac_group_update(fsrl_sac_group* g, int32_t B, const int32_t* n_updates, const double* lagrangians,
                                     const double* rescaling) {
    CHECK_ARG(g && n_updates && rescaling, "null argument");
    if (g->broken) return fail(FSRL_ESTATE, "a member of this SAC group was destroyed: destroy the group");
    CHECK_ARG(B >= 1, "batch_size must be >= 1");
    const int k = (int)g->m.size();
    fsrl_ctx* c0 = g->m[0];
    SacState* s0 = sac_of(c0);
    int n_max = 0;
    for (int i = 0; i < k; ++i) {
        fsrl_ctx* c = g->m[i];
        const SacState* s = sac_of(c);
        CHECK_ARG(n_updates[i] >= 0, "n_updates[%d] < 0", i);
        CHECK_ARG(s && !s->cvpo && !s->ddpg && !s->layered && s->cfg.n_step == s0->cfg.n_step, "member %d is no longer a SAC-Lagrangian context of the group's shape", i);
        CHECK_ARG(s->wgrad_splitk == s0->wgrad_splitk, "members must agree on fsrl_sac_set_plan bit 0 (split-K weight gradients)");
        // fsrl_tr_set_plan's one-pass streaming weight gradients (256 wide, >= 4096 rows) would give this member another kernel alone
        // (fb_wgrad2_kernel); the tiled kernel fb_wgrad3_kernel needs re-laid observations the replay agents never hand over
        CHECK_ARG(!(c->wgrad_stream && c->cfg.hidden == 256 && (B + 15) / 16 * 16 >= 4096),
                  "member %d: the streaming weight-gradient plan (fsrl_tr_set_plan wgrad = 3) is not grouped", i);
        if (n_updates[i] > 0) CHECK_ARG(fsrl_store_len(c) > 0, "member %d: empty replay store", i);
        n_max = std::max(n_max, (int)n_updates[i]);
    }
    CHECK_ARG(!s0->cfg.use_lagrangian || lagrangians, "lagrangians: [k][n_critics - 1] when use_lagrangian is on");
    if (n_max == 0) return 0;
    HIPCHK(hipSetDevice(g->device));
    HIPCHK(hipStreamSynchronize(g->stream));           // the pinned tables of the previous call have been read
    const int H = c0->cfg.hidden, nt = (B + 15) / 16, rp = nt * 16, n_q = 4;
    // tile heights: the single-context rule applied to the group's whole launch (4-row tiles while it fits one round)
    const bool t16 = c0->probe_tile16;
    const bool q_r4 = (size_t)4 * nt * n_q * k <= (size_t)c0->n_cus && !t16;
    const bool a_r4 = (size_t)4 * nt * k <= (size_t)c0->n_cus && !t16;
    const bool f_r4 = a_r4 && (size_t)8 * nt * k <= (size_t)c0->n_cus;
    const bool small_wgrad = rp <= 512 && !s0->wgrad_splitk;
    const size_t lag_stride = (size_t)std::max(1, c0->cfg.n_critics - 1);
    if ((size_t)n_max * k > g->cap_steps) {
        if (g->d_steps) HIPCHK(hipFree(g->d_steps));
        if (g->h_steps) HIPCHK(hipHostFree(g->h_steps));
        g->d_steps = nullptr; g->h_steps = nullptr; g->cap_steps = 0;
        const size_t cap = std::max<size_t>((size_t)n_max * k, 64);
        HIPCHK(hipMalloc(&g->d_steps, cap * sizeof(SacGroupStep)));
        HIPCHK(hipHostMalloc(&g->h_steps, cap * sizeof(SacGroupStep)));
        g->cap_steps = cap;
    }
    // ---- every member with work: its resident actor ends, its pushes land, its batch buffers and sub-buffer books are current
    int nsq = 1, nsa = 1, rq_total = 0, ra_total = 0;
    for (int i = 0; i < k; ++i) {
        fsrl_ctx* c = g->m[i];
        SacState* s = sac_of(c);
        if (n_updates[i] == 0) continue;
        ENTER_DEV(c);
        int rc = join_store(c);
        if (rc) return rc;
        rc = sac_alloc_batch(c, s, B);
        if (rc) return rc;
        if (s->book_version != c->store_version) {
            HIPCHK(hipStreamSynchronize(c->compute));
            if (s->pre_valid && s->pre_side) HIPCHK(hipEventSynchronize(s->pre_done));
            s->pre_valid = false;
            for (int e = 0; e < c->cfg.env_num; ++e) {
                const EnvBook& eb = c->env[(size_t)e];
                s->h_book[e] = SacBook{(int)eb.size, (int)eb.index, (int)eb.last_index, 0};
            }
            HIPCHK(hipMemcpyAsync(s->d_book, s->h_book, (size_t)c->cfg.env_num * sizeof(SacBook), hipMemcpyHostToDevice, c->compute));
            if (s->book_done && s->plan_prefetch) HIPCHK(hipEventRecord(s->book_done, c->compute));
            s->book_version = c->store_version;
        }
        // the member's own side-stream prefetch writes the other set of batch buffers only: nothing to wait for
        const double* lg = s0->cfg.use_lagrangian ? lagrangians + (size_t)i * lag_stride : nullptr;
        int q_split = 1, a_split = 1;
        rc = sac_group_member(c, s, g->h_tab[i], B, fsrl_store_len(c), lg, rescaling[i], q_r4, a_r4, f_r4, small_wgrad, &q_split, &a_split);
        if (rc) return rc;
        nsq = q_split; nsa = a_split;                  // one shape, one plan: the same for every member
        rq_total = g->h_tab[i].fq.remap_total; ra_total = g->h_tab[i].fa.remap_total;
        HIPCHK(hipEventRecord(g->ready[(size_t)i], c->compute));
        HIPCHK(hipStreamWaitEvent(g->stream, g->ready[(size_t)i], 0));
    }
    // ---- the step table: what each member's own fsrl_sac_update calls would use
    for (int u = 0; u < n_max; ++u)
        for (int i = 0; i < k; ++i) {
            SacGroupStep& st = g->h_steps[(size_t)u * k + i];
            st = SacGroupStep{};
            if (u >= n_updates[i]) continue;
            const fsrl_ctx* c = g->m[i];
            const SacState* s = sac_of(const_cast<fsrl_ctx*>(c));
            const int64_t n = s->n_updates + u, tc = s->t_critic + u + 1, ta = s->t_actor + u + 1;
            const double b1 = c->cfg.beta1, b2 = c->cfg.beta2;
            st.sa = g->h_tab[i].af.sa; st.sa.counter = (unsigned long long)n; st.row = (int)(n % SAC_RING); st.active = 1;
            st.c_step = (float)((double)s->cfg.critic_lr / (1.0 - std::pow(b1, (double)tc)));
            st.c_bc2 = (float)std::sqrt(1.0 - std::pow(b2, (double)tc));
            st.a_step = (float)((double)s->cfg.actor_lr / (1.0 - std::pow(b1, (double)ta)));
            st.a_bc2 = (float)std::sqrt(1.0 - std::pow(b2, (double)ta));
        }
    hipStream_t gs = g->stream;
    HIPCHK(hipMemcpyAsync(g->d_tab, g->h_tab, (size_t)k * sizeof(SacGroupMember), hipMemcpyHostToDevice, gs));
    HIPCHK(hipMemcpyAsync(g->d_steps, g->h_steps, (size_t)n_max * k * sizeof(SacGroupStep), hipMemcpyHostToDevice, gs));
    const ModelDesc mda = s0->mda, mdq = s0->mdq;
    const int na_dev = s0->na_dev, nq_dev = s0->nq_dev;
    const SacGroupMember* tab = g->d_tab;
    int rc = dispatch_H(H, [&](auto hc) {
        constexpr int HH = decltype(hc)::value;
        const int ft = f_r4 ? 4 * nt : nt, qt = q_r4 ? 4 * nt : nt, at = a_r4 ? 4 * nt : nt;
        const int gq = round_up(rq_total, 8), ga = round_up(ra_total, 8);
        for (int u = 0; u < n_max; ++u) {
            const SacGroupStep* st = g->d_steps + (size_t)u * k;
            // 1. both actors' forward, the sample drawn and gathered inside
            if (f_r4) hipLaunchKernelGGL((sac_actor_group_kernel<HH, 4, SAC_A_FWD>), dim3(2 * ft, k), dim3(4 * HH), 0, gs, mda, tab, st);
            else hipLaunchKernelGGL((sac_actor_group_kernel<HH, 16, SAC_A_FWD>), dim3(2 * ft, k), dim3(4 * HH), 0, gs, mda, tab, st);
            // 2. target Q-networks on (s_{t+n}, a'); 3. the critics' forward + backward with their n-step targets
            if (q_r4) {
                hipLaunchKernelGGL((sac_q_group_kernel<HH, 4, 0>), dim3(qt, n_q, k), dim3(4 * HH), 0, gs, mdq, tab, st);
                hipLaunchKernelGGL((sac_q_group_kernel<HH, 4, 1>), dim3(qt, n_q, k), dim3(4 * HH), 0, gs, mdq, tab, st);
            } else {
                hipLaunchKernelGGL((sac_q_group_kernel<HH, 16, 0>), dim3(qt, n_q, k), dim3(4 * HH), 0, gs, mdq, tab, st);
                hipLaunchKernelGGL((sac_q_group_kernel<HH, 16, 1>), dim3(qt, n_q, k), dim3(4 * HH), 0, gs, mdq, tab, st);
            }
            // 4. the critics' weight gradients; 5. their Adam with the Polyak targets
            if (small_wgrad) hipLaunchKernelGGL((sac_wgrad_group_kernel<HH, 0>), dim3(wg_grid(HH, n_q), k), dim3(1024), 0, gs, mdq, tab, st, rp);
            else hipLaunchKernelGGL((sac_wgrad_split_group_kernel<HH, 0>), dim3(gq, k), dim3(1024), 0, gs, mdq, tab, st);
            hipLaunchKernelGGL(sac_adam_group_kernel, dim3((nq_dev + 255) / 256, k), dim3(256), 0, gs, mdq, tab, st, nq_dev, nsq, nq_dev);
            // 6. Q(s, a ~ pi) with the updated critics + dQ/da; 7. the actor's backward
            if (q_r4) hipLaunchKernelGGL((sac_q_group_kernel<HH, 4, 2>), dim3(qt, n_q, k), dim3(4 * HH), 0, gs, mdq, tab, st);
            else hipLaunchKernelGGL((sac_q_group_kernel<HH, 16, 2>), dim3(qt, n_q, k), dim3(4 * HH), 0, gs, mdq, tab, st);
            if (a_r4) hipLaunchKernelGGL((sac_actor_group_kernel<HH, 4, SAC_A_BWD>), dim3(at, k), dim3(4 * HH), 0, gs, mda, tab, st);
            else hipLaunchKernelGGL((sac_actor_group_kernel<HH, 16, SAC_A_BWD>), dim3(at, k), dim3(4 * HH), 0, gs, mda, tab, st);
            // 8. the actor's weight gradients; 9. its Adam, alpha step and logged row
            if (small_wgrad) hipLaunchKernelGGL((sac_wgrad_group_kernel<HH, 1>), dim3(wg_grid(HH, 1), k), dim3(1024), 0, gs, mda, tab, st, rp);
            else hipLaunchKernelGGL((sac_wgrad_split_group_kernel<HH, 1>), dim3(ga, k), dim3(1024), 0, gs, mda, tab, st);
            hipLaunchKernelGGL(sac_adam_final_group_kernel, dim3((na_dev + 255) / 256 + 1, k), dim3(256), 0, gs, mda, tab, st, na_dev, nsa, na_dev);
            HIPCHK(hipGetLastError());
        }
        return 0;
    });
    if (rc) return rc;
    HIPCHK(hipEventRecord(g->done, gs));
    // ---- each member's streams wait for the call; its bookkeeping is that of n_i own updates
    for (int i = 0; i < k; ++i) {
        if (n_updates[i] == 0) continue;
        fsrl_ctx* c = g->m[i];
        SacState* s = sac_of(c);
        HIPCHK(hipStreamWaitEvent(c->compute, g->done, 0));
        HIPCHK(hipStreamWaitEvent(c->side, g->done, 0));     // a push must not overwrite rows the call still samples
        s->n_updates += n_updates[i]; s->t_critic += n_updates[i]; s->t_actor += n_updates[i];
        s->last_B = B;
        s->pre_valid = false;                                // no rider blocks ran: the member's next own update draws its sample
    }
    return 0;
}
