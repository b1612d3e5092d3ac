// host_trust.inc -- trust-region updates (CPO, TRPO-Lagrangian): fsrl_tr_* / fsrl_cpo_learn / fsrl_trpo_learn (part of fsrl_hip.hip).
// Included once by fsrl_hip.hip: same translation unit, so the static helpers and fsrl_ctx above are visible.
// ====================================================================================== trust region
// CPO / TRPO-Lagrangian: full-batch primitives on the device, the (tiny) flat-vector algebra of
// conjugate gradients, the dual solve and the line search on the host in float32.
struct TrState {
    fsrl_tr_config cfg{};
    bool ready = false;
    int rows_pad = 0, n_tiles = 0;      // rows_pad: per-network stride of the side buffers (multiple of 32); n_tiles: 16-row tiles covering N
    int rows16 = 0;                     // 16 * n_tiles: the rows the weight-side kernels walk
    // the rows the full-batch kernels currently work on: the whole batch in store order, or one minibatch of a permuted
    // copy (Batch.split inside learn, cpo.py:357-358 / trpo_lag.py:178): contiguous rows either way
    const float* vobs = nullptr; float* vrd = nullptr; int64_t vN = 0;
    // r6: the view's observations re-laid for fb_wgrad3_kernel's float4 operand loads (kernels_wgrad3.hpp), built once per view on
    // the compute stream BEFORE the critic lane forks (tr_ensure_pad)
    float* obs_pad = nullptr; int pad_ko = 1; bool pad_valid = false;
    // ---- r5: the critics' regression steps on a stream of their own, side by side with the actor's step (CriticLane below)
    hipStream_t cstream = nullptr;
    hipEvent_t ev_fork = nullptr;
    float *cA1 = nullptr, *cA2 = nullptr, *cD1 = nullptr, *cD2 = nullptr, *cDO = nullptr, *cstatp = nullptr;
    double *c_d_scal = nullptr, *c_d_ssq = nullptr;
    double* h_crit = nullptr;           // pinned: [C * FB_NSTAT] batch sums of the last step | [32 * C] squared-norm partials
    fsrl_ctx::Parts c_parts;            // the lane's split-K partials (swapped into fsrl_ctx::parts while the lane is current): like every
                                        // Parts block it is ensure_parts' and so the context's (c->mem), never this state's
    bool crit_pending = false; int crit_l2 = 0;
    bool opt_overlap = true;            // fsrl_tr_set_plan(tile_rows + 64): critic steps on the compute stream, one after the other (A/B)
    uint64_t rd_version = 0;            // fsrl_ctx::theta_version when mean_old / std_old of the batch (view) were computed
    bool opt_gn = true;                 // fsrl_tr_set_plan bit: the Gauss-Newton form of the KL product where it is exact (A/B: off)
    bool hvp_valid = false;             // A1 / A2 / D2 / DO hold h1 / h2 / dz2 / dout of the KL head at the current theta and batch
    uint64_t hvp_version = 0, hvp_rd_version = 0;   // fsrl_ctx::theta_version / rd_version when that cache was filled: a cached product
                                        // is taken only while both still hold (an external parameter upload or restore in between
                                        // bumps theta_version, so a caller's stale promise cannot read the old theta's activations)
    unsigned* co_counter = nullptr;     // device tile counter of the persistent co-resident launches (never reset: CoSched)
    unsigned co_base = 0u;
    bool co_static = true;              // one workgroup per tile (default); fsrl_tr_set_tile_split(-2, -2): persistent workgroups (A/B)
    int co_delay_tile = 0, co_delay_hvp = 0;   // fsrl_tr_set_co_delay: s_sleep(127) periods the second resident of a CU starts late
    int split_tile = -1, split_hvp = -1;  // fsrl_tr_set_tile_split: forced 32-row tile counts of the co-resident launches (-1 = simulate)
    int opt_tile_rows = 0, opt_hvp = 0; // fsrl_tr_set_plan: 0 = automatic; tile_rows 16 = 16-row tiles only; hvp 1 = legacy kernel, 2 = mixed without the cache
    struct Plan { int64_t N; int ny; int kind; int n32, n16; };
    std::vector<Plan> plans;            // mixed_plan results, keyed by (N, ny, kind)
    float *A1 = nullptr, *A2 = nullptr, *D1 = nullptr, *D2 = nullptr, *DO = nullptr;      // [nets][rows_pad]
    float *RA1 = nullptr, *RA2 = nullptr, *RD1 = nullptr, *RD2 = nullptr, *RDO = nullptr;  // [rows_pad]
    float *statp = nullptr, *mu_old = nullptr, *Vdev = nullptr, *Out = nullptr, *rd = nullptr;
    float *cg_r = nullptr, *cg_x = nullptr, *cg_g = nullptr;     // device-resident CG vectors (actor layout)
    float* vec = nullptr;           // [8][n_dev] g | b | H^-1 g | H^-1 b | (H + damping) H^-1 g | (H + damping) H^-1 b | dir | theta0
    double* h_part = nullptr;       // pinned [4 * CG_NB] partial dot products / [FSRL_MAX_ACT] floats of sigma_param behind them
    // r6 (late): read-backs without a copy launch and a stream synchronisation -- the reducing kernels write their sums to h_rb and one
    // completion word per block to h_rb_done (pinned), the host polls for rb_seq (rb_wait); fsrl_tr_set_plan(tile_rows + 128) keeps
    // hipMemcpyAsync + hipStreamSynchronize (A/B)
    double* h_rb = nullptr; unsigned* h_rb_done = nullptr; unsigned rb_seq = 0u;
    bool opt_poll = true;
    CgScal* cg_sc = nullptr;
    double* cg_part = nullptr;                                   // [3 * CG_NB]: p.z partials | r.r partials (two halves), float64
    double* d_scal = nullptr;
    double* d_ssq = nullptr;        // [32 * n_critics] partial sums of squares (l2 term of the logged critic loss)
    size_t cap_rows = 0;
    Mem mem;
    int64_t critic_t = 0;     // Adam step count of the critic optimiser
    int na = 0;               // flat actor parameter count (API order)
    std::vector<int32_t> ls_iters;   // line-search evaluations of every repeat of the last learn call
};
static int actor_tensors(const fsrl_ctx* c) { return c->lay ? 1 + 2 * (c->lay->L + 1) : 7; }     // sigma_param + (W, b) of every Linear
static TrState* tr_of(fsrl_ctx* c) {
    if (!c->tr) {
        c->tr = new TrState();
        c->tr->na = (int)fsrl_actor_param_count(c);
    }
    return c->tr;
}

static void tr_reset_optim(fsrl_ctx* c) { if (c->tr) c->tr->critic_t = 0; }
static int64_t tr_critic_steps_taken(fsrl_ctx* c) { return c->tr ? c->tr->critic_t : 0; }
static void tr_set_critic_steps(fsrl_ctx* c, int64_t t) { if (c->tr) { c->tr->critic_t = t; c->tr->hvp_valid = false; } }

static void tr_free(fsrl_ctx* c) {
    TrState* t = c->tr;
    if (!t) return;
    if (t->cstream) { (void)hipStreamSynchronize(t->cstream); (void)hipStreamDestroy(t->cstream); }
    if (t->ev_fork) (void)hipEventDestroy(t->ev_fork);
    t->mem.release_all();
    delete t;
    c->tr = nullptr;
}

extern "C" int64_t fsrl_actor_param_count(const fsrl_ctx* c) {
    if (!c) return 0;
    int64_t n = 0;
    for (int i = 0; i < actor_tensors(c); ++i) n += c->tmap[i].n();
    return n;
}

static void tr_set_view(TrState* t, const float* obs, float* rd, int64_t n) {
    t->vobs = obs; t->vrd = rd; t->vN = n;
    t->n_tiles = (int)((n + 15) / 16); t->rows16 = t->n_tiles * 16;
    t->hvp_valid = false;
    t->pad_valid = false;
}
// obs_pad := the current view's observations in fb_wgrad3_kernel's layout.  Called on the compute stream by everything that is
// about to launch weight-side products (and by tr_critic_enqueue before the lane's stream forks off, so both chains see it).
static int tr_ensure_pad(fsrl_ctx* c, TrState* t) {
    if (t->pad_valid || !t->obs_pad || c->lay) return 0;
    hipLaunchKernelGGL(fb_obs_pad_kernel, dim3(1024), dim3(256), 0, c->compute, t->vobs, t->obs_pad, (int)t->vN, c->cfg.obs_dim,
                       t->rows16, t->pad_ko);
    HIPCHK(hipGetLastError());
    t->pad_valid = true;
    return 0;
}
static int tr_alloc(fsrl_ctx* c, TrState* t, int64_t n) {
    t->rows_pad = 32 * (int)((n + 31) / 32);        // per-network stride of the side buffers: a 32-row tile may write 16 rows past
                                                    // the last 16-row boundary, they stay inside the network's slab
    t->hvp_valid = false;
    const int tiles = (int)((n + 15) / 16);
    if (t->cstream) HIPCHK(hipStreamSynchronize(t->cstream));     // a critic chain left in flight by a failed call
    t->crit_pending = false;
    if ((size_t)t->rows_pad <= t->cap_rows) return 0;
    HIPCHK(hipStreamSynchronize(c->compute));
    t->cap_rows = 0;            // from here until the whole working set stands: also the layered one and the once-only block
    const size_t rows = (size_t)t->rows_pad + 64, H = c->cfg.hidden, nn = c->md.n_nets;
    if (c->lay) {               // layered context: the layer-by-layer working set (host_layered.inc) instead of the tile kernels' slabs
        int rc = lay_ensure_rows(c, t->rows_pad, true);
        if (rc) return rc;
    }
    if (!t->ev_fork) {              // once; ev_fork comes last, so a failure in here is tried again
        HIPCHK(t->mem.dev(&t->Vdev, (size_t)c->n_alloc * 4)); HIPCHK(t->mem.dev(&t->Out, (size_t)c->n_dev * 4));
        for (float** p : {&t->cg_r, &t->cg_x, &t->cg_g}) {
            HIPCHK(t->mem.dev(p, (size_t)c->n_dev * 4));
            HIPCHK(hipMemsetAsync(*p, 0, (size_t)c->n_dev * 4, c->compute));
        }
        HIPCHK(t->mem.dev(&t->vec, (size_t)8 * c->n_dev * 4));
        HIPCHK(hipMemsetAsync(t->vec, 0, (size_t)8 * c->n_dev * 4, c->compute));
        HIPCHK(t->mem.pinned(&t->h_part, (4 * CG_NB + FSRL_MAX_ACT) * sizeof(double)));
        HIPCHK(t->mem.pinned(&t->h_rb, 4 * CG_NB * sizeof(double)));
        HIPCHK(t->mem.pinned(&t->h_rb_done, CG_NB * sizeof(unsigned)));
        memset(t->h_rb_done, 0, CG_NB * sizeof(unsigned));
        HIPCHK(t->mem.dev(&t->cg_sc, sizeof(CgScal)));
        HIPCHK(t->mem.dev(&t->cg_part, 4 * CG_NB * sizeof(double)));
        HIPCHK(t->mem.dev(&t->co_counter, 64));
        HIPCHK(hipMemsetAsync(t->co_counter, 0, 64, c->compute));
        t->co_base = 0u;
        HIPCHK(hipMemsetAsync(t->Vdev, 0, (size_t)c->n_alloc * 4, c->compute)); HIPCHK(hipMemsetAsync(t->Out, 0, (size_t)c->n_dev * 4, c->compute));
        HIPCHK(hipStreamSynchronize(c->compute));
        HIPCHK(t->mem.dev(&t->d_scal, 64 * sizeof(double)));
        HIPCHK(t->mem.dev(&t->d_ssq, 32 * FSRL_MAX_CRITICS * sizeof(double)));
        HIPCHK(t->mem.dev(&t->c_d_scal, 64 * sizeof(double)));
        HIPCHK(t->mem.dev(&t->c_d_ssq, 32 * FSRL_MAX_CRITICS * sizeof(double)));
        HIPCHK(t->mem.pinned(&t->h_crit, (FSRL_MAX_CRITICS * FB_NSTAT + 32 * FSRL_MAX_CRITICS) * sizeof(double)));
        if (!t->cstream) HIPCHK(hipStreamCreateWithFlags(&t->cstream, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&t->ev_fork, hipEventDisableTiming));
    }
    // the tile kernels' slabs (not layered); obs_pad at 256 wide; the critic lane's own slabs (nets 1 .. C), so that its launches
    // never touch what the actor's read
    const size_t slab = c->lay ? 0 : rows * H * 4, dow = c->lay ? 0 : rows * FSRL_DOW * 4, cn = nn > 1 ? nn - 1 : 0;
    const size_t stat = (size_t)(tiles + 4) * nn * FB_NSTAT * 4;
    if (!c->lay && H == 256) t->pad_ko = (c->cfg.obs_dim + 63) / 64;
    HIPCHK(t->mem.regrow(t->cap_rows, (size_t)t->rows_pad, (size_t)t->rows_pad,
                         {Mem::D(&t->A1, nn * slab), Mem::D(&t->A2, nn * slab), Mem::D(&t->D1, nn * slab), Mem::D(&t->D2, nn * slab),
                          Mem::D(&t->DO, nn * dow), Mem::D(&t->RA1, slab), Mem::D(&t->RA2, slab), Mem::D(&t->RD1, slab),
                          Mem::D(&t->RD2, slab), Mem::D(&t->RDO, dow),
                          Mem::D(&t->obs_pad, !c->lay && H == 256 ? rows * 64 * (size_t)t->pad_ko * 4 : 0),
                          Mem::D(&t->cA1, cn * slab), Mem::D(&t->cA2, cn * slab), Mem::D(&t->cD1, cn * slab), Mem::D(&t->cD2, cn * slab),
                          Mem::D(&t->cDO, cn * dow), Mem::D(&t->cstatp, c->lay || !cn ? 0 : stat),
                          Mem::D(&t->statp, stat), Mem::D(&t->mu_old, rows * c->cfg.act_dim * 4), Mem::D(&t->rd, rows * FSRL_RD * 4)}));
    return 0;
}

// flat ACTOR vector (API order) <-> device-layout vector
static int actor_to_dev(fsrl_ctx* c, const float* host, float* dev) {
    std::vector<float> tmp((size_t)c->md.net[0].end, 0.0f);
    for (int i = 0; i < actor_tensors(c); ++i) c->tmap[i].to_dev(tmp.data(), host);
    HIPCHK(hipStreamSynchronize(c->compute));
    HIPCHK(hipMemcpy(dev, tmp.data(), tmp.size() * 4, hipMemcpyHostToDevice));
    if (c->lay) return 0;       // no W2 mirror behind a layered parameter vector
    const int H = c->md.H;
    const NetOff& no = c->md.net[0];
    std::vector<float> mir((size_t)H * H);      // dev is P or a tangent vector: both carry the W2 mirror
    for (int n = 0; n < H; ++n)
        for (int k = 0; k < H; ++k) mir[(size_t)w2f_index(H, n, k)] = tmp[(size_t)no.W2 + (size_t)n * H + k];
    HIPCHK(hipMemcpy(dev + no.W2f, mir.data(), mir.size() * 4, hipMemcpyHostToDevice));
    return 0;
}
static int actor_from_dev(fsrl_ctx* c, const float* dev, float* host) {
    std::vector<float> tmp((size_t)c->md.net[0].end);
    HIPCHK(hipStreamSynchronize(c->compute));
    HIPCHK(hipMemcpy(tmp.data(), dev, tmp.size() * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < actor_tensors(c); ++i) c->tmap[i].to_api(host, tmp.data());
    return 0;
}

// row data of the whole batch in store order: act | logp_old | advs | rets | mean_old | std_old, the last two from the
// current policy (process_fn: cpo.py:139-143)
static int tr_build_rd(fsrl_ctx* c, TrState* t) {
    InferArgs ia{};
    ia.obs = c->b.obs; ia.obs_next = c->b.obs; ia.act = c->b.act; ia.flags = c->b.flags; ia.values = nullptr;
    ia.vnext = nullptr; ia.logp_old = nullptr; ia.mu_out = t->mu_old; ia.N = (int)c->N; ia.C = 0;
    ia.max_action = c->cfg.max_action;
    int rc = launch_infer(c, ia, 1, c->compute);
    if (rc) return rc;
    FbRowArgs ra{};
    ra.act = c->b.act; ra.advs = c->advs; ra.rets = c->rets; ra.logp_old = c->logp_old; ra.mean_old = t->mu_old;
    ra.sigma = c->P + c->md.net[0].sigma; ra.rd = t->rd; ra.N = (int)c->N; ra.C = c->cfg.n_critics; ra.Da = c->cfg.act_dim;
    hipLaunchKernelGGL(fb_rowdata_kernel, dim3(512), dim3(256), 0, c->compute, ra);
    HIPCHK(hipGetLastError());
    t->rd_version = c->theta_version;          // mean_old / std_old = the policy at this theta
    return 0;
}
// mean_old / std_old of the CURRENT VIEW's rows := current policy (TRPO recomputes old_dist at theta on every minibatch,
// trpo_lag.py:189-190); the other columns of the row data stay
static int tr_refresh_old(fsrl_ctx* c, TrState* t) {
    InferArgs ia{};
    ia.obs = t->vobs; ia.obs_next = t->vobs; ia.act = nullptr; ia.flags = c->b.flags; ia.values = nullptr;
    ia.vnext = nullptr; ia.logp_old = nullptr; ia.mu_out = t->mu_old; ia.N = (int)t->vN; ia.C = 0;
    ia.max_action = c->cfg.max_action;
    int rc = launch_infer(c, ia, 1, c->compute);
    if (rc) return rc;
    hipLaunchKernelGGL(fb_rd_old_kernel, dim3(256), dim3(256), 0, c->compute, t->vrd, t->mu_old, c->P + c->md.net[0].sigma,
                       (int)t->vN, c->cfg.act_dim);
    HIPCHK(hipGetLastError());
    t->hvp_valid = false;
    t->rd_version = c->theta_version;          // the view's mean_old / std_old = the policy at this theta
    return 0;
}

extern "C" int fsrl_tr_begin(fsrl_ctx* c, const fsrl_tr_config* cfg, int64_t* n_out) {
    CHECK_ARG(c && cfg, "null argument");
    CHECK_ARG(c->cfg.n_critics == 2, "CPO / TRPO-Lag need a reward and one cost critic");
    TrState* t = tr_of(c);
    t->cfg = *cfg;
    // reuse the PPO begin for sample(0) + V(obs), V(obs_next), GAE, logp_old (batch_size irrelevant)
    double zero = 0.0;
    int64_t n = 0;
    int rc = fsrl_ppo_begin(c, &zero, 1.0, 1 << 20, &n);
    if (rc) return rc;
    c->in_update = false;
    if (n_out) *n_out = n;
    t->ready = false;
    if (n == 0) return 0;
    rc = tr_alloc(c, t, n);
    if (rc) return rc;
    if (cfg->norm_adv) {
        hipLaunchKernelGGL(fb_advnorm_kernel, dim3(c->cfg.n_critics), dim3(1024), 0, c->compute, c->advs, (int)n);
        HIPCHK(hipGetLastError());
    }
    rc = tr_build_rd(c, t);
    if (rc) return rc;
    tr_set_view(t, c->b.obs, t->rd, n);
    HIPCHK(hipStreamSynchronize(c->compute));
    t->ready = true;
    return 0;
}

// wait for the completion words of the n blocks of the read-back launch just enqueued (bounded spin: ~2 s), else synchronise the
// stream -- which also surfaces a fault of any launch before it.  Everything enqueued on c->compute before that launch has
// completed when its words land (stream order), e.g. sigma_fetch's copy.
static unsigned rb_next(TrState* t) { t->rb_seq += 1; if (t->rb_seq == 0u) t->rb_seq = 1u; return t->rb_seq; }
static int rb_wait(fsrl_ctx* c, TrState* t, int n) {
    bool landed = true;
    for (int b = 0; b < n && landed; ++b) {
        long spins = 0;
        while (__atomic_load_n(&t->h_rb_done[b], __ATOMIC_ACQUIRE) != t->rb_seq) {
            if (++spins > 40000000L) { landed = false; break; }
            __builtin_ia32_pause();
        }
    }
    if (!landed) {
        HIPCHK(hipStreamSynchronize(c->compute));
        for (int b = 0; b < n; ++b)
            if (__atomic_load_n(&t->h_rb_done[b], __ATOMIC_ACQUIRE) != t->rb_seq) return fail(FSRL_EHIP, "read-back launch left no completion word");
    }
    return 0;
}
// One reducing launch of `blocks` blocks and its n doubles on the host.  `launch(hout, done, seq)` enqueues the kernel: with
// polled completion words (the default) it writes its sums to h_rb as well and *got = h_rb; otherwise (null words) `dev` is copied
// into `host` behind it, the stream is synchronised and *got = host.
template <class Launch>
static int tr_read_back(fsrl_ctx* c, TrState* t, int blocks, const double* dev, double* host, size_t n, const double** got, Launch&& launch) {
    const bool poll = t->opt_poll && t->h_rb && blocks <= CG_NB;
    launch(poll ? t->h_rb : nullptr, poll ? t->h_rb_done : nullptr, poll ? rb_next(t) : 0u);
    HIPCHK(hipGetLastError());
    *got = poll ? t->h_rb : host;
    if (poll) return rb_wait(c, t, blocks);
    HIPCHK(hipMemcpyAsync(host, dev, n * sizeof(double), hipMemcpyDeviceToHost, c->compute));
    HIPCHK(hipStreamSynchronize(c->compute));
    return 0;
}
static int tr_stats(fsrl_ctx* c, TrState* t, int ny, double* out) {
    const double* got = nullptr;
    int rc = tr_read_back(c, t, ny * FB_NSTAT, t->d_scal, out, (size_t)ny * FB_NSTAT, &got, [&](double* hout, unsigned* done, unsigned seq) {
        hipLaunchKernelGGL(fb_reduce_stats_kernel, dim3(ny * FB_NSTAT), dim3(256), 0, c->compute, t->statp, t->n_tiles, ny, t->d_scal,
                           hout, done, seq);
    });
    if (rc) return rc;
    if (got != out) memcpy(out, got, (size_t)ny * FB_NSTAT * sizeof(double));
    return 0;
}

// the simulated tile split (mixed_split, host_decisions.hpp) of a launch shape, computed once per (N, ny, kind)
static void mixed_plan(TrState* t, int64_t N, int ny, int n_cus, int kind, double rho, int* n32_out, int* n16_out) {
    for (const TrState::Plan& p : t->plans)
        if (p.N == N && p.ny == ny && p.kind == kind) { *n32_out = p.n32; *n16_out = p.n16; return; }
    const TileSplit sp = mixed_split(N, ny, n_cus, rho);
    t->plans.push_back({N, ny, kind, sp.n32, sp.n16});
    *n32_out = sp.n32; *n16_out = sp.n16;
}
// scheduling argument of a co-resident launch over `total` tiles on `grid` workgroups; advances the stream-ordered counter base
static CoSched co_sched(TrState* t, int total, int grid, int n_cus, int delay) {
    CoSched cs{};
    cs.total = total; cs.first_round = 2 * n_cus; cs.delay = delay;
    if (t->co_static || t->co_counter == nullptr) return cs;          // static grid: blockIdx.x is the tile
    cs.counter = t->co_counter; cs.base = t->co_base;
    t->co_base += (unsigned)(total + grid);                           // every workgroup draws once more than it processes
    return cs;
}
// tile split of a co-resident launch (two workgroups per CU): simulated, the persistent kernels' own, or forced (A/B)
static void co_split(fsrl_ctx* c, TrState* t, int ny, int kind, double rho, int forced32, int* n32, int* n16) {
    if (t->co_static) mixed_plan(t, t->vN, ny, 2 * c->n_cus, kind, rho, n32, n16);
    else co_plan(t->vN, 2 * c->n_cus, n32, n16);
    if (forced32 >= 0) forced_split(t->vN, forced32, n32, n16);
}
static constexpr double RHO_TILE = 0.62;   // fb_tile: 16-row / 32-row tile duration (profiles/r03_*)
static constexpr double RHO_HVP = 0.62;    // HVP tiles
static constexpr double RHO_HVP_CO = 0.60; // co-resident HVP tiles (two per CU)
static constexpr double RHO_TILE_CO = 0.60;
static constexpr int CO_DELAY_TILE = 0, CO_DELAY_HVP = 0;      // default start offsets of a CU's second resident (periods of 8 128 cycles)

static int tr_tile(fsrl_ctx* c, TrState* t, int mode, int net0, int ny, float cr, float cc) {
    FbArgs a{};
    a.obs = t->vobs; a.rd = t->vrd; a.A1 = t->A1; a.A2 = t->A2; a.D1 = t->D1; a.D2 = t->D2; a.DO = t->DO;
    a.statp = t->statp; a.N = (int)t->vN; a.rows_pad = t->rows_pad; a.mode = mode; a.net0 = net0; a.cr = cr; a.cc = cc;
    a.max_action = c->cfg.max_action;
#ifdef FSRL_PROBES
    { static const char* e = getenv("FSRL_TILE_PROBE"); if (e) a.eta = (float)atoi(e); }     // kernels_fbco.hpp TC_PROBE (results invalid)
#endif
    t->hvp_valid = false;                  // the side buffers now hold this launch's activations
    if (c->lay) {               // layer by layer: forward, the heads, the activation side of the backward pass
        LayState* ls = c->lay;
        int rc = lay_fwd(c, t->vobs, (int)t->vN, net0, ny);
        if (rc) return rc;
        LayFbHeadArgs h{};
        h.out = ls->out; h.dout = ls->dout; h.rd = t->vrd; h.statp = t->statp; h.P = c->P; h.sigma = ls->lm.net[0].sigma;
        h.mbp = ls->mbp; h.net0 = net0; h.ny = ny; h.Da = ls->lm.Da; h.unbounded = ls->lm.unbounded; h.N = (int)t->vN; h.mode = mode;
        h.max_action = c->cfg.max_action; h.cr = cr; h.cc = cc; h.eta = 0.0f;
        hipLaunchKernelGGL(lay_fb_head_kernel, dim3(t->n_tiles, ny), dim3(256), 0, c->compute, h);
        HIPCHK(hipGetLastError());
        return mode == FB_MODE_EVAL ? 0 : lay_bwd_dz(c, (int)t->vN, net0, ny);
    }
    // mixed 32 / 16-row tiles (fb_tile_mixed_kernel) when the plan says so; bit-identical to the 16-row grid
    int n32 = 0, n16 = t->n_tiles;
    if (c->cfg.hidden >= 128 && c->cfg.obs_dim <= 64 && t->opt_tile_rows != 16)
        mixed_plan(t, t->vN, ny, c->n_cus, 0, RHO_TILE, &n32, &n16);
    // r5: the same tiles as TWO co-resident 512-thread workgroups per CU (kernels_fbco.hpp); tile_rows plan 32 keeps r4's kernel
    const bool co = c->cfg.hidden == 256 && c->cfg.obs_dim <= 64 && c->cfg.act_dim <= 4 && t->opt_tile_rows == 0;
    if (co) co_split(c, t, ny, 3, RHO_TILE_CO, t->split_tile, &n32, &n16);
    return dispatch_H(c->cfg.hidden, [&](auto hc) {
        constexpr int H = decltype(hc)::value;
        if constexpr (H == 256) {
            if (co && n32 > 0) {
                const int total = ny * (n32 + n16);
                const int grid = t->co_static ? total : std::min(total, 2 * c->n_cus);
                const CoSched cs = co_sched(t, total, grid, c->n_cus, t->co_delay_tile);
                if (t->co_static) hipLaunchKernelGGL((fb_tile_co_kernel<H, false>), dim3(grid), dim3(2 * H), 0, c->compute, c->P, c->md, a, n32, n16, ny, cs);
                else hipLaunchKernelGGL((fb_tile_co_kernel<H, true>), dim3(grid), dim3(2 * H), 0, c->compute, c->P, c->md, a, n32, n16, ny, cs);
                HIPCHK(hipGetLastError());
                return 0;
            }
        }
        if constexpr (H >= 128) {
            if (n32 > 0) {
                hipLaunchKernelGGL(fb_tile_mixed_kernel<H>, dim3(ny * (n32 + n16)), dim3(4 * H), 0, c->compute, c->P, c->md, a,
                                   n32, n16, ny);
                HIPCHK(hipGetLastError());
                return 0;
            }
        }
        hipLaunchKernelGGL((fb_tile_kernel<H, 16>), dim3(t->n_tiles, ny), dim3(4 * H), 0, c->compute, c->P, c->md, a);
        HIPCHK(hipGetLastError());
        return 0;
    });
}

// out := the sum of the nparts split-K partials in c->wg_parts over the parameters of networks net0 .. net0 + ny - 1
static int tr_sum_parts(fsrl_ctx* c, TrState* t, int net0, int ny, float* out, int nparts) {
    const int begin = c->md.net[net0].begin, end = c->md.net[net0 + ny - 1].end;
    hipLaunchKernelGGL(fb_sum_parts_kernel, dim3((end - begin + 255) / 256), dim3(256), 0, c->compute, out, c->wg_parts,
                       begin, end, nparts, c->n_dev);
    HIPCHK(hipGetLastError());
    return 0;
}
// the observation operands of a weight-side launch over the current view (obs_pad brought up to date first)
static int tr_wgrad_obs(fsrl_ctx* c, TrState* t, FbWgradArgs& wa) {
    int rc = tr_ensure_pad(c, t);
    if (rc) return rc;
    wa.obs = t->vobs; wa.rows = t->rows16; wa.N = (int)t->vN;
    wa.obs_pad = t->pad_valid ? t->obs_pad : nullptr; wa.obs_ko = t->pad_ko;
    return 0;
}

// weight gradients from the side buffers: summed into `out`, or (parts_out) left as partials for the caller's next kernel to add up
static int tr_wgrad_plain(fsrl_ctx* c, TrState* t, int net0, int ny, float* out, int* parts_out = nullptr) {
    int nsplit = 1;
    if (c->lay) {               // one launch writes the finished gradient: handed on as a single "partial"
        int rc = lay_wgrad(c, t->vobs, (int)t->vN, net0, ny, c->lay->gvec, nullptr, false, true);
        if (rc) return rc;
        c->wg_parts = c->lay->gvec;
        nsplit = c->lay->gparts;
    } else {
        FbWgradArgs wa{};
        wgrad_fill_nets(wa, ny, net0, (size_t)c->cfg.hidden, (size_t)t->rows_pad, t->A1, t->A2, t->D1, t->D2, t->DO);
        int rc = tr_wgrad_obs(c, t, wa);
        if (rc) return rc;
        rc = wgrad_launch<false>(c, c->md, wa, ny, c->n_dev, &nsplit);
        if (rc) return rc;
    }
    if (parts_out) { *parts_out = nsplit; return 0; }
    return tr_sum_parts(c, t, net0, ny, out, nsplit);
}

// the 8 batch means of the actor's last tile launch
static int tr_means(fsrl_ctx* c, TrState* t, double* means8) {
    int rc = tr_stats(c, t, 1, means8);
    if (rc) return rc;
    for (int k = 0; k < FB_NSTAT; ++k) means8[k] /= (double)t->vN;
    return 0;
}
// gradient of a scalar actor objective into a device vector (actor layout) and the 8 batch means
static int tr_actor_grad_dev(fsrl_ctx* c, TrState* t, int mode, float cr, float cc, float* g_dev, double* means8) {
    int rc = tr_tile(c, t, mode, 0, 1, cr, cc);
    if (rc) return rc;
    rc = tr_wgrad_plain(c, t, 0, 1, g_dev);
    if (rc) return rc;
    return means8 ? tr_means(c, t, means8) : 0;
}

static int tr_eval_means(fsrl_ctx* c, TrState* t, double* means8) {
    int rc = tr_tile(c, t, FB_MODE_EVAL, 0, 1, 0.f, 0.f);
    return rc ? rc : tr_means(c, t, means8);
}

// H v for the tangent already in t->Vdev (main part + W2 mirror); result in t->Out (device).
// use_cache: the caller promises that theta, the batch and mean_old / std_old have not changed since the previous product
// (conjugate gradients: 22 products per CPO repeat at one theta); the first product after any other full-batch launch
// recomputes and re-spills the theta-only activations (t->hvp_valid), the later ones read them back.
static int tr_hvp_dev(fsrl_ctx* c, TrState* t, bool use_cache = false, int* parts_out = nullptr) {
    int rc = 0;
    if (c->lay) {
        rc = lay_hvp(c, t->vobs, t->vrd, (int)t->vN, t->Vdev, c->cfg.max_action,
                     use_cache && t->hvp_valid && t->hvp_version == c->theta_version && t->hvp_rd_version == t->rd_version);
        if (rc) return rc;
        t->hvp_valid = true; t->hvp_version = c->theta_version; t->hvp_rd_version = t->rd_version;
        c->wg_parts = c->lay->gvec;
        if (parts_out) { *parts_out = c->lay->gparts; return 0; }
        return tr_sum_parts(c, t, 0, 1, t->Out, c->lay->gparts);
    }
    HvpArgs ha{};
    ha.obs = t->vobs; ha.rd = t->vrd; ha.V = t->Vdev; ha.A1 = t->A1; ha.RA1 = t->RA1; ha.A2 = t->A2; ha.RA2 = t->RA2;
    ha.D2 = t->D2; ha.RD2 = t->RD2; ha.RD1 = t->RD1; ha.DO = t->DO; ha.RDO = t->RDO; ha.N = (int)t->vN;
    ha.rows_pad = t->rows_pad; ha.max_action = c->cfg.max_action;
    ha.ts = c->probe_ts;                 // null outside probe builds
    // Gauss-Newton form: exact whenever the batch's mean_old / std_old were computed at the present theta (every TRPO-Lag product;
    // CPO's products until its first line-search step moves theta).  All kernel plans take it alike (bit-identical plans).
    const bool gn = t->opt_gn && t->rd_version == c->theta_version;
    ha.gn = gn ? 1 : 0;
    const bool mixed = c->cfg.hidden >= 128 && c->cfg.obs_dim <= 64 && t->opt_hvp != 1;
    int n32 = 0, n16 = t->n_tiles;
    if (mixed) mixed_plan(t, t->vN, 1, c->n_cus, 1, RHO_HVP, &n32, &n16);
    const bool cached = mixed && use_cache && t->hvp_valid && t->opt_hvp != 2 && t->hvp_version == c->theta_version &&
                        t->hvp_rd_version == t->rd_version;
    // r5: the cached product as TWO co-resident 512-thread workgroups per CU (kernels_fbco.hpp); hvp plan 3 keeps r4's kernel
    // r6: the FIRST product of a solve (nothing cached yet) in the same form on the automatic plan: 262-357 -> 150-190 us per launch
    const bool co_first = !cached && mixed && use_cache && t->opt_hvp == 0 && t->co_static;
    const bool co = (cached || co_first) && c->cfg.hidden == 256 && t->opt_hvp != 3;
    if (co) co_split(c, t, 1, 2, RHO_HVP_CO, t->split_hvp, &n32, &n16);
    rc = dispatch_H(c->cfg.hidden, [&](auto hc) {
        constexpr int H = decltype(hc)::value;
        if constexpr (H == 256) {
            if (co) {
                const int total = n32 + n16;
                const int grid = t->co_static ? total : std::min(total, 2 * c->n_cus);
                const CoSched cs = co_sched(t, total, grid, c->n_cus, t->co_delay_hvp);
                if (!t->co_static && gn) hipLaunchKernelGGL((fb_hvp_co_kernel<H, true, true>), dim3(grid), dim3(2 * H), 0, c->compute, c->P, c->md, ha, n32, cs);
                else if (!t->co_static) hipLaunchKernelGGL((fb_hvp_co_kernel<H, true, false>), dim3(grid), dim3(2 * H), 0, c->compute, c->P, c->md, ha, n32, cs);
                else if (co_first && gn) hipLaunchKernelGGL((fb_hvp_co_kernel<H, false, true, true>), dim3(grid), dim3(2 * H), 0, c->compute, c->P, c->md, ha, n32, cs);
                else if (co_first) hipLaunchKernelGGL((fb_hvp_co_kernel<H, false, false, true>), dim3(grid), dim3(2 * H), 0, c->compute, c->P, c->md, ha, n32, cs);
                else if (gn) hipLaunchKernelGGL((fb_hvp_co_kernel<H, false, true>), dim3(grid), dim3(2 * H), 0, c->compute, c->P, c->md, ha, n32, cs);
                else hipLaunchKernelGGL((fb_hvp_co_kernel<H, false, false>), dim3(grid), dim3(2 * H), 0, c->compute, c->P, c->md, ha, n32, cs);
                HIPCHK(hipGetLastError());
                return 0;
            }
        }
        if constexpr (H >= 128) {
            if (mixed) {
                if (cached) hipLaunchKernelGGL((fb_hvp_mixed_kernel<H, true>), dim3(n32 + n16), dim3(4 * H), 0, c->compute, c->P, c->md, ha, n32);
                else hipLaunchKernelGGL((fb_hvp_mixed_kernel<H, false>), dim3(n32 + n16), dim3(4 * H), 0, c->compute, c->P, c->md, ha, n32);
                HIPCHK(hipGetLastError());
                return 0;
            }
        }
        hipLaunchKernelGGL(fb_hvp_tile_kernel<H>, dim3(t->n_tiles), dim3(4 * H), 0, c->compute, c->P, c->md, ha);
        HIPCHK(hipGetLastError());
        return 0;
    });
    if (rc) return rc;
    t->hvp_valid = true; t->hvp_version = c->theta_version; t->hvp_rd_version = t->rd_version;
    FbWgradArgs wa{};
    FbWgradNet& wn = wa.nets[0];
    wn.w2_ya = t->RD2; wn.w2_xa = t->A1; wn.w2_yb = t->D2; wn.w2_xb = t->RA1;     // R{dW2} = R{dz2}^T h1 + dz2^T R{h1}
    wn.w1_y = t->RD1;                                                             // R{dW1} = R{dz1}^T x
    wn.w3_xa = t->A2; wn.w3_ya = t->RDO; wn.w3_xb = t->RA2; wn.w3_yb = t->DO;     // R{dW3} = R{dout}^T h2 + dout^T R{h2}
    wn.b1_src = t->RD1; wn.b2_src = t->RD2; wn.do_src = t->RDO; wn.net = 0;
    int nsplit = 1;
    rc = tr_wgrad_obs(c, t, wa);
    if (rc) return rc;
    if (gn) {                    // dz2 = dout = 0: the second operand pairs vanish -- the one-pair weight-side launch, half the matrix work
        wn.w2_yb = wn.w2_xb = wn.w3_xb = wn.w3_yb = nullptr;
        rc = wgrad_launch<false>(c, c->md, wa, 1, c->n_dev, &nsplit);
    } else
    rc = wgrad_launch<true>(c, c->md, wa, 1, c->n_dev, &nsplit);
    if (rc) return rc;
    if (parts_out) { *parts_out = nsplit; return 0; }       // the caller's next kernel adds the partials up itself (tr_cg_dev)
    return tr_sum_parts(c, t, 0, 1, t->Out, nsplit);
}
static int tr_hvp(fsrl_ctx* c, TrState* t, const float* v, float* out, bool use_cache = false) {
    int rc = actor_to_dev(c, v, t->Vdev);
    if (rc) return rc;
    rc = tr_hvp_dev(c, t, use_cache);
    if (rc) return rc;
    return actor_from_dev(c, t->Out, out);
}

// Line-search evaluations (policy forwards over the batch) of every repeat of the last fsrl_cpo_learn /
// fsrl_trpo_learn call; returns how many were written.
extern "C" int32_t fsrl_tr_linesearch_evals(fsrl_ctx* c, int32_t* out, int32_t cap) {
    CHECK_ARG(c && out && cap >= 0, "bad argument");
    TrState* t = tr_of(c);
    const int32_t n = std::min<int32_t>(cap, (int32_t)t->ls_iters.size());
    for (int32_t i = 0; i < n; ++i) out[i] = t->ls_iters[(size_t)i];
    return n;
}

// what fsrl_tr_grad / _hvp / _hvp_cached check before they touch the device
static int tr_product_enter(fsrl_ctx* c, bool args, const char* name, int64_t n) {
    CHECK_ARG(c && args, "null argument");
    TrState* t = tr_of(c);
    if (!t->ready) return fail(FSRL_ESTATE, "%s before fsrl_tr_begin", name);
    CHECK_ARG(n == t->na, "expected %d actor parameters", t->na);
    ENTER_DEV(c);
    return 0;
}
extern "C" int fsrl_tr_grad(fsrl_ctx* c, int32_t which, float* out, int64_t n) {
    int rc = tr_product_enter(c, out != nullptr, "fsrl_tr_grad", n);
    if (rc) return rc;
    TrState* t = c->tr;
    CHECK_ARG(which >= 0 && which <= 2, "which must be 0, 1 or 2");      // reward surrogate | cost surrogate (negated) | KL
    rc = tr_actor_grad_dev(c, t, which == 2 ? FB_MODE_KL : FB_MODE_SUR, which == 0 ? 1.0f : 0.0f, which == 1 ? -1.0f : 0.0f, t->Out, nullptr);
    return rc ? rc : actor_from_dev(c, t->Out, out);
}
extern "C" int fsrl_tr_hvp(fsrl_ctx* c, const float* v, float* out, int64_t n) {
    int rc = tr_product_enter(c, v && out, "fsrl_tr_hvp", n);
    return rc ? rc : tr_hvp(c, c->tr, v, out);
}
// the same product for a caller that promises theta, the batch and mean_old / std_old are those of its previous fsrl_tr_hvp /
// fsrl_tr_hvp_cached call: the theta-only activations are read back (what conjugate gradients do inside the learn calls)
extern "C" int fsrl_tr_hvp_cached(fsrl_ctx* c, const float* v, float* out, int64_t n) {
    int rc = tr_product_enter(c, v && out, "fsrl_tr_hvp_cached", n);
    return rc ? rc : tr_hvp(c, c->tr, v, out, true);
}
/* kernel plan of the full-batch path (A/B runs and the bit-identity tests; 0 = automatic everywhere) */
extern "C" int fsrl_tr_set_plan(fsrl_ctx* c, int32_t tile_rows, int32_t hvp, int32_t wgrad) {
    CHECK_ARG(c, "null argument");
    const bool overlap = (tile_rows & 64) == 0;
    const bool poll = (tile_rows & 128) == 0;
    tile_rows &= 63;
    CHECK_ARG(tile_rows == 0 || tile_rows == 16 || tile_rows == 32, "tile_rows: 0 (automatic: mixed 32 / 16-row tiles, two co-resident workgroups per CU at 256 wide), 16, or 32 (mixed tiles, one 1024-thread workgroup per CU: round 4's kernel); + 64: the critics' steps on the compute stream instead of beside the actor's step; + 128: read-backs by hipMemcpyAsync + hipStreamSynchronize instead of polled completion words");
    CHECK_ARG(hvp >= 0 && hvp <= 7, "hvp: 0 (automatic), 1 (16-row kernel, no cache), 2 (mixed tiles, no cache), 3 (mixed tiles + cache, one 1024-thread workgroup per CU: round 4's kernel); + 4: never take the Gauss-Newton form of the product");
    CHECK_ARG(wgrad >= 0 && wgrad <= 6, "wgrad: 0 (automatic: 64 x 64 tile jobs, two workgroups per CU, XCD-aware order, at 256 wide / >= 4096 rows; else round 5's split-K kernel), 1 (split-K kernel, XCD-aware order), 2 (split-K kernel), 3 (one-pass streaming kernel), 4 (tile jobs, plain block order), 5 (the same, XCD-aware order, half the row splits), 6 (both)");
    // every argument is valid: only now does the plan change
    TrState* t = tr_of(c);
    t->opt_overlap = overlap;
    t->opt_poll = poll;
    t->opt_gn = (hvp & 4) == 0;
    hvp &= 3;
    t->opt_tile_rows = tile_rows; t->opt_hvp = hvp; t->hvp_valid = false;
    c->wgrad_xcd = (wgrad == 1);
    c->wgrad_stream = (wgrad == 3);
    c->wgrad_tiles = wgrad == 0 ? 1 : wgrad == 4 ? 3 : wgrad == 5 ? 5 : wgrad == 6 ? 7 : 0;
    return 0;
}
extern "C" int fsrl_tr_set_tile_split(fsrl_ctx* c, int32_t n32_tile, int32_t n32_hvp) {
    CHECK_ARG(c, "null argument");
    CHECK_ARG(n32_tile >= -2 && n32_hvp >= -2, "tile counts: -1 (automatic: one workgroup per tile), -2 (automatic, PERSISTENT workgroups drawing tiles from a device counter instead of one workgroup per tile) or >= 0");
    TrState* t = tr_of(c);
    t->co_static = !(n32_tile == -2 || n32_hvp == -2);
    t->split_tile = std::max(n32_tile, -1); t->split_hvp = std::max(n32_hvp, -1);
    return 0;
}
extern "C" int fsrl_tr_set_co_delay(fsrl_ctx* c, int32_t tile_periods, int32_t hvp_periods) {
    CHECK_ARG(c, "null argument");
    CHECK_ARG(tile_periods >= -1 && tile_periods <= 64 && hvp_periods >= -1 && hvp_periods <= 64, "delays: -1 (default) or 0 .. 64 periods of 8 128 cycles");
    TrState* t = tr_of(c);
    t->co_delay_tile = tile_periods < 0 ? CO_DELAY_TILE : tile_periods;
    t->co_delay_hvp = hvp_periods < 0 ? CO_DELAY_HVP : hvp_periods;
    return 0;
}
extern "C" int fsrl_tr_eval(fsrl_ctx* c, double* stats8) {
    CHECK_ARG(c && stats8, "null argument");
    TrState* t = tr_of(c);
    if (!t->ready) return fail(FSRL_ESTATE, "fsrl_tr_eval before fsrl_tr_begin");
    ENTER_DEV(c);
    return tr_eval_means(c, t, stats8);
}

// x = H^-1 g by conjugate gradients with damped HVPs (cpo.py:184-204 / trpo_lag.py:261-283), device-resident: g and x are
// device vectors in the actor layout, no host synchronisation per iteration (after an early convergence the remaining
// steps are no-ops on the device)
static int tr_cg_dev(fsrl_ctx* c, TrState* t, const float* g_dev, float damping, int nsteps, float tol, float* x_dev) {
    const int nd = c->md.net[0].end;
    double* part_pz = t->cg_part; double* part_rr = t->cg_part + CG_NB;
    hipLaunchKernelGGL(cg_init_kernel, dim3(CG_NB), dim3(256), 0, c->compute, g_dev, t->cg_r, t->Vdev, t->cg_x, t->cg_sc,
                       part_rr, nd, c->md);
    HIPCHK(hipGetLastError());
    for (int it = 0; it < nsteps; ++it) {
        int nparts = 0;
        int rc = tr_hvp_dev(c, t, true, &nparts);            // H p as split-K partials: cg_pz_kernel sums them on its way
        if (rc) return rc;
        hipLaunchKernelGGL(cg_pz_kernel, dim3(CG_NB), dim3(256), 0, c->compute, t->Out, t->Vdev, t->cg_sc, part_pz, nd, damping,
                           (const float*)c->wg_parts, nparts, c->n_dev);
        hipLaunchKernelGGL(cg_xr_kernel, dim3(CG_NB), dim3(256), 0, c->compute, t->Out, t->cg_r, t->Vdev, t->cg_x, t->cg_sc,
                           part_pz, part_rr, nd, it);
        hipLaunchKernelGGL(cg_p_kernel, dim3(CG_NB), dim3(256), 0, c->compute, t->cg_r, t->Vdev, t->cg_sc, part_rr, nd, it, tol,
                           c->md);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(x_dev, t->cg_x, (size_t)nd * 4, hipMemcpyDeviceToDevice, c->compute));
    return 0;
}

// the solver alone, for the parity tests: x = (H + damping)^-1 rhs at the current theta over the batch of the last fsrl_tr_begin,
// exactly as the learn calls run it (tr_cg_dev on device vectors), then the scalars of the chain.  rhs goes up through t->Vdev:
// actor_to_dev writes the W2 mirror behind the main vector, and only P-sized buffers have room for it -- a t->vec slot does not.
extern "C" int fsrl_tr_cg(fsrl_ctx* c, const float* rhs, int64_t n, float damping, int32_t nsteps, float tol, float* x_out,
                          int32_t* iters_out, float* rs_out) {
    int rc = tr_product_enter(c, rhs && x_out && iters_out && rs_out, "fsrl_tr_cg", n);
    if (rc) return rc;
    CHECK_ARG(nsteps >= 0 && nsteps <= 64, "nsteps must be 0 .. 64");
    TrState* t = c->tr;
    const int nd = c->md.net[0].end;
    float *vrhs = t->vec, *vx = t->vec + 2 * (size_t)c->n_dev;            // the g and H^-1 g slots: free between learn calls
    rc = actor_to_dev(c, rhs, t->Vdev);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(vrhs, t->Vdev, (size_t)nd * 4, hipMemcpyDeviceToDevice, c->compute));
    rc = tr_cg_dev(c, t, vrhs, damping, nsteps, tol, vx);
    if (rc) return rc;
    rc = actor_from_dev(c, vx, x_out);                                    // synchronises the compute stream
    if (rc) return rc;
    CgScal sc{};
    HIPCHK(hipMemcpy(&sc, t->cg_sc, sizeof(CgScal), hipMemcpyDeviceToHost));
    *iters_out = sc.iters;
    if (nsteps > 0) *rs_out = sc.rs[sc.iters & 1];                        // cg_p_kernel: rs[(it + 1) & 1] = r.r leaving iteration `it`
    else {                                                                // no iteration ran: r.r of cg_init_kernel, still in partials
        double part[CG_NB], s = 0.0;
        HIPCHK(hipMemcpy(part, t->cg_part + CG_NB, sizeof(part), hipMemcpyDeviceToHost));
        for (int b = 0; b < CG_NB; ++b) s += part[b];
        *rs_out = (float)s;
    }
    return 0;
}

// out = H v + damping v for a device vector v (cpo.py:177-182 with the damping of its callers)
static int tr_mvp_dev(fsrl_ctx* c, TrState* t, const float* v_dev, float damping, float* out_dev) {
    const int nd = c->md.net[0].end;
    hipLaunchKernelGGL(tr_copy_kernel, dim3(CG_NB), dim3(256), 0, c->compute, t->Vdev, v_dev, nd, 1, 1.0f, c->md);
    HIPCHK(hipGetLastError());
    int rc = tr_hvp_dev(c, t, true);
    if (rc) return rc;
    hipLaunchKernelGGL(tr_damp_kernel, dim3(CG_NB), dim3(256), 0, c->compute, out_dev, t->Out, v_dev, damping, nd);
    HIPCHK(hipGetLastError());
    return 0;
}

// up to four dot products of device vectors: float64 accumulation, rounded to fp32 once (as the host's vdot did).  One
// synchronisation.  `sigma_out`: the actor's sigma_param comes back with the same copy (entropy of the logged row).
static int tr_dots(fsrl_ctx* c, TrState* t, std::initializer_list<std::pair<const float*, const float*>> pairs, float* out) {
    TrDotArgs da{};
    const int n_pairs = da.n_pairs = (int)pairs.size();
    for (int k = 0; k < n_pairs; ++k) { da.a[k] = pairs.begin()[k].first; da.b[k] = pairs.begin()[k].second; }
    double* part = t->cg_part;                       // free between CG solves
    const double* hp = nullptr;
    int rc = tr_read_back(c, t, CG_NB, part, t->h_part, (size_t)n_pairs * CG_NB, &hp, [&](double* hout, unsigned* done, unsigned seq) {
        hipLaunchKernelGGL(tr_dots_kernel, dim3(CG_NB), dim3(256), 0, c->compute, da, part, c->md.net[0].end, hout, done, seq);
    });
    if (rc) return rc;
    for (int k = 0; k < n_pairs; ++k) {
        double s = 0.0;
        for (int bl = 0; bl < CG_NB; ++bl) s += hp[k * CG_NB + bl];
        out[k] = (float)s;
    }
    return 0;
}

// sum_d (0.5 + 0.5 log(2 pi) + log sigma_d) from the device's sigma_param (read with the next synchronisation)
static int sigma_fetch(fsrl_ctx* c, TrState* t) {
    float* hs = reinterpret_cast<float*>(t->h_part + 4 * CG_NB);
    HIPCHK(hipMemcpyAsync(hs, c->P + c->md.net[0].sigma, (size_t)c->cfg.act_dim * 4, hipMemcpyDeviceToHost, c->compute));
    return 0;
}
static float sigma_entropy(fsrl_ctx* c, TrState* t) {
    const float* hs = reinterpret_cast<const float*>(t->h_part + 4 * CG_NB);
    float e = 0.0f;
    for (int d = 0; d < c->cfg.act_dim; ++d) e += 1.4189385332046727f + std::log(std::exp(hs[d]));
    return e;
}

// ---- The critics' regression steps do not depend on the actor's step of the same minibatch (cpo.py:360-364 runs them first,
// trpo_lag.py:234-239 last; both read the batch's returns and the critics only) -- and a trust-region update is two chains of
// full-chip launches that each leave the matrix pipes idle half the time (tails of partly filled rounds, the gaps between
// dependent launches, host round trips of the line search).  So the critic chain is enqueued FIRST, on a stream of its own with
// its own side buffers / statistics / split-K partials, and the actor's chain runs beside it; the losses of the last step come
// back through pinned memory when the actor is done (tr_critic_collect).  Same kernels, same arguments, same order inside each
// chain: the results are bit-identical to running the chains one after the other (fsrl_tr_set_plan(tile_rows + 64): A/B).
// While a CriticLane object lives, the context's compute stream and the trust-region state's side buffers ARE the lane's, so the
// launch helpers (tr_tile, tr_wgrad_plain, wgrad_launch, ensure_parts) run unchanged.
struct CriticLane {
    fsrl_ctx* c; TrState* t; bool on;
    hipStream_t s0; float* parts0; bool valid0; int slot;
    CriticLane(fsrl_ctx* c_, TrState* t_, bool on_) : c(c_), t(t_), on(on_), s0(nullptr), parts0(nullptr), valid0(false), slot(-1) {
        if (!on) return;
        s0 = c->compute; c->compute = t->cstream;
        parts0 = c->wg_parts; valid0 = t->hvp_valid;
        for (int k = 0; k < 3 && slot < 0; ++k)
            if (c->parts[k].stride == c->n_dev || c->parts[k].stride == 0) slot = k;
        if (slot >= 0) std::swap(c->parts[slot], t->c_parts);
        swap_bufs();
    }
    ~CriticLane() {
        if (!on) return;
        swap_bufs();
        if (slot >= 0) std::swap(c->parts[slot], t->c_parts);
        c->compute = s0; c->wg_parts = parts0; t->hvp_valid = valid0;
    }
    void swap_bufs() {
        std::swap(t->A1, t->cA1); std::swap(t->A2, t->cA2); std::swap(t->D1, t->cD1); std::swap(t->D2, t->cD2);
        std::swap(t->DO, t->cDO); std::swap(t->statp, t->cstatp); std::swap(t->d_scal, t->c_d_scal); std::swap(t->d_ssq, t->c_d_ssq);
    }
};
static bool tr_overlap(const fsrl_ctx* c, const TrState* t) { return t->opt_overlap && !c->lay && t->cstream && t->cA1 && t->co_static; }

// critic regression: `iters` Adam steps on all critics (full batch), ENQUEUED (no host synchronisation); the batch sums of the
// last step's losses and the pre-update squared norms land in t->h_crit.  With the lane on they run on t->cstream behind
// everything the compute stream has been given so far.
static int tr_critic_enqueue(fsrl_ctx* c, TrState* t, int iters, float l2) {
    const int C = c->cfg.n_critics;
    const int begin = c->md.net[1].begin, end = c->md.net[C].end;
    const bool lane_on = tr_overlap(c, t);
    { int rc0 = tr_ensure_pad(c, t); if (rc0) return rc0; }     // on the compute stream, before the lane forks off
    if (lane_on) {
        HIPCHK(hipEventRecord(t->ev_fork, c->compute));
        HIPCHK(hipStreamWaitEvent(t->cstream, t->ev_fork, 0));
    }
    CriticLane lane(c, t, lane_on);
    constexpr int SQB = 32;
    t->crit_pending = iters > 0;            // set BEFORE the first launch: a failure below still leaves work in flight that the caller must join
    for (int it = 0; it < iters; ++it) {
        int rc = tr_tile(c, t, FB_MODE_VF, 1, C, 0.f, 0.f);
        if (rc) return rc;
        int nparts = 1;
        rc = tr_wgrad_plain(c, t, 1, C, nullptr, &nparts);   // partials stay in c->wg_parts: the Adam kernel below adds them up
        if (rc) return rc;
        if (it == iters - 1) {
            hipLaunchKernelGGL(fb_reduce_stats_kernel, dim3(C * FB_NSTAT), dim3(256), 0, c->compute, t->statp, t->n_tiles, C, t->d_scal);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(t->h_crit, t->d_scal, (size_t)C * FB_NSTAT * sizeof(double), hipMemcpyDeviceToHost, c->compute));
            // + l2 * sum(theta^2) over each critic's parameters, pre-update: one launch of 32 blocks per critic
            if (l2 > 0.0f) {
                SumsqRanges rg{};
                for (int k = 0; k < C; ++k) { rg.begin[k] = c->md.net[1 + k].begin; rg.end[k] = c->md.net[1 + k].end; }
                hipLaunchKernelGGL(sumsq_range_kernel, dim3(SQB, C), dim3(256), 0, c->compute, c->P, rg, t->d_ssq);
                HIPCHK(hipMemcpyAsync(t->h_crit + FSRL_MAX_CRITICS * FB_NSTAT, t->d_ssq, (size_t)SQB * C * sizeof(double),
                                      hipMemcpyDeviceToHost, c->compute));
            }
        }
        t->critic_t += 1;
        const double b1 = c->cfg.beta1, b2 = c->cfg.beta2;
        const AdamStep as = adam_step(t->cfg.critic_lr, c->cfg.beta1, c->cfg.beta2, t->critic_t);
        hipLaunchKernelGGL(adam_range_kernel, dim3((end - begin + 255) / 256), dim3(256), 0, c->compute, c->P, c->M,
                           c->V, (const float*)c->wg_parts, begin, end, l2, (float)(1.0 - b1), c->cfg.beta2, (float)(1.0 - b2),
                           as.step_size, as.bc2_sqrt, c->cfg.adam_eps, nparts, c->n_dev, c->md,
                           (const float*)nullptr, 0, 0.0f, (float*)nullptr, (float*)nullptr, 0.0f, 0.0f, 1);   // 1: float64 sum of the partials
        HIPCHK(hipGetLastError());
    }
    return 0;
}
// wait for the critic chain and turn its sums into the logged losses vf_out[C] (zeros when no step ran)
static int tr_critic_collect(fsrl_ctx* c, TrState* t, float l2, float* vf_out) {
    const int C = c->cfg.n_critics;
    constexpr int SQB = 32;
    for (int k = 0; k < C; ++k) vf_out[k] = 0.0f;
    if (!t->crit_pending) return 0;
    HIPCHK(hipStreamSynchronize(tr_overlap(c, t) ? t->cstream : c->compute));
    t->crit_pending = false;
    for (int k = 0; k < C; ++k) {
        float vf = (float)(t->h_crit[k * FB_NSTAT] / (double)t->vN);
        if (l2 > 0.0f) {
            double ssq = 0.0;
            for (int b = 0; b < SQB; ++b) ssq += t->h_crit[FSRL_MAX_CRITICS * FB_NSTAT + k * SQB + b];
            vf += (float)ssq * l2;
        }
        vf_out[k] = vf;
    }
    return 0;
}

// Minibatches of one repeat (Batch.split(batch_size, shuffle=True, merge_last=True) inside learn: cpo.py:357-358,
// trpo_lag.py:178).  One chunk covering the batch: the view stays the whole batch in STORE order (the reference's shuffle of
// a full batch only reorders sums).  Several chunks: the rows are gathered into `perm` order (the caller's
// np.random.permutation, or the library's shuffle when perm == NULL) and every chunk is a contiguous slice of that copy.
static int tr_prepare_repeat(fsrl_ctx* c, TrState* t, int32_t batch_size, const int64_t* perm, uint64_t seed,
                             std::vector<int>& st, std::vector<int>& sz) {
    const int n = (int)c->N;
    split_plan(n, std::max(1, std::min<int>(batch_size, std::max(n, 1))), st, sz);
    if (st.size() <= 1) { tr_set_view(t, c->b.obs, t->rd, n); return 0; }
    int rc = perm_upload(c, n, perm, seed);
    if (rc) return rc;
    hipLaunchKernelGGL(fb_gather_rows_kernel, dim3(1024), dim3(256), 0, c->compute, c->obs_p, c->rd_p, c->b.obs, t->rd, c->d_perm,
                       n, c->cfg.obs_dim);
    HIPCHK(hipGetLastError());
    return 0;
}

// Joins the critic lane on EVERY exit of a step: an early `return rc` between tr_critic_enqueue and tr_critic_collect would leave
// the lane's tile / weight-gradient / Adam launches in flight (still writing the critics' P / M / V) while the caller handles the
// error -- fsrl_params_get / fsrl_state_restore on the compute stream would race with them.
struct CriticJoin {
    TrState* t;
    ~CriticJoin() { if (t->crit_pending && t->cstream) { (void)hipStreamSynchronize(t->cstream); t->crit_pending = false; } }
};

// Puts the view back on the whole batch on EVERY exit of a learn call: one that fails after its first minibatch (a bad permutation
// of a later repeat, a HIP error) would otherwise leave fsrl_tr_eval / _grad / _hvp working on one chunk of the permuted copy.
struct WholeBatchView { fsrl_ctx* c; TrState* t; ~WholeBatchView() { tr_set_view(t, c->b.obs, t->rd, c->N); } };

// one try of a line search: theta := theta0 + step * dir, then the batch means at the new theta
static int tr_try_step(fsrl_ctx* c, TrState* t, const float* th0, const float* dir, float step, double* means8) {
    t->hvp_valid = false;
    c->theta_version += 1;
    hipLaunchKernelGGL(tr_step_kernel, dim3(CG_NB), dim3(256), 0, c->compute, c->P, th0, dir, step, c->md.net[0].end, c->md);
    HIPCHK(hipGetLastError());
    return tr_eval_means(c, t, means8);
}

// one minibatch of CPO.learn on the current view: optim_critic_iters critic steps, then policy_loss (cpo.py:360-364)
static int cpo_step(fsrl_ctx* c, TrState* t, double ave_cost_return, float* st, int* evals_out) {
    const fsrl_tr_config& k = t->cfg;
    const float delta = k.target_kl;
    const int nd = c->md.net[0].end;
    const size_t vs = (size_t)c->n_dev;
    float *vg = t->vec, *vb = t->vec + vs, *vHg = t->vec + 2 * vs, *vHb = t->vec + 3 * vs, *vag = t->vec + 4 * vs,
          *vab = t->vec + 5 * vs, *vdir = t->vec + 6 * vs, *vth0 = t->vec + 7 * vs;
    CriticJoin join{t};                                                    // whatever happens below, the lane is joined on the way out
    int rc = tr_critic_enqueue(c, t, k.optim_critic_iters, k.l2_reg);      // on their own stream, beside everything below
    if (rc) return rc;
    // ---- objective, cost surrogate, KL and their gradients (cpo.py:238-254); g, b and everything derived from them
    //      stay on the device
    double m[FB_NSTAT];
    rc = sigma_fetch(c, t);
    if (rc) return rc;
    rc = tr_actor_grad_dev(c, t, FB_MODE_SUR, 1.0f, 0.0f, vg, m);
    if (rc) return rc;
    const float ent = sigma_entropy(c, t);
    rc = tr_actor_grad_dev(c, t, FB_MODE_SUR, 0.0f, -1.0f, vb, nullptr);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(vth0, c->P, (size_t)nd * 4, hipMemcpyDeviceToDevice, c->compute));
    const float objective = (float)m[0];
    const float cost_sur = ((float)ave_cost_return + (float)m[1]) - (float)m[5];
    const float kl = (float)m[2];
    rc = tr_cg_dev(c, t, vg, k.damping, k.cg_iters, 1e-8f, vHg);
    if (rc) return rc;
    rc = tr_mvp_dev(c, t, vHg, k.damping, vag);
    if (rc) return rc;
    const float c_value = cost_sur - (float)k.cost_limit;
    float s_r = 0.f, s_s = 0.f, d2[2];
    rc = tr_dots(c, t, {{vb, vb}, {vag, vHg}}, d2);
    if (rc) return rc;
    const float bb = d2[0], s_q = d2[1];
    if (cpo_cost_solve_skipped(bb, c_value)) {
        HIPCHK(hipMemsetAsync(vHb, 0, (size_t)nd * 4, c->compute));
    } else {
        rc = tr_cg_dev(c, t, vb, k.damping, k.cg_iters, 1e-8f, vHb);
        if (rc) return rc;
        rc = tr_mvp_dev(c, t, vHb, k.damping, vab);
        if (rc) return rc;
        rc = tr_dots(c, t, {{vag, vHb}, {vab, vHb}}, d2);
        if (rc) return rc;
        s_r = d2[0]; s_s = d2[1];
    }
    const CpoDual d = cpo_dual_solve(s_q, s_r, s_s, c_value, delta, bb);
    // ---- line search (cpo.py:306-333); on failure the LAST tried theta stays in place
    hipLaunchKernelGGL(tr_dir_kernel, dim3(CG_NB), dim3(256), 0, c->compute, vdir, vHg, vHb, 1.0f / (d.lam + CPO_EPS), d.nu,
                       d.ocase > 0 ? 1 : 0, t->cg_part, nd);
    hipLaunchKernelGGL(tr_unit_kernel, dim3(CG_NB), dim3(256), 0, c->compute, vdir, t->cg_part, nd);
    HIPCHK(hipGetLastError());
    const CpoSearch ls = cpo_line_search(d.lam, (double)k.backtrack_coeff, k.max_backtracks, [&](double beta) {
        double e8[FB_NSTAT];
        rc = tr_try_step(c, t, vth0, vdir, (float)beta, e8);
        if (rc) return true;                                               // an error ends the search; it is returned below
        const float new_cs = ((float)ave_cost_return + (float)e8[1]) - (float)e8[5];
        return cpo_accepts((float)e8[2], (float)e8[0], new_cs, delta, d.ocase, objective, cost_sur, c_value);
    });
    if (rc) return rc;
    rc = tr_critic_collect(c, t, k.l2_reg, st + 14);
    if (rc) return rc;
    st[16] = st[14] + st[15];
    st[0] = kl; st[1] = ent; st[2] = objective; st[3] = cost_sur; st[4] = d.A; st[5] = d.B; st[6] = c_value;
    st[7] = s_q; st[8] = s_r; st[9] = s_s; st[10] = d.lam; st[11] = d.nu; st[12] = (float)d.ocase; st[13] = (float)ls.beta;
    *evals_out = ls.evals;
    return 0;
}

// The frame of both learn calls: `repeat` passes over the batch, each split into minibatches (tr_prepare_repeat), `step` on every
// minibatch's view writing one row of `nstats` floats.  `step(t, row, &evals)`; `name` is the entry point's in the state error.
template <class Step>
static int tr_learn(fsrl_ctx* c, const char* name, int32_t repeat, int32_t batch_size, const int64_t* perms, uint64_t seed,
                    float* stats_out, int nstats, int64_t cap_rows, int64_t* n_rows_out, Step&& step) {
    CHECK_ARG(c && stats_out, "null argument");
    CHECK_ARG(batch_size >= 1 && repeat >= 0, "batch_size must be >= 1, repeat >= 0");
    TrState* t = tr_of(c);
    if (!t->ready) return fail(FSRL_ESTATE, "%s before fsrl_tr_begin", name);
    ENTER_DEV(c);
    WholeBatchView whole{c, t};                      // on every way out
    t->ls_iters.clear();
    std::vector<int> mst, msz;
    int64_t row = 0;
    for (int rep = 0; rep < repeat; ++rep) {
        int rc = tr_prepare_repeat(c, t, batch_size, perms ? perms + (size_t)rep * (size_t)c->N : nullptr, seed ? seed + rep : 0, mst, msz);
        if (rc) return rc;
        for (size_t mb = 0; mb < mst.size(); ++mb, ++row) {
            CHECK_ARG(row < cap_rows, "stats_out holds %lld rows, the update has more", (long long)cap_rows);
            if (mst.size() > 1) tr_set_view(t, c->obs_p + (size_t)mst[mb] * c->cfg.obs_dim, c->rd_p + (size_t)mst[mb] * FSRL_RD, msz[mb]);
            int evals = 0;
            rc = step(t, stats_out + (size_t)row * (size_t)nstats, &evals);
            if (rc) return rc;
            t->ls_iters.push_back(evals);
        }
    }
    if (n_rows_out) *n_rows_out = row;
    return 0;
}

extern "C" int fsrl_cpo_learn_mb(fsrl_ctx* c, double ave_cost_return, int32_t repeat, int32_t batch_size, const int64_t* perms,
                                 uint64_t seed, float* stats_out, int64_t cap_rows, int64_t* n_rows_out) {
    return tr_learn(c, "fsrl_cpo_learn", repeat, batch_size, perms, seed, stats_out, FSRL_CPO_NSTATS, cap_rows, n_rows_out,
                    [&](TrState* t, float* st, int* evals) { return cpo_step(c, t, ave_cost_return, st, evals); });
}
extern "C" int fsrl_cpo_learn(fsrl_ctx* c, double ave_cost_return, int32_t repeat, float* stats_out) {
    return fsrl_cpo_learn_mb(c, ave_cost_return, repeat, INT_MAX, nullptr, 0, stats_out, repeat, nullptr);
}

// one minibatch of TRPOLagrangian.learn on the current view (trpo_lag.py:179-249)
static int trpo_step(fsrl_ctx* c, TrState* t, float lam0, float resc, float* st, int* evals_out) {
    const fsrl_tr_config& k = t->cfg;
    const int nd = c->md.net[0].end;
    const size_t vs = (size_t)c->n_dev;
    float *vg = t->vec, *vx = t->vec + 2 * vs, *vHd = t->vec + 4 * vs, *vdir = t->vec + 6 * vs, *vth0 = t->vec + 7 * vs;
    const float delta = k.target_kl;
    // the critics' steps (trpo_lag.py:234-239) read the returns and the critics only: enqueued now on their own stream, they run
    // beside the actor's step instead of behind it
    CriticJoin join{t};
    int rc = tr_critic_enqueue(c, t, k.optim_critic_iters, 0.0f);
    if (rc) return rc;
    rc = tr_refresh_old(c, t);         // old_dist = pi_theta (detached), trpo_lag.py:189-190
    if (rc) return rc;
    double m[FB_NSTAT];
    // loss_actor = rescaling * ( -mean(ratio A_r) + lambda * mean(ratio A_c) )
    rc = sigma_fetch(c, t);
    if (rc) return rc;
    rc = tr_actor_grad_dev(c, t, FB_MODE_SUR, -resc, resc * lam0, vg, m);
    if (rc) return rc;
    const float ent = sigma_entropy(c, t);
    HIPCHK(hipMemcpyAsync(vth0, c->P, (size_t)nd * 4, hipMemcpyDeviceToDevice, c->compute));
    const float loss_rew = -(float)m[0];
    const float loss_safety = c->cfg.use_lagrangian ? (float)m[1] * lam0 : 0.0f;
    const float loss_actor = resc * (loss_rew + loss_safety);
    rc = tr_cg_dev(c, t, vg, k.damping, k.cg_iters, 1e-10f, vx);
    if (rc) return rc;
    hipLaunchKernelGGL(tr_copy_kernel, dim3(CG_NB), dim3(256), 0, c->compute, vdir, vx, nd, 0, -1.0f, c->md);   // dir = -x
    HIPCHK(hipGetLastError());
    rc = tr_mvp_dev(c, t, vdir, k.damping, vHd);
    if (rc) return rc;
    float dHd;
    rc = tr_dots(c, t, {{vdir, vHd}}, &dHd);
    if (rc) return rc;
    float kl = 0.0f;
    const TrpoSearch ls = trpo_line_search(std::sqrt(2.0f * delta / dHd), k.backtrack_coeff, k.max_backtracks, [&](float step) {
        double e8[FB_NSTAT];
        rc = tr_try_step(c, t, vth0, vdir, step, e8);
        if (rc) return true;                                               // an error ends the search; it is returned below
        kl = (float)e8[2];
        const float loss_new = resc * (-(float)e8[0] + (c->cfg.use_lagrangian ? (float)e8[1] * lam0 : 0.0f));
        return trpo_accepts(kl, delta, loss_new, loss_actor);
    });
    if (rc) return rc;
    float vf[FSRL_MAX_CRITICS] = {0, 0, 0, 0};
    rc = tr_critic_collect(c, t, 0.0f, vf);
    if (rc) return rc;
    st[0] = resc; st[1] = lam0; st[2] = loss_safety; st[3] = loss_rew; st[4] = loss_actor;
    st[5] = vf[0]; st[6] = vf[1]; st[7] = vf[0] + vf[1]; st[8] = kl; st[9] = ls.step; st[10] = ent;
    *evals_out = ls.evals;
    return 0;
}

extern "C" int fsrl_trpo_learn_mb(fsrl_ctx* c, const double* lagrangians, double rescaling, int32_t repeat, int32_t batch_size,
                                  const int64_t* perms, uint64_t seed, float* stats_out, int64_t cap_rows, int64_t* n_rows_out) {
    return tr_learn(c, "fsrl_trpo_learn", repeat, batch_size, perms, seed, stats_out, FSRL_TRPO_NSTATS, cap_rows, n_rows_out,
                    [&](TrState* t, float* st, int* evals) {
        const float lam0 = (c->cfg.use_lagrangian && lagrangians) ? (float)lagrangians[0] : 0.0f;
        return trpo_step(c, t, lam0, (float)rescaling, st, evals);
    });
}
extern "C" int fsrl_trpo_learn(fsrl_ctx* c, const double* lagrangians, double rescaling, int32_t repeat,
                               float* stats_out) {
    return fsrl_trpo_learn_mb(c, lagrangians, rescaling, repeat, INT_MAX, nullptr, 0, stats_out, repeat, nullptr);
}
