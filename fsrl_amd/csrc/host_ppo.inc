// host_ppo.inc -- PPO-Lagrangian update: fsrl_ppo_begin / _pass / _end / _update, fsrl_batch_get (part of fsrl_hip.hip).
// Included once by fsrl_hip.hip: same translation unit, so the static helpers and fsrl_ctx above are visible.
// ------------------------------------------------------------------------------ PPO-Lagrangian
static int launch_gae(fsrl_ctx* c);
static int perm_send(fsrl_ctx* c, int n);
static int clip_fuse_begin(fsrl_ctx* c);
// This pass's / repeat's permutation to the device: np.random.permutation on the caller's side, checked, or the library's own
// shuffle (perm_fill).  Built in pageable memory first: the GPU keeps working on the previous pass meanwhile.  Only the previous
// H2D copy out of the pinned buffer has to be over (an event, not a stream drain).
static int perm_upload(fsrl_ctx* c, int n, const int64_t* perm, uint64_t seed) {
    c->perm_tmp.resize((size_t)n);
    const PermFill pf = perm_fill(c->perm_tmp.data(), n, perm, c->shuffle_rng, seed);
    CHECK_ARG(pf.code != PERM_RANGE, "perm[%d]=%lld out of range", pf.index, pf.value);
    CHECK_ARG(pf.code != PERM_TWICE, "perm is not a permutation: %lld appears twice", pf.value);
    return perm_send(c, n);
}
// c->perm_tmp[0 .. n) to the device (perm_upload, and the replay of a kept pass: clip_fuse_check)
static int perm_send(fsrl_ctx* c, int n) {
    if (c->perm_in_flight) { HIPCHK(hipEventSynchronize(c->perm_copied)); c->perm_in_flight = false; }
    memcpy(c->h_perm, c->perm_tmp.data(), (size_t)n * 4);
    HIPCHK(hipMemcpyAsync(c->d_perm, c->h_perm, (size_t)n * 4, hipMemcpyHostToDevice, c->compute));
    HIPCHK(hipEventRecord(c->perm_copied, c->compute));
    c->perm_in_flight = true;
    return 0;
}

static int ensure_ppo_buffers(fsrl_ctx* c, int B) {
    const int mbp = round_up(2 * B, 32);      // 32: a grouped launch's 32-row tiles may cover one 16-row group past the last minibatch row
    if (mbp <= c->mbp_max) return 0;
    HIPCHK(hipStreamSynchronize(c->compute));
    const int H = c->cfg.hidden, nn = c->md.n_nets;
    const size_t act = (size_t)nn * mbp * H * 4;
    HIPCHK(c->mem.regrow(c->mbp_max, mbp, mbp,
                         {Mem::D(&c->A1, act), Mem::D(&c->A2, act), Mem::D(&c->D1, act), Mem::D(&c->D2, act),
                          Mem::D(&c->DO, (size_t)nn * mbp * FSRL_DOW * 4),
                          Mem::D(&c->statp, (size_t)(mbp / 4) * nn * 4 * 4),      // one slot per 4-row tile
                          Mem::D(&c->gsq_part, (size_t)std::max(wg_grid(H, nn), c->n_dev / 256 + 2) * 4)}));   // per-block squared norms (either wgrad path)
    c->n_tiles_max = mbp / 16;
    return 0;
}

// A/B and test switch: 32-row tiles in the forward / backward launch of a minibatch step.  -1: automatic (all tiles once the 16-row tiles
// exceed the CU count), 0: none, n > 0: min(n, tiles / 2) leading tiles of every network.  Every plan gives the same bits.
extern "C" int fsrl_ppo_set_plan(fsrl_ctx* c, int32_t tall_tiles) {
    CHECK_ARG(c, "null ctx");
    CHECK_ARG(tall_tiles >= -1 && tall_tiles <= 4096, "tall_tiles: -1 (automatic), 0 (none) or a count");
    c->tall_tiles = tall_tiles;
    return 0;
}

extern "C" int fsrl_ppo_begin(fsrl_ctx* c, const double* lagrangians, double rescaling,
                              int32_t batch_size, int64_t* n_out) {
    CHECK_ARG(c, "null ctx");
    CHECK_ARG(batch_size >= 1, "batch_size must be >= 1");
    CHECK_ARG(!c->in_update, "fsrl_ppo_begin called twice without fsrl_ppo_end");
    ENTER_DEV(c);
    int rc = flush_stage(c);
    if (rc) return rc;
    HIPCHK(hipEventRecord(c->store_ready, c->side));
    HIPCHK(hipStreamWaitEvent(c->compute, c->store_ready, 0));   // join side stream -> compute
    const int C = c->cfg.n_critics;
    for (int i = 0; i < FSRL_MAX_CRITICS; ++i) c->lagr[i] = 0.0;
    if (c->cfg.use_lagrangian && C > 1) {
        CHECK_ARG(lagrangians, "lags and values length must be equal");
        for (int i = 0; i < C - 1; ++i) c->lagr[i] = lagrangians[i];
    }
    c->rescaling = rescaling;
    c->batch_size = batch_size;
    // ---- batch, indices = buffer.sample(0)
    const int64_t n = sample0(c, c->h_indices, c->h_end);
    c->N = n;
    if (n_out) *n_out = n;
    c->n_steps = 0;
    c->pass_index = 0;
    c->in_update = true;
    c->verdict_pending = false;
    c->t_fwdbwd_ms = 0; c->n_fwdbwd = 0; c->k_ev_used = 0;
    CtrlBlock init{INT_MAX, 0, 0.0, 0.0f, 0.0f};
    *c->h_ctrl = init;
    *reinterpret_cast<int*>(c->h_up + upload_layout(0, 0, 0).miss_count) = 0;
    hipStream_t s = c->compute;
    c->clip_fuse_active = false;
    c->vnext_reuse_active = false;
    c->clip_perms.clear();
    if (n == 0) {               // the head alone: control block + miss counter
        HIPCHK(hipMemcpyAsync(c->d_up, c->h_up, UPLOAD_HEAD, hipMemcpyHostToDevice, s));
        c->batch_ready = true;
        return 0;
    }
    // episode segments for the GAE scan
    int nseg = 0;
    c->h_seg[nseg++] = 0;
    for (int64_t i = 0; i + 1 < n; ++i) if (c->h_end[i]) c->h_seg[nseg++] = (int)i + 1;
    c->h_seg[nseg] = (int)n;
    // ---- minibatch plan of every pass (same for all passes)
    split_plan((int)n, batch_size, c->mb_start, c->mb_size);
    // working set of one minibatch: never more rows than the batch has (CPO / TRPO-Lag begin with batch_size = 2^20 = "the
    // whole batch": sized by that, the four activation arrays alone were 25 GB)
    const int bs_rows = (int)std::min<int64_t>(batch_size, std::max<int64_t>(n, 1));
    rc = c->lay ? lay_ensure_mb(c, bs_rows) : ensure_ppo_buffers(c, bs_rows);
    if (rc) return rc;
    // ---- the one upload: control block, miss counter, indices (in place since sample0), end flags, segments, minibatch plan
    const size_t nmb = c->mb_start.size();
    const UploadLayout u = upload_layout((size_t)n, (size_t)nseg, nmb);
    memcpy(c->h_up + u.end, c->h_end, (size_t)n);
    memcpy(c->h_up + u.seg, c->h_seg, (size_t)(nseg + 1) * 4);
    memcpy(c->h_up + u.mb_start, c->mb_start.data(), nmb * 4);
    memcpy(c->h_up + u.mb_size, c->mb_size.data(), nmb * 4);
    c->d_end = reinterpret_cast<uint8_t*>(c->d_up + u.end); c->d_seg = reinterpret_cast<int*>(c->d_up + u.seg);
    c->d_mbstart = reinterpret_cast<int*>(c->d_up + u.mb_start); c->d_mbsize = reinterpret_cast<int*>(c->d_up + u.mb_size);
    rc = clip_fuse_begin(c);
    if (rc) return rc;
    HIPCHK(hipEventRecord(c->ev_a, s));
    HIPCHK(hipMemcpyAsync(c->d_up, c->h_up, u.total, hipMemcpyHostToDevice, s));
    const int Do = c->cfg.obs_dim, Da = c->cfg.act_dim;
    // V(obs_next) from V(obs) where the rows coincide: the fused PPO-Lagrangian contexts (layered contexts and the other algorithms run
    // process_fn as before)
    const bool reuse = !c->no_vnext_reuse && !c->lay && c->cfg.algo == FSRL_ALGO_PPO_LAG && c->cfg.n_critics >= 1;
    {
        const size_t work = (size_t)n * (2 * Do + Da + 1);
        const int blocks = (int)std::min<size_t>(2048, (work + 255) / 256);
        if (reuse) {
            const int fblocks = (int)((n + 255) / 256);
            hipLaunchKernelGGL(batch_gather_flag_kernel, dim3(blocks + fblocks), dim3(256), 0, s, c->st, c->b, c->d_indices,
                               c->d_end, (int)n, Do, Da, blocks, NextSamePtrs{c->next_same, c->miss_list, c->miss_count});
        } else {
            hipLaunchKernelGGL(batch_gather_kernel, dim3(blocks), dim3(256), 0, s, c->st, c->b, c->d_indices,
                               c->d_end, (int)n, Do, Da);
        }
        HIPCHK(hipGetLastError());
    }
    c->vnext_reuse_active = reuse;
    // ---- process_fn: V_i(obs), V_i(obs_next)*~terminated, logp_old, then float64 GAE per critic
    InferArgs ia{};
    ia.obs = c->b.obs; ia.obs_next = c->b.obs_next; ia.act = c->b.act; ia.flags = c->b.flags;
    ia.values = c->values; ia.vnext = c->vnext; ia.logp_old = c->logp_old; ia.mu_out = nullptr;
    if (reuse) { ia.next_same = c->next_same; ia.miss_list = c->miss_list; ia.miss_count = c->miss_count; }
    if (c->cfg.algo == FSRL_ALGO_FOCOPS) {      // old distribution of the pass batches: means + sigma_param snapshot
        if (!c->mu_old) {
            HIPCHK(c->mem.dev(&c->mu_old, (size_t)c->alloc_rows * Da * 4));
            HIPCHK(c->mem.dev(&c->sigma_old, FSRL_MAX_ACT * 4));
        }
        ia.mu_out = c->mu_old;
        HIPCHK(hipMemcpyAsync(c->sigma_old, c->P + c->md.net[0].sigma, (size_t)Da * 4, hipMemcpyDeviceToDevice, s));
    }
    ia.N = (int)n; ia.C = C; ia.max_action = c->cfg.max_action;
    rc = launch_infer(c, ia, 2 * C + 1, s);
    if (rc) return rc;
    c->n_seg = nseg;
    rc = launch_gae(c);
    if (rc) return rc;
    HIPCHK(hipEventRecord(c->ev_b, s));
    c->batch_ready = true;
    return 0;
}


// float64 GAE of every critic over the episode segments of the current batch (values / vnext already on the device)
static int launch_gae(fsrl_ctx* c) {
    GaeArgs ga{};
    ga.values = c->values; ga.vnext = c->vnext; ga.rew = c->b.rew; ga.cost = c->b.cost; ga.flags = c->b.flags;
    ga.seg_start = c->d_seg; ga.advs = c->advs; ga.rets = c->rets; ga.adv64 = nullptr; ga.N = (int)c->N;
    ga.gamma = c->cfg.gamma; ga.gl = c->cfg.gamma * c->cfg.gae_lambda;
    if (c->cfg.rew_norm) {
        if (c->ret64_cap < c->N) {
            HIPCHK(hipStreamSynchronize(c->compute));
            HIPCHK(c->mem.regrow(c->ret64_cap, c->N, c->alloc_rows, {Mem::D(&c->ret64, (size_t)c->cfg.n_critics * c->alloc_rows * 8)}));
        }
        ga.rms = c->d_rms; ga.ret64 = c->ret64;
    }
    hipLaunchKernelGGL(gae_kernel, dim3(c->n_seg, c->cfg.n_critics), dim3(64), 0, c->compute, ga);
    HIPCHK(hipGetLastError());
    if (c->cfg.rew_norm) {      // self.ret_rms[i].update(ret): after the scan, which used the previous variance
        hipLaunchKernelGGL(ret_rms_update_kernel, dim3(c->cfg.n_critics), dim3(1024), 0, c->compute, c->ret64, c->d_rms,
                           (int)c->N);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

// recompute_advantage (ppo_lag.py:218-221): before every pass after the first, V_i(obs), V_i(obs_next) of the CURRENT
// critics and the GAE / returns built on them; the batch, its end flags and logp_old stay those of process_fn
static int ppo_recompute_advantages(fsrl_ctx* c) {
    const int C = c->cfg.n_critics;
    InferArgs ia{};
    ia.obs = c->b.obs; ia.obs_next = c->b.obs_next; ia.act = nullptr; ia.flags = c->b.flags;
    ia.values = c->values; ia.vnext = c->vnext; ia.logp_old = nullptr; ia.mu_out = nullptr;
    ia.N = (int)c->N; ia.C = C; ia.max_action = c->cfg.max_action;
    // the batch has not changed since fsrl_ppo_begin: its flags and its list of misses still hold
    if (c->vnext_reuse_active) { ia.next_same = c->next_same; ia.miss_list = c->miss_list; ia.miss_count = c->miss_count; }
    int rc = launch_infer(c, ia, 2 * C, c->compute);          // jobs 0 .. 2C-1: the critics (job 2C would be the actor)
    if (rc) return rc;
    return launch_gae(c);
}

static int ensure_stats(fsrl_ctx* c, int64_t steps) {
    if (steps <= c->stats_cap) return 0;
    int64_t cap = std::max<int64_t>(steps, c->stats_cap * 2);
    cap = std::max<int64_t>(cap, 1024);
    float* nw = nullptr;
    HIPCHK(c->mem.dev(&nw, (size_t)cap * FSRL_PPO_NSTATS * 4));      // the rows so far are kept: the old block goes after the copy
    if (c->d_stats) {
        HIPCHK(hipStreamSynchronize(c->compute));
        HIPCHK(hipMemcpy(nw, c->d_stats, (size_t)c->stats_cap * FSRL_PPO_NSTATS * 4, hipMemcpyDeviceToDevice));
        HIPCHK(c->mem.release(&c->d_stats));
    }
    c->d_stats = nw;
    c->stats_cap = cap;
    return 0;
}

// first half of a pass, shared by fsrl_ppo_pass and the grouped update: this pass's permutation to the device and the
// per-pass batch preparation (per-minibatch advantage statistics + rows in pass order)
// kept: a permutation as an earlier call uploaded it (the replay of a pass), instead of perm / seed
static int ppo_pass_prepare(fsrl_ctx* c, const int64_t* perm, uint64_t seed, const std::vector<int>* kept = nullptr) {
    const int n = (int)c->N;
    hipStream_t s = c->compute;
    const int C = c->cfg.n_critics;
    if (c->cfg.recompute_adv && c->pass_index > 0 &&           // ppo_lag.py:218-221, focops.py:223-226
        (c->cfg.algo == FSRL_ALGO_PPO_LAG || c->cfg.algo == FSRL_ALGO_FOCOPS)) {
        int rc0 = ppo_recompute_advantages(c);
        if (rc0) return rc0;
    }
    int rc;
    if (kept) { c->perm_tmp = *kept; rc = perm_send(c, n); }
    else rc = perm_upload(c, n, perm, seed);
    if (rc) return rc;
    if (c->clip_fuse_active && !kept) c->clip_perms.push_back(c->perm_tmp);      // what a replay of this pass uploads again
    const int nmb = (int)c->mb_start.size();
    rc = ensure_stats(c, c->n_steps + nmb);
    if (rc) return rc;
    {
        PrepArgs pa{};
        pa.obs = c->b.obs; pa.act = c->b.act; pa.advs = c->advs; pa.rets = c->rets; pa.logp_old = c->logp_old;
        pa.perm = c->d_perm; pa.mb_start = c->d_mbstart; pa.mb_size = c->d_mbsize; pa.obs_p = c->obs_p;
        pa.rd_p = c->rd_p; pa.N = n; pa.C = C; pa.Do = c->cfg.obs_dim; pa.Da = c->cfg.act_dim;
        pa.norm_adv = c->cfg.norm_adv;
        pa.values = c->cfg.value_clip ? c->values : nullptr;
        pa.mean_old = (c->cfg.algo == FSRL_ALGO_FOCOPS) ? c->mu_old : nullptr; pa.sigma_old = c->sigma_old;
        if ((size_t)nmb > c->mbstat_cap) {
            HIPCHK(hipStreamSynchronize(s));
            HIPCHK(c->mem.regrow(c->mbstat_cap, (size_t)nmb, (size_t)nmb * 2, {Mem::D(&c->mbstat, (size_t)nmb * 2 * FSRL_MAX_CRITICS * 2 * sizeof(float))}));
        }
        pa.mbstat = c->mbstat; pa.batch = c->mb_size[0]; pa.nmb = nmb;
        if (pa.norm_adv) hipLaunchKernelGGL(ppo_adv_stats_kernel, dim3(nmb), dim3(1024), 0, s, pa);
        hipLaunchKernelGGL(ppo_permute_rows_kernel, dim3((n + 63) / 64), dim3(256), 0, s, pa);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

// the step scalars that do not change inside an update (everything but the minibatch geometry and Adam's bias terms)
static PpoStepArgs ppo_base_args(const fsrl_ctx* c) {
    PpoStepArgs sa{};
    sa.rescale = (float)c->rescaling;
    for (int i = 0; i < FSRL_MAX_CRITICS; ++i) sa.lam[i] = (float)c->lagr[i];
    sa.eps_clip = c->cfg.eps_clip; sa.dual_clip = c->cfg.dual_clip; sa.vf_coef = c->cfg.vf_coef;
    sa.max_action = c->cfg.max_action; sa.max_grad_norm = c->cfg.max_grad_norm; sa.target_kl = c->cfg.target_kl;
    sa.norm_adv = c->cfg.norm_adv; sa.use_lagrangian = c->cfg.use_lagrangian;
    sa.value_clip = c->cfg.value_clip;
    sa.lr = c->cfg.lr; sa.beta1 = c->cfg.beta1; sa.beta2 = c->cfg.beta2; sa.adam_eps = c->cfg.adam_eps;
    sa.one_minus_b1 = (float)(1.0 - (double)c->cfg.beta1);
    sa.one_minus_b2 = (float)(1.0 - (double)c->cfg.beta2);
    sa.kl_thresh = 1.5 * (double)c->cfg.target_kl;
    sa.pass = c->pass_index;
    sa.dbg_phase = c->probe_phase;      // 0 unless this is a -DFSRL_PROBES build (read once at context creation)
    // no gradient-norm clip (PPOLagAgent's default): nothing global stands between a reduced gradient element and its Adam
    // update, so the weight-gradient kernel applies it and the step is 2 launches instead of 3
    sa.fuse_adam = (c->cfg.max_grad_norm <= 0.0f && !c->no_fuse_adam) ? 1 : 0;
    return sa;
}

// a context's pointer blocks of the fused minibatch step: fsrl_ppo_pass and the group's member table (host_group.inc).  wp.X is the
// first row; wp.stats is the caller's to set after ppo_pass_prepare, which may regrow the statistics table
static PpoBatchPtrs ppo_batch_ptrs(const fsrl_ctx* c) {
    PpoBatchPtrs bp{};
    bp.obs_p = c->obs_p; bp.rd_p = c->rd_p; bp.A1 = c->A1; bp.A2 = c->A2; bp.D1 = c->D1; bp.D2 = c->D2;
    bp.DO = c->DO; bp.statp = c->statp; bp.mbp_max = c->mbp_max;
    bp.ts = c->probe_ts;                 // null outside probe builds
    return bp;
}
static WgradPtrs ppo_wgrad_ptrs(const fsrl_ctx* c) {
    WgradPtrs wp{};
    wp.A1 = c->A1; wp.A2 = c->A2; wp.D1 = c->D1; wp.D2 = c->D2; wp.DO = c->DO; wp.X = c->obs_p; wp.grad = c->G;
    wp.gsq_part = c->gsq_part; wp.ctrl = c->ctrl; wp.mbp_max = c->mbp_max; wp.P = c->P; wp.statp = c->statp;
    wp.Pw = c->P; wp.M = c->M; wp.V = c->V;
    return wp;
}
// a member's row of a group's member table, zeroed, with what fused (host_group.inc) and layered (host_layered_group.inc) members
// have in common.  hp: the member's OWN hyper-parameters, taken from its ppo_base_args so that every derived value (kl_thresh,
// one_minus_b*) is the one its solo step would use; group_step_args lays them over the group-wide arguments.
static void group_agent_common(const fsrl_ctx* c, GroupAgent& a) {
    memset(&a, 0, sizeof(a));
    a.P = c->P; a.Pw = c->P; a.M = c->M; a.V = c->V; a.G = c->G; a.ctrl = c->ctrl; a.n_dev = c->n_dev;
    a.rescale = (float)c->rescaling;
    for (int j = 0; j < FSRL_MAX_CRITICS; ++j) a.lam[j] = (float)c->lagr[j];
    const PpoStepArgs sa = ppo_base_args(c);
    GroupHyper& h = a.hp;
    h.eps_clip = sa.eps_clip; h.dual_clip = sa.dual_clip; h.vf_coef = sa.vf_coef; h.max_grad_norm = sa.max_grad_norm;
    h.target_kl = sa.target_kl; h.kl_thresh = sa.kl_thresh;
    h.norm_adv = sa.norm_adv; h.use_lagrangian = sa.use_lagrangian; h.value_clip = sa.value_clip;
    h.beta1 = sa.beta1; h.beta2 = sa.beta2; h.adam_eps = sa.adam_eps;
    h.one_minus_b1 = sa.one_minus_b1; h.one_minus_b2 = sa.one_minus_b2;
}
// what of the step arguments is the same for every member of a group (its first member's; fsrl_group_create checks what the
// members must agree on): everything else comes from the member and step tables (group_step_args)
static PpoStepArgs group_base_args(const fsrl_ctx* c0) {
    const PpoStepArgs m0 = ppo_base_args(c0);
    PpoStepArgs sa{};
    sa.max_action = m0.max_action; sa.fuse_adam = m0.fuse_adam; sa.xcd_pair = m0.xcd_pair; sa.dbg_phase = m0.dbg_phase;
    return sa;
}

// Tile height of the fused step's forward / backward launch: `tiles` 16-row tiles per network, nn networks, n_act members in the launch
// (fsrl_ppo_pass: 1, the group: the members active in the pass).
//   rows4: 4-row tiles (4x4x1 MFMA) while the launch still fits the chip in one round: four times the CUs, a quarter of the MFMA time each
//   rows8: 8-row tiles (two 4x4x1 passes on one fragment ingest) when the 4-row grid is more than one round but the 8-row grid is not:
//          batch 512 ran 96 sixteen-row workgroups on a 256-CU chip
//   n32:   tall tiles (r6 late): once the 16-row tiles need a second round of workgroups (a lone context: minibatches above ~1 360 rows
//          with three networks) every (member, network) runs 32-row tiles (a trailing odd 16-row group keeps a 16-row tile): 8 members x
//          3 networks x 256 rows = 192 workgroups instead of 384, half the L2 -> register weight ingest per row.  Same-box alternations
//          (tools/bench_group.py --tall): k = 8 245 -> 283 updates/s aggregate, k = 6 207 -> 252, k = 12 260 -> 270, k = 16 309 -> 309;
//          groups whose 16-row tiles fit one round LOSE with tall tiles (k = 4 245 -> 200, k = 5 266 -> 232) and keep them.  A mix sized
//          to exactly one round (6 of 32 + 4 of 16 rows per pair at k = 8) was slower than either (228-240) and 7 + 2 differed by box
//          (288 / 222): not used.  tall_tiles (fsrl_ppo_set_plan / fsrl_group_set_plan): -1 automatic, 0 none, n > 0 exactly
//          min(n, tiles / 2) leading tiles.  Same bits either way.
struct PpoTilePlan { bool rows4, rows8; int n32; };
static PpoTilePlan ppo_tile_plan(const fsrl_ctx* c0, int tiles, int nn, int n_act, int tall_tiles) {
    PpoTilePlan p{false, false, 0};
    if (c0->probe_tile16) return p;
    const size_t per16 = (size_t)tiles * nn * n_act, n_cus = (size_t)c0->n_cus;
    p.rows4 = per16 * 4 <= n_cus;
    p.rows8 = !p.rows4 && per16 * 2 <= n_cus;
    if (!p.rows4 && !p.rows8 && c0->cfg.hidden >= 128 && c0->md.Do <= TileSmem<256, 32>::XK)
        p.n32 = tall_tiles < 0 ? (per16 > n_cus ? tiles / 2 : 0) : std::min(tiles / 2, tall_tiles);
    return p;
}

static int ppo_pass_enqueue(fsrl_ctx* c, const int64_t* perm, uint64_t seed, const std::vector<int>* kept);
extern "C" int fsrl_ppo_pass(fsrl_ctx* c, const int64_t* perm, uint64_t seed, int32_t* stopped_out) {
    CHECK_ARG(c, "null ctx");
    if (!c->in_update || !c->batch_ready) return fail(FSRL_ESTATE, "fsrl_ppo_pass before fsrl_ppo_begin");
    c->theta_version += 1;                   // optimiser steps follow (PPO-Lag, FOCOPS, layered contexts: all pass through here)
    ENTER_DEV(c);
    if (stopped_out) *stopped_out = 0;
    const int n = (int)c->N;
    if (n == 0) return 0;
    int rc;
    if (c->cfg.algo == FSRL_ALGO_FOCOPS || c->lay) {
        rc = ppo_pass_prepare(c, perm, seed);
        if (rc) return rc;
        if (c->cfg.algo == FSRL_ALGO_FOCOPS) return focops_pass(c, stopped_out);
    }
    if (c->lay) {               // hidden_sizes of another depth / width: one launch per Linear (host_layered.inc)
        rc = lay_ppo_steps(c);
        if (rc) return rc;
        c->n_steps += (int)c->mb_start.size();
        c->pass_index += 1;
        if (c->cfg.target_kl > 0.0f) return pass_verdict(c, stopped_out);
        return 0;
    }
    rc = ppo_pass_enqueue(c, perm, seed, nullptr);
    if (rc) return rc;
    // ---- pass-level KL early stop: one small readback per pass (the reference's `break`)
    if (c->cfg.target_kl > 0.0f) return pass_verdict(c, stopped_out);
    return 0;
}
// one pass of the fused PPO-Lagrangian step, enqueued: preparation, then every minibatch step (fsrl_ppo_pass, and the replay of a
// kept pass: clip_fuse_check)
static int ppo_pass_enqueue(fsrl_ctx* c, const int64_t* perm, uint64_t seed, const std::vector<int>* kept) {
    hipStream_t s = c->compute;
    const int H = c->cfg.hidden, nn = c->md.n_nets;
    int rc = ppo_pass_prepare(c, perm, seed, kept);
    if (rc) return rc;
    const int nmb = (int)c->mb_start.size();
    const PpoBatchPtrs bp = ppo_batch_ptrs(c);
    WgradPtrs wp = ppo_wgrad_ptrs(c);
    wp.stats = c->d_stats;
    wp.clip_slots = c->clip_slots;
    const int nparts = wg_grid(H, nn);   // tiles + aux parts of every network, + one extra block per network, + the logged-row block

    PpoStepArgs sa = ppo_base_args(c);
    sa.iters_in_pass = nmb;

    for (int mb = 0; mb < nmb; ++mb) {
        sa.mb_start = c->mb_start[mb]; sa.mb_size = c->mb_size[mb]; sa.mb_index = mb;
        sa.step = (int)c->n_steps + mb;
        sa.first_in_pass = (mb == 0); sa.last_in_pass = (mb == nmb - 1);
        c->adam_t += 1;
        const AdamStep as = adam_step(c->cfg.lr, c->cfg.beta1, c->cfg.beta2, c->adam_t);
        sa.step_size = as.step_size; sa.bc2_sqrt = as.bc2_sqrt;
        const int tiles = (sa.mb_size + 15) / 16;
        wp.X = c->obs_p + (size_t)sa.mb_start * c->cfg.obs_dim;
        const bool prof = c->profiling;
        if (prof) {
            while (c->k_ev.size() < c->k_ev_used + 3) {
                hipEvent_t e; HIPCHK(hipEventCreate(&e)); c->k_ev.push_back(e);
            }
            HIPCHK(hipEventRecord(c->k_ev[c->k_ev_used], s));
        }
        const PpoTilePlan tp = ppo_tile_plan(c, tiles, nn, 1, c->tall_tiles);
        const int n32 = tp.n32, stat_tiles = tp.rows4 ? tiles * 4 : tp.rows8 ? tiles * 2 : tiles;
        rc = dispatch_H(H, [&](auto hc) {
            constexpr int HH = decltype(hc)::value;
            // one network per XCD pair (see ppo_fwd_bwd_body): grid = 8 x ceil(tiles / 2), the blocks of XCD pairs beyond the networks exit
            sa.xcd_pair = (nn <= 4 && !c->no_xcd_pair) ? 1 : 0;
            auto fb_grid = [&](int nt) { return sa.xcd_pair ? dim3(8 * ((nt + 1) / 2)) : dim3(nt * nn); };
            // 4- and 8-row tiles: part of the backward W2 fragment trickles in under the forward pass (W2bEarly, kernels_mlp.hpp);
            // FSRL_NO_W2B_EARLY launches the one-burst instantiation (A/B; same bits)
            const bool early = !c->no_w2b_early;
            if (tp.rows4 && early) hipLaunchKernelGGL((ppo_fwd_bwd_kernel<HH, 4, true>), fb_grid(tiles * 4), dim3(4 * HH), 0, s, c->P, c->md, bp, sa);
            else if (tp.rows4) hipLaunchKernelGGL((ppo_fwd_bwd_kernel<HH, 4>), fb_grid(tiles * 4), dim3(4 * HH), 0, s, c->P, c->md, bp, sa);
            else if (tp.rows8 && early) hipLaunchKernelGGL((ppo_fwd_bwd_kernel<HH, 8, true>), fb_grid(tiles * 2), dim3(4 * HH), 0, s, c->P, c->md, bp, sa);
            else if (tp.rows8) hipLaunchKernelGGL((ppo_fwd_bwd_kernel<HH, 8>), fb_grid(tiles * 2), dim3(4 * HH), 0, s, c->P, c->md, bp, sa);
            else if (n32 > 0) {
                if constexpr (HH >= 128)
                    hipLaunchKernelGGL((ppo_fwd_bwd_tall_kernel<HH>), dim3((tiles - n32) * nn), dim3(4 * HH), 0, s, c->P, c->md, bp, sa, n32, tiles - n32);
            } else hipLaunchKernelGGL((ppo_fwd_bwd_kernel<HH, 16>), fb_grid(tiles), dim3(4 * HH), 0, s, c->P, c->md, bp, sa);
            return 0;
        });
        if (rc) return rc;
        if (prof) {
            // e0 | kernel | e1 | e2 : (e2 - e1) is the cost of an empty event bracket on this
            // stream.  Half of it overlaps the kernel's own dispatch, so (e1 - e0) - (e2 - e1)/2
            // is reported (calibrated against rocprofv3: 22.4 vs 22.1 us); raw sums are kept too
            HIPCHK(hipEventRecord(c->k_ev[c->k_ev_used + 1], s));
            HIPCHK(hipEventRecord(c->k_ev[c->k_ev_used + 2], s));
            c->k_ev_used += 3;
        }
        const bool big = tiles * 16 > 512;
        // clip + Adam inside the weight-gradient launch (two launches for this step): its slots carry a tag of their own
        const bool clip_step = clip_fuse_step_ok(c->clip_fuse_active, tiles * 16);
        if (clip_step) {
            c->clip_epoch += 1;
            if (c->clip_epoch == 0) c->clip_epoch = 1;      // 0 is the tag of a slot never written
            sa.clip_epoch = c->clip_epoch; sa.clip_limit = c->clip_fuse_limit;
            c->clip_fuse_steps += 1;
        }
        if (big) {
            // More than 512 rows (batch sizes above 256, or the merged last minibatch of batch 512): the one-workgroup-per-
            // output-tile kernel would walk the rows in chunks (66 us at 1 024 rows: 64 % of such a step).  The full-batch
            // weight-gradient kernel splits the rows over workgroups instead (17 us), followed by the sum of its partials
            // (+ the per-block squared norms), the logged row and the Adam kernel: 5 launches for a step of this size.
            FbWgradArgs wa{};
            wgrad_fill_nets(wa, nn, 0, (size_t)H, (size_t)c->mbp_max, c->A1, c->A2, c->D1, c->D2, c->DO);
            wa.obs = wp.X; wa.rows = tiles * 16; wa.N = sa.mb_size;
            int nsplit = 1;
            rc = wgrad_launch<false>(c, c->md, wa, nn, c->n_dev, &nsplit);
            if (rc) return rc;
            const int nsum = (c->n_dev + 255) / 256;
            hipLaunchKernelGGL(fb_sum_parts_kernel, dim3(nsum), dim3(256), 0, s, c->G, c->wg_parts, 0, c->n_dev, nsplit, c->n_dev,
                               c->gsq_part);
            hipLaunchKernelGGL(ppo_stats_kernel, dim3(1), dim3(64), 0, s, c->md, wp, sa, stat_tiles);
            hipLaunchKernelGGL(adam_clip_kernel, dim3((c->n_dev + 4 * ADAM_NT - 1) / (4 * ADAM_NT)), dim3(ADAM_NT), 0, s, c->P, c->M,
                               c->V, c->G, c->gsq_part, nsum, c->n_dev, sa, c->ctrl, c->md);
            HIPCHK(hipGetLastError());
            continue;
        }
        rc = dispatch_H(H, [&](auto hc) {
            constexpr int HH = decltype(hc)::value;
            // (more than 512 rows took the split-K route above: the chunked BIG form of this kernel runs in the grouped launches only)
            if (sa.fuse_adam) hipLaunchKernelGGL((ppo_wgrad_kernel<HH, false, true>), dim3(nparts), dim3(1024), 0, s, c->md, wp, tiles * 16, sa, stat_tiles);
            else if (clip_step) hipLaunchKernelGGL((ppo_wgrad_kernel<HH, false, true, true>), dim3(nparts), dim3(1024), 0, s, c->md, wp, tiles * 16, sa, stat_tiles);
            else hipLaunchKernelGGL((ppo_wgrad_kernel<HH, false, false>), dim3(nparts), dim3(1024), 0, s, c->md, wp, tiles * 16, sa, stat_tiles);
            return 0;
        });
        if (rc) return rc;
        if (!sa.fuse_adam && !clip_step)
            hipLaunchKernelGGL(adam_clip_kernel, dim3((c->n_dev + 4 * ADAM_NT - 1) / (4 * ADAM_NT)), dim3(ADAM_NT), 0, s, c->P, c->M, c->V, c->G,
                               c->gsq_part, nparts, c->n_dev, sa, c->ctrl, c->md);
        HIPCHK(hipGetLastError());
    }
    c->n_steps += nmb;
    c->pass_index += 1;
    return 0;
}

// ---- the two-launch clipped step's host side.  fsrl_ppo_begin decides (host_decisions.hpp: clip_fuse_update_ok) and snapshots P, M, V:
// one device-to-device copy of their shared allocation on the compute stream, next to process_fn, which writes none of them.  Every read of the control block (pass_verdict,
// fsrl_ppo_pass_result, fsrl_ppo_end) looks at `poisoned`: a block of some weight-gradient launch gave up waiting for the others.
static int clip_fuse_begin(fsrl_ctx* c) {
    ClipFuseFacts f{};
    f.mode = c->clip_fuse_mode; f.env_off = c->no_clip_fuse; f.dead = c->clip_fuse_dead;
    f.ppo_lag = c->cfg.algo == FSRL_ALGO_PPO_LAG; f.layered = c->lay != nullptr; f.grouped = c->group != nullptr;
    f.recompute_adv = c->cfg.recompute_adv != 0; f.rew_norm = c->cfg.rew_norm != 0;
    f.max_grad_norm = c->cfg.max_grad_norm;
    f.nparts = c->lay ? 0 : wg_grid(c->cfg.hidden, c->md.n_nets); f.n_cus = c->n_cus; f.obs_dim = c->cfg.obs_dim;
    f.live_contexts = live_contexts_on(c->device);
    if (!clip_fuse_update_ok(f)) return 0;
    hipStream_t s = c->compute;
    if (!c->clip_slots) {
        HIPCHK(c->mem.dev(&c->clip_slots, (size_t)1024 * CLIP_SLOT_STRIDE * sizeof(unsigned long long)));
        HIPCHK(hipMemsetAsync(c->clip_slots, 0, (size_t)1024 * CLIP_SLOT_STRIDE * sizeof(unsigned long long), s));
    }
    if (!c->clip_snap) HIPCHK(c->mem.dev(&c->clip_snap, c->pmv_bytes));
    HIPCHK(hipMemcpyAsync(c->clip_snap, c->pmv, c->pmv_bytes, hipMemcpyDeviceToDevice, s));      // P, M and V share one allocation
    c->clip_snap_adam_t = c->adam_t;
    c->clip_fuse_active = true;
    return 0;
}
// The compute stream is drained and h_ctrl holds the control block.  A poisoned update: back to the snapshot, the three-launch step
// for good, every pass enqueued so far again with the permutation it ran with; then h_ctrl holds the replay's control block.
static int clip_fuse_check(fsrl_ctx* c) {
    if (!clip_fuse_must_replay(c->clip_fuse_active, c->h_ctrl->poisoned)) return 0;
    hipStream_t s = c->compute;
    const ClipFuseReplay rp = clip_fuse_replay_plan(c->clip_snap_adam_t, c->pass_index);
    c->clip_fuse_active = false; c->clip_fuse_dead = true;
    c->clip_fuse_fallbacks += 1;
    HIPCHK(hipMemcpyAsync(c->pmv, c->clip_snap, c->pmv_bytes, hipMemcpyDeviceToDevice, s));
    c->adam_t = rp.adam_t; c->n_steps = rp.n_steps; c->pass_index = rp.pass_index;
    c->k_ev_used = 0;
    CtrlBlock init{INT_MAX, 0, 0.0, 0.0f, 0.0f};
    *c->h_ctrl = init;
    HIPCHK(hipMemcpyAsync(c->ctrl, c->h_ctrl, sizeof(CtrlBlock), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));                      // h_ctrl is read back below: the upload out of it has to be over
    for (int k = 0; k < rp.passes; ++k) {
        int rc = ppo_pass_enqueue(c, nullptr, 0, &c->clip_perms[(size_t)k]);
        if (rc) return rc;
    }
    HIPCHK(hipMemcpyAsync(c->h_ctrl, c->ctrl, sizeof(CtrlBlock), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    c->clip_perms.clear();
    return 0;
}
// mode: -1 automatic, 0 off, 1 on (where the kernel and the replay allow it: clip_fuse_update_ok); limit_ticks: a block's longest wait
// for another block's squared norm in 10 ns ticks, 0 = every block gives up at once (the fallback, on demand), < 0 = the default
extern "C" int fsrl_ppo_set_clip_fuse(fsrl_ctx* c, int32_t mode, int32_t limit_ticks) {
    CHECK_ARG(c, "null ctx");
    CHECK_ARG(mode >= -1 && mode <= 1, "mode: -1 (automatic), 0 (off) or 1 (on)");
    CHECK_ARG(limit_ticks <= 100000000, "limit_ticks: at most 10^8 (one second)");
    CHECK_ARG(!c->in_update, "fsrl_ppo_set_clip_fuse inside an update");
    c->clip_fuse_mode = mode;
    c->clip_fuse_limit = limit_ticks < 0 ? CLIP_FUSE_DEFAULT_TICKS : limit_ticks;
    return 0;
}
// out[0] = 1 if the next update may take the two-launch step (mode, switch, no fallback so far; the shape rule is applied per update),
// out[1] = updates replayed after a wait ran out, out[2] = two-launch steps enqueued, out[3] = 1 if the LAST update took the step.
// grad_norm_out (optional, between updates): the gradient norm the last clipped step saw, read from the control block
extern "C" int fsrl_ppo_clip_fuse_stats(fsrl_ctx* c, int64_t* out, float* grad_norm_out) {
    CHECK_ARG(c && out, "null argument");
    if (grad_norm_out) {
        CHECK_ARG(!c->in_update, "the gradient norm is read between updates");
        ENTER_DEV(c);
        CtrlBlock cb;
        HIPCHK(hipStreamSynchronize(c->compute));
        HIPCHK(hipMemcpy(&cb, c->ctrl, sizeof(CtrlBlock), hipMemcpyDeviceToHost));
        *grad_norm_out = cb.last_grad_norm;
    }
    out[0] = (c->clip_fuse_mode != 0 && !c->no_clip_fuse && !c->clip_fuse_dead) ? 1 : 0;
    out[1] = c->clip_fuse_fallbacks; out[2] = c->clip_fuse_steps; out[3] = c->clip_fuse_active ? 1 : 0;
    return 0;
}

// process_fn of the last fsrl_ppo_begin (between launches or updates; waits for the compute stream): out[0] = batch rows whose V(obs_next) the
// V(obs) pass gave, out[1] = rows the next jobs evaluated (per critic; out[0] + out[1] = N), out[2] = 1 if the launch ran the equal split,
// out[3] = 1 if the reuse was on (0: FSRL_NO_VNEXT_REUSE, a layered context or another algorithm -- then out[1] = N and out[2] = 1)
extern "C" int fsrl_ppo_process_stats(fsrl_ctx* c, int64_t* out) {
    CHECK_ARG(c && out, "null argument");
    if (!c->batch_ready) return fail(FSRL_ESTATE, "no batch: call fsrl_ppo_begin first");
    ENTER_DEV(c);
    out[0] = 0; out[1] = c->N; out[2] = 1; out[3] = c->vnext_reuse_active ? 1 : 0;
    if (!c->vnext_reuse_active || c->N == 0) return 0;
    int m = 0;
    HIPCHK(hipStreamSynchronize(c->compute));
    HIPCHK(hipMemcpy(&m, c->miss_count, sizeof(int), hipMemcpyDeviceToHost));
    const int tiles = (int)((c->N + 15) / 16), jobs_y = 2 * c->cfg.n_critics + 1;
    const InferSplit sp = infer_split(infer_grid_x(tiles, c->n_cus, jobs_y), jobs_y, c->cfg.n_critics, tiles, (m + 15) / 16);
    out[0] = c->N - m; out[1] = m; out[2] = sp.equal;
    return 0;
}

// The pass-level stop flag travels back in the control block.  stopped_out != NULL: wait for it here.  NULL: only enqueue
// the readback -- the caller prepares the next pass (its permutation) while the device finishes this one and asks
// fsrl_ppo_pass_result before it enqueues anything else.
static int pass_verdict(fsrl_ctx* c, int32_t* stopped_out) {
    HIPCHK(hipMemcpyAsync(c->h_ctrl, c->ctrl, sizeof(CtrlBlock), hipMemcpyDeviceToHost, c->compute));
    if (!stopped_out) { c->verdict_pending = true; return 0; }
    HIPCHK(hipStreamSynchronize(c->compute));
    int rc = clip_fuse_check(c);
    if (rc) return rc;
    if (c->h_ctrl->stopped_after != INT_MAX) *stopped_out = 1;
    return 0;
}

extern "C" int fsrl_ppo_pass_result(fsrl_ctx* c, int32_t* stopped_out) {
    CHECK_ARG(c && stopped_out, "null argument");
    if (!c->in_update) return fail(FSRL_ESTATE, "fsrl_ppo_pass_result outside an update");
    ENTER_DEV(c);
    if (c->verdict_pending) {
        HIPCHK(hipStreamSynchronize(c->compute)); c->verdict_pending = false;
        int rc = clip_fuse_check(c);
        if (rc) return rc;
    }
    const bool watched = c->cfg.target_kl > 0.0f || c->cfg.algo == FSRL_ALGO_FOCOPS;
    *stopped_out = (watched && c->pass_index > 0 && c->h_ctrl->stopped_after != INT_MAX) ? 1 : 0;
    return 0;
}

extern "C" int fsrl_ppo_end(fsrl_ctx* c, float* stats_out, int64_t cap_steps, int64_t* n_steps_out) {
    CHECK_ARG(c, "null ctx");
    if (!c->in_update) return fail(FSRL_ESTATE, "fsrl_ppo_end without fsrl_ppo_begin");
    ENTER_DEV(c);
    hipStream_t s = c->compute;
    HIPCHK(hipEventRecord(c->ev_c, s));
    // two-launch steps: the control block once more, with the statistics (was a wait cut short since the last look?)
    const bool look = c->clip_fuse_active;
    if (look) HIPCHK(hipMemcpyAsync(c->h_ctrl, c->ctrl, sizeof(CtrlBlock), hipMemcpyDeviceToHost, s));
    if (stats_out && c->n_steps > 0) {
        CHECK_ARG(cap_steps >= c->n_steps, "stats_out holds %lld steps, need %lld", (long long)cap_steps,
                  (long long)c->n_steps);
        HIPCHK(hipMemcpyAsync(stats_out, c->d_stats, (size_t)c->n_steps * FSRL_PPO_NSTATS * 4,
                              hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    if (look) {
        c->verdict_pending = false;
        const int64_t before = c->clip_fuse_fallbacks;
        int rc = clip_fuse_check(c);
        if (rc) { c->in_update = false; return rc; }
        if (c->clip_fuse_fallbacks != before) {           // replayed: the statistics of the replay, and its time
            HIPCHK(hipEventRecord(c->ev_c, s));
            if (stats_out && c->n_steps > 0)
                HIPCHK(hipMemcpyAsync(stats_out, c->d_stats, (size_t)c->n_steps * FSRL_PPO_NSTATS * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        }
    }
    if (n_steps_out) *n_steps_out = c->n_steps;
    c->in_update = false;
    if (c->N > 0) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, c->ev_a, c->ev_b) == hipSuccess) c->t_process_ms = ms;
        if (hipEventElapsedTime(&ms, c->ev_b, c->ev_c) == hipSuccess) c->t_learn_ms = ms;
        double tot = 0;
        c->t_fwdbwd_raw_ms = 0;
        for (size_t i = 0; i + 2 < c->k_ev_used; i += 3) {
            float a = 0, b = 0;
            if (hipEventElapsedTime(&a, c->k_ev[i], c->k_ev[i + 1]) == hipSuccess &&
                hipEventElapsedTime(&b, c->k_ev[i + 1], c->k_ev[i + 2]) == hipSuccess)
            { tot += (double)a - 0.5 * (double)b; c->t_fwdbwd_raw_ms += (double)a; }
        }
        c->t_fwdbwd_ms = tot;
        c->n_fwdbwd = (int64_t)(c->k_ev_used / 3);
    }
    return 0;
}

extern "C" int fsrl_ppo_update(fsrl_ctx* c, const double* lagrangians, double rescaling,
                               int32_t batch_size, int32_t repeat, const int64_t* perms, uint64_t seed,
                               float* stats_out, int64_t cap_steps, int64_t* n_steps_out,
                               int32_t* stopped_pass_out) {
    CHECK_ARG(c, "null ctx");
    CHECK_ARG(repeat >= 0, "repeat must be >= 0");
    int64_t n = 0;
    int rc = fsrl_ppo_begin(c, lagrangians, rescaling, batch_size, &n);
    if (rc) return rc;
    if (stopped_pass_out) *stopped_pass_out = -1;
    for (int k = 0; k < repeat; ++k) {
        int32_t stopped = 0;
        rc = fsrl_ppo_pass(c, perms ? perms + (size_t)k * n : nullptr, seed ? seed + k : 0, &stopped);
        if (rc) { c->in_update = false; return rc; }
        if (stopped) { if (stopped_pass_out) *stopped_pass_out = k; break; }
    }
    return fsrl_ppo_end(c, stats_out, cap_steps, n_steps_out);
}

extern "C" int fsrl_batch_get(fsrl_ctx* c, const char* which, float* out, int64_t cap) {
    CHECK_ARG(c && which && out, "null argument");
    if (!c->batch_ready) return fail(FSRL_ESTATE, "no batch: call fsrl_ppo_begin first");
    ENTER_DEV(c);
    const int64_t n = c->N;
    const int C = c->cfg.n_critics;
    const float* src = nullptr;
    int cols = C;
    if (!strcmp(which, "values")) src = c->values;
    else if (!strcmp(which, "rets")) src = c->rets;
    else if (!strcmp(which, "advs")) src = c->advs;
    else if (!strcmp(which, "vnext")) src = c->vnext;
    else if (!strcmp(which, "logp_old")) { src = c->logp_old; cols = 1; }
    else return fail(FSRL_EINVAL, "unknown batch field '%s'", which);
    CHECK_ARG(cap >= n * cols, "out too small");
    HIPCHK(hipStreamSynchronize(c->compute));
    std::vector<float> tmp((size_t)n * cols);
    if (n) HIPCHK(hipMemcpy(tmp.data(), src, (size_t)n * cols * 4, hipMemcpyDeviceToHost));
    // device layout is [C][N]; the reference stacks on the last axis: [N][C]
    for (int64_t r = 0; r < n; ++r)
        for (int k = 0; k < cols; ++k) out[r * cols + k] = tmp[(size_t)k * n + r];
    return 0;
}
