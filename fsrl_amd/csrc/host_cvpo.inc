// host_cvpo.inc -- CVPO on the replay store: fsrl_cvpo_* (part of fsrl_hip.hip).
// Included once by fsrl_hip.hip: same translation unit, so the static helpers and fsrl_ctx above are visible.
// ============================================================================== CVPO (cvpo.py:71-430)
extern "C" int fsrl_cvpo_init(fsrl_ctx* c, const fsrl_cvpo_config* cfg) {
    CHECK_ARG(c && cfg, "null argument");
    CHECK_ARG(c->cfg.algo == FSRL_ALGO_SAC_LAG, "CVPO runs on a replay context (FSRL_ALGO_SAC_LAG)");
    CHECK_ARG(c->cfg.act_dim <= 8, "the actor head has at most 16 outputs (act_dim <= 8)");
    CHECK_ARG(c->cfg.obs_dim + c->cfg.act_dim <= FSRL_MAX_OBS, "obs_dim + act_dim too large");
    CHECK_ARG(cfg->n_step >= 1 && cfg->n_step <= 8, "n_step must be in [1, 8]");
    CHECK_ARG(cfg->tau >= 0.0f && cfg->tau <= 1.0f, "tau should be in [0, 1]");
    CHECK_ARG(cfg->sample_act_num >= 1 && cfg->sample_act_num <= 64, "sample_act_num must be in [1, 64]");
    CHECK_ARG(cfg->estep_iter_num >= 1 && cfg->mstep_iter_num >= 1, "estep_iter_num and mstep_iter_num must be >= 1");
    CHECK_ARG(!c->per, "this context has prioritised replay on (fsrl_per_enable), which is not built for CVPO");
    CHECK_ARG(cfg->actor_mean >= FSRL_ACTOR_MEAN_DEFAULT && cfg->actor_mean <= FSRL_ACTOR_MEAN_TANH,
              "actor_mean must be 0 (default), 1 (unbounded) or 2 (max_action * tanh), got %d", cfg->actor_mean);
    ENTER_DEV(c);
    if (c->sac) sac_free(c);
    SacState* s = new SacState();
    c->sac = s;
    s->cvpo = true; s->ccfg = *cfg; s->nstats = FSRL_CVPO_NSTATS_K;
    s->mean_tanh = cfg->actor_mean == FSRL_ACTOR_MEAN_UNBOUNDED ? 0 : 1;      // CVPO's default: max_action * tanh
    s->n_q = cfg->double_critic ? 4 : 2;
    s->cfg.actor_lr = cfg->actor_lr; s->cfg.critic_lr = cfg->critic_lr; s->cfg.tau = cfg->tau; s->cfg.n_step = cfg->n_step;
    s->cfg.auto_alpha = 0; s->cfg.alpha = 0.0f; s->cfg.use_lagrangian = 0;      // no entropy term, no PID multiplier
    const int rc = sac_alloc_state(c, s);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(s->sc, 0, sizeof(SacScalars), c->compute));
    HIPCHK(s->mem.dev(&s->csc, sizeof(CvpoScalars)));
    HIPCHK(hipMemsetAsync(s->csc, 0, sizeof(CvpoScalars), c->compute));
    HIPCHK(hipStreamSynchronize(c->compute));
    const float eta0 = 1.0f;                                                     // estep_dual = [1, 0]  (cvpo.py:150-152)
    HIPCHK(hipMemcpy(&s->csc->eta, &eta0, 4, hipMemcpyHostToDevice));
    return 0;
}

static SacState* cvpo_of(fsrl_ctx* c) { SacState* s = c ? sac_of(c) : nullptr; return (s && s->cvpo) ? s : nullptr; }

extern "C" int fsrl_cvpo_pre_update(fsrl_ctx* c) {
    SacState* s = cvpo_of(c);
    if (!s) return fail(FSRL_ESTATE, "fsrl_cvpo_init first");
    ENTER_DEV(c);
    // mdual .. dual_std are contiguous: multipliers, Adam moments, step count, clipped copies
    const size_t off = offsetof(CvpoScalars, mdual), end = offsetof(CvpoScalars, estep_loss);
    HIPCHK(hipMemsetAsync((char*)s->csc + off, 0, end - off, c->compute));
    return 0;
}

extern "C" int fsrl_cvpo_post_update(fsrl_ctx* c) {
    SacState* s = cvpo_of(c);
    if (!s) return fail(FSRL_ESTATE, "fsrl_cvpo_init first");
    ENTER_DEV(c);
    HIPCHK(hipMemcpyAsync(s->PAT, s->PA, sac_actor_bytes(c, s), hipMemcpyDeviceToDevice, c->compute));
    return 0;
}

extern "C" int fsrl_cvpo_set_thres(fsrl_ctx* c, double qc_thres) {
    SacState* s = cvpo_of(c);
    if (!s) return fail(FSRL_ESTATE, "fsrl_cvpo_init first");
    s->ccfg.qc_thres = qc_thres;
    return 0;
}

extern "C" int fsrl_cvpo_duals_get(fsrl_ctx* c, float* out4) {
    CHECK_ARG(c && out4, "null argument");
    SacState* s = cvpo_of(c);
    if (!s) return fail(FSRL_ESTATE, "fsrl_cvpo_init first");
    ENTER_DEV(c);
    CvpoScalars h;
    HIPCHK(hipMemcpyAsync(&h, s->csc, sizeof(h), hipMemcpyDeviceToHost, c->compute));
    HIPCHK(hipStreamSynchronize(c->compute));
    out4[0] = h.eta; out4[1] = h.lam; out4[2] = h.mdual[0]; out4[3] = h.mdual[1];
    return 0;
}

extern "C" int fsrl_cvpo_last_particles(fsrl_ctx* c, float* eps_particles, int64_t n) {
    CHECK_ARG(c && eps_particles, "null argument");
    SacState* s = cvpo_of(c);
    if (!s) return fail(FSRL_ESTATE, "fsrl_cvpo_init first");
    CHECK_ARG(s->last_B > 0 && n == (int64_t)s->ccfg.sample_act_num * s->last_B * c->cfg.act_dim,
              "expected K * batch_size * act_dim floats of the last update (batch_size %d)", s->last_B);
    ENTER_DEV(c);
    HIPCHK(hipMemcpyAsync(eps_particles, s->eps_k, (size_t)n * 4, hipMemcpyDeviceToHost, c->compute));
    HIPCHK(hipStreamSynchronize(c->compute));
    return 0;
}

// ---- the arguments of one update's launches.  fsrl_cvpo_update and the grouped update (host_cvpo_group.inc) both form them
//      here (sample, gather and n-step: on the SAC builders of host_sac.inc), so a member of a group cannot be handed anything its
//      own update would not be.
// library RNG: the sample of the update that s->n_updates counts (the grouped update sets the counter per step), with the
// particles' noise
static SacSampleArgs cvpo_sample_args(const fsrl_ctx* c, const SacState* s, int B, int64_t stored) {
    SacSampleArgs sa = sac_sample_args(c, s, B, s->ccfg.n_step, stored, s->n_updates);
    sa.eps_k = s->eps_k; sa.K = s->ccfg.sample_act_num;
    return sa;
}
// with_particles: the launch's second batch is CVPO_A_PARTICLES (actor_old on OBS / eps_k -> MU_OLD, STD_OLD, XK); tiles: the
// workgroups of one batch
static CvpoActorArgs cvpo_actor_args(const fsrl_ctx* c, const SacState* s, int B, int mode, const float* obs, const float* eps,
                                     float* X, bool with_particles, int tiles) {
    CvpoActorArgs aa{};
    if (with_particles) {
        aa.P2 = s->PAT; aa.obs2 = s->OBS; aa.eps2 = s->eps_k; aa.X2 = s->XK; aa.mode2 = CVPO_A_PARTICLES; aa.tiles_half = tiles;
    }
    aa.obs = obs; aa.eps = eps; aa.X = X; aa.mu_old = s->MU_OLD; aa.std_old = s->STD_OLD; aa.W = s->Wk; aa.XK = s->XK;
    aa.sc = s->csc; aa.A1 = s->A1; aa.A2 = s->A2; aa.D1 = s->D1; aa.D2 = s->D2; aa.DO = s->DO; aa.statp = s->stpi;
    aa.B = B; aa.K = s->ccfg.sample_act_num; aa.mode = mode; aa.max_action = c->cfg.max_action; aa.mean_tanh = s->mean_tanh;
    return aa;
}
// the head of a layered actor pass (lay_cvpo_actor_head_kernel behind lay_fwd_k); the M-step's modes take no noise and write no X
static LayCvpoActorArgs lay_cvpo_actor_head_args(const fsrl_ctx* c, const SacState* s, int B, int mode, const float* obs,
                                                 const float* eps, float* X) {
    LayCvpoActorArgs h{};
    h.out = s->ka.out; h.dout = s->ka.dout; h.obs = obs; h.eps = eps; h.X = X; h.mu_old = s->MU_OLD; h.std_old = s->STD_OLD;
    h.W = s->Wk; h.XK = s->XK; h.sc = s->csc; h.statp = s->stpi; h.B = B; h.K = s->ccfg.sample_act_num; h.Do = c->cfg.obs_dim;
    h.Da = c->cfg.act_dim; h.mode = mode; h.max_action = c->cfg.max_action; h.mean_tanh = s->mean_tanh;
    return h;
}
static SacNstepArgs cvpo_nstep_args(const fsrl_ctx* c, const SacState* s, int B) {
    SacNstepArgs na = sac_nstep_args(c, s, B);       // n_step: fsrl_cvpo_init copies it into s->cfg
    na.auto_alpha = 0; na.alpha_fixed = 0.0f; na.single = s->n_q == 2 ? 1 : 0;    // LPN stays zero: no entropy term
    return na;
}
static CvpoEstepArgs cvpo_estep_args(const fsrl_ctx* c, const SacState* s, int B) {
    const fsrl_cvpo_config& cc = s->ccfg;
    CvpoEstepArgs ea{};
    ea.QK = s->QK; ea.q0 = s->q0; ea.q1 = s->q1; ea.W = s->Wk; ea.sc = s->csc; ea.B = B; ea.K = cc.sample_act_num; ea.n_q = s->n_q;
    ea.iters = cc.estep_iter_num; ea.kl = cc.estep_kl; ea.thres = (float)cc.qc_thres; ea.lr = cc.estep_dual_lr;
    ea.dual_max = cc.estep_dual_max; ea.beta1 = c->cfg.beta1; ea.beta2 = c->cfg.beta2; ea.adam_eps = c->cfg.adam_eps;
    return ea;
}
static CvpoMdualArgs cvpo_mdual_args(const fsrl_ctx* c, const SacState* s, int B, int n_tiles_pi, int log_it) {
    const fsrl_cvpo_config& cc = s->ccfg;
    CvpoMdualArgs ma{};
    ma.statp = s->stpi; ma.n_tiles = n_tiles_pi; ma.B = B; ma.K = cc.sample_act_num; ma.sc = s->csc; ma.kl_mu_eps = cc.mstep_kl_mu;
    ma.kl_std_eps = cc.mstep_kl_std; ma.dual_max = cc.mstep_dual_max; ma.lr = cc.mstep_dual_lr; ma.beta1 = c->cfg.beta1;
    ma.beta2 = c->cfg.beta2; ma.adam_eps = c->cfg.adam_eps; ma.log_it = log_it;
    return ma;
}
static CvpoFinalArgs cvpo_final_args(const fsrl_ctx* c, const SacState* s, int B, int n_tiles_q, float* stats_row) {
    CvpoFinalArgs fa{};
    fa.statp_q = s->stq; fa.Y = s->Y; fa.sc = s->csc; fa.stats = stats_row;
    fa.n_tiles_q = n_tiles_q; fa.n_q = s->n_q; fa.B = B; fa.thres = (float)s->ccfg.qc_thres;
    return fa;
}

// the layered actor pass of a CVPO context, layer by layer: the forward and the actor head of the mode; with_particles: then, as the
// fused launch's second batch, actor_old on (OBS, eps_k) and the PARTICLES head; CVPO_A_MBWD: also the activation side of the
// backward pass
static int lay_cvpo_actor_pass(fsrl_ctx* c, SacState* s, int B, int mode, const float* PAx, const float* obs, const float* eps,
                               float* X, bool with_particles) {
    auto one = [&](int md_, const float* Pn, const float* obs_, const float* eps_, float* X_) -> int {
        int rc = lay_fwd_k(c, s->ka, Pn, obs_, B);
        if (rc) return rc;
        const LayCvpoActorArgs h = lay_cvpo_actor_head_args(c, s, B, md_, obs_, eps_, X_);
        hipLaunchKernelGGL(lay_cvpo_actor_head_kernel, dim3((B + 15) / 16), dim3(256), 0, c->compute, h);
        HIPCHK(hipGetLastError());
        return 0;
    };
    int rc = one(mode, PAx, obs, eps, X);
    if (rc) return rc;
    if (with_particles) { rc = one(CVPO_A_PARTICLES, s->PAT, s->OBS, s->eps_k, s->XK); if (rc) return rc; }
    return mode == CVPO_A_MBWD ? lay_bwd_dz_k(c, s->ka, PAx, B) : 0;
}

// The frame of the update is host_sac.inc's (replay_join .. replay_finish); CVPO's own: its sample launch, the TARGET + PARTICLES
// actor launch, and behind the critic half the E-step and the M-step loop.
extern "C" int fsrl_cvpo_update(fsrl_ctx* c, int32_t B, const int64_t* indices, const float* eps_target,
                                const float* eps_particles, uint64_t seed, float* stats_out) {
    CHECK_ARG(c, "null ctx");
    SacState* s = cvpo_of(c);
    if (!s) return fail(FSRL_ESTATE, "fsrl_cvpo_init first");
    CHECK_ARG(B >= 1, "batch_size must be >= 1");
    const int64_t stored = fsrl_store_len(c);
    CHECK_ARG(stored > 0, "empty replay store");
    CHECK_ARG((indices != nullptr) == (eps_target != nullptr) && (indices != nullptr) == (eps_particles != nullptr),
              "indices, eps_target and eps_particles are given together (caller RNG) or all NULL (library RNG)");
    int rc = replay_join(c, s, B);
    if (rc) return rc;
    hipStream_t st = c->compute;
    const fsrl_cvpo_config& cc = s->ccfg;
    const int Do = c->cfg.obs_dim, Da = c->cfg.act_dim, K = cc.sample_act_num;
    replay_seed_key(s, seed);          // SAC's hash (host_sac.inc): if (seed) s->key = seed * 0x9E3779B97F4A7C15ull + 0x243F6A8885A308D3ull;
    bool fused_sg = false;
    const SacGatherArgs ga = sac_gather_args(c, s, B, cc.n_step);
    if (indices) {
        rc = sac_stage_indices(c, s, B, indices, eps_target, eps_particles, (size_t)K * B * Da, s->h_epsk, s->eps_k);
        if (rc) return rc;
    } else {
        rc = sac_upload_book(c, s);
        if (rc) return rc;
        const SacSampleArgs sa = cvpo_sample_args(c, s, B, stored);
        fused_sg = !s->plan_separate;
        if (fused_sg) {          // r6: sample + gather + the particles' noise in one launch (fsrl_sac_set_plan bit 1 keeps the two)
            hipLaunchKernelGGL(cvpo_sample_gather_kernel, dim3((B + SG_ROWS - 1) / SG_ROWS + (B * K + 255) / 256), dim3(256), 0, st, sa, ga);
        } else
        hipLaunchKernelGGL(sac_sample_kernel, dim3((B * K + 255) / 256), dim3(256), 0, st, sa);
        HIPCHK(hipGetLastError());
    }
    s->last_B = B;
    // ---- gather (the caller's indices, or the two-launch plan)
    if (!fused_sg) {
        hipLaunchKernelGGL(sac_gather_kernel, dim3(std::min(1024, (B * (Do + Da) + 255) / 256)), dim3(256), 0, st, ga);
        HIPCHK(hipGetLastError());
    }
    // with_particles: the launch's second batch is CVPO_A_PARTICLES (actor_old on OBS / eps_k -> MU_OLD, STD_OLD, XK)
    auto actor_launch = [&](int mode, const float* PAx, const float* obs, const float* eps, float* X, bool with_particles = false) {
        if (s->layered) return lay_cvpo_actor_pass(c, s, B, mode, PAx, obs, eps, X, with_particles);
        const bool r4 = s->a_rows4 && (!with_particles || 8 * s->n_tiles <= c->n_cus);
        const int tiles = r4 ? 4 * s->n_tiles : s->n_tiles;
        const int grid = with_particles ? 2 * tiles : tiles;
        const CvpoActorArgs aa = cvpo_actor_args(c, s, B, mode, obs, eps, X, with_particles, tiles);
        return dispatch_H(c->cfg.hidden, [&](auto hc) {
            constexpr int H = decltype(hc)::value;
            if (r4) hipLaunchKernelGGL((cvpo_actor_tile_kernel<H, 4>), dim3(grid), dim3(4 * H), 0, st, PAx, s->mda, aa);
            else hipLaunchKernelGGL((cvpo_actor_tile_kernel<H, 16>), dim3(grid), dim3(4 * H), 0, st, PAx, s->mda, aa);
            HIPCHK(hipGetLastError());
            return 0;
        });
    };
    // ---- n-step target: a' ~ actor(s_{t+n}), critics_old.predict, float64 return      (cvpo.py:206-222)
    //      and, in the same launch, the K particles of actor_old at s_t for the E-step (they do not depend on the critic step)
    rc = actor_launch(CVPO_A_TARGET, s->PA, s->OBSN, s->eps_t, s->XN, true);
    if (rc) return rc;
    // ---- critics_old.predict, the float64 return, the critic step                     (cvpo.py:206-222, 248-276)
    int nsplit = 1;
    rc = replay_critic_half(c, s, B, cvpo_nstep_args(c, s, B), cc.critic_lr, cc.tau, &nsplit);
    if (rc) return rc;
    // ---- E-step: K particles of actor_old through the UPDATED critics                (cvpo.py:319-371)
    rc = sac_q_launch(c, s, s->PQ, s->XK, FB_MODE_Q_FWD, 0.f, 0.f, s->stqk, K * B, s->QK, s->n_tiles_k, s->k_rows4 ? 1 : 0);
    if (rc) return rc;
    const CvpoEstepArgs ea = cvpo_estep_args(c, s, B);
    hipLaunchKernelGGL(cvpo_estep_kernel, dim3(1), dim3(1024), 0, st, ea);
    HIPCHK(hipGetLastError());
    // ---- M-step                                                                     (cvpo.py:378-417)
    const int n_tiles_pi = s->a_rows4 ? 4 * s->n_tiles : s->n_tiles;
    for (int it = 0; it < cc.mstep_iter_num; ++it) {
        rc = actor_launch(CVPO_A_MFWD, s->PA, s->OBS, nullptr, nullptr);
        if (rc) return rc;
        const CvpoMdualArgs ma = cvpo_mdual_args(c, s, B, n_tiles_pi, it == 0);
        hipLaunchKernelGGL(cvpo_mdual_kernel, dim3(1), dim3(64), 0, st, ma);
        HIPCHK(hipGetLastError());
        rc = actor_launch(CVPO_A_MBWD, s->PA, s->OBS, nullptr, nullptr);
        if (rc) return rc;
        rc = sac_wgrad(c, s, s->mda, 1, s->OBS, s->na_dev, B, &nsplit);
        if (rc) return rc;
        s->t_actor += 1;
        if (it < cc.mstep_iter_num - 1)
            adam_launch(c, s->mda, s->PA, s->MA, s->VA, c->wg_parts, s->na_dev, cc.actor_lr, s->t_actor, nsplit, s->na_dev);
    }
    // ---- the last actor Adam carries the logged-row block                             (cvpo.py:422-430)
    float* stats_row = replay_stats_row(s);
    const CvpoFinalArgs fa = cvpo_final_args(c, s, B, s->q_rows4 ? 4 * s->n_tiles : s->n_tiles, stats_row);
    adam_final_launch<CvpoFinalArgs, cvpo_finalize_row>(c, s->mda, s->PA, s->MA, s->VA, c->wg_parts, s->na_dev, cc.actor_lr,
                                                        s->t_actor, nsplit, s->na_dev, nullptr, 0.0f, fa);
    HIPCHK(hipGetLastError());
    return replay_finish(c, s, stats_row, stats_out, (size_t)s->nstats);
}

// Rows of logged statistics of the updates issued with stats_out == NULL since the last drain
// (oldest first; at most SAC_RING = 4096 are kept).  Returns the number of rows written, < 0 on error.
extern "C" int64_t fsrl_sac_stats_drain(fsrl_ctx* c, float* out, int64_t max_rows) {
    CHECK_ARG(c && out && max_rows >= 0, "bad argument");
    SacState* s = sac_of(c);
    if (!s) return fail(FSRL_ESTATE, "fsrl_sac_init first");
    ENTER_DEV(c);
    int64_t first = std::max(s->n_drained, s->n_updates - SAC_RING);
    int64_t n = std::min(s->n_updates - first, max_rows);
    for (int64_t i = 0; i < n;) {              // at most two contiguous pieces of the ring
        const int64_t slot = (first + i) % SAC_RING;
        const int64_t run = std::min(n - i, (int64_t)SAC_RING - slot);
        HIPCHK(hipMemcpyAsync(out + i * s->nstats, s->d_stats + slot * s->nstats,
                              (size_t)run * s->nstats * 4, hipMemcpyDeviceToHost, c->compute));
        i += run;
    }
    HIPCHK(hipStreamSynchronize(c->compute));
    s->n_drained = first + n;
    return n;
}

// The sample the last fsrl_sac_update used (either RNG mode): store indices and both N(0,1) blocks.
extern "C" int fsrl_sac_last_sample(fsrl_ctx* c, int64_t* indices, float* eps_target, float* eps_pi, int32_t B) {
    CHECK_ARG(c && indices && eps_target && eps_pi, "null argument");
    SacState* s = sac_of(c);
    if (!s) return fail(FSRL_ESTATE, "fsrl_sac_init first");
    CHECK_ARG(B == s->last_B && B > 0, "last update used batch_size %d", s->last_B);
    ENTER_DEV(c);
    std::vector<int> idx((size_t)B);
    const size_t eb = (size_t)B * c->cfg.act_dim * 4;
    HIPCHK(hipMemcpyAsync(idx.data(), s->d_idx, (size_t)B * 4, hipMemcpyDeviceToHost, c->compute));
    HIPCHK(hipMemcpyAsync(eps_target, s->eps_t, eb, hipMemcpyDeviceToHost, c->compute));
    HIPCHK(hipMemcpyAsync(eps_pi, s->eps_p, eb, hipMemcpyDeviceToHost, c->compute));
    HIPCHK(hipStreamSynchronize(c->compute));
    for (int b = 0; b < B; ++b) indices[b] = idx[(size_t)b];
    return 0;
}

// replay-context halves of actor_eval_launch / actor_eval_finish: mlp_infer_kernel writes the raw head outputs
// [mu | log sigma] (2*Da per row; DDPG-Lag: the mean head only, Da per row) straight into pinned host memory
static int sac_raw_cols(const fsrl_ctx* c) {
    const SacState* s = sac_of(const_cast<fsrl_ctx*>(c));
    return (s && s->ddpg ? 1 : 2) * c->cfg.act_dim;       // never more than a head row (FSRL_MAX_ACT): DDPG allows act_dim 16
}
static int sac_actor_launch(fsrl_ctx* c, const float* h_obs, float* h_raw, int k) {
    SacState* s = sac_of(c);
    if (!s) return fail(FSRL_ESTATE, "fsrl_sac_init / fsrl_cvpo_init first");
    if (s->layered) {           // forward layer by layer, then the raw head outputs to the pinned staging + the completion words
        int rc = lay_work_ensure(c, s->mem, s->ka, k);
        if (rc) return rc;
        rc = lay_fwd_k(c, s->ka, s->PA, h_obs, k);
        if (rc) return rc;
        hipLaunchKernelGGL(lay_raw_out_kernel, dim3((k + 15) / 16), dim3(64), 0, c->compute, s->ka.out, h_raw, sac_raw_cols(c), k,
                           c->h_done, c->actor_seq);
        HIPCHK(hipGetLastError());
        return 0;
    }
    InferArgs ia{};
    ia.obs = h_obs; ia.obs_next = h_obs; ia.N = k; ia.C = 0; ia.max_action = 1.0f; ia.raw_out = h_raw;
    ia.raw_cols = sac_raw_cols(c); ia.done = c->h_done; ia.seq = c->actor_seq;
    return dispatch_H(c->cfg.hidden, [&](auto hc) {
        constexpr int H = decltype(hc)::value;
        hipLaunchKernelGGL(mlp_infer_kernel<H>, dim3((k + 15) / 16, 1), dim3(4 * H), 0, c->compute, s->PA, s->mda, ia);
        HIPCHK(hipGetLastError());
        return 0;
    });
}
static bool sac_actor_resident_args(fsrl_ctx* c, const float** P, const ModelDesc** md) {
    SacState* s = sac_of(c);
    if (!s || s->layered) return false;
    *P = s->PA; *md = &s->mda;
    return true;
}
static void sac_actor_finish(fsrl_ctx* c, const float* raw, int k, float* mu_out, float* sigma_out) {
    SacState* s = sac_of(c);
    const int Da = c->cfg.act_dim, rc = sac_raw_cols(c);
    for (int r = 0; r < k; ++r)
        for (int d = 0; d < Da; ++d) {
            if (s->ddpg) {     // deterministic actor: the action itself, and the exploration-noise std
                mu_out[(size_t)r * Da + d] = c->cfg.max_action * std::tanh(raw[(size_t)r * rc + d]);
                if (sigma_out) sigma_out[(size_t)r * Da + d] = s->cfg.exploration_sigma;
                continue;
            }
            mu_out[(size_t)r * Da + d] = s->mean_tanh ? c->cfg.max_action * std::tanh(raw[(size_t)r * rc + d])
                                                      : raw[(size_t)r * rc + d];
            if (sigma_out) {
                const float l = std::min(std::max(raw[(size_t)r * rc + Da + d], -20.0f), 2.0f);
                sigma_out[(size_t)r * Da + d] = std::exp(l);
            }
        }
}

extern "C" int fsrl_sac_actor_forward(fsrl_ctx* c, const float* obs, int32_t k, float* mu_out, float* sigma_out) {
    CHECK_ARG(c && obs && mu_out && sigma_out, "null argument");
    if (!sac_of(c)) return fail(FSRL_ESTATE, "fsrl_sac_init first");
    if (k <= 0) return 0;
    HIPCHK(hipSetDevice(c->device));      // keeps a resident actor alive (ENTER_DEV would end it)
    int rc = actor_eval_launch(c, obs, k, true);
    if (rc) return rc;
    return actor_eval_finish(c, mu_out, sigma_out);
}

static bool sac_squashes(fsrl_ctx* c) { SacState* s = sac_of(c); return s && !s->ddpg && !s->cvpo; }

// A device collect on a replay context (host_devcollect.inc devcollect_begin): the head arithmetic of sac_actor_finish + actor_draw
// as the collect kernels' arguments.  false: no actor of the asked kind (fused / layered), or not initialised
static bool sac_devcollect_head(fsrl_ctx* c, DevCollectArgs* a, int* head, bool layered) {
    SacState* s = sac_of(c);
    if (!s || s->layered != layered) return false;
    *head = s->ddpg ? DC_HEAD_DDPG : DC_HEAD_GAUSS;
    a->mean_tanh = s->mean_tanh; a->squash = sac_squashes(c) ? 1 : 0; a->exploration_sigma = s->cfg.exploration_sigma;
    return true;
}
// ... and what a push does to a sample drawn ahead: the store_version bump drops it at the next update; one still in flight on the
// side stream reads rows the kernel is about to overwrite, so the kernel goes behind it
static int sac_devcollect_enter(fsrl_ctx* c) {
    SacState* s = sac_of(c);
    if (s->pre_valid && s->pre_side) HIPCHK(hipStreamWaitEvent(c->compute, s->pre_done, 0));
    s->pre_valid = false;
    return 0;
}
