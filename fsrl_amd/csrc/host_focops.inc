// host_focops.inc -- FOCOPS on the PPO entry points: fsrl_focops_* and the minibatch pass (part of fsrl_hip.hip).
// Included once by fsrl_hip.hip: same translation unit, so the static helpers and fsrl_ctx above are visible.
// ====================================================================================== FOCOPS
struct FocState {
    fsrl_focops_config cfg{};
    Mem mem;
    double nu = 0.0, nu_loss = 0.0;
    int64_t t_actor = 0, t_critic = 0;
    float *statp_pi = nullptr, *psq = nullptr, *gsq = nullptr, *sig_stash = nullptr;   // statp_pi: [tiles][3 networks][FB_NSTAT]
    float* gsq_net = nullptr;          // [3] the extra block's share of the squared gradient norm per network (three-launch step)
    int pp = 0;                        // psq / sig_stash are double-buffered: [pp] is read by this step's logged row, [pp ^ 1] written by its Adam
    int cap_tiles = 0, cap_psq = 0;
    bool no_fast = false;              // fsrl_focops_set_plan(ctx, 1): always the four-launch step (A/B, tests)
};
static void foc_reset_optim(fsrl_ctx* c) { if (c->foc) { c->foc->t_actor = 0; c->foc->t_critic = 0; } }
static void foc_steps(fsrl_ctx* c, int64_t* t_actor, int64_t* t_critic, bool set) {      // fsrl_state_snapshot / _restore
    if (!c->foc) return;
    if (set) { c->foc->t_actor = *t_actor; c->foc->t_critic = *t_critic; }
    else { *t_actor = c->foc->t_actor; *t_critic = c->foc->t_critic; }
}
static void foc_free(fsrl_ctx* c) {
    FocState* f = c->foc;
    if (!f) return;
    f->mem.release_all();
    delete f;
    c->foc = nullptr;
}
extern "C" int fsrl_focops_init(fsrl_ctx* c, const fsrl_focops_config* cfg) {
    CHECK_ARG(c && cfg, "null argument");
    CHECK_ARG(c->cfg.algo == FSRL_ALGO_FOCOPS, "context was not created with FSRL_ALGO_FOCOPS");
    CHECK_ARG(c->cfg.n_critics == 2, "FOCOPS uses a reward and a cost critic");
    CHECK_ARG(cfg->tem_lambda > 0.0f, "tem_lambda must be positive");
    foc_free(c);
    c->foc = new FocState();
    c->foc->cfg = *cfg;
    return 0;
}
extern "C" int fsrl_focops_set_plan(fsrl_ctx* c, int32_t four_launch) {
    CHECK_ARG(c, "null ctx");
    if (!c->foc) return fail(FSRL_ESTATE, "fsrl_focops_init first");
    c->foc->no_fast = four_launch != 0;
    return 0;
}
extern "C" int fsrl_focops_set_nu(fsrl_ctx* c, double nu, double nu_loss) {
    CHECK_ARG(c, "null ctx");
    if (!c->foc) return fail(FSRL_ESTATE, "fsrl_focops_init first");
    c->foc->nu = nu; c->foc->nu_loss = nu_loss;
    return 0;
}

// parameter blocks of 256 of the three networks (focops_prep_kernel / focops_step_kernel lay them out actor | critic 0 | critic 1)
static void focops_blocks(const fsrl_ctx* c, int* nb_a, int* nb_c0, int* nb_c1) {
    *nb_a = (c->md.net[0].end - c->md.net[0].begin + 255) / 256;
    *nb_c0 = (c->md.net[1].end - c->md.net[1].begin + 255) / 256;
    *nb_c1 = (c->md.net[2].end - c->md.net[2].begin + 255) / 256;
}
// 4-row tiles of the fused tile launch only while the three networks of its n_act members (focops_pass: 1) fit the chip in one round
static bool focops_rows4(const fsrl_ctx* c, int tiles, int n_act) { return (size_t)tiles * 4 * 3 * n_act <= (size_t)c->n_cus; }
// the FOCOPS working set for the current minibatch plan (c->mbp_max): allocated on first use, regrown with the minibatch
// (focops_pass and, per member, the grouped update)
static int focops_alloc(fsrl_ctx* c) {
    FocState* f = c->foc;
    const int max_tiles = c->mbp_max / 16;
    int nb_a, nb_c0, nb_c1;
    focops_blocks(c, &nb_a, &nb_c0, &nb_c1);
    if (f->cap_tiles < max_tiles || f->cap_psq < nb_c0 + nb_c1) {
        HIPCHK(hipStreamSynchronize(c->compute));
        if (!f->sig_stash) HIPCHK(f->mem.dev(&f->sig_stash, 2 * FSRL_MAX_ACT * 4));
        if (!f->gsq_net) HIPCHK(f->mem.dev(&f->gsq_net, FSRL_MAX_NETS * 4));
        f->cap_tiles = f->cap_psq = 0;      // one set behind both capacities: either growing regrows it
        HIPCHK(f->mem.regrow(f->cap_tiles, std::max(max_tiles, 1), std::max(max_tiles, 1),
                             {Mem::D(&f->statp_pi, (size_t)(4 * max_tiles + 4) * 3 * FB_NSTAT * 4),      // three networks per tile
                              Mem::D(&f->psq, (size_t)2 * (nb_c0 + nb_c1) * 4), Mem::D(&f->gsq, (size_t)nb_a * 4)}));
        f->cap_psq = nb_c0 + nb_c1;
    }
    return 0;
}
// the step / prep launch's arguments that do not depend on the minibatch; pp: the psq / sig_stash parity of the step
static FocopsStepArgs focops_step_args(const fsrl_ctx* c, int pp) {
    const FocState* f = c->foc;
    int nb_a, nb_c0, nb_c1;
    focops_blocks(c, &nb_a, &nb_c0, &nb_c1);
    const int npsq = nb_c0 + nb_c1;
    const double b1 = c->cfg.beta1, b2 = c->cfg.beta2;
    FocopsStepArgs sa{};
    sa.P = c->P; sa.M = c->M; sa.V = c->V; sa.stride = c->n_dev;
    sa.G = c->G; sa.gsq = f->gsq; sa.psq = f->psq + (size_t)pp * npsq; sa.sig_stash = f->sig_stash + pp * FSRL_MAX_ACT;
    sa.psq_next = f->psq + (size_t)(pp ^ 1) * npsq; sa.sig_next = f->sig_stash + (pp ^ 1) * FSRL_MAX_ACT;
    sa.nb_a = nb_a; sa.nb_c0 = nb_c0; sa.nb_c1 = nb_c1; sa.max_norm = f->cfg.max_grad_norm; sa.l2 = f->cfg.l2_reg;
    sa.one_minus_b1 = (float)(1.0 - b1); sa.beta2 = c->cfg.beta2; sa.one_minus_b2 = (float)(1.0 - b2);
    sa.adam_eps = c->cfg.adam_eps;
    return sa;
}
// the tile launch's arguments for the minibatch of `size` rows at `start` (the rows prepared by ppo_pass_prepare)
static FbArgs focops_tile_args(const fsrl_ctx* c, int start, int size) {
    const FocState* f = c->foc;
    FbArgs a{};
    a.obs = c->obs_p + (size_t)start * c->cfg.obs_dim; a.rd = c->rd_p + (size_t)start * FSRL_RD;
    a.A1 = c->A1; a.A2 = c->A2; a.D1 = c->D1; a.D2 = c->D2; a.DO = c->DO;
    a.N = size; a.rows_pad = (size + 15) / 16 * 16; a.max_action = c->cfg.max_action;
    a.cr = 1.0f / f->cfg.tem_lambda; a.cc = (float)f->nu; a.eta = f->cfg.eta;
    a.mode = FB_MODE_FOCOPS; a.net0 = 0; a.statp = f->statp_pi;      // [tiles][3][FB_NSTAT]
    return a;
}
// the minibatch's weight gradients of all three networks in ppo_wgrad_kernel's layout (three-launch step)
static WgradPtrs focops_wgrad_ptrs(const fsrl_ctx* c, const float* obs, int rows_pad) {
    WgradPtrs wp{};
    wp.A1 = c->A1; wp.A2 = c->A2; wp.D1 = c->D1; wp.D2 = c->D2; wp.DO = c->DO; wp.X = obs; wp.grad = c->G;
    wp.gsq_part = c->gsq_part; wp.ctrl = c->ctrl; wp.mbp_max = rows_pad;     // the tile kernel laid network y out at y * rows_pad
    wp.P = c->P; wp.statp = nullptr; wp.stats = nullptr;                      // no PPO row: focops_step_kernel's extra block logs
    wp.gsq_net = c->foc->gsq_net;
    return wp;
}
// ... and in fb_wgrad_kernel's (four-launch step; wgrad_launch fills in the split-K plan)
static FbWgradArgs focops_split_args(const fsrl_ctx* c, const float* obs, int size, int rows_pad) {
    FbWgradArgs wa{};
    wgrad_fill_nets(wa, 3, 0, (size_t)c->cfg.hidden, (size_t)rows_pad, c->A1, c->A2, c->D1, c->D2, c->DO);
    wa.obs = obs; wa.rows = rows_pad; wa.N = size;
    return wa;
}
// one minibatch step's optimiser side: both Adam step counters advance, the logged row goes to statistics row `row`
static void focops_step_fill(fsrl_ctx* c, FocopsStepArgs& sa, int64_t row, int mb, int nmb, int size, int n_tiles) {
    FocState* f = c->foc;
    f->t_critic += 1; f->t_actor += 1;
    const AdamStep aa = adam_step(f->cfg.actor_lr, c->cfg.beta1, c->cfg.beta2, f->t_actor);
    const AdamStep ac = adam_step(f->cfg.critic_lr, c->cfg.beta1, c->cfg.beta2, f->t_critic);
    sa.step_a = aa.step_size; sa.bc2s_a = aa.bc2_sqrt; sa.step_c = ac.step_size; sa.bc2s_c = ac.bc2_sqrt;
    // ---- logged row, pass KL sum, pass-level early stop flag (the extra block of the step launch)
    FocopsFinalArgs& fa = sa.fin;
    fa.statp_vf = f->statp_pi + FB_NSTAT; fa.statp_pi = f->statp_pi; fa.vf_stride = 3; fa.pi_stride = 3;
    fa.psq0 = sa.psq; fa.psq1 = sa.psq + sa.nb_c0; fa.n_psq0 = sa.nb_c0; fa.n_psq1 = sa.nb_c1;
    fa.P = sa.sig_stash; fa.sigma_off = 0; fa.Da = c->cfg.act_dim;          // entropy of the PRE-update policy
    fa.stats = c->d_stats + (size_t)row * FSRL_PPO_NSTATS; fa.ctrl = c->ctrl;
    fa.n_tiles = n_tiles; fa.n_tiles_pi = fa.n_tiles; fa.mb = size;
    fa.first_in_pass = mb == 0; fa.last_in_pass = mb == nmb - 1;
    fa.iters_in_pass = nmb; fa.pass = (int)c->pass_index; fa.l2 = f->cfg.l2_reg; fa.nu_loss = (float)f->nu_loss;
    fa.nu_value = (float)f->nu; fa.delta = f->cfg.delta;
}

// one pass of FOCOPS minibatch steps over the batch prepared by fsrl_ppo_pass (permuted rows, per-minibatch
// normalised advantages, old means / stds in the row data).  Per minibatch (focops.py:226-241):
//   critics:  fb_tile(VF, 2 nets) -> fb_wgrad -> Adam per critic (+ l2, records sum(theta^2))
//   actor:    fb_tile(FOCOPS)     -> fb_wgrad -> sum (+ ||g||^2 partials) -> clip + Adam
//   stats row + pass KL sum (focops_finalize_kernel)
static int focops_pass(fsrl_ctx* c, int32_t* stopped_out) {
    FocState* f = c->foc;
    if (!f) return fail(FSRL_ESTATE, "fsrl_focops_init first");
    hipStream_t s = c->compute;
    const int H = c->cfg.hidden;
    const int nmb = (int)c->mb_start.size();
    int rc0 = focops_alloc(c);
    if (rc0) return rc0;
    int nb_a, nb_c0, nb_c1;
    focops_blocks(c, &nb_a, &nb_c0, &nb_c1);
    const int nb_all = nb_a + nb_c0 + nb_c1;
    auto step_args = [&]() { return focops_step_args(c, f->pp); };
    // A minibatch step is THREE launches when its rows fit ppo_wgrad_kernel's one-workgroup-per-output-tile layout (<= 512 rows:
    // every batch size up to 256 incl. its merged last minibatch): the activation side of all three networks (actor: FOCOPS
    // loss head, critics: regression head), ppo_wgrad_kernel (final gradients + per-block squared norms, no split-K partials
    // to add up), focops_step_kernel (clip over the actor alone, Adam of the three networks, logged row).  sum(theta^2) of the
    // critics and sigma_param as they were BEFORE the step -- the logged row wants them -- are left behind by the previous
    // step's Adam (double-buffered) and computed once at the start of the pass.  Larger minibatches keep the four-launch step
    // (fb_wgrad_kernel's split-K over workgroups + focops_prep_kernel).  The critics' and the actor's updates do not read each
    // other's parameters, so one launch each is the reference's critics_loss -> policy_loss order (focops.py:236-246) with
    // nothing reordered inside a network.
    // A layered context (hidden_sizes of another depth / width, host_layered.inc) runs the activation side layer by layer and
    // hands the finished gradient of all three networks to the prep / step pair as ONE "partial".
    const bool layered = c->lay != nullptr;
    const bool fast_pass = !layered && !f->no_fast && c->mbp_max <= 512;
    if (fast_pass) {
        FocopsStepArgs sa = step_args();
        sa.nparts = 0;
        hipLaunchKernelGGL(focops_prep_kernel, dim3(nb_all), dim3(256), 0, s, c->md, sa);     // psq / sig_stash of [pp]
    }
    for (int mb = 0; mb < nmb; ++mb) {
        const int start = c->mb_start[(size_t)mb], size = c->mb_size[(size_t)mb];
        const int tiles = (size + 15) / 16, rows_pad = tiles * 16;
        FbArgs a = focops_tile_args(c, start, size);
        const bool rows4 = !layered && focops_rows4(c, tiles, 1);
        int rc = 0;
        if (layered) {
            LayState* ls = c->lay;
            rc = lay_fwd(c, a.obs, size);
            if (rc) return rc;
            LayFbHeadArgs h{};
            h.out = ls->out; h.dout = ls->dout; h.rd = a.rd; h.statp = f->statp_pi; h.P = c->P; h.sigma = ls->lm.net[0].sigma;
            h.mbp = ls->mbp; h.net0 = 0; h.ny = 3; h.Da = ls->lm.Da; h.unbounded = ls->lm.unbounded; h.N = size; h.mode = FB_MODE_FOCOPS;
            h.max_action = a.max_action; h.cr = a.cr; h.cc = a.cc; h.eta = a.eta;
            hipLaunchKernelGGL(lay_fb_head_kernel, dim3(tiles, 3), dim3(256), 0, s, h);
            HIPCHK(hipGetLastError());
            rc = lay_bwd(c, a.obs, size);
        } else
        rc = dispatch_H(H, [&](auto hc) {
            constexpr int HH = decltype(hc)::value;
            if (rows4) hipLaunchKernelGGL((fb_tile_kernel<HH, 4>), dim3(4 * tiles, 3), dim3(4 * HH), 0, s, c->P, c->md, a);
            else hipLaunchKernelGGL((fb_tile_kernel<HH, 16>), dim3(tiles, 3), dim3(4 * HH), 0, s, c->P, c->md, a);
            HIPCHK(hipGetLastError());
            return 0;
        });
        if (rc) return rc;
        FocopsStepArgs sa = step_args();
        const int pb = wg_blocks_per_net(H);                  // ppo_wgrad_kernel: tile + aux blocks per network
        if (fast_pass) {
            const WgradPtrs wp = focops_wgrad_ptrs(c, a.obs, rows_pad);
            const PpoStepArgs none{};
            rc = dispatch_H(H, [&](auto hc) {
                constexpr int HH = decltype(hc)::value;
                hipLaunchKernelGGL((ppo_wgrad_kernel<HH, false, false>), dim3(wg_grid(H, 3)), dim3(1024), 0, s, c->md, wp, rows_pad, none, 0);
                HIPCHK(hipGetLastError());
                return 0;
            });
            if (rc) return rc;
            sa.nparts = 0; sa.parts = nullptr;
            sa.gsq_part = c->gsq_part; sa.n_gsq_part = pb; sa.gsq_net = f->gsq_net;
        } else if (layered) {
            sa.parts = c->G; sa.nparts = 1;          // lay_bwd left the whole gradient in G
        } else {
            FbWgradArgs wa = focops_split_args(c, a.obs, size, rows_pad);
            int nsplit = 1;
            rc = wgrad_launch<false>(c, c->md, wa, 3, c->n_dev, &nsplit);
            if (rc) return rc;
            sa.parts = c->wg_parts; sa.nparts = nsplit;
        }
        focops_step_fill(c, sa, c->n_steps + mb, mb, nmb, size, rows4 ? 4 * tiles : tiles);
        if (!fast_pass) hipLaunchKernelGGL(focops_prep_kernel, dim3(nb_all), dim3(256), 0, s, c->md, sa);
        hipLaunchKernelGGL(focops_step_kernel, dim3(nb_all + 1), dim3(256), 0, s, c->md, sa);
        HIPCHK(hipGetLastError());
        f->pp ^= 1;
    }
    c->n_steps += nmb;
    c->pass_index += 1;
    return pass_verdict(c, stopped_out);                     // the reference's `break`
}
