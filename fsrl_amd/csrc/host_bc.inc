// host_bc.inc -- behaviour cloning: fsrl_bc_update (part of fsrl_hip.hip; kernels_bc.hpp).
// Included once by fsrl_hip.hip: same translation unit, so the static helpers, fsrl_ctx and SacState above are visible.
// ====================================================================================== behaviour cloning
// Whose optimiser a BC step is (the ACTOR's parameters only; the critics' parameters and moments are never touched):
//   PPO-Lag            the shared Adam: the actor's slots of M / V, its one step count (adam_t) advances, lr = cfg.lr
//   FOCOPS             the actor's Adam: t_actor, actor_lr (no l2 term, no clip)
//   CPO / TRPO-Lag     the trust-region step has no actor optimiser: the actor's slots of M / V, which nothing else reads, adam_t
//                      (these contexts' critics count their own steps), lr = cfg.lr
//   SAC / DDPG / CVPO  the actor's Adam: MA / VA, t_actor, actor_lr
// The W2 mirror of the actor is written with W2 (adam_element), so every collector and update reads the stepped weights.  The replay
// agents' actor_old (DDPG-Lag's target actor, CVPO's old policy) is set EQUAL to the actor at the end of the call: a pre-trained
// actor with a target that still holds the initial weights would start the RL phase from targets of an untrained policy.
struct BcState {
    Mem mem;
    int cap_rows = 0; size_t cap_idx = 0; int cap_updates = 0;
    float *A1 = nullptr, *A2 = nullptr, *D1 = nullptr, *D2 = nullptr, *DO = nullptr, *lossp = nullptr;
    float* G = nullptr;                       // replay contexts: the actor gradient (on-policy contexts write c->G)
    int *d_idx = nullptr, *h_idx = nullptr;   // [n_updates][B], device / pinned
    float *d_loss = nullptr, *h_loss = nullptr;
};
static void bc_free(fsrl_ctx* c) {
    if (!c->bc) return;
    c->bc->mem.release_all();
    delete c->bc;
    c->bc = nullptr;
}

// fsrl_grads_get on a replay context that has run a BC step: the actor gradient of the last one, in the actor's API order
static int bc_grads_get(fsrl_ctx* c, float* flat, int64_t n, bool* served) {
    SacState* s = sac_of(c);
    *served = s && c->bc && c->bc->G;
    if (!*served) return 0;
    CHECK_ARG(n == s->na_api, "fsrl_grads_get after fsrl_bc_update: n must be the actor's parameter count");
    ENTER_DEV(c);
    return sac_copy(c, s->tmap_a, s->mda, s->na_dev, c->bc->G, nullptr, flat);
}

extern "C" int fsrl_bc_update(fsrl_ctx* c, int32_t batch_size, int32_t n_updates, int32_t loss, const int64_t* indices, uint64_t seed,
                              float* loss_out) {
    CHECK_ARG(c, "null ctx");
    CHECK_ARG(!c->lay, "fsrl_bc_update: layered contexts are not supported (two hidden layers of at most 256 units only)");
    CHECK_ARG(batch_size >= 1 && n_updates >= 1, "batch_size and n_updates must be >= 1");
    CHECK_ARG((int64_t)batch_size * n_updates < (int64_t)1 << 28, "batch_size * n_updates too large");
    CHECK_ARG(loss == BC_LOSS_MSE || loss == BC_LOSS_NLL, "loss must be 0 (mse) or 1 (nll)");
    CHECK_ARG(!c->in_update, "fsrl_bc_update inside an update");
    CHECK_ARG(!c->group && !c->sac_group && !c->cvpo_group && !c->cgroup,
              "fsrl_bc_update: the context is a member of a live group (destroy the group first)");
    SacState* s = sac_of(c);
    if (ctx_is_replay(c) && !s) return fail(FSRL_ESTATE, "fsrl_bc_update before fsrl_sac_init / fsrl_cvpo_init");
    if (c->cfg.algo == FSRL_ALGO_FOCOPS && !c->foc) return fail(FSRL_ESTATE, "fsrl_bc_update before fsrl_focops_init");
    CHECK_ARG(!(s && s->ddpg && loss == BC_LOSS_NLL), "fsrl_bc_update: nll needs a Gaussian actor; the DDPG-Lagrangian actor is deterministic");
    const int64_t stored = fsrl_store_len(c);
    CHECK_ARG(stored > 0, "fsrl_bc_update: the store is empty");
    const int B = batch_size;
    const size_t n_idx = (size_t)B * n_updates;
    auto slot_live = [&](int64_t i) {
        if (i < 0 || i >= c->maxsize) return false;
        return i % c->sub_size < c->env[(size_t)(i / c->sub_size)].size;
    };
    if (indices)
        for (size_t j = 0; j < n_idx; ++j)
            CHECK_ARG(slot_live(indices[j]), "fsrl_bc_update: index %lld (position %lld) is outside the stored rows", (long long)indices[j],
                      (long long)j);
    // ---- nothing has been touched up to here
    ENTER_DEV(c);
    int rc = join_store(c);
    if (rc) return rc;
    if (!c->bc) c->bc = new BcState();
    BcState* k = c->bc;
    const int H = c->cfg.hidden, rows_pad = round_up(B, 16), tiles = rows_pad / 16;
    const ModelDesc& md = s ? s->mda : c->md;
    if (k->cap_rows < rows_pad) {
        HIPCHK(hipStreamSynchronize(c->compute));
        const size_t rh = (size_t)rows_pad * H * 4;
        HIPCHK(k->mem.regrow(k->cap_rows, rows_pad, rows_pad,
                             {Mem::D(&k->A1, rh), Mem::D(&k->A2, rh), Mem::D(&k->D1, rh), Mem::D(&k->D2, rh),
                              Mem::D(&k->DO, (size_t)rows_pad * FSRL_DOW * 4), Mem::D(&k->lossp, (size_t)tiles * 4)}));
    }
    if (s && !k->G) { HIPCHK(k->mem.dev(&k->G, (size_t)s->na_dev * 4)); HIPCHK(hipMemsetAsync(k->G, 0, (size_t)s->na_dev * 4, c->compute)); }
    if (k->cap_idx < n_idx) {
        HIPCHK(hipStreamSynchronize(c->compute));
        HIPCHK(k->mem.regrow(k->cap_idx, n_idx, n_idx, {Mem::D(&k->d_idx, n_idx * 4), Mem::H(&k->h_idx, n_idx * 4)}));
    }
    if (k->cap_updates < n_updates) {
        HIPCHK(hipStreamSynchronize(c->compute));
        HIPCHK(k->mem.regrow(k->cap_updates, n_updates, n_updates, {Mem::D(&k->d_loss, (size_t)n_updates * 4), Mem::H(&k->h_loss, (size_t)n_updates * 4)}));
    }
    // an earlier call's copy has left the pinned index buffer: every call waits here for the context's stream to drain before it
    // enqueues its own work (with loss_out == NULL it returns without waiting for THAT work)
    HIPCHK(hipStreamSynchronize(c->compute));
    if (indices) {
        for (size_t j = 0; j < n_idx; ++j) k->h_idx[j] = (int)indices[j];
    } else {              // the library's own draw: uniform over the stored rows in sample(0) order, a xoshiro256** stream of the seed
        const int64_t n = sample0(c, c->h_indices, nullptr);
        uint64_t st[4] = {0x9E3779B97F4A7C15ull ^ seed, 0xBF58476D1CE4E5B9ull + seed * 0x94D049BB133111EBull, 0xD6E8FEB86659FD93ull, seed | 1};
        for (int w = 0; w < 8; ++w) (void)xoshiro_next(st);
        for (size_t j = 0; j < n_idx; ++j) k->h_idx[j] = c->h_indices[(size_t)(xoshiro_next(st) % (uint64_t)n)];
    }
    hipStream_t st = c->compute;
    HIPCHK(hipMemcpyAsync(k->d_idx, k->h_idx, n_idx * 4, hipMemcpyHostToDevice, st));

    float *P = c->P, *M = c->M, *V = c->V, *G = c->G, lr = c->cfg.lr;
    int64_t* t = &c->adam_t;
    int head = DC_HEAD_ONPOLICY, mean_tanh = md.unbounded ? 0 : 1;
    if (s) {
        P = s->PA; M = s->MA; V = s->VA; G = k->G; t = &s->t_actor;
        lr = s->cvpo ? s->ccfg.actor_lr : s->cfg.actor_lr;
        head = s->ddpg ? DC_HEAD_DDPG : DC_HEAD_GAUSS; mean_tanh = s->ddpg ? 1 : s->mean_tanh;
    } else if (c->foc) {
        t = &c->foc->t_actor; lr = c->foc->cfg.actor_lr;
    }
    c->theta_version += 1;
    BcArgs a{};
    a.obs = c->st.obs; a.act = c->st.act;
    a.A1 = k->A1; a.A2 = k->A2; a.D1 = k->D1; a.D2 = k->D2; a.DO = k->DO; a.lossp = k->lossp;
    a.B = B; a.loss = loss; a.mean_tanh = mean_tanh; a.max_action = c->cfg.max_action;
    BcWgradArgs w{};
    w.A1 = k->A1; w.A2 = k->A2; w.D1 = k->D1; w.D2 = k->D2; w.DO = k->DO; w.obs = c->st.obs;
    w.P = P; w.M = M; w.V = V; w.G = G; w.lossp = k->lossp; w.tiles = tiles; w.B = B; w.rows_pad = rows_pad;
    w.sigma_job = (head == DC_HEAD_ONPOLICY && loss == BC_LOSS_NLL) ? 1 : 0;
    w.sigma_zero = (head == DC_HEAD_ONPOLICY && loss == BC_LOSS_MSE) ? 1 : 0;
    w.one_minus_b1 = (float)(1.0 - (double)c->cfg.beta1); w.beta2 = c->cfg.beta2; w.one_minus_b2 = (float)(1.0 - (double)c->cfg.beta2);
    w.eps = c->cfg.adam_eps;
    const int grid_w = bc_wg_grid(H, md.Do, w.sigma_job);
    for (int u = 0; u < n_updates; ++u) {
        a.idx = w.idx = k->d_idx + (size_t)u * B;
        w.loss_out = k->d_loss + u;
        *t += 1;
        const AdamStep as = adam_step(lr, c->cfg.beta1, c->cfg.beta2, *t);
        w.step_size = as.step_size; w.bc2_sqrt = as.bc2_sqrt;
        rc = dispatch_H(H, [&](auto hc) {
            constexpr int HH = decltype(hc)::value;
            if (head == DC_HEAD_ONPOLICY) hipLaunchKernelGGL((bc_fwd_bwd_kernel<HH, DC_HEAD_ONPOLICY>), dim3(tiles), dim3(4 * HH), 0, st, P, md, a);
            else if (head == DC_HEAD_GAUSS) hipLaunchKernelGGL((bc_fwd_bwd_kernel<HH, DC_HEAD_GAUSS>), dim3(tiles), dim3(4 * HH), 0, st, P, md, a);
            else hipLaunchKernelGGL((bc_fwd_bwd_kernel<HH, DC_HEAD_DDPG>), dim3(tiles), dim3(4 * HH), 0, st, P, md, a);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(bc_wgrad_kernel<HH>, dim3(grid_w), dim3(256), 0, st, md, w);
            HIPCHK(hipGetLastError());
            return 0;
        });
        if (rc) return rc;
    }
    if (s && (s->ddpg || s->cvpo))         // actor_old := the pre-trained actor, W2 mirror included
        HIPCHK(hipMemcpyAsync(s->PAT, s->PA, sac_actor_bytes(c, s), hipMemcpyDeviceToDevice, st));
    if (loss_out) {
        HIPCHK(hipMemcpyAsync(k->h_loss, k->d_loss, (size_t)n_updates * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        memcpy(loss_out, k->h_loss, (size_t)n_updates * 4);
    }
    return 0;
}
