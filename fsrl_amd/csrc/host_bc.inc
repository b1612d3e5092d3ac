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
//
// The call is four steps that fsrl_bc_update_group (host_bc_group.inc) takes per member as well: bc_check_ctx / bc_check_call (every
// refusal, nothing touched), bc_prepare (the working set, the indices on their way to the device), bc_member (the kernels' arguments,
// whose optimiser), and per update bc_advance (the step count and the host's Adam scalars).  fsrl_bc_update_layered
// (host_bc_layered.inc) shares the checks, bc_prepare's index half (bc_prepare_idx), bc_who, bc_advance and bc_actor_old.
struct BcState {
    Mem mem;
    int cap_rows = 0; size_t cap_idx = 0; int cap_updates = 0;
    float *A1 = nullptr, *A2 = nullptr, *D1 = nullptr, *D2 = nullptr, *DO = nullptr, *lossp = nullptr;
    float* G = nullptr;                       // replay contexts: the actor gradient (on-policy contexts write c->G)
    int *d_idx = nullptr, *h_idx = nullptr;   // [n_updates][B], device / pinned
    float *d_loss = nullptr, *h_loss = nullptr;
    // member 0 of a grouped call (host_bc_group.inc): the call's tables and the event behind its last launch
    BcGroupTable *d_tab = nullptr, *h_tab = nullptr;
    BcGroupStep *d_steps = nullptr, *h_steps = nullptr;
    int cap_steps = 0;
    hipEvent_t g_done = nullptr;
};
static void bc_free(fsrl_ctx* c) {
    if (!c->bc) return;
    if (c->bc->g_done) (void)hipEventDestroy(c->bc->g_done);
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

// what is refused of a context, whatever the call asks of it
static int bc_check_state(fsrl_ctx* c) {
    CHECK_ARG(!c->in_update, "fsrl_bc_update inside an update");
    CHECK_ARG(!c->group && !c->sac_group && !c->cvpo_group && !c->cgroup,
              "fsrl_bc_update: the context is a member of a live group (destroy the group first)");
    if (ctx_is_replay(c) && !sac_of(c)) return fail(FSRL_ESTATE, "fsrl_bc_update before fsrl_sac_init / fsrl_cvpo_init");
    if (c->cfg.algo == FSRL_ALGO_FOCOPS && !c->foc) return fail(FSRL_ESTATE, "fsrl_bc_update before fsrl_focops_init");
    return 0;
}
// the fused calls (solo and grouped) and the layered one each refuse the other's contexts, then share the rest
static int bc_check_ctx(fsrl_ctx* c) {
    CHECK_ARG(!c->lay, "fsrl_bc_update: layered contexts are not supported (two hidden layers of at most 256 units only): use fsrl_bc_update_layered");
    return bc_check_state(c);
}
static int bc_check_ctx_layered(fsrl_ctx* c) {
    CHECK_ARG(c->lay, "fsrl_bc_update_layered: the context is fused (two hidden layers of at most 256 units): use fsrl_bc_update");
    return bc_check_state(c);
}
// ... and of n_updates updates of batch_size rows on it, the rows taken from `store`'s store (the context's own; a grouped call
// with shared_store: member 0's)
static int bc_check_call(fsrl_ctx* c, const fsrl_ctx* store, int32_t batch_size, int32_t n_updates, int32_t loss, const int64_t* indices) {
    CHECK_ARG(batch_size >= 1 && n_updates >= 1, "batch_size and n_updates must be >= 1");
    CHECK_ARG((int64_t)batch_size * n_updates < (int64_t)1 << 28, "batch_size * n_updates too large");
    CHECK_ARG(loss == BC_LOSS_MSE || loss == BC_LOSS_NLL, "loss must be 0 (mse) or 1 (nll)");
    const SacState* s = sac_of(c);
    CHECK_ARG(!(s && s->ddpg && loss == BC_LOSS_NLL), "fsrl_bc_update: nll needs a Gaussian actor; the DDPG-Lagrangian actor is deterministic");
    CHECK_ARG(fsrl_store_len(const_cast<fsrl_ctx*>(store)) > 0, "fsrl_bc_update: the store is empty");
    auto slot_live = [&](int64_t i) {
        if (i < 0 || i >= store->maxsize) return false;
        return i % store->sub_size < store->env[(size_t)(i / store->sub_size)].size;
    };
    if (indices)
        for (size_t j = 0, n_idx = (size_t)batch_size * n_updates; j < n_idx; ++j)
            CHECK_ARG(slot_live(indices[j]), "fsrl_bc_update: index %lld (position %lld) is outside the stored rows", (long long)indices[j],
                      (long long)j);
    return 0;
}

// The call's [n_updates][B] indices on their way to the device on stream `st`, with the per-update loss slots and a replay context's
// gradient vector: the half of bc_prepare that the fused and the layered call share.  The caller has drained the streams.
static int bc_prepare_idx(fsrl_ctx* c, const fsrl_ctx* store, int B, int n_updates, const int64_t* indices, uint64_t seed, hipStream_t st) {
    BcState* k = c->bc;
    SacState* s = sac_of(c);
    const size_t n_idx = (size_t)B * n_updates;
    if (s && !k->G) { HIPCHK(k->mem.dev(&k->G, (size_t)s->na_dev * 4)); HIPCHK(hipMemsetAsync(k->G, 0, (size_t)s->na_dev * 4, st)); }
    if (k->cap_idx < n_idx) HIPCHK(k->mem.regrow(k->cap_idx, n_idx, n_idx, {Mem::D(&k->d_idx, n_idx * 4), Mem::H(&k->h_idx, n_idx * 4)}));
    if (k->cap_updates < n_updates)
        HIPCHK(k->mem.regrow(k->cap_updates, n_updates, n_updates, {Mem::D(&k->d_loss, (size_t)n_updates * 4), Mem::H(&k->h_loss, (size_t)n_updates * 4)}));
    if (indices) {
        for (size_t j = 0; j < n_idx; ++j) k->h_idx[j] = (int)indices[j];
    } else {              // the library's own draw: uniform over the stored rows in sample(0) order, a xoshiro256** stream of the seed
        const int64_t n = sample0(store, store->h_indices, nullptr);
        uint64_t x[4] = {0x9E3779B97F4A7C15ull ^ seed, 0xBF58476D1CE4E5B9ull + seed * 0x94D049BB133111EBull, 0xD6E8FEB86659FD93ull, seed | 1};
        for (int w = 0; w < 8; ++w) (void)xoshiro_next(x);
        for (size_t j = 0; j < n_idx; ++j) k->h_idx[j] = store->h_indices[(size_t)(xoshiro_next(x) % (uint64_t)n)];
    }
    HIPCHK(hipMemcpyAsync(k->d_idx, k->h_idx, n_idx * 4, hipMemcpyHostToDevice, st));
    return 0;
}
// The working set at the call's size and the call's [n_updates][B] indices on their way to the device, on stream `st` (the context's
// compute stream; a grouped call: member 0's).  The caller has joined `store`'s store.
static int bc_prepare(fsrl_ctx* c, const fsrl_ctx* store, int B, int n_updates, const int64_t* indices, uint64_t seed, hipStream_t st) {
    if (!c->bc) c->bc = new BcState();
    BcState* k = c->bc;
    const int H = c->cfg.hidden, rows_pad = round_up(B, 16), tiles = rows_pad / 16;
    // an earlier call's copies have left the pinned buffers and its kernels the side buffers: every call waits here for the context's
    // stream to drain before it enqueues its own work (with loss_out == NULL it returns without waiting for THAT work); a grouped
    // call leaves every member's stream behind its last launch
    HIPCHK(hipStreamSynchronize(c->compute));
    if (st != c->compute) HIPCHK(hipStreamSynchronize(st));
    if (k->cap_rows < rows_pad) {
        const size_t rh = (size_t)rows_pad * H * 4;
        HIPCHK(k->mem.regrow(k->cap_rows, rows_pad, rows_pad,
                             {Mem::D(&k->A1, rh), Mem::D(&k->A2, rh), Mem::D(&k->D1, rh), Mem::D(&k->D2, rh),
                              Mem::D(&k->DO, (size_t)rows_pad * FSRL_DOW * 4), Mem::D(&k->lossp, (size_t)tiles * 4)}));
    }
    return bc_prepare_idx(c, store, B, n_updates, indices, seed, st);
}

// A prepared context as the kernels and the step loop take it: both kernels' arguments for update 0 (idx, loss_out: the call's first
// block and slot), the actor's parameters, the head, and whose step count and rate the updates use.
struct BcMember {
    BcArgs a; BcWgradArgs w;
    const float* P; const ModelDesc* md;
    int head, tiles, grid_w;
    int64_t* t; float lr;
};
// whose optimiser a BC step is (the table above) and what the loss head makes of the actor's output; G: where the step's gradient goes
struct BcWho { float *P, *M, *V, *G; int64_t* t; float lr; int head, mean_tanh; };
static BcWho bc_who(fsrl_ctx* c, const ModelDesc* md) {
    SacState* s = sac_of(c);
    BcWho w{c->P, c->M, c->V, c->G, &c->adam_t, c->cfg.lr, DC_HEAD_ONPOLICY, md->unbounded ? 0 : 1};
    if (s) {
        w.P = s->PA; w.M = s->MA; w.V = s->VA; w.G = c->bc->G; w.t = &s->t_actor;
        w.lr = s->cvpo ? s->ccfg.actor_lr : s->cfg.actor_lr;
        w.head = s->ddpg ? DC_HEAD_DDPG : DC_HEAD_GAUSS; w.mean_tanh = s->ddpg ? 1 : s->mean_tanh;
    } else if (c->foc) {
        w.t = &c->foc->t_actor; w.lr = c->foc->cfg.actor_lr;
    }
    return w;
}
static BcMember bc_member(fsrl_ctx* c, const fsrl_ctx* store, int B, int loss) {
    BcState* k = c->bc;
    SacState* s = sac_of(c);
    BcMember m{};
    m.md = s ? &s->mda : &c->md;
    const BcWho who = bc_who(c, m.md);
    float *P = who.P, *M = who.M, *V = who.V, *G = who.G;
    m.lr = who.lr; m.t = who.t; m.head = who.head;
    const int mean_tanh = who.mean_tanh;
    m.P = P;
    const int rows_pad = round_up(B, 16);
    m.tiles = rows_pad / 16;
    BcArgs& a = m.a;
    a.obs = store->st.obs; a.act = store->st.act; a.idx = k->d_idx;
    a.A1 = k->A1; a.A2 = k->A2; a.D1 = k->D1; a.D2 = k->D2; a.DO = k->DO; a.lossp = k->lossp;
    a.B = B; a.loss = loss; a.mean_tanh = mean_tanh; a.max_action = c->cfg.max_action;
    BcWgradArgs& w = m.w;
    w.A1 = k->A1; w.A2 = k->A2; w.D1 = k->D1; w.D2 = k->D2; w.DO = k->DO; w.obs = store->st.obs; w.idx = k->d_idx;
    w.P = P; w.M = M; w.V = V; w.G = G; w.lossp = k->lossp; w.loss_out = k->d_loss; w.tiles = m.tiles; w.B = B; w.rows_pad = rows_pad;
    w.sigma_job = (m.head == DC_HEAD_ONPOLICY && loss == BC_LOSS_NLL) ? 1 : 0;
    w.sigma_zero = (m.head == DC_HEAD_ONPOLICY && loss == BC_LOSS_MSE) ? 1 : 0;
    w.one_minus_b1 = (float)(1.0 - (double)c->cfg.beta1); w.beta2 = c->cfg.beta2; w.one_minus_b2 = (float)(1.0 - (double)c->cfg.beta2);
    w.eps = c->cfg.adam_eps;
    m.grid_w = bc_wg_grid(c->cfg.hidden, m.md->Do, w.sigma_job);
    return m;
}
// one more update of the member's optimiser: its step count moves, the host's Adam scalars of that step
static AdamStep bc_advance(const fsrl_ctx* c, const BcMember& m) {
    *m.t += 1;
    return adam_step(m.lr, c->cfg.beta1, c->cfg.beta2, *m.t);
}
// behind the member's last update, on the stream that ran it: actor_old := the pre-trained actor, W2 mirror included
static int bc_actor_old(fsrl_ctx* c, hipStream_t st) {
    SacState* s = sac_of(c);
    if (s && (s->ddpg || s->cvpo)) HIPCHK(hipMemcpyAsync(s->PAT, s->PA, sac_actor_bytes(c, s), hipMemcpyDeviceToDevice, st));
    return 0;
}

extern "C" int fsrl_bc_update(fsrl_ctx* c, int32_t batch_size, int32_t n_updates, int32_t loss, const int64_t* indices, uint64_t seed,
                              float* loss_out) {
    CHECK_ARG(c, "null ctx");
    int rc = bc_check_ctx(c);
    if (!rc) rc = bc_check_call(c, c, batch_size, n_updates, loss, indices);
    if (rc) return rc;
    // ---- nothing has been touched up to here
    ENTER_DEV(c);
    rc = join_store(c);
    if (rc) return rc;
    hipStream_t st = c->compute;
    rc = bc_prepare(c, c, batch_size, n_updates, indices, seed, st);
    if (rc) return rc;
    BcState* k = c->bc;
    BcMember m = bc_member(c, c, batch_size, loss);
    const int H = c->cfg.hidden, B = batch_size;
    const ModelDesc& md = *m.md;
    c->theta_version += 1;
    for (int u = 0; u < n_updates; ++u) {
        m.a.idx = m.w.idx = k->d_idx + (size_t)u * B;
        m.w.loss_out = k->d_loss + u;
        const AdamStep as = bc_advance(c, m);
        m.w.step_size = as.step_size; m.w.bc2_sqrt = as.bc2_sqrt;
        rc = dispatch_H(H, [&](auto hc) {
            constexpr int HH = decltype(hc)::value;
            if (m.head == DC_HEAD_ONPOLICY) hipLaunchKernelGGL((bc_fwd_bwd_kernel<HH, DC_HEAD_ONPOLICY>), dim3(m.tiles), dim3(4 * HH), 0, st, m.P, md, m.a);
            else if (m.head == DC_HEAD_GAUSS) hipLaunchKernelGGL((bc_fwd_bwd_kernel<HH, DC_HEAD_GAUSS>), dim3(m.tiles), dim3(4 * HH), 0, st, m.P, md, m.a);
            else hipLaunchKernelGGL((bc_fwd_bwd_kernel<HH, DC_HEAD_DDPG>), dim3(m.tiles), dim3(4 * HH), 0, st, m.P, md, m.a);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(bc_wgrad_kernel<HH>, dim3(m.grid_w), dim3(256), 0, st, md, m.w);
            HIPCHK(hipGetLastError());
            return 0;
        });
        if (rc) return rc;
    }
    rc = bc_actor_old(c, st);
    if (rc) return rc;
    if (loss_out) {
        HIPCHK(hipMemcpyAsync(k->h_loss, k->d_loss, (size_t)n_updates * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        memcpy(loss_out, k->h_loss, (size_t)n_updates * 4);
    }
    return 0;
}
