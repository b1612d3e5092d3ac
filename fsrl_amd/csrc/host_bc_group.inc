// host_bc_group.inc -- fsrl_bc_update_group: k contexts' behaviour-cloning updates, TWO launches per step for all of them (part of
// fsrl_hip.hip, behind host_bc.inc; kernels_bc_group.hpp; include/fsrl_hip.h "Behaviour cloning").
//
// A free function over contexts, like fsrl_collect_device_group: pre-training comes before the update and collect groups exist, and
// its members are not owned here.  Per member the checks, the working set, the kernels' arguments and the optimiser's step are
// fsrl_bc_update's (bc_check_ctx / bc_check_call, bc_prepare, bc_member, bc_advance); what the members must agree on is what the ONE
// instantiation and the shared ModelDesc stand for (bc_group_agree).  The call runs max_i n_updates[i] steps; member i is active in
// the first n_updates[i] of them, and with n_updates[i] == 0 nothing of it is read or written.
// Ordering.  The launches go on member 0's compute stream.  bc_prepare drains every active member's own stream on the host (as the
// solo call does) and sends its indices down member 0's stream, so the launches are behind everything the members had enqueued;
// behind the last launch an event puts every other member's stream behind the call, so that whatever a member enqueues next -- on
// its own stream -- sees the pre-trained actor, also when loss_out == NULL and the call returns with its work in flight.
// The member table, the step table and the event hang off member 0's BcState and are kept.
static int bc_head_kind(const fsrl_ctx* c) {
    const SacState* s = sac_of(const_cast<fsrl_ctx*>(c));
    return !s ? DC_HEAD_ONPOLICY : s->ddpg ? DC_HEAD_DDPG : DC_HEAD_GAUSS;
}
// member i against member 0.  What travels in each member's own row may differ: max_action, the learning rate, Adam's betas and eps,
// batch size, loss, update count.
static int bc_group_agree(const fsrl_ctx* c, const fsrl_ctx* c0, int i) {
    static const char* const heads[] = {"an on-policy", "a Gaussian replay (SAC-Lag, CVPO)", "a DDPG-Lag"};
    CHECK_ARG(c->device == c0->device, "member %d: members live on one device", i);
    CHECK_ARG(bc_head_kind(c) == bc_head_kind(c0), "member %d is %s context and member 0 %s one: a grouped behaviour-cloning update has "
              "one head kind (on-policy, Gaussian or DDPG)", i, heads[bc_head_kind(c)], heads[bc_head_kind(c0)]);
    CHECK_ARG(c->cfg.obs_dim == c0->cfg.obs_dim && c->cfg.act_dim == c0->cfg.act_dim && c->cfg.hidden == c0->cfg.hidden &&
              c->cfg.hidden1 == c0->cfg.hidden1 && c->cfg.hidden2 == c0->cfg.hidden2,
              "member %d: members must have one network shape (obs_dim, act_dim, hidden, hidden1, hidden2): (%d, %d, %d, %d, %d), member "
              "0's (%d, %d, %d, %d, %d)", i, c->cfg.obs_dim, c->cfg.act_dim, c->cfg.hidden, c->cfg.hidden1, c->cfg.hidden2, c0->cfg.obs_dim,
              c0->cfg.act_dim, c0->cfg.hidden, c0->cfg.hidden1, c0->cfg.hidden2);
    const SacState* s = sac_of(const_cast<fsrl_ctx*>(c)); const SacState* s0 = sac_of(const_cast<fsrl_ctx*>(c0));
    if (!s)
        CHECK_ARG((c->cfg.unbounded != 0) == (c0->cfg.unbounded != 0), "member %d: members must share unbounded (the actor's mean is %s, "
                  "member 0's %s)", i, c->cfg.unbounded ? "the head itself" : "max_action * tanh(head)",
                  c0->cfg.unbounded ? "the head itself" : "max_action * tanh(head)");
    else
        CHECK_ARG(s->mean_tanh == s0->mean_tanh, "member %d: members must share actor_mean (the actor's mean is %s, member 0's %s)", i,
                  s->mean_tanh ? "max_action * tanh(head)" : "unbounded", s0->mean_tanh ? "max_action * tanh(head)" : "unbounded");
    return 0;
}

// everything behind the checks; the caller waits for the launch stream when this fails half-way
static int bc_group_run(fsrl_ctx** ctxs, int k, const int32_t* batch_size, const int32_t* n_updates, const int32_t* loss,
                        const int64_t* indices, const uint64_t* seeds, bool shared_store, float* loss_out) {
    fsrl_ctx* c0 = ctxs[0];
    hipStream_t st = c0->compute;
    int steps = 0;
    for (int i = 0; i < k; ++i) steps = std::max(steps, (int)n_updates[i]);
    if (!steps) return 0;
    for (int i = 0; i < k; ++i) {
        if (i && !n_updates[i]) continue;       // member 0's stream carries the launches also where it sits out: its resident actor ends
        ENTER_DEV(ctxs[i]);
        if (shared_store ? i == 0 : n_updates[i] != 0) {       // the store's rows behind its owner's compute stream, drained below
            const int rc = join_store(ctxs[i]);
            if (rc) return rc;
        }
    }
    HIPCHK(hipStreamSynchronize(st));
    BcMember mem[FSRL_MAX_GROUP];
    const int64_t* ind = indices;
    for (int i = 0; i < k; ++i) {
        if (!n_updates[i]) continue;
        const fsrl_ctx* store = shared_store ? c0 : ctxs[i];
        const int rc = bc_prepare(ctxs[i], store, batch_size[i], n_updates[i], ind, seeds ? seeds[i] : 0, st);
        if (rc) return rc;
        if (ind) ind += (size_t)batch_size[i] * n_updates[i];
        mem[i] = bc_member(ctxs[i], store, batch_size[i], loss[i]);
    }
    if (!c0->bc) c0->bc = new BcState();
    BcState* k0 = c0->bc;
    if (!k0->g_done) HIPCHK(hipEventCreateWithFlags(&k0->g_done, hipEventDisableTiming));
    if (!k0->d_tab) HIPCHK(k0->mem.dev(&k0->d_tab, sizeof(BcGroupTable)));
    if (!k0->h_tab) HIPCHK(k0->mem.pinned(&k0->h_tab, sizeof(BcGroupTable)));
    HIPCHK(k0->mem.regrow(k0->cap_steps, steps, steps, {Mem::D(&k0->d_steps, (size_t)steps * sizeof(BcGroupStep)),
                                                        Mem::H(&k0->h_steps, (size_t)steps * sizeof(BcGroupStep))}));
    // ---- the tables: the members' rows, and per step the active members' tile prefix and Adam scalars (the members' step counts
    //      move here, in the order the solo calls move them)
    *k0->h_tab = BcGroupTable{};
    int first = -1, grid_w = 0;
    for (int i = 0; i < k; ++i) {
        if (!n_updates[i]) continue;
        if (first < 0) first = i;
        BcGroupMember& g = k0->h_tab->m[i];
        g.P = mem[i].P; g.n_updates = n_updates[i]; g.a = mem[i].a; g.w = mem[i].w;
        grid_w = std::max(grid_w, mem[i].grid_w);
        ctxs[i]->theta_version += 1;
    }
    for (int u = 0; u < steps; ++u) {
        BcGroupStep& sp = k0->h_steps[u];
        sp = BcGroupStep{};
        int at = 0;
        for (int i = 0; i < DCWG_MAX_MEMBERS; ++i) {
            sp.prefix[i] = at;
            if (i >= k || u >= n_updates[i]) continue;
            at += mem[i].tiles;
            const AdamStep as = bc_advance(ctxs[i], mem[i]);
            sp.step_size[i] = as.step_size; sp.bc2_sqrt[i] = as.bc2_sqrt;
        }
    }
    HIPCHK(hipMemcpyAsync(k0->d_tab, k0->h_tab, sizeof(BcGroupTable), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(k0->d_steps, k0->h_steps, (size_t)steps * sizeof(BcGroupStep), hipMemcpyHostToDevice, st));
    const ModelDesc md = *mem[first].md;
    const int head = mem[first].head;
    for (int u = 0; u < steps; ++u) {
        int tiles = 0, active = 0;
        for (int i = 0; i < k; ++i)
            if (u < n_updates[i]) { tiles += mem[i].tiles; active = i + 1; }
        const BcGroupTable* tab = k0->d_tab;
        const BcGroupStep* sp = k0->d_steps + u;
        const int rc = dispatch_H(c0->cfg.hidden, [&](auto hc) {
            constexpr int HH = decltype(hc)::value;
            const dim3 g(tiles), b(4 * HH);
            if (head == DC_HEAD_ONPOLICY) hipLaunchKernelGGL((bc_fwd_bwd_group_kernel<HH, DC_HEAD_ONPOLICY>), g, b, 0, st, md, tab, sp, u);
            else if (head == DC_HEAD_GAUSS) hipLaunchKernelGGL((bc_fwd_bwd_group_kernel<HH, DC_HEAD_GAUSS>), g, b, 0, st, md, tab, sp, u);
            else hipLaunchKernelGGL((bc_fwd_bwd_group_kernel<HH, DC_HEAD_DDPG>), g, b, 0, st, md, tab, sp, u);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(bc_wgrad_group_kernel<HH>, dim3(grid_w, active), dim3(256), 0, st, md, tab, sp, u);      // members behind the last active one: no workgroups
            HIPCHK(hipGetLastError());
            return 0;
        });
        if (rc) return rc;
    }
    size_t at = 0;
    for (int i = 0; i < k; ++i) {
        if (!n_updates[i]) continue;
        const int rc = bc_actor_old(ctxs[i], st);
        if (rc) return rc;
        if (loss_out) HIPCHK(hipMemcpyAsync(ctxs[i]->bc->h_loss, ctxs[i]->bc->d_loss, (size_t)n_updates[i] * 4, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipEventRecord(k0->g_done, st));
    for (int i = 0; i < k; ++i)
        if (n_updates[i] && ctxs[i]->compute != st) HIPCHK(hipStreamWaitEvent(ctxs[i]->compute, k0->g_done, 0));
    if (loss_out) {
        HIPCHK(hipStreamSynchronize(st));
        for (int i = 0; i < k; ++i) {
            if (!n_updates[i]) continue;
            memcpy(loss_out + at, ctxs[i]->bc->h_loss, (size_t)n_updates[i] * 4);
            at += (size_t)n_updates[i];
        }
    }
    return 0;
}

extern "C" int fsrl_bc_update_group(fsrl_ctx** ctxs, int32_t k, const int32_t* batch_size, const int32_t* n_updates, const int32_t* loss,
                                    const int64_t* indices, const uint64_t* seeds, int32_t shared_store, float* loss_out) {
    // ---- every refusal before anything is touched
    CHECK_ARG(k >= 1 && k <= FSRL_MAX_GROUP, "k %d: a grouped behaviour-cloning update has 1..%d members", k, FSRL_MAX_GROUP);
    CHECK_ARG(ctxs && batch_size && n_updates && loss, "null argument");
    CHECK_ARG(indices || seeds, "null argument: indices or seeds (the library draws the indices from the members' seeds)");
    for (int i = 0; i < k; ++i) {
        CHECK_ARG(ctxs[i], "member %d: null context", i);
        for (int j = 0; j < i; ++j) CHECK_ARG(ctxs[j] != ctxs[i], "member %d: its context is listed twice (member %d)", i, j);
        CHECK_ARG(n_updates[i] >= 0, "member %d: n_updates %d (0: the member sits the call out)", i, n_updates[i]);
    }
    const auto named = [](int i, int rc) { g_err = "member " + std::to_string(i) + ": " + g_err; return rc; };
    for (int i = 0; i < k; ++i) {
        const int rc = bc_check_ctx(ctxs[i]);
        if (rc) return named(i, rc);
    }
    for (int i = 1; i < k; ++i) {
        const int rc = bc_group_agree(ctxs[i], ctxs[0], i);
        if (rc) return rc;
    }
    const int64_t* ind = indices;
    for (int i = 0; i < k; ++i) {
        if (!n_updates[i]) continue;
        const int rc = bc_check_call(ctxs[i], shared_store ? ctxs[0] : ctxs[i], batch_size[i], n_updates[i], loss[i], ind);
        if (rc) return named(i, rc);
        if (ind) ind += (size_t)batch_size[i] * n_updates[i];
    }
    const int rc = bc_group_run(ctxs, k, batch_size, n_updates, loss, indices, seeds, shared_store != 0, loss_out);
    if (rc) {       // leave nothing of the call in flight: the kernels read every member's arrays from member 0's stream
        const std::string why = g_err;
        (void)hipStreamSynchronize(ctxs[0]->compute);
        g_err = why;
    }
    return rc;
}
