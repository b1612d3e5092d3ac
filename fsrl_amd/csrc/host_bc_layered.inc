// host_bc_layered.inc -- behaviour cloning for layered contexts: fsrl_bc_update_layered (part of fsrl_hip.hip; kernels_bc_layered.hpp).
// fsrl_bc_update's call around the layered kernel pair: the same checks (bc_check_call), index draw (bc_prepare_idx), optimiser table
// (bc_who), step loop (bc_advance) and end (bc_actor_old); two launches per update at any depth.  The working set is the actor's own
// LayWork (on-policy: the context's LayState; replay: SacState::ka) grown to round_up(B, 16) rows -- act[0][l] / dz[0][l] at the row
// stride round_up(w_l, 4), out-of-use `out`, and dout; BcState holds the indices, the per-tile loss slots and the per-update losses.
static int bc_lay_launch(int device, int head, bool devws, int tiles, size_t lds, hipStream_t st, const BcLayArgs& a) {
#define BCL_GO(HEAD_) (devws ? devcollect_wide_layered_go<&bc_lay_fwd_bwd_kernel<HEAD_, true>>(device, dim3(tiles), lds, st, a) \
                             : devcollect_wide_layered_go<&bc_lay_fwd_bwd_kernel<HEAD_, false>>(device, dim3(tiles), lds, st, a))
    return head == DC_HEAD_GAUSS ? BCL_GO(DC_HEAD_GAUSS) : head == DC_HEAD_DDPG ? BCL_GO(DC_HEAD_DDPG) : BCL_GO(DC_HEAD_ONPOLICY);
#undef BCL_GO
}

extern "C" int fsrl_bc_update_layered(fsrl_ctx* c, int32_t batch_size, int32_t n_updates, int32_t loss, const int64_t* indices, uint64_t seed,
                                      float* loss_out) {
    CHECK_ARG(c, "null ctx");
    int rc = bc_check_ctx_layered(c);
    if (!rc) rc = bc_check_call(c, c, batch_size, n_updates, loss, indices);
    if (rc) return rc;
    SacState* s = sac_of(c);
    const LayWork& lw = s ? s->ka : *static_cast<LayWork*>(c->lay);
    const LayNet& net = lw.lm.net[0];
    const int L = lw.L, Do = c->cfg.obs_dim, Da = c->cfg.act_dim;
    CHECK_ARG(net.l[L].out <= FSRL_MAX_ACT, "fsrl_bc_update_layered: the actor's head is %d wide (limit %d)", net.l[L].out, FSRL_MAX_ACT);
    // ---- nothing has been touched up to here
    ENTER_DEV(c);
    rc = join_store(c);
    if (rc) return rc;
    hipStream_t st = c->compute;
    const int B = batch_size, rows_pad = round_up(B, 16), tiles = rows_pad / 16;
    if (!c->bc) c->bc = new BcState();
    BcState* k = c->bc;
    HIPCHK(hipStreamSynchronize(st));         // an earlier call's copies have left the pinned buffers (bc_prepare)
    rc = s ? lay_work_ensure(c, s->mem, s->ka, rows_pad) : lay_ensure_rows(c, rows_pad, false);
    if (rc) return rc;
    if (k->cap_rows < rows_pad) HIPCHK(k->mem.regrow(k->cap_rows, rows_pad, rows_pad, {Mem::D(&k->lossp, (size_t)tiles * 4)}));
    rc = bc_prepare_idx(c, c, B, n_updates, indices, seed, st);
    if (rc) return rc;
    const BcWho who = bc_who(c, s ? &s->mda : &c->md);
    BcMember m{};
    m.t = who.t; m.lr = who.lr;
    // ---- both kernels' arguments, the weight-gradient launch's job table: once per call
    BcLayArgs a{};
    a.P = who.P; a.obs = c->st.obs; a.act = c->st.act; a.dout = lw.dout; a.lossp = k->lossp;
    a.B = B; a.loss = loss; a.mean_tanh = who.mean_tanh; a.Do = Do; a.Da = Da; a.max_action = c->cfg.max_action; a.net = net;
    BcLayWgradArgs w{};
    w.obs = c->st.obs; w.dout = lw.dout; w.P = who.P; w.M = who.M; w.V = who.V; w.G = who.G; w.lossp = k->lossp; w.tiles = tiles;
    w.B = B; w.rows_pad = rows_pad; w.Do = Do; w.Da = Da; w.net = net;
    w.sigma_job = (who.head == DC_HEAD_ONPOLICY && loss == BC_LOSS_NLL) ? 1 : 0;
    w.sigma_zero = (who.head == DC_HEAD_ONPOLICY && loss == BC_LOSS_MSE) ? 1 : 0;
    w.one_minus_b1 = (float)(1.0 - (double)c->cfg.beta1); w.beta2 = c->cfg.beta2; w.one_minus_b2 = (float)(1.0 - (double)c->cfg.beta2);
    w.eps = c->cfg.adam_eps;
    for (int l = 0; l < L; ++l) { a.actb[l] = lw.act[0][l]; a.dzb[l] = lw.dz[0][l]; w.actb[l] = lw.act[0][l]; w.dzb[l] = lw.dz[0][l]; }
    const int grid_w = bc_lay_wg_table(w);
    // the operand rows' home: every width the tile reads as an A operand (obs, the hidden layers, the head) in one LDS stride, or HBM
    const int ld = round_up(std::max(std::max(lw.hmax, Do), net.l[L].out), 4);
    const bool devws = !dc_wl_in_lds(ld);
    a.ldp = dc_wl_stride(devws ? round_up(Do, 4) : ld);
    const size_t lds = (size_t)(devws ? 1 : 2) * 16 * a.ldp * 4;
    c->theta_version += 1;
    for (int u = 0; u < n_updates; ++u) {
        a.idx = w.idx = k->d_idx + (size_t)u * B;
        w.loss_out = k->d_loss + u;
        const AdamStep as = bc_advance(c, m);
        w.step_size = as.step_size; w.bc2_sqrt = as.bc2_sqrt;
        rc = bc_lay_launch(c->device, who.head, devws, tiles, lds, st, a);
        if (rc) return rc;
        hipLaunchKernelGGL(bc_lay_wgrad_kernel, dim3(grid_w), dim3(256), 0, st, w);
        HIPCHK(hipGetLastError());
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
