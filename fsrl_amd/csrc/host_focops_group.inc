// host_focops_group.inc -- grouped FOCOPS updates: fsrl_group_create / fsrl_group_ppo_update for a group of FOCOPS contexts
// (part of fsrl_hip.hip, kernels: kernels_focops_group.hpp).  k x Engine.focops_update in lock step inside the frame of a grouped
// on-policy update (ogroup_*, host_group.inc: begin, per pass the batch preparation, counters and KL verdicts, end, the error
// path); here: the FOCOPS checks, working sets, tables and launches, every launch carrying all members still active.  Each
// member keeps its own nu / nu_loss (fsrl_focops_set_nu), Adam counters, psq / sig_stash parity, store, statistics rows and KL
// early stop (the `delta` check, always watched: a member that stops sits the later passes out).
// Bit-identity with focops_pass: the step table holds exactly the arguments focops_pass builds for the member's minibatch
// (the same host helpers, host_focops.inc), each member keeps its own three- or four-launch plan, and the kernels run the
// single-context bodies.  The tile height of a launch is focops_pass's rule over the whole launch (focops_rows4: 4-row tiles
// only while every active member fits one round of workgroups), so a group of one is bit-identical to its solo run, and larger
// groups are wherever the tile height does not change (tests/test_gpu_group_focops.py).
// A group of LAYERED members (all of one shape) runs focops_pass's layered step instead: 2 L + 5 launches per minibatch step for
// all members -- the PPO group's forward / backward / weight-side launches over its job tables (host_layered_group.inc), the
// loss heads (lay_fb_head_group_kernel), prep with the finished gradient in G as the one partial, step.  No tile plan, no
// split-K: a member's update is its own Engine.focops_update bit for bit at every group size
// (tests/test_gpu_group_focops_layered.py).
// ====================================================================================== grouped FOCOPS

// what grouped FOCOPS needs of its members beyond fsrl_group_create's shape / PPO checks; run at create and at every
// update, since fsrl_focops_init / _set_plan can be called again in between
static int focops_group_check(fsrl_ctx* const* ctxs, int k) {
    const fsrl_ctx* c0 = ctxs[0];
    for (int i = 0; i < k; ++i) {
        const fsrl_ctx* c = ctxs[i];
        CHECK_ARG(c->foc, "member %d: fsrl_focops_init first (a grouped FOCOPS member needs its FOCOPS configuration)", i);
        CHECK_ARG((c->lay != nullptr) == (c0->lay != nullptr), "member %d: members must have one network shape (a FOCOPS group is all fused or all layered contexts)", i);
        CHECK_ARG(!c->lay || lay_same_shape(c->cfg, c0->cfg), "member %d: members must have one network shape", i);
        CHECK_ARG(!(c->wgrad_stream && c->cfg.hidden == 256),
                  "member %d: fsrl_tr_set_plan's streaming weight-gradient plan is not grouped", i);
        const fsrl_focops_config &a = c->foc->cfg, &b = c0->foc->cfg;
        CHECK_ARG(a.l2_reg == b.l2_reg && a.delta == b.delta && a.eta == b.eta && a.tem_lambda == b.tem_lambda &&
                  a.max_grad_norm == b.max_grad_norm,
                  "member %d: members must share l2_reg, delta, eta, tem_lambda and max_grad_norm (learning rates may differ)", i);
        CHECK_ARG(c->foc->no_fast == c0->foc->no_fast, "member %d: members must agree on fsrl_focops_set_plan", i);
    }
    return 0;
}

static int focops_group_update(GroupUpdate& u) {
    fsrl_group* g = u.g; fsrl_ctx* c0 = g->m[0];
    const int k = u.k; hipStream_t s = g->stream;
    int rc = focops_group_check(g->m.data(), k);
    if (rc) return rc;
    const int H = c0->cfg.hidden, nn = 3;
    const bool layered = c0->lay != nullptr;
    // ---- begin (FOCOPS: no multipliers, rescaling 1, as Engine.focops_update).  The layered step's launches read the PPO group's
    // tables too: per pass the step rows' active / mb_size / mb_start
    const double zero_lag[FSRL_MAX_CRITICS] = {};
    rc = ogroup_begin(u, zero_lag, 0, nullptr, true, layered);
    if (rc) return rc;
    char fast[FSRL_MAX_GROUP] = {};
    for (int i = 0; i < k; ++i) {
        fsrl_ctx* c = g->m[i];
        if (!u.active[i]) continue;
        rc = focops_alloc(c);                   // the members' working sets before the first grouped pass
        if (rc) return rc;
        fast[i] = !layered && !c->foc->no_fast && c->mbp_max <= 512;
    }
    rc = table_ensure(g->ftab, (size_t)k, (size_t)k);
    if (rc) return rc;
    if (layered) {
        // job tables of this update (the members' working sets are in place now) and the member table for the observation operands
        rc = lay_group_tables(g->lay, g->m.data(), k, u.active, s);
        if (rc) return rc;
        for (int i = 0; i < k; ++i) lay_group_agent(g->m[i], g->tab.h[i]);
        HIPCHK(hipMemcpyAsync(g->tab.d, g->tab.h, (size_t)k * sizeof(GroupAgent), hipMemcpyHostToDevice, s));
    }
    int nb_a, nb_c0, nb_c1;
    focops_blocks(c0, &nb_a, &nb_c0, &nb_c1);
    const int nb_all = nb_a + nb_c0 + nb_c1;
    // fb_wgrad_kernel's plan in wgrad_launch (PAIR2 = false): blocks of one split and network (fused members)
    const WgradBlocks wb = layered ? WgradBlocks{} : wgrad_blocks(c0->md.Do, H, false);
    const int passes = wb.passes, NB = wb.NB;
    std::vector<char> rows4;
    for (int pass = 0; pass < u.max_repeat; ++pass) {
        // ---- per member: permutation + batch preparation of this pass; split-K buffers for its largest minibatch
        rc = ogroup_pass_begin(u, pass, [&](int i, fsrl_ctx* c) {
            if (fast[i] || layered) return 0;
            int ns = 1;
            for (int sz : c->mb_size) ns = std::max(ns, wgrad_plan((sz + 15) / 16 * 16, NB * nn, c->n_cus).nsplit);
            return ensure_parts(c, c->n_dev, ns);
        });
        if (rc) return rc;
        if (u.n_act == 0) break;
        const size_t max_nmb = u.max_nmb;
        // ---- tile height per minibatch step: focops_pass's rule over the members active in the pass (the layered step has no
        // tile plan: 16-row tiles of the loss head, as the member's own pass)
        rows4.assign(max_nmb, 0);
        for (size_t mb = 0; mb < max_nmb && !layered; ++mb) {
            int tiles = 0;
            for (int i = 0; i < k; ++i)
                if (u.active[i] && mb < g->m[i]->mb_size.size()) tiles = std::max(tiles, (g->m[i]->mb_size[mb] + 15) / 16);
            rows4[mb] = focops_rows4(c0, tiles, u.n_act);
        }
        // ---- member table and step table of the pass: focops_pass's arguments, member by member
        memset(g->fsteps.h, 0, max_nmb * k * sizeof(FocGroupStep));
        if (layered) memset(g->steps.h, 0, max_nmb * k * sizeof(GroupStep));
        for (int i = 0; i < k; ++i) {
            fsrl_ctx* c = g->m[i];
            FocGroupMember& t = g->ftab.h[i];
            memset(&t, 0, sizeof(t));
            t.P = c->P;
            if (!u.active[i]) continue;
            FocState* f = c->foc;
            t.fast = fast[i];
            t.pass_prep = focops_step_args(c, f->pp);
            t.pass_prep.nparts = 0;
            const int nmb = (int)c->mb_start.size();
            for (size_t mb = 0; mb < max_nmb; ++mb) {
                if ((int)mb >= nmb) break;
                FocGroupStep& st = g->fsteps.h[mb * k + i];
                const int start = c->mb_start[mb], size = c->mb_size[mb];
                const int tiles = (size + 15) / 16, rows_pad = tiles * 16;
                st.active = 1;
                st.n_tiles = rows4[mb] ? 4 * tiles : tiles;
                st.rows_pad = rows_pad;
                st.fb = focops_tile_args(c, start, size);
                st.sa = focops_step_args(c, f->pp);
                if (layered) {
                    st.sa.parts = c->G; st.sa.nparts = 1;            // the weight-side launch leaves the whole gradient in G
                    GroupStep& gs = g->steps.h[mb * k + i];
                    gs.active = 1; gs.mb_start = start; gs.mb_size = size; gs.mb_index = (int)mb;
                } else if (t.fast) {
                    st.wp = focops_wgrad_ptrs(c, st.fb.obs, rows_pad);
                    st.sa.nparts = 0; st.sa.parts = nullptr;
                    st.sa.gsq_part = c->gsq_part; st.sa.n_gsq_part = wg_blocks_per_net(H); st.sa.gsq_net = f->gsq_net;
                } else {
                    FbWgradArgs& wa = st.wa;
                    wa = focops_split_args(c, st.fb.obs, size, rows_pad);
                    const WgradPlan pl = wgrad_plan(rows_pad, NB * nn, c->n_cus);
                    wa.out = c->wg_parts; wa.ks_per_split = pl.ks_per_split; wa.split_stride = c->n_dev;
                    wa.dbg_skip = c->probe_wgrad_skip; wa.aux_passes = passes;
                    wa.remap_total = NB * nn * pl.nsplit; wa.remap_ny = nn;
                    st.sa.parts = c->wg_parts; st.sa.nparts = pl.nsplit;
                }
                focops_step_fill(c, st.sa, c->n_steps + (int64_t)mb, (int)mb, nmb, size, st.n_tiles);
                f->pp ^= 1;
            }
        }
        HIPCHK(hipMemcpyAsync(g->ftab.d, g->ftab.h, (size_t)k * sizeof(FocGroupMember), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(g->fsteps.d, g->fsteps.h, max_nmb * k * sizeof(FocGroupStep), hipMemcpyHostToDevice, s));
        if (layered) HIPCHK(hipMemcpyAsync(g->steps.d, g->steps.h, max_nmb * k * sizeof(GroupStep), hipMemcpyHostToDevice, s));
        HIPCHK(hipEventRecord(g->steps_copied, s));
        g->steps_in_flight = true;
        // ---- the pass: one pass-start prep for the three-launch members, then per minibatch step 3 or 4 launches for all
        bool any_fast = false;
        for (int i = 0; i < k; ++i) any_fast = any_fast || (u.active[i] && fast[i]);
        if (any_fast)
            hipLaunchKernelGGL((focops_prep_group_kernel<1>), dim3(nb_all, k), dim3(256), 0, s, c0->md, g->ftab.d, g->fsteps.d);
        for (size_t mb = 0; mb < max_nmb; ++mb) {
            const FocGroupStep* hst = g->fsteps.h + mb * k;
            const FocGroupStep* st = g->fsteps.d + mb * k;
            int tiles = 0, remap = 0;
            bool f3 = false, f4 = false;
            for (int i = 0; i < k; ++i) {
                if (!hst[i].active) continue;
                tiles = std::max(tiles, hst[i].n_tiles);
                if (fast[i]) f3 = true;
                else { f4 = true; remap = std::max(remap, hst[i].wa.remap_total); }
            }
            if (tiles == 0) continue;                            // no active member has a minibatch at this index
            if (layered) {
                // 2 L + 5 launches for all members: focops_pass's layered step (lay_fwd, the loss heads, lay_bwd, prep with G as
                // the one partial, step)
                const LayGroupLaunch ll(g->lay, g->m.data(), k, s, g->tab.d, g->steps.d + mb * k, g->steps.h + mb * k);
                ll.forward();
                hipLaunchKernelGGL(lay_fb_head_group_kernel, dim3(ll.tiles, nn, k), dim3(256), 0, s, g->lay.heads.d, st);
                ll.backward();
                hipLaunchKernelGGL((focops_prep_group_kernel<0>), dim3(nb_all, k), dim3(256), 0, s, c0->md, g->ftab.d, st);
                hipLaunchKernelGGL(focops_step_group_kernel, dim3(nb_all + 1, k), dim3(256), 0, s, c0->md, st);
                HIPCHK(hipGetLastError());
                continue;
            }
            rc = dispatch_H(H, [&](auto hc) {
                constexpr int HH = decltype(hc)::value;
                if (rows4[mb]) hipLaunchKernelGGL((focops_tile_group_kernel<HH, 4>), dim3(tiles, nn, k), dim3(4 * HH), 0, s, c0->md, g->ftab.d, st);
                else hipLaunchKernelGGL((focops_tile_group_kernel<HH, 16>), dim3(tiles, nn, k), dim3(4 * HH), 0, s, c0->md, g->ftab.d, st);
                if (f3) hipLaunchKernelGGL((focops_wgrad_group_kernel<HH>), dim3(wg_grid(HH, nn), k), dim3(1024), 0, s, c0->md, g->ftab.d, st);
                if (f4) hipLaunchKernelGGL((focops_wgrad_split_group_kernel<HH>), dim3(round_up(remap, 8), k), dim3(1024), 0, s, c0->md,
                                           g->ftab.d, st);
                return 0;
            });
            if (rc) return rc;
            if (f4) hipLaunchKernelGGL((focops_prep_group_kernel<0>), dim3(nb_all, k), dim3(256), 0, s, c0->md, g->ftab.d, st);
            hipLaunchKernelGGL(focops_step_group_kernel, dim3(nb_all + 1, k), dim3(256), 0, s, c0->md, st);
            HIPCHK(hipGetLastError());
        }
        // ---- counters (the Adam steps are FocState's: focops_step_fill) and the KL early stop: focops_pass's verdict, always watched
        rc = ogroup_pass_end(u, pass, false, true);
        if (rc) return rc;
    }
    return 0;
}
