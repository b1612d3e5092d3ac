// host_group.inc -- grouped PPO-Lagrangian updates: k agents of one shape, one stream, every launch of the minibatch step
// carries all of them as grid.y (part of fsrl_hip.hip; SURVEY 8e "optional within-GPU batching of k seeds").
// The kernels inline the single-agent bodies; a member's update is bit-identical to fsrl_ppo_update on that member alone
// only when the launch shapes agree (a group of ONE with at most 512 rows per minibatch): the group picks its tile height
// from the number of active members and the largest member, and above 512 rows it keeps the in-kernel reduction where the
// single path goes through the split-K kernels.  Otherwise: the golden tests' tolerances (tests/test_gpu_group.py).
// A group of FOCOPS contexts runs the same entry points through host_focops_group.inc (one algorithm per group).
// A group of LAYERED PPO-Lagrangian or FOCOPS contexts (any other `hidden_sizes`, all members of one shape) runs the layered
// minibatch step with every member in each of its 2 L + 5 launches (host_layered_group.inc); there a member's update IS its own
// fsrl_ppo_update / Engine.focops_update bit for bit, whatever the group.
// ====================================================================================== groups
#define FSRL_MAX_GROUP 16

struct fsrl_group {
    std::vector<fsrl_ctx*> m;                   // members (not owned)
    std::vector<hipStream_t> own_stream;        // each member's own compute stream, restored at destroy
    hipStream_t stream = nullptr;               // the shared stream: the group's own (a member's death must not take it along)
    DevTable<GroupAgent> tab;                   // [k]
    DevTable<GroupStep> steps;                  // [minibatch steps of a pass][k]
    hipEvent_t steps_copied = nullptr; bool steps_in_flight = false;
    bool broken = false;                        // a member was destroyed: no more updates
    int tall_tiles = -1;                        // fsrl_group_set_plan: 32-row tiles per (member, network) of the forward / backward launch
    // FOCOPS groups (host_focops_group.inc): member table and [minibatch steps of a pass][k] step table
    DevTable<FocGroupMember> ftab;
    DevTable<FocGroupStep> fsteps;
    // lock-step collection (host_group_collect.inc): ONE resident actor kernel for every member, rung through ONE doorbell
    GaRing ga;                                  // ring, protocol state and counters (host_actor_ring.inc); its stream is `stream`
    LayGroup lay;                               // a group of layered contexts (host_layered_group.inc): job tables, the shared actor request
};

extern "C" int fsrl_group_create(fsrl_ctx** ctxs, int32_t k, fsrl_group** out) {
    CHECK_ARG(ctxs && out, "null argument");
    CHECK_ARG(k >= 1 && k <= FSRL_MAX_GROUP, "a group has 1..%d members", FSRL_MAX_GROUP);
    const fsrl_ctx* c0 = ctxs[0];
    CHECK_ARG(c0, "null member");
    for (int i = 0; i < k; ++i) {
        const fsrl_ctx* c = ctxs[i];
        CHECK_ARG(c, "null member");
        CHECK_ARG(c->cfg.algo == FSRL_ALGO_PPO_LAG || c->cfg.algo == FSRL_ALGO_FOCOPS,
                  "member %d: grouped updates are PPO-Lagrangian or FOCOPS contexts", i);
        CHECK_ARG(c->cfg.algo == c0->cfg.algo, "member %d: a group has one algorithm (all PPO-Lagrangian or all FOCOPS members)", i);
        // layered members: all members layered and of one shape (checked below); a FOCOPS group names the mix of kinds
        CHECK_ARG(c->cfg.algo != FSRL_ALGO_FOCOPS || (c->lay != nullptr) == (c0->lay != nullptr),
                  "member %d: members must have one network shape (a FOCOPS group is all fused or all layered contexts)", i);
        CHECK_ARG(c->device == c0->device, "members live on one device");
        CHECK_ARG(!c->in_update && !c->group, "member %d is inside an update or already grouped", i);
        const fsrl_config &a = c->cfg, &b = c0->cfg;
        CHECK_ARG(a.obs_dim == b.obs_dim && a.act_dim == b.act_dim && a.n_critics == b.n_critics && (c->lay != nullptr) == (c0->lay != nullptr) &&
                  (c->lay ? lay_same_shape(a, b) : a.hidden == b.hidden),
                  "members must have one network shape");
        CHECK_ARG(a.eps_clip == b.eps_clip && a.dual_clip == b.dual_clip && a.vf_coef == b.vf_coef &&
                  a.max_grad_norm == b.max_grad_norm && a.target_kl == b.target_kl && a.norm_adv == b.norm_adv &&
                  a.use_lagrangian == b.use_lagrangian && a.beta1 == b.beta1 && a.beta2 == b.beta2 &&
                  a.adam_eps == b.adam_eps && a.max_action == b.max_action && a.unbounded == b.unbounded &&
                  a.rew_norm == b.rew_norm && a.value_clip == b.value_clip,
                  "members must share the PPO hyper-parameters (learning rates, seeds and data may differ)");
        for (int j = 0; j < i; ++j) CHECK_ARG(ctxs[j] != c, "member listed twice");
    }
    if (c0->cfg.algo == FSRL_ALGO_FOCOPS) {
        int rc = focops_group_check(ctxs, k);
        if (rc) return rc;
    }
    HIPCHK(hipSetDevice(c0->device));
    for (int i = 0; i < k; ++i) pactor_release(ctxs[i]);      // members share the group's stream from here on: no resident actors (pactor_ok)
    fsrl_group* g = new fsrl_group();
    {
        hipError_t es = hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking);
        if (es != hipSuccess) { delete g; return fail(FSRL_EHIP, "group stream: %s", hipGetErrorString(es)); }
    }
    for (int i = 0; i < k; ++i) {
        fsrl_ctx* c = ctxs[i];
        (void)hipStreamSynchronize(c->compute);
        g->m.push_back(c);
        g->own_stream.push_back(c->compute);
        c->compute = g->stream;                 // everything a member enqueues from now on goes to the shared stream
        c->group = g;
    }
    hipError_t e = hipMalloc(&g->tab.d, (size_t)k * sizeof(GroupAgent));
    if (e == hipSuccess) e = hipHostMalloc(&g->tab.h, (size_t)k * sizeof(GroupAgent));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&g->steps_copied, hipEventDisableTiming);
    if (e != hipSuccess) {
        fail(FSRL_EHIP, "group allocation failed: %s", hipGetErrorString(e));
        (void)fsrl_group_destroy(g);            // gives the members their own streams back
        return FSRL_EHIP;
    }
    *out = g;
    return 0;
}

// A member is being destroyed: the group is over (it can only be destroyed from here on).  EVERY member goes back to its
// own compute stream now, so that the survivors' own calls keep working whatever order the host tears things down in
// (Python's GC does not promise EngineGroup before Engine).
static void group_detach(fsrl_ctx* c) {
    fsrl_group* g = c->group;
    if (!g) return;
    group_actor_release(g);
    (void)hipStreamSynchronize(g->stream);
    lay_group_free(g->lay);                     // job tables and collect buffers of a layered group: they name this member's memory
    for (size_t i = 0; i < g->m.size(); ++i) {
        fsrl_ctx* m = g->m[i];
        if (!m) continue;
        m->compute = g->own_stream[i];
        m->group = nullptr;
        g->m[i] = nullptr;
    }
    g->broken = true;
}

extern "C" int fsrl_group_destroy(fsrl_group* g) {
    if (!g) return 0;
    for (fsrl_ctx* c : g->m) if (c) { (void)hipSetDevice(c->device); break; }
    group_actor_release(g);
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    for (size_t i = 0; i < g->m.size(); ++i)
        if (g->m[i]) { g->m[i]->compute = g->own_stream[i]; g->m[i]->group = nullptr; }
    if (g->stream) (void)hipStreamDestroy(g->stream);
    table_free(g->tab); table_free(g->steps);
    if (g->steps_copied) (void)hipEventDestroy(g->steps_copied);
    if (g->ga.h) (void)hipHostFree(g->ga.h);
    table_free(g->ftab); table_free(g->fsteps);
    lay_group_free(g->lay);
    delete g;
    return 0;
}

// (a group of layered contexts accepts the call and ignores it: the layered step has no tile plan)
// A/B and test switch: how many of a (member, network)'s leading tiles are 32 rows tall in the forward / backward launch of the minibatch
// step.  -1: automatic (just enough for one round of workgroups once the 16-row tiles exceed the CU count), 0: none (the plan up to r6
// early), n > 0: min(n, tiles / 2).  Every plan gives the same bits.
extern "C" int fsrl_group_set_plan(fsrl_group* g, int32_t tall_tiles) {
    CHECK_ARG(g, "null group");
    CHECK_ARG(tall_tiles >= -1 && tall_tiles <= 1024, "tall_tiles: -1 (automatic), 0 (none) or a count");
    g->tall_tiles = tall_tiles;
    return 0;
}

// k x BasePolicy.update (base_policy.py:332-355) in lock step.  lagrangians: [k][n_critics - 1]; rescaling: [k];
// perms: NULL (library shuffles) or k pointers, member i's = [repeat][n_i]; stats_out: k pointers or NULL.
// A FOCOPS group: k x Engine.focops_update (lagrangians / rescaling ignored, host_focops_group.inc).
extern "C" int fsrl_group_ppo_update(fsrl_group* g, const double* lagrangians, const double* rescaling, int32_t batch_size,
                                     int32_t repeat, const int64_t* const* perms, uint64_t seed, float* const* stats_out,
                                     int64_t cap_steps, int64_t* n_steps_out, int32_t* stopped_pass_out) {
    CHECK_ARG(g, "null argument");
    CHECK_ARG(repeat >= 0, "repeat must be >= 0");
    if (g->broken) return fail(FSRL_ESTATE, "a member of this group has been destroyed");
    if (g->m[0]->cfg.algo == FSRL_ALGO_FOCOPS)
        return focops_group_update(g, batch_size, repeat, perms, seed, stats_out, cap_steps, n_steps_out, stopped_pass_out);
    CHECK_ARG(rescaling, "null argument");
    group_actor_release(g);                     // the update goes behind the collect kernel, which ends
    const int k = (int)g->m.size();
    fsrl_ctx* c0 = g->m[0];
    for (fsrl_ctx* m : g->m) m->theta_version += 1;
    HIPCHK(hipSetDevice(c0->device));
    hipStream_t s = g->stream;
    const int C = c0->cfg.n_critics, H = c0->cfg.hidden, nn = c0->md.n_nets, Do = c0->cfg.obs_dim;
    const bool layered = c0->lay != nullptr;
    auto abort_all = [&](int rc) { for (fsrl_ctx* c : g->m) c->in_update = false; return rc; };
    // ---- begin: sample(0) + process_fn of every member, back to back on the shared stream
    std::vector<int64_t> n((size_t)k, 0);
    for (int i = 0; i < k; ++i) {
        int rc = fsrl_ppo_begin(g->m[i], lagrangians ? lagrangians + (size_t)i * (C - 1) : nullptr, rescaling[i], batch_size, &n[i]);
        if (rc) return abort_all(rc);
        if (stopped_pass_out) stopped_pass_out[i] = -1;
    }
    // ---- member table
    const int nparts = layered ? 0 : wg_grid(H, nn);
    for (int i = 0; i < k; ++i) {
        fsrl_ctx* c = g->m[i];
        GroupAgent& a = g->tab.h[i];
        if (layered) { lay_group_agent(c, a); continue; }
        memset(&a, 0, sizeof(a));
        a.P = c->P; a.Pw = c->P; a.M = c->M; a.V = c->V; a.G = c->G;
        a.bp.obs_p = c->obs_p; a.bp.rd_p = c->rd_p; a.bp.A1 = c->A1; a.bp.A2 = c->A2; a.bp.D1 = c->D1; a.bp.D2 = c->D2;
        a.bp.DO = c->DO; a.bp.statp = c->statp; a.bp.mbp_max = c->mbp_max; a.bp.ts = nullptr;
        WgradPtrs& wp = a.wp;
        wp.A1 = c->A1; wp.A2 = c->A2; wp.D1 = c->D1; wp.D2 = c->D2; wp.DO = c->DO; wp.X = c->obs_p; wp.grad = c->G;
        wp.gsq_part = c->gsq_part; wp.ctrl = c->ctrl; wp.mbp_max = c->mbp_max; wp.P = c->P; wp.statp = c->statp;
        wp.Pw = c->P; wp.M = c->M; wp.V = c->V;
        a.gsq_part = c->gsq_part; a.ctrl = c->ctrl;
        a.rescale = (float)c->rescaling;
        for (int j = 0; j < FSRL_MAX_CRITICS; ++j) a.lam[j] = (float)c->lagr[j];
        a.n_dev = c->n_dev; a.nparts = nparts;
    }
    PpoStepArgs base = ppo_base_args(c0);
    std::vector<char> active((size_t)k, 1);
    for (int i = 0; i < k; ++i) if (n[i] == 0) active[(size_t)i] = 0;
    // minibatch steps of a pass = the longest plan among the members still ACTIVE in it (an empty member keeps a stale plan
    // from an earlier update; a member that stopped on KL no longer counts): recomputed per pass
    size_t cap_nmb = 0;
    for (int i = 0; i < k; ++i) if (active[(size_t)i]) cap_nmb = std::max(cap_nmb, g->m[i]->mb_start.size());
    // grown to twice what this call needs, behind the stream's reads of the old tables
    const size_t n_steps = std::max<size_t>(cap_nmb, 1) * k;
    int rc = table_ensure(g->steps, n_steps, 2 * n_steps, g->stream);
    if (rc) return abort_all(rc);
    if (layered) {                              // job tables of this update: the members' working sets are in place now
        rc = lay_group_tables(g->lay, g->m.data(), k, active.data(), s);
        if (rc) return abort_all(rc);
        base.fuse_adam = 0;                     // the layered step keeps the separate Adam launch (lay_ppo_steps)
    }
    for (int pass = 0; pass < repeat; ++pass) {
        bool any = false;
        for (int i = 0; i < k; ++i) any = any || active[(size_t)i];
        if (!any) break;
        size_t max_nmb = 0;
        for (int i = 0; i < k; ++i) if (active[(size_t)i]) max_nmb = std::max(max_nmb, g->m[i]->mb_start.size());
        // the pinned tables of the previous pass must have left host memory before they are rewritten
        if (g->steps_in_flight) { HIPCHK(hipEventSynchronize(g->steps_copied)); g->steps_in_flight = false; }
        // ---- per member: permutation + batch preparation of this pass; stats pointer (the table may have been regrown)
        int max_mbsize = 0;
        for (int i = 0; i < k; ++i) {
            if (!active[(size_t)i]) continue;
            fsrl_ctx* c = g->m[i];
            rc = ppo_pass_prepare(c, perms ? perms[i] + (size_t)pass * (size_t)n[i] : nullptr, seed ? seed + 1000003ull * i + pass : 0);
            if (rc) return abort_all(rc);
            g->tab.h[i].wp.stats = c->d_stats;
            for (int sz : c->mb_size) max_mbsize = std::max(max_mbsize, sz);
        }
        HIPCHK(hipMemcpyAsync(g->tab.d, g->tab.h, (size_t)k * sizeof(GroupAgent), hipMemcpyHostToDevice, s));
        // ---- step table of the pass
        for (size_t mb = 0; mb < max_nmb; ++mb) {
            for (int i = 0; i < k; ++i) {
                fsrl_ctx* c = g->m[i];
                GroupStep& st = g->steps.h[mb * k + i];
                memset(&st, 0, sizeof(st));
                const size_t nmb = c->mb_start.size();
                if (!active[(size_t)i] || mb >= nmb) continue;
                st.active = 1;
                st.mb_start = c->mb_start[mb]; st.mb_size = c->mb_size[mb]; st.mb_index = (int)mb;
                st.step = (int)c->n_steps + (int)mb;
                st.first_in_pass = (mb == 0); st.last_in_pass = (mb == nmb - 1); st.iters_in_pass = (int)nmb;
                st.pass = c->pass_index;
                const AdamStep as = adam_step(c->cfg.lr, c->cfg.beta1, c->cfg.beta2, c->adam_t + (int64_t)mb + 1);
                st.step_size = as.step_size; st.bc2_sqrt = as.bc2_sqrt;
            }
        }
        HIPCHK(hipMemcpyAsync(g->steps.d, g->steps.h, max_nmb * k * sizeof(GroupStep), hipMemcpyHostToDevice, s));
        HIPCHK(hipEventRecord(g->steps_copied, s));
        g->steps_in_flight = true;
        // ---- the minibatch steps: 3 (2 without a clip) launches for all members
        int n_act = 0;
        for (int i = 0; i < k; ++i) n_act += active[(size_t)i] ? 1 : 0;
        (void)max_mbsize;
        for (size_t mb = 0; mb < max_nmb; ++mb) {
            const GroupStep* st = g->steps.d + mb * k;
            int mbs = 0;                                         // the largest minibatch any member has at this step
            for (int i = 0; i < k; ++i) mbs = std::max(mbs, g->steps.h[mb * k + i].active ? g->steps.h[mb * k + i].mb_size : 0);
            if (mbs == 0) continue;                              // no active member has a minibatch at this index: nothing to launch
            if (layered) {                                       // 2 L + 5 launches for all members (host_layered_group.inc)
                rc = lay_group_step(g->lay, g->m.data(), k, s, g->tab.d, st, g->steps.h + mb * k, base);
                if (rc) return abort_all(rc);
                continue;
            }
            const int tiles = (mbs + 15) / 16;
            // 4-row tiles only while the whole group still fits the chip in one round (a lone member: the single-agent rule)
            const bool rows4 = (size_t)tiles * 4 * nn * n_act <= (size_t)c0->n_cus && !c0->probe_tile16;
            const bool rows8 = !rows4 && (size_t)tiles * 2 * nn * n_act <= (size_t)c0->n_cus && !c0->probe_tile16;   // as in fsrl_ppo_pass
            // tall tiles (r6 late): once the 16-row tiles need a second round of workgroups, every (member, network) runs 32-row tiles (a
            // trailing odd 16-row group keeps a 16-row tile): 8 members x 3 networks x 256 rows = 192 workgroups instead of 384, half the
            // L2 -> register weight ingest per row.  Same-box alternations (tools/bench_group.py --tall): k = 8 245 -> 283 updates/s aggregate,
            // k = 6 207 -> 252, k = 12 260 -> 270, k = 16 309 -> 309; groups whose 16-row tiles fit one round LOSE with tall tiles (k = 4
            // 245 -> 200, k = 5 266 -> 232) and keep them.  A mix sized to exactly one round (6 of 32 + 4 of 16 rows per pair at k = 8) was
            // slower than either (228-240) and 7 + 2 differed by box (288 / 222): not used.  g->tall_tiles: -1 automatic, 0 none, n > 0
            // exactly min(n, tiles / 2) leading tiles.
            int n32 = 0;
            if (!rows4 && !rows8 && H >= 128 && c0->md.Do <= TileSmem<256, 32>::XK && !c0->probe_tile16) {
                if (g->tall_tiles < 0) n32 = tiles * nn * n_act > c0->n_cus ? tiles / 2 : 0;
                else n32 = std::min(tiles / 2, g->tall_tiles);
            }
            const int per_net = tiles - n32;
            const bool big = tiles * 16 > 256;                  // up to 256 rows: bursts of 4 k-steps, two workgroups per CU; above: the chunked 512-row form
            rc = dispatch_H(H, [&](auto hc) {
                constexpr int HH = decltype(hc)::value;
                if (rows4) hipLaunchKernelGGL((ppo_fwd_bwd_group_kernel<HH, 4>), dim3(tiles * 4 * nn, k), dim3(4 * HH), 0, s, c0->md, g->tab.d, st, base);
                else if (rows8) hipLaunchKernelGGL((ppo_fwd_bwd_group_kernel<HH, 8>), dim3(tiles * 2 * nn, k), dim3(4 * HH), 0, s, c0->md, g->tab.d, st, base);
                else if (n32 > 0) {
                    if constexpr (HH >= 128)
                        hipLaunchKernelGGL((ppo_fwd_bwd_group_mix_kernel<HH>), dim3(per_net * nn, k), dim3(4 * HH), 0, s, c0->md, g->tab.d, st, base,
                                           n32, per_net);
                } else hipLaunchKernelGGL((ppo_fwd_bwd_group_kernel<HH, 16>), dim3(tiles * nn, k), dim3(4 * HH), 0, s, c0->md, g->tab.d, st, base);
#define FSRL_WG(BIGV, FUSEV)                                                                                                      \
    do {                                                                                                                          \
        if (rows4) hipLaunchKernelGGL((ppo_wgrad_group_kernel<HH, BIGV, FUSEV, 4>), dim3(nparts, k), dim3(1024), 0, s, c0->md, g->tab.d, st, base); \
        else if (rows8) hipLaunchKernelGGL((ppo_wgrad_group_kernel<HH, BIGV, FUSEV, 8>), dim3(nparts, k), dim3(1024), 0, s, c0->md, g->tab.d, st, base); \
        else hipLaunchKernelGGL((ppo_wgrad_group_kernel<HH, BIGV, FUSEV, 16>), dim3(nparts, k), dim3(1024), 0, s, c0->md, g->tab.d, st, base);      \
    } while (0)
                if (base.fuse_adam) { if (big) FSRL_WG(true, true); else FSRL_WG(false, true); }
                else { if (big) FSRL_WG(true, false); else FSRL_WG(false, false); }
#undef FSRL_WG
                return 0;
            });
            if (rc) return abort_all(rc);
            if (!base.fuse_adam)
                hipLaunchKernelGGL(adam_clip_group_kernel, dim3((c0->n_dev + 4 * ADAM_NT - 1) / (4 * ADAM_NT), k), dim3(ADAM_NT), 0, s,
                                   c0->md, g->tab.d, st, base);
            HIPCHK(hipGetLastError());
        }
        for (int i = 0; i < k; ++i) {
            if (!active[(size_t)i]) continue;
            fsrl_ctx* c = g->m[i];
            const int64_t nmb = (int64_t)c->mb_start.size();
            c->n_steps += nmb; c->adam_t += nmb; c->pass_index += 1;
        }
        // ---- pass-level KL early stop, per member (the reference's `break`): one readback per pass for the group
        if (c0->cfg.target_kl > 0.0f) {
            for (int i = 0; i < k; ++i)
                if (active[(size_t)i])
                    HIPCHK(hipMemcpyAsync(g->m[i]->h_ctrl, g->m[i]->ctrl, sizeof(CtrlBlock), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            for (int i = 0; i < k; ++i) {
                if (active[(size_t)i] && g->m[i]->h_ctrl->stopped_after != INT_MAX) {
                    active[(size_t)i] = 0;
                    if (stopped_pass_out) stopped_pass_out[i] = pass;
                }
            }
        }
    }
    // ---- end: statistics of every member
    for (int i = 0; i < k; ++i) {
        rc = fsrl_ppo_end(g->m[i], stats_out ? stats_out[i] : nullptr, cap_steps, n_steps_out ? n_steps_out + i : nullptr);
        if (rc) return abort_all(rc);
    }
    return 0;
}
