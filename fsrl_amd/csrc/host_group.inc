// host_group.inc -- grouped PPO-Lagrangian updates: k agents of one shape, one stream, every launch of the minibatch step
// carries all of them as grid.y (part of fsrl_hip.hip; SURVEY 8e "optional within-GPU batching of k seeds").
// The kernels inline the single-agent bodies; a member's update is bit-identical to fsrl_ppo_update on that member alone
// only when the launch shapes agree (a group of ONE with at most 512 rows per minibatch): the group picks its tile height
// from the number of active members and the largest member (ppo_tile_plan, host_ppo.inc: fsrl_ppo_pass's rule), and above 512
// rows it keeps the in-kernel reduction where the single path goes through the split-K kernels.  Otherwise: the golden tests'
// tolerances (tests/test_gpu_group.py).
// A group of FOCOPS contexts runs the same entry points through host_focops_group.inc (one algorithm per group).
// A group of LAYERED PPO-Lagrangian or FOCOPS contexts (any other `hidden_sizes`, all members of one shape) runs the layered
// minibatch step with every member in each of its 2 L + 5 launches (host_layered_group.inc); there a member's update IS its own
// fsrl_ppo_update / Engine.focops_update bit for bit, whatever the group.  All four run inside one frame (ogroup_*, below).
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
        const bool ppo = c->cfg.algo == FSRL_ALGO_PPO_LAG;
        CHECK_ARG(!ppo || a.n_critics == b.n_critics, "member %d: members must share n_critics (one set of networks per launch)", i);
        CHECK_ARG(a.obs_dim == b.obs_dim && a.act_dim == b.act_dim && a.n_critics == b.n_critics && (c->lay != nullptr) == (c0->lay != nullptr) &&
                  (c->lay ? lay_same_shape(a, b) : a.hidden == b.hidden),
                  "member %d: members must have one network shape", i);
        if (ppo) {
            // A PPO-Lagrangian group may be a SWEEP: every member's own eps_clip, dual_clip, vf_coef, max_grad_norm value, target_kl,
            // norm_adv, use_lagrangian, beta1 / beta2 / adam_eps, rew_norm and value_clip reach the kernels through its row of the
            // member table (GroupAgent::hp) and its own host preparation.  What stays shared is what the launches themselves depend on.
            CHECK_ARG(a.max_action == b.max_action, "member %d: members must share max_action (the shared collect kernel scales every member's actions by it)", i);
            CHECK_ARG(a.unbounded == b.unbounded, "member %d: members must share unbounded (the shared collect kernel has one action head)", i);
            CHECK_ARG((a.max_grad_norm > 0.0f) == (b.max_grad_norm > 0.0f),
                      "member %d: members must agree on whether max_grad_norm is on (the step has 2 launches without the clip, 3 with it)", i);
        } else {
            // A FOCOPS group keeps the equality of every field: its kernels take their scalars from the FOCOPS step rows, and
            // focops_group_check (below) asks for one l2_reg / delta / eta / tem_lambda / max_grad_norm per group.
            CHECK_ARG(a.eps_clip == b.eps_clip && a.dual_clip == b.dual_clip && a.vf_coef == b.vf_coef &&
                      a.max_grad_norm == b.max_grad_norm && a.target_kl == b.target_kl && a.norm_adv == b.norm_adv &&
                      a.use_lagrangian == b.use_lagrangian && a.beta1 == b.beta1 && a.beta2 == b.beta2 &&
                      a.adam_eps == b.adam_eps && a.max_action == b.max_action && a.unbounded == b.unbounded &&
                      a.rew_norm == b.rew_norm && a.value_clip == b.value_clip,
                      "members must share the PPO hyper-parameters (learning rates, seeds and data may differ)");
        }
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
    int rc_tab = table_ensure(g->tab, (size_t)k, (size_t)k);
    if (!rc_tab && hipEventCreateWithFlags(&g->steps_copied, hipEventDisableTiming) != hipSuccess) rc_tab = fail(FSRL_EHIP, "group allocation failed");
    if (rc_tab) {
        (void)fsrl_group_destroy(g);            // gives the members their own streams back
        return rc_tab;
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
    lay_group_free(g->lay, g->ga.mem);          // job tables and collect buffers of a layered group: they name this member's memory
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
    table_free(g->ftab); table_free(g->fsteps);
    lay_group_free(g->lay, g->ga.mem);
    g->ga.mem.release_all();
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

// ---- the frame of one grouped on-policy update, the same for the PPO-Lagrangian update below and the FOCOPS update
//      (host_focops_group.inc), fused and layered: fsrl_group_ppo_update_each (fsrl_group_ppo_update: the same call with its scalars
//      repeated) -> the update's own pre-checks, ogroup_begin, per pass
//      ogroup_pass_begin / the update's tables, their copies and the steps_copied event behind them / its launches / ogroup_pass_end ->
//      every member's fsrl_ppo_end.  One error path, in fsrl_group_ppo_update_each: once a member has been through fsrl_ppo_begin, a
//      failure clears in_update on every member and does nothing else.
//      Member i has its own minibatch size (batch_sizes[i], its fsrl_ppo_begin's) and its own number of passes (repeats[i]): it
//      leaves the update after its last pass the way a member that stopped on KL does, without a stopped pass.
struct GroupUpdate {
    fsrl_group* g = nullptr; int k = 0;
    const int32_t* batch_sizes = nullptr; const int32_t* repeats = nullptr;     // [k]
    const int64_t* const* perms = nullptr; uint64_t seed = 0;      // ppo_pass_prepare's, per member and pass
    int32_t* stopped_pass_out = nullptr;
    int max_repeat = 0;                         // passes of the update: the most any member asks for
    bool begun = false;                         // a member has been through fsrl_ppo_begin
    int64_t n[FSRL_MAX_GROUP] = {};             // rows of each member's batch
    char active[FSRL_MAX_GROUP] = {};           // still stepping: has rows and has not stopped on KL
    int n_act = 0; size_t max_nmb = 0;          // of the current pass: the active members, the longest plan among them
};
// sample(0) + process_fn of every member, back to back on the shared stream; member i's multipliers are lagrangians + i * lag_stride
// (NULL: none) and rescaling[i] (NULL: 1).  Then the step tables the update names (fsteps: the FOCOPS rows, steps: the GroupStep
// rows): [minibatch steps of the longest plan][k] rows, grown to twice what this call needs, behind the stream's reads of the old tables.
static int ogroup_begin(GroupUpdate& u, const double* lagrangians, size_t lag_stride, const double* rescaling, bool fsteps, bool steps) {
    fsrl_group* g = u.g;
    group_actor_release(g);                     // the update goes behind the collect kernel, which ends
    for (fsrl_ctx* m : g->m) m->theta_version += 1;
    HIPCHK(hipSetDevice(g->m[0]->device));
    u.begun = true;
    size_t cap_nmb = 1;
    for (int i = 0; i < u.k; ++i) {
        int rc = fsrl_ppo_begin(g->m[i], lagrangians ? lagrangians + i * lag_stride : nullptr, rescaling ? rescaling[i] : 1.0, u.batch_sizes[i], &u.n[i]);
        if (rc) return rc;
        if (u.stopped_pass_out) u.stopped_pass_out[i] = -1;
        // an empty member sits the update out (it keeps a stale plan from an earlier update), and so does one that asks for no pass
        u.active[i] = u.n[i] != 0 && u.repeats[i] > 0;
        if (u.active[i]) cap_nmb = std::max(cap_nmb, g->m[i]->mb_start.size());
    }
    const size_t rows = cap_nmb * u.k;
    int rc = fsteps ? table_ensure(g->fsteps, rows, 2 * rows, g->stream) : 0;
    if (!rc && steps) rc = table_ensure(g->steps, rows, 2 * rows, g->stream);
    return rc;
}
// Start of a pass.  u.n_act == 0 afterwards: every member is empty or has stopped, the update is over.  Otherwise the pass has the steps
// of the longest plan among the members still active (one that stopped on KL or has run its own passes no longer counts), the previous pass's pinned tables have
// left host memory, and every active member's permutation + batch preparation is enqueued, each followed by the update's prepared(i, c).
template <class Prepared>
static int ogroup_pass_begin(GroupUpdate& u, int pass, Prepared&& prepared) {
    u.n_act = 0; u.max_nmb = 0;
    for (int i = 0; i < u.k; ++i) {
        if (pass >= u.repeats[i]) u.active[i] = 0;               // the member's own pass count
        if (u.active[i]) { u.n_act += 1; u.max_nmb = std::max(u.max_nmb, u.g->m[i]->mb_start.size()); }
    }
    if (u.n_act == 0) return 0;
    if (u.g->steps_in_flight) { HIPCHK(hipEventSynchronize(u.g->steps_copied)); u.g->steps_in_flight = false; }
    for (int i = 0; i < u.k; ++i) {
        if (!u.active[i]) continue;
        int rc = ppo_pass_prepare(u.g->m[i], u.perms ? u.perms[i] + (size_t)pass * (size_t)u.n[i] : nullptr, u.seed ? u.seed + 1000003ull * i + pass : 0);
        if (!rc) rc = prepared(i, u.g->m[i]);
        if (rc) return rc;
    }
    return 0;
}
// After the launches of a pass: the active members' counters (ppo_adam_t: the context's Adam step count too; FOCOPS keeps its own in
// FocState) and, if watch_kl, the pass-level KL early stop per member (the reference's `break`): one readback per pass for the group.
static int ogroup_pass_end(GroupUpdate& u, int pass, bool ppo_adam_t, bool watch_kl) {
    for (int i = 0; i < u.k; ++i) {
        if (!u.active[i]) continue;
        fsrl_ctx* c = u.g->m[i];
        const int64_t nmb = (int64_t)c->mb_start.size();
        c->n_steps += nmb; c->pass_index += 1;
        if (ppo_adam_t) c->adam_t += nmb;
        if (watch_kl) HIPCHK(hipMemcpyAsync(c->h_ctrl, c->ctrl, sizeof(CtrlBlock), hipMemcpyDeviceToHost, u.g->stream));
    }
    if (!watch_kl) return 0;
    HIPCHK(hipStreamSynchronize(u.g->stream));
    for (int i = 0; i < u.k; ++i) {
        if (!u.active[i] || u.g->m[i]->h_ctrl->stopped_after == INT_MAX) continue;
        u.active[i] = 0;
        if (u.stopped_pass_out) u.stopped_pass_out[i] = pass;
    }
    return 0;
}

// k x BasePolicy.update (base_policy.py:332-355) in lock step: the member table, the step table of a pass and the launches of a
// minibatch step -- 3 (2 without a clip) for all fused members, 2 L + 5 for all layered ones (host_layered_group.inc)
static int ppo_group_update(GroupUpdate& u, const double* lagrangians, const double* rescaling) {
    CHECK_ARG(rescaling, "null argument");
    fsrl_group* g = u.g; fsrl_ctx* c0 = g->m[0];
    const int k = u.k; hipStream_t s = g->stream;
    const int C = c0->cfg.n_critics, H = c0->cfg.hidden, nn = c0->md.n_nets;
    const bool layered = c0->lay != nullptr;
    int rc = ogroup_begin(u, lagrangians, (size_t)(C - 1), rescaling, false, true);
    if (rc) return rc;
    // ---- member table (wp.stats: per pass, the statistics table may be regrown)
    const int nparts = layered ? 0 : wg_grid(H, nn);
    for (int i = 0; i < k; ++i) {
        fsrl_ctx* c = g->m[i];
        GroupAgent& a = g->tab.h[i];
        if (layered) { lay_group_agent(c, a); continue; }
        group_agent_common(c, a);
        a.bp = ppo_batch_ptrs(c); a.bp.ts = nullptr;
        a.wp = ppo_wgrad_ptrs(c);
        a.gsq_part = c->gsq_part; a.nparts = nparts;
    }
    // group-wide arguments only; a member's hyper-parameters are in its table row (group_agent_common: GroupAgent::hp)
    PpoStepArgs base = group_base_args(c0);
    bool watch_kl = false;                      // the pass-level KL readback: on when ANY member has a target
    for (int i = 0; i < k; ++i) watch_kl = watch_kl || g->m[i]->cfg.target_kl > 0.0f;
    if (layered) {                              // job tables of this update: the members' working sets are in place now
        rc = lay_group_tables(g->lay, g->m.data(), k, u.active, s);
        if (rc) return rc;
        base.fuse_adam = 0;                     // the layered step keeps the separate Adam launch (lay_ppo_steps)
    }
    for (int pass = 0; pass < u.max_repeat; ++pass) {
        rc = ogroup_pass_begin(u, pass, [&](int i, fsrl_ctx* c) { g->tab.h[i].wp.stats = c->d_stats; return 0; });
        if (rc) return rc;
        if (u.n_act == 0) break;
        const size_t max_nmb = u.max_nmb;
        HIPCHK(hipMemcpyAsync(g->tab.d, g->tab.h, (size_t)k * sizeof(GroupAgent), hipMemcpyHostToDevice, s));
        // ---- step table of the pass
        for (size_t mb = 0; mb < max_nmb; ++mb) {
            for (int i = 0; i < k; ++i) {
                fsrl_ctx* c = g->m[i];
                GroupStep& st = g->steps.h[mb * k + i];
                memset(&st, 0, sizeof(st));
                const size_t nmb = c->mb_start.size();
                if (!u.active[i] || mb >= nmb) continue;
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
        HIPCHK(hipEventRecord(g->steps_copied, s));              // ogroup_pass_begin waits for it before the tables are rewritten
        g->steps_in_flight = true;
        // ---- the minibatch steps
        for (size_t mb = 0; mb < max_nmb; ++mb) {
            const GroupStep* st = g->steps.d + mb * k;
            int mbs = 0;                                         // the largest minibatch any member has at this step
            for (int i = 0; i < k; ++i) mbs = std::max(mbs, g->steps.h[mb * k + i].active ? g->steps.h[mb * k + i].mb_size : 0);
            if (mbs == 0) continue;                              // no active member has a minibatch at this index: nothing to launch
            if (layered) {
                rc = lay_group_step(g->lay, g->m.data(), k, s, g->tab.d, st, g->steps.h + mb * k, base);
                if (rc) return rc;
                continue;
            }
            const int tiles = (mbs + 15) / 16;
            // fsrl_ppo_pass's rule over the whole launch: a lone member gets its solo tiles
            const PpoTilePlan tp = ppo_tile_plan(c0, tiles, nn, u.n_act, g->tall_tiles);
            const int n32 = tp.n32, per_net = tiles - n32;
            const bool big = tiles * 16 > 256;                  // up to 256 rows: bursts of 4 k-steps, two workgroups per CU; above: the chunked 512-row form
            rc = dispatch_H(H, [&](auto hc) {
                constexpr int HH = decltype(hc)::value;
                if (tp.rows4) hipLaunchKernelGGL((ppo_fwd_bwd_group_kernel<HH, 4>), dim3(tiles * 4 * nn, k), dim3(4 * HH), 0, s, c0->md, g->tab.d, st, base);
                else if (tp.rows8) hipLaunchKernelGGL((ppo_fwd_bwd_group_kernel<HH, 8>), dim3(tiles * 2 * nn, k), dim3(4 * HH), 0, s, c0->md, g->tab.d, st, base);
                else if (n32 > 0) {
                    if constexpr (HH >= 128)
                        hipLaunchKernelGGL((ppo_fwd_bwd_group_mix_kernel<HH>), dim3(per_net * nn, k), dim3(4 * HH), 0, s, c0->md, g->tab.d, st, base,
                                           n32, per_net);
                } else hipLaunchKernelGGL((ppo_fwd_bwd_group_kernel<HH, 16>), dim3(tiles * nn, k), dim3(4 * HH), 0, s, c0->md, g->tab.d, st, base);
#define FSRL_WG(BIGV, FUSEV)                                                                                                      \
    do {                                                                                                                          \
        if (tp.rows4) hipLaunchKernelGGL((ppo_wgrad_group_kernel<HH, BIGV, FUSEV, 4>), dim3(nparts, k), dim3(1024), 0, s, c0->md, g->tab.d, st, base); \
        else if (tp.rows8) hipLaunchKernelGGL((ppo_wgrad_group_kernel<HH, BIGV, FUSEV, 8>), dim3(nparts, k), dim3(1024), 0, s, c0->md, g->tab.d, st, base); \
        else hipLaunchKernelGGL((ppo_wgrad_group_kernel<HH, BIGV, FUSEV, 16>), dim3(nparts, k), dim3(1024), 0, s, c0->md, g->tab.d, st, base);      \
    } while (0)
                if (base.fuse_adam) { if (big) FSRL_WG(true, true); else FSRL_WG(false, true); }
                else { if (big) FSRL_WG(true, false); else FSRL_WG(false, false); }
#undef FSRL_WG
                return 0;
            });
            if (rc) return rc;
            if (!base.fuse_adam)
                hipLaunchKernelGGL(adam_clip_group_kernel, dim3((c0->n_dev + 4 * ADAM_NT - 1) / (4 * ADAM_NT), k), dim3(ADAM_NT), 0, s,
                                   c0->md, g->tab.d, st, base);
            HIPCHK(hipGetLastError());
        }
        rc = ogroup_pass_end(u, pass, true, watch_kl);
        if (rc) return rc;
    }
    return 0;
}

// lagrangians: [k][n_critics - 1]; rescaling: [k]; batch_sizes, repeats: [k], member i's minibatch size and number of passes (0: the
// member sits the update out); perms: NULL (library shuffles) or k pointers, member i's = [repeats[i]][n_i]; stats_out: k pointers
// or NULL, member i's holds cap_steps[i] rows.  A FOCOPS group: k x Engine.focops_update (lagrangians / rescaling ignored).
extern "C" int fsrl_group_ppo_update_each(fsrl_group* g, const double* lagrangians, const double* rescaling, const int32_t* batch_sizes,
                                          const int32_t* repeats, const int64_t* const* perms, uint64_t seed, float* const* stats_out,
                                          const int64_t* cap_steps, int64_t* n_steps_out, int32_t* stopped_pass_out) {
    CHECK_ARG(g && batch_sizes && repeats, "null argument");
    CHECK_ARG(!stats_out || cap_steps, "null argument");
    if (g->broken) return fail(FSRL_ESTATE, "a member of this group has been destroyed");
    GroupUpdate u;
    u.g = g; u.k = (int)g->m.size(); u.batch_sizes = batch_sizes; u.repeats = repeats;
    u.perms = perms; u.seed = seed; u.stopped_pass_out = stopped_pass_out;
    for (int i = 0; i < u.k; ++i) {
        CHECK_ARG(repeats[i] >= 0, "member %d: repeat must be >= 0", i);
        u.max_repeat = std::max(u.max_repeat, (int)repeats[i]);
    }
    int rc = g->m[0]->cfg.algo == FSRL_ALGO_FOCOPS ? focops_group_update(u) : ppo_group_update(u, lagrangians, rescaling);
    for (int i = 0; i < u.k && !rc; ++i)        // end: statistics of every member
        rc = fsrl_ppo_end(g->m[i], stats_out ? stats_out[i] : nullptr, stats_out ? cap_steps[i] : 0, n_steps_out ? n_steps_out + i : nullptr);
    if (rc && u.begun) for (fsrl_ctx* c : g->m) c->in_update = false;
    return rc;
}

// the same with one batch_size, one repeat and one row capacity for every member
extern "C" int fsrl_group_ppo_update(fsrl_group* g, const double* lagrangians, const double* rescaling, int32_t batch_size,
                                     int32_t repeat, const int64_t* const* perms, uint64_t seed, float* const* stats_out,
                                     int64_t cap_steps, int64_t* n_steps_out, int32_t* stopped_pass_out) {
    CHECK_ARG(g, "null argument");
    CHECK_ARG(repeat >= 0, "repeat must be >= 0");
    int32_t bs[FSRL_MAX_GROUP], rp[FSRL_MAX_GROUP]; int64_t cap[FSRL_MAX_GROUP];
    for (int i = 0; i < FSRL_MAX_GROUP; ++i) { bs[i] = batch_size; rp[i] = repeat; cap[i] = cap_steps; }
    return fsrl_group_ppo_update_each(g, lagrangians, rescaling, bs, rp, perms, seed, stats_out, cap, n_steps_out, stopped_pass_out);
}
