// host_sac_group.inc -- grouped SAC-Lagrangian and DDPG-Lagrangian updates: fsrl_sac_group_* (part of fsrl_hip.hip, kernels:
// kernels_sac_group.hpp).
// k SAC-Lag contexts -- or k DDPG-Lag contexts (fsrl_sac_init with deterministic = 1); the group's kind is member 0's and the two
// do not mix -- of one network shape, each stepped n_i times per call in lock step: every launch of an update carries all
// members that still have updates to run (nine launches per update, whatever k is).  Members keep their own streams, stores,
// parameters, targets, Adam state, alpha, Philox key and statistics ring; the group has a stream of its own that waits on each
// member's stream before the call and that each member's streams wait on after it.  Between grouped calls a member is an ordinary
// context (its resident actor included: a grouped call ends it, the member's next collect launches it again).
// Bit-identity with fsrl_sac_update: the member's arithmetic is the single path's body with the single path's split-K plan; the
// tile height of a launch is the single-context rule applied to the whole group's launch (4-row tiles while the group still fits
// one round of workgroups), so a group of one is bit-identical to its solo run, and larger groups are wherever the tile height
// does not change a row's result (tests/test_gpu_sac_group.py, tests/test_gpu_ddpg_group.py).
// A DDPG-Lag group is the same nine launches with the DDPG context's arguments: n_q = 2 single critics (the Q grids, the small
// weight-gradient grid, the split-K plan and the tile-height rule all take the group's n_q), the deterministic actor, the target
// actor in the first half of the forward launch, and its Polyak update in the actor's Adam pass, where SAC-Lag steps alpha.
// A group of PRIORITISED members (fsrl_per_enable on every one of them before the group is made; alpha, beta and weight_norm are
// the member's own) runs fsrl_sac_update's prioritised sequence, thirteen launches whatever k is: per_sample_group (one workgroup
// per member: the descent of its sum tree, its weights) -> gather -> the actors' forward with the fold off -> target Q -> the n-step
// targets as a launch of their own -> Q_TRAIN with the member's weights -> per_update_group (one workgroup per member: its new
// priorities) -> the rest as above.  Ordering: the group's stream is behind each member's compute stream, which has joined its
// side stream and any per_ingest / per_fill on it; after the call both of the member's streams wait for `done`, and upd_done is
// recorded behind that wait, so the side stream's next tree write follows the call's priorities (kernels_per_group.hpp).
// ====================================================================================== grouped SAC-Lagrangian
// ---- what the grouped SAC and CVPO updates share: the members, the group's stream and the events that order it against the
//      members' streams (each group type embeds one as `core`), and further down the frame of one grouped call.
struct ReplayGroupCore {
    std::vector<fsrl_ctx*> m;                  // members (not owned; nullptr once destroyed)
    int device = 0;
    hipStream_t stream = nullptr;              // the group's own stream
    hipEvent_t done = nullptr;                 // end of the last grouped call on `stream`
    std::vector<hipEvent_t> ready;             // per member: its stream's work before the call
    bool broken = false;                       // a member was destroyed first: no more updates
};
// the stream and events of a group of k on `device` (made current by the caller)
static hipError_t rgroup_create(ReplayGroupCore& g, int device, int k) {
    g.device = device;
    g.ready.assign((size_t)k, nullptr);
    hipError_t e = hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&g.done, hipEventDisableTiming);
    for (int i = 0; i < k && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&g.ready[(size_t)i], hipEventDisableTiming);
    return e;
}
// waits for the group's stream; the caller frees its own tables afterwards
static void rgroup_destroy(ReplayGroupCore& g) {
    (void)hipSetDevice(g.device);
    if (g.stream) (void)hipStreamSynchronize(g.stream);
    for (hipEvent_t e : g.ready) if (e) (void)hipEventDestroy(e);
    if (g.done) (void)hipEventDestroy(g.done);
    if (g.stream) (void)hipStreamDestroy(g.stream);
}
// a member destroyed before its group (fsrl_ctx_destroy): the group stops updating, its destroy still works
static void rgroup_detach(ReplayGroupCore& g, fsrl_ctx* c) {
    if (g.stream) (void)hipStreamSynchronize(g.stream);
    for (auto& x : g.m) if (x == c) x = nullptr;
    g.broken = true;
}
// member c before a grouped call: its resident actor ends, its pushes land, its batch buffers and sub-buffer books are current
static int rgroup_join(fsrl_ctx* c, int B) {
    int rc = replay_join(c, sac_of(c), B);
    if (!rc && c->per) rc = per_alloc_batch(c, B);         // a prioritised member: its weights and TD averages
    return rc ? rc : sac_upload_book(c, sac_of(c));
}
// the group's stream goes behind member i's stream; recorded once the member's table entry is built
static int rgroup_ready(ReplayGroupCore& g, int i) {
    HIPCHK(hipEventRecord(g.ready[(size_t)i], g.m[i]->compute));
    HIPCHK(hipStreamWaitEvent(g.stream, g.ready[(size_t)i], 0));
    return 0;
}
// after the call (`done` recorded): member i's streams wait for it
static int rgroup_fanout(ReplayGroupCore& g, int i) {
    HIPCHK(hipStreamWaitEvent(g.m[i]->compute, g.done, 0));
    HIPCHK(hipStreamWaitEvent(g.m[i]->side, g.done, 0));     // a push must not overwrite rows the call still samples
    return 0;
}

// ---- the frame of one grouped call, the same for the fused, the layered (host_sac_group_layered.inc) and the CVPO
//      (host_cvpo_group.inc) update: rgroup_begin validates, rgroup_enter joins the members and fills the step table, the update
//      copies its tables and launches, rgroup_end fans out and books.  An update adds its own member checks, its member tables
//      and whatever its step rows hold beyond the common part.
struct ReplayGroupCall {
    const int32_t* n = nullptr;                // [k]: the updates each member runs
    int k = 0, n_max = 0;
    char work[FSRL_MAX_GROUP] = {};            // n[i] > 0
};
// All validation, before anything is enqueued or any member's state changes.  cvpo: the kind the group was made for (fsrl_sac_init
// / fsrl_cvpo_init re-create a member's state without telling its group).  member_ok(i, c, s): the update's own checks of a
// member that is still of the group's kind.  call.n_max == 0 afterwards: nothing to do.
// A CVPO context's cfg mirrors its ccfg in n_step and both learning rates (fsrl_cvpo_init and fsrl_set_lr keep the two equal), so
// the frame reads cfg for every kind.
template <class MemberOk>
static int rgroup_begin(const ReplayGroupCore& g, bool cvpo, const int32_t* n_updates, ReplayGroupCall& call, MemberOk&& member_ok) {
    call.n = n_updates; call.k = (int)g.m.size();
    const SacState* s0 = sac_of(g.m[0]);
    for (int i = 0; i < call.k; ++i) {
        fsrl_ctx* c = g.m[i];
        const SacState* s = sac_of(c);
        CHECK_ARG(n_updates[i] >= 0, "n_updates[%d] < 0", i);
        CHECK_ARG(s && s->cvpo == cvpo && s->ddpg == s0->ddpg && s->layered == s0->layered && s->cfg.n_step == s0->cfg.n_step,
                  "member %d is no longer a context of the group's kind and shape", i);
        const int rc = member_ok(i, c, s);
        if (rc) return rc;
        if (n_updates[i] > 0) CHECK_ARG(fsrl_store_len(c) > 0, "member %d: empty replay store", i);
        call.n_max = std::max(call.n_max, (int)n_updates[i]);
        call.work[i] = n_updates[i] > 0;
    }
    return 0;
}
// Every member with work joins (a join may regrow a member's working set and move its buffers); THEN build_tables() forms the
// update's member tables; then the group's stream goes behind each member's.  Last the step table, what each member's own
// updates would use: row(u, i, st, c, s) adds the update's own part to an active row, (u, i, st, nullptr, nullptr) to a row member
// i sits out.
template <class BuildTables, class Row>
static int rgroup_enter(ReplayGroupCore& g, DevTable<SacGroupStep>& steps, const ReplayGroupCall& call, int B, BuildTables&& build_tables,
                        Row&& row) {
    const int k = call.k;
    HIPCHK(hipSetDevice(g.device));
    HIPCHK(hipStreamSynchronize(g.stream));            // the pinned tables of the previous call have been read
    int rc = table_ensure(steps, (size_t)call.n_max * k, std::max<size_t>((size_t)call.n_max * k, 64));
    if (rc) return rc;
    for (int i = 0; i < k; ++i)
        if (call.work[i]) { rc = rgroup_join(g.m[i], B); if (rc) return rc; }
    rc = build_tables();
    if (rc) return rc;
    SacSampleArgs sa[FSRL_MAX_GROUP];                  // the member's sample; the counter is the step's
    for (int i = 0; i < k; ++i) {
        if (!call.work[i]) continue;
        rc = rgroup_ready(g, i);
        if (rc) return rc;
        const fsrl_ctx* c = g.m[i];
        const SacState* s = sac_of(g.m[i]);
        sa[i] = s->cvpo ? cvpo_sample_args(c, s, B, fsrl_store_len(g.m[i])) : sac_sample_args(c, s, B, s->cfg.n_step, fsrl_store_len(g.m[i]), 0);
    }
    for (int u = 0; u < call.n_max; ++u)
        for (int i = 0; i < k; ++i) {
            SacGroupStep& st = steps.h[(size_t)u * k + i];
            st = SacGroupStep{};
            if (u >= call.n[i]) { row(u, i, st, nullptr, nullptr); continue; }
            const fsrl_ctx* c = g.m[i];
            const SacState* s = sac_of(g.m[i]);
            const int64_t n = s->n_updates + u;
            st.sa = sa[i]; st.sa.counter = (unsigned long long)n; st.row = (int)(n % SAC_RING); st.active = 1;
            const AdamStep cs = adam_step(s->cfg.critic_lr, c->cfg.beta1, c->cfg.beta2, s->t_critic + u + 1);
            st.c_step = cs.step_size; st.c_bc2 = cs.bc2_sqrt;
            row(u, i, st, c, s);
        }
    return 0;
}
// After the launches: `done`, each member's streams wait for the call, and its bookkeeping is that of n_i own updates with
// actor_steps Adam steps of the actor each.
static int rgroup_end(ReplayGroupCore& g, const ReplayGroupCall& call, int B, int actor_steps) {
    HIPCHK(hipEventRecord(g.done, g.stream));
    for (int i = 0; i < call.k; ++i) {
        if (!call.work[i]) continue;
        int rc = rgroup_fanout(g, i);
        // a prioritised member: the call's priorities are the last update's for the side stream's next tree write (per_side_enter)
        if (!rc && g.m[i]->per) rc = per_mark_update(g.m[i]);
        if (rc) return rc;
        SacState* s = sac_of(g.m[i]);
        s->n_updates += call.n[i]; s->t_critic += call.n[i]; s->t_actor += (int64_t)call.n[i] * actor_steps;
        s->last_B = B;
        s->pre_valid = false;                          // no rider blocks ran: the member's next own update draws its sample
    }
    return 0;
}
// the step row of a SAC-Lag or DDPG-Lag member: one Adam step of the actor per update
static void sac_group_step_row(int u, SacGroupStep& st, const fsrl_ctx* c, const SacState* s) {
    if (!s) return;
    const AdamStep as = adam_step(s->cfg.actor_lr, c->cfg.beta1, c->cfg.beta2, s->t_actor + u + 1);
    st.a_step = as.step_size; st.a_bc2 = as.bc2_sqrt;
}

// Adam's constants of member c in its row of a member table (SacGroupMember and CvpoGroupMember name them alike), as adam_launch
// passes them ...
template <class Row>
static void member_adam_consts(Row& r, const fsrl_ctx* c) {
    const double b1 = c->cfg.beta1, b2 = c->cfg.beta2;
    r.one_minus_b1 = (float)(1.0 - b1); r.beta2 = c->cfg.beta2; r.one_minus_b2 = (float)(1.0 - b2); r.adam_eps = c->cfg.adam_eps;
}
// ... and the Polyak pass that rides on the critics' Adam (DDPG-Lag: on the actor's too)
static void member_adam_consts(SacGroupMember& t, const fsrl_ctx* c, float tau) {
    member_adam_consts(t, c);
    t.tau = tau; t.one_minus_tau = (float)(1.0 - (double)tau);
}

// a group of layered members (all fused or all layered): host_sac_group_layered.inc
struct LaySacGroup;
static void lay_sac_group_free(LaySacGroup* lg);
static int lay_sac_group_update(fsrl_sac_group* g, int32_t B, const int32_t* n_updates, const double* lagrangians, const double* rescaling);

struct fsrl_sac_group {
    ReplayGroupCore core;
    DevTable<SacGroupMember> tab;              // [k]
    DevTable<SacGroupStep> steps;              // [updates][k]
    LaySacGroup* lay = nullptr;                // job and head tables of a layered group, made by its first update
    DevTable<PerGroupMember> per;              // [k], a group of prioritised members: their tree arguments, rebuilt per call
    DevTable<SacNstepArgs> per_na;             // [k], ... fused: the stand-alone n-step launch's (a layered group has its own)
};
// the members of a group agree on prioritised replay, and stay so: fsrl_sac_group_create checks it, fsrl_per_enable refuses a
// context in a group, and nothing else switches it on or off
static bool sac_group_per(const fsrl_sac_group* g) { return g->core.m[0] && g->core.m[0]->per; }
// The tree arguments of every member with work, as its own per_sample_launch / per_update_launch would pass them: alpha, beta and
// weight_norm are the member's as of this call, the buffers the ones its join left (rgroup_enter's build_tables step).
static int per_group_table(fsrl_sac_group* g, const ReplayGroupCall& call, int B) {
    const size_t k = (size_t)call.k;
    const int rc = table_ensure(g->per, k, k);
    if (rc) return rc;
    memset(g->per.h, 0, k * sizeof(PerGroupMember));
    for (int i = 0; i < call.k; ++i) {
        if (!call.work[i]) continue;
        fsrl_ctx* c = g->core.m[i];
        PerGroupMember& m = g->per.h[i];
        m.p = per_dev(c->per); m.pb = per_batch_args(c->per, B); m.u = per_upd_args(c->per, sac_of(c), B);
    }
    HIPCHK(hipMemcpyAsync(g->per.d, g->per.h, k * sizeof(PerGroupMember), hipMemcpyHostToDevice, g->core.stream));
    return 0;
}

static void sac_group_detach(fsrl_ctx* c) {
    if (!c->sac_group) return;
    rgroup_detach(c->sac_group->core, c);
    c->sac_group = nullptr;
}

extern "C" int fsrl_sac_group_destroy(fsrl_sac_group* g) {
    if (!g) return 0;
    for (fsrl_ctx* c : g->core.m) if (c) c->sac_group = nullptr;
    rgroup_destroy(g->core);
    table_free(g->tab); table_free(g->steps); table_free(g->per); table_free(g->per_na);
    lay_sac_group_free(g->lay);
    delete g;
    return 0;
}

extern "C" int fsrl_sac_group_create(fsrl_ctx** ctxs, int32_t k, fsrl_sac_group** out) {
    CHECK_ARG(ctxs && out, "null argument");
    CHECK_ARG(k >= 1 && k <= FSRL_MAX_GROUP, "a SAC group has 1..%d members", FSRL_MAX_GROUP);
    const fsrl_ctx* c0 = ctxs[0];
    CHECK_ARG(c0, "null member");
    for (int i = 0; i < k; ++i) {
        const fsrl_ctx* c = ctxs[i];
        CHECK_ARG(c, "null member");
        const SacState* s = reinterpret_cast<const SacState*>(c->sac);
        CHECK_ARG(c->cfg.algo == FSRL_ALGO_SAC_LAG && s, "member %d: grouped SAC updates take SAC-Lagrangian contexts (fsrl_sac_init)", i);
        if ((c->per != nullptr) != (c0->per != nullptr))
            return fail(FSRL_EINVAL, "member %d has prioritised replay on and member %d does not: a group's members all have it on "
                        "(fsrl_per_enable before the group is made; alpha, beta and weight_norm may differ) or all off", c->per ? i : 0,
                        c->per ? 0 : i);
        CHECK_ARG(!s->cvpo, "member %d runs CVPO: grouped SAC updates take SAC-Lagrangian contexts only", i);
        const SacState* s0 = reinterpret_cast<const SacState*>(c0->sac);
        CHECK_ARG(s->layered == s0->layered, "member %d is a %s context and member 0 a %s one: a group is all fused (two hidden layers of at "
                  "most 256 units) or all layered contexts", i, s->layered ? "layered" : "fused", s0->layered ? "layered" : "fused");
        CHECK_ARG(c->device == c0->device, "member %d: members live on one device", i);
        CHECK_ARG(!c->sac_group, "member %d is already in a SAC group", i);
        CHECK_ARG(s->ddpg == s0->ddpg, "member %d: a group is all SAC-Lagrangian or all DDPG-Lagrangian (deterministic actor) contexts, "
                  "and member 0 is %s", i, s0->ddpg ? "DDPG-Lagrangian" : "SAC-Lagrangian");
        CHECK_ARG(c->cfg.obs_dim == c0->cfg.obs_dim && c->cfg.act_dim == c0->cfg.act_dim && c->cfg.hidden == c0->cfg.hidden &&
                  (!s->layered || lay_same_shape(c->cfg, c0->cfg)),
                  "member %d: members must have one network shape (obs_dim, act_dim, hidden; layered: every hidden_sizes[l] and force_layered)", i);
        CHECK_ARG(s->cfg.n_step == s0->cfg.n_step && (s->cfg.auto_alpha != 0) == (s0->cfg.auto_alpha != 0) &&
                  (s->cfg.use_lagrangian != 0) == (s0->cfg.use_lagrangian != 0),
                  "member %d: members must share n_step, auto_alpha and use_lagrangian (learning rates, tau, seeds and data may differ)", i);
        CHECK_ARG(c->cfg.n_critics == c0->cfg.n_critics, "member %d: members must share n_critics (the lagrangians' row length)", i);
        CHECK_ARG(s->mean_tanh == s0->mean_tanh, "member %d: members must share actor_mean (the actor's mean is %s, member 0's %s)", i,
                  s->mean_tanh ? "max_action * tanh(head)" : "unbounded", s0->mean_tanh ? "max_action * tanh(head)" : "unbounded");
        for (int j = 0; j < i; ++j) CHECK_ARG(ctxs[j] != c, "member %d is listed twice", i);
    }
    HIPCHK(hipSetDevice(c0->device));
    fsrl_sac_group* g = new fsrl_sac_group();
    hipError_t e = rgroup_create(g->core, c0->device, k);
    if (e != hipSuccess) fail(FSRL_EHIP, "SAC group allocation failed: %s", hipGetErrorString(e));
    if (e != hipSuccess || table_ensure(g->tab, (size_t)k, (size_t)k)) {
        (void)fsrl_sac_group_destroy(g);
        return FSRL_EHIP;
    }
    for (int i = 0; i < k; ++i) { g->core.m.push_back(ctxs[i]); ctxs[i]->sac_group = g; }
    *out = g;
    return 0;
}

// a member's weight-gradient arguments (the grouped CVPO update, host_cvpo_group.inc, forms its members' here too).  Batches of up
// to 512 padded rows: sac_wgrad_small_args (host_sac.inc).
// larger batches: sac_wgrad's split-K plan of `ny` networks for this member alone, its partials in the member's own buffer *G
static int group_wgrad_split(fsrl_ctx* c, const SacState* s, FbWgradArgs& wa, const ModelDesc& md, int ny, const float* X, int stride,
                             int B, const float** G, int* nsplit) {
    wa = sac_wgrad_args(c, s, ny, X, B);
    // wgrad_launch's fb_wgrad_kernel plan (PAIR2 = false)
    const WgradBlocks wb = wgrad_blocks(md.Do, c->cfg.hidden, false);
    const int passes = wb.passes, NB = wb.NB;
    const WgradPlan pl = wgrad_plan(wa.rows, NB * ny, c->n_cus);
    int rc = ensure_parts(c, stride, pl.nsplit);
    if (rc) return rc;
    wa.out = c->wg_parts; wa.ks_per_split = pl.ks_per_split; wa.split_stride = stride; wa.dbg_skip = 0;
    wa.aux_passes = passes; wa.remap_total = NB * ny * pl.nsplit; wa.remap_ny = ny;
    *G = c->wg_parts; *nsplit = pl.nsplit;
    return 0;
}
// a fused member's check (rgroup_begin): fsrl_tr_set_plan's one-pass streaming weight gradients (256 wide, >= 4096 rows) would give
// this member another kernel alone (fb_wgrad2_kernel); the tiled kernel fb_wgrad3_kernel needs re-laid observations the replay
// agents never hand over
static int rgroup_no_stream_wgrad(int i, const fsrl_ctx* c, int B) {
    CHECK_ARG(!(c->wgrad_stream && c->cfg.hidden == 256 && (B + 15) / 16 * 16 >= 4096),
              "member %d: the streaming weight-gradient plan (fsrl_tr_set_plan wgrad = 3) is not grouped", i);
    return 0;
}
// what a SAC-Lag / DDPG-Lag and a CVPO member fill alike in the table the SAC group's kernels read: the parameter and Adam stores
// with Adam's constants and the Polyak tau, the critic half's two tile launches (na: the member's n-step arguments), and both
// weight-gradient launches, the critics' over XQ and the actor's over OBS, by sac_wgrad's plan for this member alone
static int group_member_base(fsrl_ctx* c, SacState* s, SacGroupMember& t, int B, const SacNstepArgs& na, float tau, bool small_wgrad,
                             int* nsplit_q, int* nsplit_a) {
    t = SacGroupMember{};
    t.PA = s->PA; t.MA = s->MA; t.VA = s->VA; t.PQ = s->PQ; t.PQT = s->PQT; t.MQ = s->MQ; t.VQ = s->VQ;
    member_adam_consts(t, c, tau);
    t.qf = sac_q_args(c, s, s->PQT, s->XN, FB_MODE_Q_FWD, 0.f, 0.f, s->stq, B, nullptr, s->n_tiles, nullptr);
    // (a prioritised member's training launch reads its targets from Y: the stand-alone n-step launch runs, per_update reads them too)
    t.qt = sac_q_args(c, s, s->PQ, s->XQ, FB_MODE_Q_TRAIN, 0.f, 0.f, s->stq, B, nullptr, s->n_tiles, c->per ? nullptr : &na);
    if (!small_wgrad) {
        const int rc = group_wgrad_split(c, s, t.fq, s->mdq, s->n_q, s->XQ, s->nq_dev, B, &t.GQ, nsplit_q);
        return rc ? rc : group_wgrad_split(c, s, t.fa, s->mda, 1, s->OBS, s->na_dev, B, &t.GA, nsplit_a);
    }
    const int rp = s->n_tiles * 16;
    int rc = ensure_parts(c, s->nq_dev, 1);
    if (rc) return rc;
    t.GQ = c->wg_parts;
    rc = ensure_parts(c, s->na_dev, 1);
    if (rc) return rc;
    t.GA = c->wg_parts;
    if (!s->gsq_scratch) HIPCHK(s->mem.dev(&s->gsq_scratch, (size_t)wg_grid(256, FSRL_MAX_NETS) * 4));
    t.wq = sac_wgrad_small_args(s, rp, s->XQ, const_cast<float*>(t.GQ));
    t.wa = sac_wgrad_small_args(s, rp, s->OBS, const_cast<float*>(t.GA));
    *nsplit_q = *nsplit_a = 1;
    return 0;
}

// the member's table entry: every argument of the nine launches as fsrl_sac_update forms it (library RNG, fold path)
static int sac_group_member(fsrl_ctx* c, SacState* s, SacGroupMember& t, int B, const double* lags, double rescaling,
                            bool q_r4, bool a_r4, bool f_r4, bool small_wgrad, int* nsplit_q, int* nsplit_a) {
    const int ns = s->cfg.n_step, nt = s->n_tiles;
    const float lam = (s->cfg.use_lagrangian && lags) ? (float)lags[0] : 0.0f;
    const float resc = (float)rescaling;
    const int rc = group_member_base(c, s, t, B, sac_nstep_args(c, s, B), s->cfg.tau, small_wgrad, nsplit_q, nsplit_a);
    if (rc) return rc;
    t.PAT = s->ddpg ? s->PAT : nullptr;        // DDPG-Lag: the forward launch's first half runs it, the actor's Adam pass moves it
    // ---- actors (probe = 0: a probe build's phases are the solo path's); the forward launch carries the current actor's batch
    //      and the sample + gather (the sample's arguments: the step table's, rgroup_enter)
    const int det = s->ddpg ? 1 : 0;
    t.af = sac_actor_args(c, s, B, SAC_A_FWD, s->OBSN, s->eps_t, s->XN, s->LPN, resc, lam, det, 0);
    t.af.P2 = s->PA; t.af.obs2 = s->OBS; t.af.eps2 = s->eps_p; t.af.X2 = s->XP; t.af.lp2 = s->LP; t.af.tiles_half = f_r4 ? 4 * nt : nt;
    // a prioritised member's sample is per_sample_group's and its gather a launch of its own (weight_norm needs the whole batch's
    // maximum before the first weight is used): the fold stays off, as in fsrl_sac_update
    t.af.sg_on = c->per ? 0 : 1; t.af.ga = sac_gather_args(c, s, B, ns);
    t.ab = sac_actor_args(c, s, B, SAC_A_BWD, s->OBS, s->eps_p, s->XP, s->LP, resc, lam, det, 0);
    // ---- Q(s, a ~ pi) with the updated critics + dQ/da
    t.qd = sac_q_args(c, s, s->PQ, s->XP, FB_MODE_Q_DIN, 0.f, 0.f, s->stdin_, B, nullptr, nt, nullptr);
    // ---- the logged row (fin.stats per step)
    t.fin = sac_final_args(c, s, B, resc, lam, q_r4 ? 4 * nt : nt, a_r4 ? 4 * nt : nt, nullptr);
    t.stats = s->d_stats; t.nstats = s->nstats;
    return 0;
}

// ---- the critic half of one grouped update, the same four launches for SAC and CVPO members: target Q-networks on (s_{t+n}, a'),
//      the critics' forward + backward with their n-step targets, their weight gradients, their Adam with the Polyak targets.
//      mdq_w: the ModelDesc of the small weight-gradient launch (its n_nets = the networks the launch covers)
//      per != NULL (a group of prioritised members): the n-step targets as a launch of their own (na) before the training launch,
//      and behind it the sampled rows' new priorities
struct ReplayGroupCritic {
    int k, n_q, qt, rp, gq, nq_dev, nsq; bool q_r4, small_wgrad;
    const PerGroupMember* per = nullptr; const SacNstepArgs* na = nullptr; int B = 0;
};
template <int HH>
static void rgroup_critic_half(hipStream_t gs, const ReplayGroupCritic& p, const ModelDesc& mdq, const ModelDesc& mdq_w,
                               const SacGroupMember* tab, const SacGroupStep* st) {
    const int k = p.k, n_q = p.n_q, qt = p.qt;
    if (p.q_r4) hipLaunchKernelGGL((sac_q_group_kernel<HH, 4, 0>), dim3(qt, n_q, k), dim3(4 * HH), 0, gs, mdq, tab, st);
    else hipLaunchKernelGGL((sac_q_group_kernel<HH, 16, 0>), dim3(qt, n_q, k), dim3(4 * HH), 0, gs, mdq, tab, st);
    if (p.per) hipLaunchKernelGGL(sac_nstep_group_kernel, dim3((p.B + 255) / 256, k), dim3(256), 0, gs, p.na, st);
    if (p.q_r4) hipLaunchKernelGGL((sac_q_group_kernel<HH, 4, 1>), dim3(qt, n_q, k), dim3(4 * HH), 0, gs, mdq, tab, st);
    else hipLaunchKernelGGL((sac_q_group_kernel<HH, 16, 1>), dim3(qt, n_q, k), dim3(4 * HH), 0, gs, mdq, tab, st);
    if (p.per) hipLaunchKernelGGL(per_update_group_kernel, dim3(k), dim3(PER_THREADS), 0, gs, p.per, st);
    if (p.small_wgrad) hipLaunchKernelGGL((sac_wgrad_group_kernel<HH, 0>), dim3(wg_grid(HH, n_q), k), dim3(1024), 0, gs, mdq_w, tab, st, p.rp);
    else hipLaunchKernelGGL((sac_wgrad_split_group_kernel<HH, 0>), dim3(p.gq, k), dim3(1024), 0, gs, mdq, tab, st);
    hipLaunchKernelGGL(sac_adam_group_kernel, dim3((p.nq_dev + 255) / 256, k), dim3(256), 0, gs, mdq, tab, st, p.nq_dev, p.nsq, p.nq_dev);
}

extern "C" int fsrl_sac_group_update(fsrl_sac_group* g, int32_t B, const int32_t* n_updates, const double* lagrangians,
                                     const double* rescaling) {
    CHECK_ARG(g && n_updates && rescaling, "null argument");
    ReplayGroupCore& gc = g->core;
    if (gc.broken) return fail(FSRL_ESTATE, "a member of this SAC group was destroyed: destroy the group");
    CHECK_ARG(B >= 1, "batch_size must be >= 1");
    const int k = (int)gc.m.size();
    fsrl_ctx* c0 = gc.m[0];
    SacState* s0 = sac_of(c0);
    if (s0 && s0->layered) return lay_sac_group_update(g, B, n_updates, lagrangians, rescaling);
    ReplayGroupCall call;
    int rc = rgroup_begin(gc, false, n_updates, call, [&](int i, const fsrl_ctx* c, const SacState* s) {
        CHECK_ARG(s->wgrad_splitk == s0->wgrad_splitk, "members must agree on fsrl_sac_set_plan bit 0 (split-K weight gradients)");
        return rgroup_no_stream_wgrad(i, c, B);
    });
    if (rc) return rc;
    CHECK_ARG(!s0->cfg.use_lagrangian || lagrangians, "lagrangians: [k][n_critics - 1] when use_lagrangian is on");
    const int n_max = call.n_max;
    if (n_max == 0) return 0;
    const int H = c0->cfg.hidden, nt = (B + 15) / 16, rp = nt * 16, n_q = s0->n_q;     // 4 (SAC-Lag) or 2 (DDPG-Lag)
    // tile heights: the single-context rule applied to the group's whole launch (4-row tiles while it fits one round)
    const bool t16 = c0->probe_tile16;
    const bool q_r4 = (size_t)4 * nt * n_q * k <= (size_t)c0->n_cus && !t16;
    const bool a_r4 = (size_t)4 * nt * k <= (size_t)c0->n_cus && !t16;
    const bool f_r4 = a_r4 && (size_t)8 * nt * k <= (size_t)c0->n_cus;
    const bool small_wgrad = rp <= 512 && !s0->wgrad_splitk;
    const size_t lag_stride = (size_t)std::max(1, c0->cfg.n_critics - 1);
    int nsq = 1, nsa = 1, rq_total = 0, ra_total = 0;
    const bool per_on = sac_group_per(g);
    rc = rgroup_enter(gc, g->steps, call, B, [&]() {
        if (per_on) {
            int rc = per_group_table(g, call, B);
            if (!rc) rc = table_ensure(g->per_na, (size_t)k, (size_t)k);
            if (rc) return rc;
            memset(g->per_na.h, 0, (size_t)k * sizeof(SacNstepArgs));
            for (int i = 0; i < k; ++i)
                if (call.work[i]) g->per_na.h[i] = sac_nstep_args(gc.m[i], sac_of(gc.m[i]), B);
            HIPCHK(hipMemcpyAsync(g->per_na.d, g->per_na.h, (size_t)k * sizeof(SacNstepArgs), hipMemcpyHostToDevice, gc.stream));
        }
        for (int i = 0; i < k; ++i) {
            if (!call.work[i]) continue;
            // the member's own side-stream prefetch writes the other set of batch buffers only: nothing to wait for
            fsrl_ctx* c = gc.m[i];
            const double* lg = s0->cfg.use_lagrangian ? lagrangians + (size_t)i * lag_stride : nullptr;
            SacGroupMember& t = g->tab.h[i];
            const int rc = sac_group_member(c, sac_of(c), t, B, lg, rescaling[i], q_r4, a_r4, f_r4, small_wgrad, &nsq, &nsa);
            if (rc) return rc;                         // nsq, nsa, remap totals: one shape, one plan -- the same for every member
            rq_total = t.fq.remap_total; ra_total = t.fa.remap_total;
        }
        return 0;
    }, [](int u, int, SacGroupStep& st, const fsrl_ctx* c, const SacState* s) { sac_group_step_row(u, st, c, s); });
    if (rc) return rc;
    hipStream_t gs = gc.stream;
    HIPCHK(hipMemcpyAsync(g->tab.d, g->tab.h, (size_t)k * sizeof(SacGroupMember), hipMemcpyHostToDevice, gs));
    HIPCHK(hipMemcpyAsync(g->steps.d, g->steps.h, (size_t)n_max * k * sizeof(SacGroupStep), hipMemcpyHostToDevice, gs));
    const ModelDesc mda = s0->mda, mdq = s0->mdq;
    const int na_dev = s0->na_dev;
    const SacGroupMember* tab = g->tab.d;
    rc = dispatch_H(H, [&](auto hc) {
        constexpr int HH = decltype(hc)::value;
        const int ft = f_r4 ? 4 * nt : nt, qt = q_r4 ? 4 * nt : nt, at = a_r4 ? 4 * nt : nt;
        const int ga = round_up(ra_total, 8);
        ReplayGroupCritic cr{k, n_q, qt, rp, round_up(rq_total, 8), s0->nq_dev, nsq, q_r4, small_wgrad};
        if (per_on) { cr.per = g->per.d; cr.na = g->per_na.d; cr.B = B; }
        const int gather_blocks = std::min(1024, (B * (c0->cfg.obs_dim + c0->cfg.act_dim) + 255) / 256);
        for (int u = 0; u < n_max; ++u) {
            const SacGroupStep* st = g->steps.d + (size_t)u * k;
            // a group of prioritised members: the descent of each member's sum tree with its weights, then the plain gather
            if (per_on) {
                hipLaunchKernelGGL(per_sample_group_kernel, dim3(k), dim3(PER_THREADS), 0, gs, g->per.d, st);
                hipLaunchKernelGGL(sac_gather_group_kernel, dim3(gather_blocks, k), dim3(256), 0, gs, &tab->af.ga, sizeof(SacGroupMember), st);
            }
            // 1. both actors' forward, the sample drawn and gathered inside (prioritised: drawn and gathered above)
            if (f_r4) hipLaunchKernelGGL((sac_actor_group_kernel<HH, 4, SAC_A_FWD>), dim3(2 * ft, k), dim3(4 * HH), 0, gs, mda, tab, st);
            else hipLaunchKernelGGL((sac_actor_group_kernel<HH, 16, SAC_A_FWD>), dim3(2 * ft, k), dim3(4 * HH), 0, gs, mda, tab, st);
            // 2. - 5. the critic half
            rgroup_critic_half<HH>(gs, cr, mdq, mdq, tab, st);
            // 6. Q(s, a ~ pi) with the updated critics + dQ/da; 7. the actor's backward
            if (q_r4) hipLaunchKernelGGL((sac_q_group_kernel<HH, 4, 2>), dim3(qt, n_q, k), dim3(4 * HH), 0, gs, mdq, tab, st);
            else hipLaunchKernelGGL((sac_q_group_kernel<HH, 16, 2>), dim3(qt, n_q, k), dim3(4 * HH), 0, gs, mdq, tab, st);
            if (a_r4) hipLaunchKernelGGL((sac_actor_group_kernel<HH, 4, SAC_A_BWD>), dim3(at, k), dim3(4 * HH), 0, gs, mda, tab, st);
            else hipLaunchKernelGGL((sac_actor_group_kernel<HH, 16, SAC_A_BWD>), dim3(at, k), dim3(4 * HH), 0, gs, mda, tab, st);
            // 8. the actor's weight gradients; 9. its Adam, alpha step (DDPG-Lag: the target actor's Polyak update) and logged row
            if (small_wgrad) hipLaunchKernelGGL((sac_wgrad_group_kernel<HH, 1>), dim3(wg_grid(HH, 1), k), dim3(1024), 0, gs, mda, tab, st, rp);
            else hipLaunchKernelGGL((sac_wgrad_split_group_kernel<HH, 1>), dim3(ga, k), dim3(1024), 0, gs, mda, tab, st);
            hipLaunchKernelGGL(sac_adam_final_group_kernel, dim3((na_dev + 255) / 256 + 1, k), dim3(256), 0, gs, mda, tab, st, na_dev, nsa, na_dev);
            HIPCHK(hipGetLastError());
        }
        return 0;
    });
    if (rc) return rc;
    return rgroup_end(gc, call, B, 1);
}
