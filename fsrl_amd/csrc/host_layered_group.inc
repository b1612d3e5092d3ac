// host_layered_group.inc -- a group of LAYERED PPO-Lagrangian or FOCOPS contexts of one shape (part of fsrl_hip.hip, before
// host_group.inc; kernels_layered_group.hpp has the kernels): the minibatch step of fsrl_group_ppo_update and the shared actor
// request of fsrl_group_collect_step.  A FOCOPS group shares the job tables, the forward / backward / weight-side launches and the
// collection below; its loss head, prep and step launches are host_focops_group.inc's.
//   update:  lay_ppo_steps' 2 L + 5 launches, each carrying every member (job tables in device memory, built once per grouped
//            update; rows and the minibatch's offset come from the member's GroupStep row).  Bit-identical to the member's own
//            fsrl_ppo_update: see kernels_layered_group.hpp.
//   collect: no resident kernel -- the members' observation rows side by side in pinned memory, L + 1 lin_kernel<LIN_F> launches
//            with one job per member that has rows, one lay_infer_out_group_kernel launch that leaves means, sigma_param rows
//            and completion words in pinned memory: L + 2 launches per vector step instead of k (L + 2).
struct LayGroup {
    DevTable<LinGroupJob> jobs;                 // forward layers 0 .. L | backward layers L - 1 .. 0 | the weight side
    DevTable<LayHeadArgs> heads;                // [k]
    int k = 0, nn = 0, L = 0, J = 0;            // J: weight-side jobs of one member
    bool vec_f[FSRL_MAX_HIDDEN + 1] = {}, vec_x[FSRL_MAX_HIDDEN] = {}, vec_w = true;
    int nw_w = 4;                               // NW of the weight-side launch: the one a member's own launch has
    hipEvent_t copied = nullptr; bool in_flight = false;     // the pinned tables have left host memory
    // lock-step collection
    void* ch = nullptr;                         // pinned: [done k x cap / 16 | pad | obs k x cap x Do | mu k x cap x cols | sigma_param k x 16]
                                                // (cols: Da for the on-policy group, the raw head columns for the replay agents)
    float* cd = nullptr;                        // device: two activation buffers k x cap x hm, head outputs k x cap x 16
    int ccap = 0, ck = 0;                       // rows reserved per member; members the buffers were made for
    unsigned cseq = 0;
    int crow[GACTOR_MAX_MEMBERS] = {};          // rows of each member in the request in flight
};
struct LayGroupPinned { unsigned* done; float* obs; float* mu; float* sp; };
static LayGroupPinned lay_group_pinned(const LayGroup& lg, int Do, int cols) {
    char* b = (char*)lg.ch;
    LayGroupPinned p;
    p.done = (unsigned*)b;
    p.obs = (float*)(b + round_up(lg.ck * (lg.ccap / 16) * 4, 256));
    p.mu = p.obs + (size_t)lg.ck * lg.ccap * Do;
    p.sp = p.mu + (size_t)lg.ck * lg.ccap * cols;
    return p;
}

static void lay_group_free(LayGroup& lg, Mem& m) {       // m: the embedding group's ring owner (GaRing::mem)
    table_free(lg.jobs); table_free(lg.heads);
    if (lg.copied) (void)hipEventDestroy(lg.copied);
    (void)m.release(&lg.ch); (void)m.release(&lg.cd);
    lg = LayGroup{};
}

// members of a layered group have one shape: the widths and the switch that made a two-layer network layered
static bool lay_same_shape(const fsrl_config& a, const fsrl_config& b) {
    if (a.n_hidden != b.n_hidden || a.force_layered != b.force_layered) return false;
    for (int l = 0; l < a.n_hidden && l < FSRL_MAX_HIDDEN; ++l) if (a.hidden_sizes[l] != b.hidden_sizes[l]) return false;
    return true;
}

// Job tables of one grouped update, after every member's fsrl_ppo_begin (working sets may have been regrown): the jobs
// lay_fwd_k / lay_bwd_dz_k / lay_wgrad_k build for a member, with the rows left to the step table.  has_rows[i] == 0: member i
// sits the whole update out (its working set may not exist yet); its jobs stay empty.
static int lay_group_tables(LayGroup& lg, fsrl_ctx* const* m, int k, const char* has_rows, hipStream_t s) {
    const LayState* l0 = m[0]->lay;
    const int nn = l0->lm.n_nets, L = l0->L, J = nn * (L + 1) + 1;
    const size_t total = (size_t)(2 * L + 1) * k * nn + (size_t)k * J;
    int rc = table_ensure(lg.jobs, total, total, s);
    if (!rc) rc = table_ensure(lg.heads, (size_t)k, (size_t)k, s);
    if (rc) return rc;
    if (!lg.copied) HIPCHK(hipEventCreateWithFlags(&lg.copied, hipEventDisableTiming));
    if (lg.in_flight) { HIPCHK(hipEventSynchronize(lg.copied)); lg.in_flight = false; }
    lg.k = k; lg.nn = nn; lg.L = L; lg.J = J;
    memset(lg.jobs.h, 0, total * sizeof(LinGroupJob));
    memset(lg.heads.h, 0, (size_t)k * sizeof(LayHeadArgs));
    for (int l = 0; l <= L; ++l) lg.vec_f[l] = true;
    for (int l = 0; l < L; ++l) lg.vec_x[l] = true;
    lg.vec_w = true;
    for (int i = 0; i < k; ++i) {
        fsrl_ctx* c = m[i];
        LayState* ls = c->lay;
        const LayModel& lm = ls->lm;
        LinGroupJob* fw = lg.jobs.h;
        LinGroupJob* bw = fw + (size_t)(L + 1) * k * nn;
        LinGroupJob* wg = bw + (size_t)L * k * nn;
        for (int l = 0; l <= L; ++l)
            for (int net = 0; net < nn; ++net) fw[((size_t)l * k + i) * nn + net].member = i;
        for (int l = 0; l < L; ++l)
            for (int net = 0; net < nn; ++net) bw[((size_t)l * k + i) * nn + net].member = i;
        for (int j = 0; j < J; ++j) { wg[(size_t)i * J + j].member = i; wg[(size_t)i * J + j].first = i * J; }
        if (!has_rows[i]) continue;
        const float* P = c->P;
        // ---- forward (lay_fwd_k): table l = layer l
        for (int l = 0; l <= L; ++l)
            for (int net = 0; net < nn; ++net) {
                const LayLayer& ll = lm.net[net].l[l];
                LinGroupJob& gj = fw[((size_t)l * k + i) * nn + net];
                LinJob& jb = gj.j;
                if (l == 0) { jb.A = c->obs_p; gj.flags = LGJ_A_OBS; } else jb.A = ls->act[net][l - 1];
                jb.lda = ll.in;
                jb.B = P + ll.W; jb.ldb = ll.in;
                jb.aux = P + ll.b;
                jb.N = ll.out; jb.K = ll.in;
                if (l < L) { jb.C = ls->act[net][l]; jb.ldc = ll.out; jb.relu = 1; }
                else { jb.C = ls->out + (size_t)net * ls->mbp * FSRL_MAX_ACT; jb.ldc = FSRL_MAX_ACT; jb.relu = 0; }
                lg.vec_f[l] = lg.vec_f[l] && lay_vec_ok(jb.A, jb.lda, jb.K) && lay_vec_ok(jb.B, jb.ldb, jb.K);
            }
        // ---- backward, activation side (lay_bwd_dz_k): table t = hidden layer L - 1 - t
        for (int t = 0; t < L; ++t) {
            const int l = L - 1 - t;
            for (int net = 0; net < nn; ++net) {
                const LayLayer& up = lm.net[net].l[l + 1];
                LinJob& jb = bw[((size_t)t * k + i) * nn + net].j;
                if (l == L - 1) { jb.A = ls->dout + (size_t)net * ls->mbp * FSRL_DOW; jb.lda = FSRL_DOW; jb.a_len = 16; }
                else { jb.A = ls->dz[net][l + 1]; jb.lda = up.out; }
                jb.B = P + up.W; jb.ldb = up.in;
                jb.C = ls->dz[net][l]; jb.ldc = up.in; jb.aux = ls->act[net][l]; jb.ldaux = up.in;
                jb.N = up.in; jb.K = up.out;
                lg.vec_x[t] = lg.vec_x[t] && lay_vec_ok(jb.A, jb.lda, jb.a_len ? jb.a_len : jb.K) && lay_vec_ok(jb.B, jb.ldb, jb.N);
            }
        }
        // ---- weight side (lay_wgrad_k): actor layers, sigma_param, critic layers
        int nj = 0;
        long wgs = 0;
        for (int net = 0; net < nn; ++net) {
            for (int l = 0; l <= L; ++l) {
                const LayLayer& ll = lm.net[net].l[l];
                LinGroupJob& gj = wg[(size_t)i * J + nj++];
                LinJob& jb = gj.j;
                jb.A = (l < L) ? ls->dz[net][l] : ls->dout + (size_t)net * ls->mbp * FSRL_DOW;
                jb.lda = (l < L) ? ll.out : FSRL_DOW; jb.a_len = (l < L) ? 0 : 16;
                if (l == 0) { jb.B = c->obs_p; gj.flags = LGJ_B_OBS; } else jb.B = ls->act[net][l - 1];
                jb.ldb = ll.in;
                jb.C = c->G + ll.W; jb.ldc = ll.in;
                jb.bias_out = c->G + ll.b;
                jb.M = ll.out; jb.N = ll.in;
                gj.gsq = ls->gsq;
            }
            if (lm.net[net].sigma >= 0) {
                LinGroupJob& gj = wg[(size_t)i * J + nj++];
                LinJob& jb = gj.j;
                jb.A = ls->dout + (size_t)net * ls->mbp * FSRL_DOW + 16; jb.lda = FSRL_DOW; jb.a_len = 16;
                jb.B = c->obs_p; gj.flags = LGJ_B_OBS; jb.ldb = lm.net[net].l[0].in; jb.C = c->G; jb.ldc = 0;
                jb.bias_out = c->G + lm.net[net].sigma;
                jb.M = lm.Da; jb.N = 0;
                gj.gsq = ls->gsq;
            }
        }
        for (int j = 0; j < nj; ++j) {
            const LinJob& jb = wg[(size_t)i * J + j].j;
            lg.vec_w = lg.vec_w && lay_vec_ok(jb.A, jb.lda, jb.a_len ? jb.a_len : jb.M) && lay_vec_ok(jb.N > 0 ? jb.B : nullptr, jb.ldb, jb.N);
            wgs += (long)std::max(1, (jb.N + 63) / 64) * ((jb.M + 63) / 64);
        }
        lg.nw_w = wgs <= 2 * c->n_cus ? 4 : (wgs <= 4 * c->n_cus ? 2 : 1);      // lay_launch's rule on ONE member's launch
        // ---- heads
        LayHeadArgs& h = lg.heads.h[i];
        h.out = ls->out; h.dout = ls->dout; h.rd = c->rd_p; h.statp = c->statp; h.P = c->P; h.sigma = lm.net[0].sigma;
        h.mbp = ls->mbp; h.n_nets = nn; h.Da = lm.Da; h.unbounded = lm.unbounded;
    }
    HIPCHK(hipMemcpyAsync(lg.jobs.d, lg.jobs.h, total * sizeof(LinGroupJob), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(lg.heads.d, lg.heads.h, (size_t)k * sizeof(LayHeadArgs), hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(lg.copied, s));
    lg.in_flight = true;
    return 0;
}

// member i's row of the member table: what ppo_stats_group_kernel / adam_clip_group_kernel / the obs operands read
static void lay_group_agent(fsrl_ctx* c, GroupAgent& a) {
    LayState* ls = c->lay;
    group_agent_common(c, a);
    a.bp.obs_p = c->obs_p; a.bp.rd_p = c->rd_p; a.bp.statp = c->statp; a.bp.mbp_max = ls->mbp;
    a.wp.statp = c->statp; a.wp.ctrl = c->ctrl; a.wp.P = c->P; a.wp.grad = c->G; a.wp.mbp_max = ls->mbp;
    a.gsq_part = ls->gsq; a.nparts = ls->nparts;
}

template <int FORM>
static void lay_group_launch(bool vec, int nw, dim3 grid, hipStream_t s, const LinGroupJob* jobs, const GroupAgent* tab,
                             const GroupStep* st) {
#define LAYG_GO(V, NW_) hipLaunchKernelGGL((lin_group_kernel<FORM, V, NW_>), grid, dim3(256 * NW_), 0, s, jobs, tab, st)
    if (vec) { if (nw == 4) LAYG_GO(true, 4); else if (nw == 2) LAYG_GO(true, 2); else LAYG_GO(true, 1); }
    else { if (nw == 4) LAYG_GO(false, 4); else if (nw == 2) LAYG_GO(false, 2); else LAYG_GO(false, 1); }
#undef LAYG_GO
}

// The launches of a minibatch step that do not depend on the algorithm, for every member that has a minibatch at this index
// (st_h: the pinned twin of the step rows st_d): forward() the L + 1 LIN_F launches, backward() the L LIN_X launches and the
// LIN_W launch.  The loss heads go in between and the optimiser behind: lay_group_step (PPO-Lagrangian) below,
// focops_group_update's layered branch (host_focops_group.inc).
struct LayGroupLaunch {
    const LayGroup& lg;
    const fsrl_ctx* c0;
    int k;
    hipStream_t s;
    const GroupAgent* tab;
    const GroupStep* st_d;
    int mbs = 0, gy = 0, tiles = 0;             // the largest minibatch of the step: rows, 64-row tiles, 16-row tiles
    long row_tiles = 0;                         // 64-row tiles of the members that step
    LayGroupLaunch(const LayGroup& lg_, fsrl_ctx* const* m, int k_, hipStream_t s_, const GroupAgent* tab_, const GroupStep* st_d_,
                   const GroupStep* st_h)
        : lg(lg_), c0(m[0]), k(k_), s(s_), tab(tab_), st_d(st_d_) {
        for (int i = 0; i < k; ++i)
            if (st_h[i].active) { mbs = std::max(mbs, st_h[i].mb_size); row_tiles += (st_h[i].mb_size + 63) / 64; }
        gy = (mbs + 63) / 64; tiles = (mbs + 15) / 16;
    }
    // NW of a forward / backward launch from the workgroups of the WHOLE launch (any NW gives the same bits there)
    int nw_of(long col_tiles) const {
        const long wgs = col_tiles * row_tiles;
        return wgs <= 2 * c0->n_cus ? 4 : (wgs <= 4 * c0->n_cus ? 2 : 1);
    }
    void forward() const {
        const LayModel& lm = c0->lay->lm;
        const int nn = lg.nn, L = lg.L;
        const LinGroupJob* fw = lg.jobs.d;
        for (int l = 0; l <= L; ++l) {
            int gx = 1; long ct = 0;
            for (int net = 0; net < nn; ++net) { const int t = (lm.net[net].l[l].out + 63) / 64; gx = std::max(gx, t); ct += t; }
            lay_group_launch<LIN_F>(lg.vec_f[l], nw_of(ct), dim3(gx, gy, k * nn), s, fw + (size_t)l * k * nn, tab, st_d);
        }
    }
    void backward() const {
        const LayState* l0 = c0->lay;
        const LayModel& lm = l0->lm;
        const int nn = lg.nn, L = lg.L;
        const LinGroupJob* bw = lg.jobs.d + (size_t)(L + 1) * k * nn;
        const LinGroupJob* wg = bw + (size_t)L * k * nn;
        for (int t = 0; t < L; ++t) {
            const int l = L - 1 - t;
            int gx = 1; long ct = 0;
            for (int net = 0; net < nn; ++net) { const int u = (lm.net[net].l[l + 1].in + 63) / 64; gx = std::max(gx, u); ct += u; }
            lay_group_launch<LIN_X>(lg.vec_x[t], nw_of(ct), dim3(gx, gy, k * nn), s, bw + (size_t)t * k * nn, tab, st_d);
        }
        lay_group_launch<LIN_W>(lg.vec_w, lg.nw_w, dim3(l0->wgrid.x, l0->wgrid.y, k * lg.J), s, wg, tab, st_d);
    }
};

// one PPO-Lagrangian minibatch step of every member that has one at this index: 2 L + 5 launches
static int lay_group_step(LayGroup& lg, fsrl_ctx* const* m, int k, hipStream_t s, const GroupAgent* tab, const GroupStep* st_d,
                          const GroupStep* st_h, const PpoStepArgs& base) {
    const fsrl_ctx* c0 = m[0];
    const LayGroupLaunch ll(lg, m, k, s, tab, st_d, st_h);
    if (ll.mbs == 0) return 0;
    ll.forward();
    hipLaunchKernelGGL(lay_ppo_head_group_kernel, dim3(ll.tiles, lg.nn, k), dim3(256), 0, s, lg.heads.d, tab, st_d, base);
    ll.backward();
    hipLaunchKernelGGL(ppo_stats_group_kernel, dim3(k), dim3(64), 0, s, c0->md, tab, st_d, base);
    hipLaunchKernelGGL(adam_clip_group_kernel, dim3((c0->n_dev + 4 * ADAM_NT - 1) / (4 * ADAM_NT), k), dim3(ADAM_NT), 0, s, c0->md,
                       tab, st_d, base);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------- lock-step collection
// the shared request: k_act[i] rows of obs_act (concatenated over members) -> L + 2 launches on the group's stream.  The staging is
// shared by the on-policy group below and the replay agents' collect group (host_sac_group_layered.inc): `net` is the actor
// network's layers, P(i) member i's parameter vector of it, `cols` the floats per answered row in pinned memory, and
// tail(outb, pin, maxk) the last launch, which leaves the answer and the completion words there.
static_assert(GACTOR_MAX_MEMBERS <= LAY_MAX_JOBS, "lay_group_collect_stage: one inference job per member in a launch's table");
template <class ParamOf, class Tail>
static int lay_group_collect_stage(LayGroup& lg, GaRing& ga, fsrl_ctx* c0, const LayNet& net, int Do, int hmax, int k, int cols,
                                   const int32_t* k_act, const float* obs_act, ParamOf&& P, Tail&& tail) {
    CHECK_ARG(k >= 1 && k <= LAY_MAX_JOBS, "too many members for one inference launch (limit %d)", LAY_MAX_JOBS);
    const int L = net.nl - 1;
    const size_t hm = (size_t)round_up(hmax, 4);
    hipStream_t s = ga.stream;
    int maxk = 0;
    for (int i = 0; i < k; ++i) maxk = std::max(maxk, (int)k_act[i]);
    if (maxk > lg.ccap || k != lg.ck) {
        HIPCHK(hipStreamSynchronize(s));
        const int cap = round_up(std::max(2 * maxk, 64), 16);
        const size_t hbytes = (size_t)round_up(k * (cap / 16) * 4, 256) + ((size_t)k * cap * (Do + cols) + (size_t)k * FSRL_MAX_ACT) * 4;
        lg.ccap = 0;                // regrows for another member count too
        HIPCHK(ga.mem.regrow(lg.ccap, cap, cap, {Mem::H(&lg.ch, hbytes), Mem::D(&lg.cd, (size_t)k * cap * (2 * hm + FSRL_MAX_ACT) * 4)}));
        memset(lg.ch, 0, hbytes);
        lg.ck = k;
    }
    const LayGroupPinned pin = lay_group_pinned(lg, Do, cols);
    const int cap = lg.ccap;
    lg.cseq += 1;
    if (lg.cseq == 0) lg.cseq = 1;
    size_t off = 0;
    for (int i = 0; i < k; ++i) {
        lg.crow[i] = k_act[i];
        if (k_act[i] > 0) memcpy(pin.obs + (size_t)i * cap * Do, obs_act + off * Do, (size_t)k_act[i] * Do * 4);
        off += (size_t)k_act[i];
    }
    float* bufs[2] = {lg.cd, lg.cd + (size_t)k * cap * hm};
    float* outb = lg.cd + 2 * (size_t)k * cap * hm;
    for (int l = 0; l <= L; ++l) {
        const LayLayer& ll = net.l[l];
        LinJobs jobs{};
        for (int i = 0; i < k; ++i) {
            if (k_act[i] <= 0) continue;
            LinJob& jb = jobs.j[jobs.n++];
            jb.A = (l == 0) ? pin.obs + (size_t)i * cap * Do : bufs[(l - 1) & 1] + (size_t)i * cap * hm;
            jb.lda = ll.in;
            jb.B = P(i) + ll.W; jb.ldb = ll.in;
            jb.aux = P(i) + ll.b;
            jb.M = k_act[i]; jb.N = ll.out; jb.K = ll.in;
            if (l < L) { jb.C = bufs[l & 1] + (size_t)i * cap * hm; jb.ldc = ll.out; jb.relu = 1; }
            else { jb.C = outb + (size_t)i * cap * FSRL_MAX_ACT; jb.ldc = FSRL_MAX_ACT; jb.relu = 0; }
        }
        const int rc = lay_launch<LIN_F>(c0, jobs, nullptr, s);
        if (rc) return rc;
    }
    tail(outb, pin, maxk);
    HIPCHK(hipGetLastError());
    ga.launches += 1; ga.requests += 1;
    return 0;
}
static int lay_group_collect_post(LayGroup& lg, GaRing& ga, fsrl_ctx* const* m, int k, const int32_t* k_act, const float* obs_act) {
    fsrl_ctx* c0 = m[0];
    const LayState* l0 = c0->lay;
    const LayModel& lm = l0->lm;
    const int Da = lm.Da;
    return lay_group_collect_stage(
        lg, ga, c0, lm.net[0], lm.Do, l0->hmax, k, Da, k_act, obs_act, [&](int i) { return m[i]->P; },
        [&](float* outb, const LayGroupPinned& pin, int maxk) {
            LayInferGroupArgs a{};
            for (int i = 0; i < k; ++i) { a.P[i] = m[i]->P; a.rows[i] = k_act[i]; }
            a.out = outb; a.mu = pin.mu; a.sp = pin.sp; a.done = pin.done;
            a.cap = lg.ccap; a.tiles_cap = lg.ccap / 16;
            a.sigma = lm.net[0].sigma; a.Da = Da; a.unbounded = lm.unbounded; a.max_action = c0->cfg.max_action; a.seq = lg.cseq;
            hipLaunchKernelGGL(lay_infer_out_group_kernel, dim3((maxk + 15) / 16, k), dim3(64), 0, ga.stream, a);
        });
}

// the answer of the request in flight is in pinned memory: the ring's bounded wait (rr_poll) on the completion words
static int lay_group_collect_wait(LayGroup& lg, GaRing& ga, int k, int Do, int cols) {
    const LayGroupPinned pin = lay_group_pinned(lg, Do, cols);
    const int tc = lg.ccap / 16;
    auto served = [&]() {
        for (int i = 0; i < k; ++i)
            for (int t = 0; t < (lg.crow[i] + 15) / 16; ++t)
                if (__atomic_load_n(pin.done + (size_t)i * tc + t, __ATOMIC_ACQUIRE) != lg.cseq) return false;
        return true;
    };
    const int rc = rr_poll(ga, served);
    if (rc == RR_IDLE) return fail(FSRL_EHIP, "the group's actor launches ended without an answer");
    return rr_code(rc, "the group's actor launches");
}
