// host_layered.inc -- networks of any depth / width (part of fsrl_hip.hip; kernels_layered.hpp has the kernels): the primitives
// (LayWork, lay_fwd_k / lay_bwd_dz_k / lay_wgrad_k, lay_hvp, lay_infer) every algorithm's layered branch is built from, and the
// PPO-Lagrangian minibatch step.  FOCOPS: host_focops.inc; CPO / TRPO-Lag: host_trust.inc; SAC / DDPG / CVPO: host_sac.inc, host_cvpo.inc.
// A context is "layered" when fsrl_config.n_hidden names hidden layers that are not two layers of at most 256 units
// (fsrl/agent/ppo_lag_agent.py:91,136-145: `hidden_sizes` is any tuple).  Everything around the network math -- the store, the
// batch gather, float64 GAE, reward normalisation, the per-pass permutation and advantage statistics, the logged row, the
// gradient clip + Adam, the KL early stop -- is the code the fused path runs; only launch_infer and the minibatch step differ.
#define LAY_KSPLIT_MAX 24
// One family of networks of common hidden widths (the on-policy actor + critics; a replay agent's actor; its Q-networks) with
// the working set of one batch of rows: what lay_fwd_k / lay_bwd_dz_k / lay_wgrad_k operate on.
struct LayWork {
    LayModel lm{};
    int L = 0;                          // hidden layers
    int w[FSRL_MAX_HIDDEN] = {0};       // their widths
    int hmax = 0;
    // working set (one allocation): relu(Z_l) and dL/dZ_l per network and layer, head outputs, head gradients
    int mbp = 0;
    float* ws = nullptr;
    float* act[FSRL_MAX_NETS][FSRL_MAX_HIDDEN] = {{nullptr}};
    float* dz[FSRL_MAX_NETS][FSRL_MAX_HIDDEN] = {{nullptr}};
    float* out = nullptr;               // [nn][mbp][FSRL_MAX_ACT]
    float* dout = nullptr;              // [nn][mbp][FSRL_DOW]
};
// m: the owner of k's state (LayWork itself goes by value into launches and holds no owner)
static int lay_work_ensure(fsrl_ctx* c, Mem& m, LayWork& k, int rows) {
    const int mbp = round_up(std::max(rows, 16), 16);
    if (mbp <= k.mbp) return 0;
    HIPCHK(hipStreamSynchronize(c->compute));
    const int nn = k.lm.n_nets, L = k.L;
    size_t per_net = 0;
    for (int l = 0; l < L; ++l) per_net += (size_t)mbp * round_up(k.w[l], 4);
    const size_t floats = (size_t)nn * (2 * per_net + (size_t)mbp * (FSRL_MAX_ACT + FSRL_DOW));
    HIPCHK(m.regrow(k.mbp, mbp, mbp, {Mem::D(&k.ws, floats * 4)}));
    HIPCHK(hipMemsetAsync(k.ws, 0, floats * 4, c->compute));
    float* p = k.ws;
    for (int net = 0; net < nn; ++net)
        for (int l = 0; l < L; ++l) {
            k.act[net][l] = p; p += (size_t)mbp * round_up(k.w[l], 4);
            k.dz[net][l] = p; p += (size_t)mbp * round_up(k.w[l], 4);
        }
    k.out = p; p += (size_t)nn * mbp * FSRL_MAX_ACT;
    k.dout = p;
    return 0;
}

struct LayState : LayWork {
    Mem mem;                            // owns ws, gsq, rws, gvec, inf (c->statp stays the context's)
    float* gsq = nullptr; int nparts = 0; dim3 wgrid{1, 1, 1};
    // trust-region extras (host_trust.inc): tangents of the actor's activations / their gradients (R-operator), and a
    // parameter-layout vector the weight-side launch writes a gradient / a Hessian-vector product into
    bool rop = false;
    float* rws = nullptr;
    float* ract[FSRL_MAX_HIDDEN] = {nullptr};
    float* rdz[FSRL_MAX_HIDDEN] = {nullptr};
    float* rout = nullptr;              // [mbp][FSRL_MAX_ACT]
    float* rdout = nullptr;             // [mbp][FSRL_DOW]
    float* gvec = nullptr;              // [LAY_KSPLIT_MAX][n_dev] split-K partials of the weight-side launch, zero between the tensors for ever
    int gparts = 1;                     // partials the last lay_wgrad(..., split) wrote
    // whole-batch inference working set (process_fn, recompute_advantage, the collector's actor)
    float* inf = nullptr; size_t inf_floats = 0;
};

static void lay_free(fsrl_ctx* c) {
    if (!c->lay) return;
    c->lay->mem.release_all();
    delete c->lay;
    c->lay = nullptr;
}

// flat layout = torch parameters() order (oracle/layout.py): per network [sigma_param] W1 b1 ... W{L+1} b{L+1}; on the device
// every tensor starts 256-byte aligned, rows dense (no padded units: these kernels take ragged shapes)
static void lay_build_layout(fsrl_ctx* c, const int* widths, int L) {
    LayState* ls = new LayState();
    c->lay = ls;
    ls->L = L;
    for (int l = 0; l < L; ++l) { ls->w[l] = widths[l]; ls->hmax = std::max(ls->hmax, widths[l]); }
    const int Do = c->cfg.obs_dim, Da = c->cfg.act_dim, nn = 1 + c->cfg.n_critics;
    LayModel& lm = ls->lm;
    lm.Do = Do; lm.Da = Da; lm.n_nets = nn; lm.unbounded = c->cfg.unbounded ? 1 : 0;
    int api = 0, dev = 0;
    auto add = [&](int rows, int cols) {
        TensorMap t{api, dev, rows, cols, cols};
        c->tmap.push_back(t);
        api += rows * cols;
        dev = round_up(dev + rows * cols, 64);
        return t.dev_off;
    };
    for (int net = 0; net < nn; ++net) {
        LayNet& ln = lm.net[net];
        c->md.net[net].begin = dev;
        ln.sigma = (net == 0) ? add(1, Da) : -1;
        ln.nl = L + 1;
        int in = Do;
        for (int l = 0; l <= L; ++l) {
            const int out = (l < L) ? widths[l] : (net == 0 ? Da : 1);
            ln.l[l].in = in; ln.l[l].out = out;
            ln.l[l].W = add(out, in); ln.l[l].b = add(1, out);
            in = out;
        }
        c->md.net[net].end = dev;
    }
    c->n_api = api;
    c->n_dev = round_up(dev, 1024);
    c->n_alloc = c->n_dev;
    // what the shared kernels read of a ModelDesc: the network count, Da, the actor's sigma_param; H = 0 -> no W2 mirrors
    ModelDesc& md = c->md;
    md.Do = Do; md.Da = Da; md.H = 0; md.n_nets = nn; md.unbounded = lm.unbounded;
    md.net[0].sigma = lm.net[0].sigma;
    // grid of the one weight-gradient launch of a step: jobs = every Linear of every network + the sigma_param column sums
    int gx = 1, gy = 1;
    for (int net = 0; net < nn; ++net)
        for (int l = 0; l <= L; ++l) {
            gx = std::max(gx, (lm.net[net].l[l].in + 63) / 64);
            gy = std::max(gy, (lm.net[net].l[l].out + 63) / 64);
        }
    ls->wgrid = dim3(gx, gy, nn * (L + 1) + 1);
    ls->nparts = gx * gy * (nn * (L + 1) + 1);
}

// working set for `rows` rows (a minibatch of the PPO / FOCOPS step, or the whole batch of the trust-region path); rop: also the
// tangent buffers of the actor
static int lay_ensure_rows(fsrl_ctx* c, int rows, bool rop) {
    LayState* ls = c->lay;
    const int mbp = round_up(std::max(rows, 16), 16);
    if (!ls->gsq) HIPCHK(ls->mem.dev(&ls->gsq, (size_t)ls->nparts * 4));
    const int nn = ls->lm.n_nets, L = ls->L;
    if (mbp > ls->mbp || mbp > c->mbp_max) {      // the second: statp (the context's own block) failed after the working set grew
        HIPCHK(hipStreamSynchronize(c->compute));
        ls->rop = false; c->mbp_max = 0;
        HIPCHK(ls->mem.release(&ls->rws));
        HIPCHK(c->mem.release(&c->statp));
        int rc = lay_work_ensure(c, ls->mem, *ls, mbp);
        if (rc) return rc;
        HIPCHK(c->mem.regrow(c->mbp_max, mbp, mbp, {Mem::D(&c->statp, (size_t)(mbp / 16) * nn * 4 * 4)}));
    }
    if (rop && !ls->rop) {
        HIPCHK(hipStreamSynchronize(c->compute));
        size_t per = 0;
        for (int l = 0; l < L; ++l) per += (size_t)ls->mbp * round_up(ls->w[l], 4);
        const size_t floats = 2 * per + (size_t)ls->mbp * (FSRL_MAX_ACT + FSRL_DOW);
        HIPCHK(ls->mem.regrow(ls->rop, true, true, {Mem::D(&ls->rws, floats * 4)}));
        HIPCHK(hipMemsetAsync(ls->rws, 0, floats * 4, c->compute));
        float* p = ls->rws;
        for (int l = 0; l < L; ++l) {
            ls->ract[l] = p; p += (size_t)ls->mbp * round_up(ls->w[l], 4);
            ls->rdz[l] = p; p += (size_t)ls->mbp * round_up(ls->w[l], 4);
        }
        ls->rout = p; p += (size_t)ls->mbp * FSRL_MAX_ACT;
        ls->rdout = p;
    }
    if (rop && !ls->gvec) {
        HIPCHK(ls->mem.dev(&ls->gvec, (size_t)LAY_KSPLIT_MAX * c->n_dev * 4));
        HIPCHK(hipMemsetAsync(ls->gvec, 0, (size_t)LAY_KSPLIT_MAX * c->n_dev * 4, c->compute));
    }
    return 0;
}
static int lay_ensure_mb(fsrl_ctx* c, int B) { return lay_ensure_rows(c, round_up(2 * B, 16), false); }

// VEC instantiation when every operand row of every job is 16-byte aligned and a multiple of 4 floats long (widths % 4 == 0:
// the usual case); otherwise the dword-load instantiation for the whole launch (e.g. the first layer of an obs_dim 17 network)
static bool lay_vec_ok(const float* p, int ld, int len) {
    return p == nullptr || len <= 0 || (((ld & 3) == 0) && ((len & 3) == 0) && ((reinterpret_cast<uintptr_t>(p) & 15) == 0));
}
template <int FORM>
static int lay_launch(fsrl_ctx* c, const LinJobs& jobs, float* gsq, hipStream_t s, const dim3* grid_fixed = nullptr) {
    int gx = 1, gy = 1;
    bool vec = true;
    for (int j = 0; j < jobs.n; ++j) {
        const LinJob& jb = jobs.j[j];
        gx = std::max(gx, (jb.N + 63) / 64); gy = std::max(gy, (jb.M + 63) / 64);
        // row length of an operand = its contiguous dimension: K for a k-minor operand, M / N for a k-major one
        vec = vec && lay_vec_ok(jb.A, jb.lda, jb.a_len ? jb.a_len : (FORM == LIN_W ? jb.M : jb.K)) && lay_vec_ok(jb.N > 0 ? jb.B : nullptr, jb.ldb, FORM == LIN_F ? jb.K : jb.N);
    }
    const int ks = (FORM == LIN_W && jobs.ksplit > 1) ? jobs.ksplit : 1;
    const dim3 grid = grid_fixed ? *grid_fixed : dim3(gx, gy * ks, jobs.n);
    // active workgroups of the launch: few of them (a minibatch-sized product) -> 16 waves each, so that every SIMD of a CU
    // holds several; many (a full batch) -> 4 waves each with four column tiles per wave (more reuse of a staged fragment)
    long wgs = 0;
    for (int j = 0; j < jobs.n; ++j)
        wgs += (long)std::max(1, (jobs.j[j].N + 63) / 64) * ((jobs.j[j].M + 63) / 64) * ks;
    const int nw = wgs <= 2 * c->n_cus ? 4 : (wgs <= 4 * c->n_cus ? 2 : 1);
#define LAY_GO(V, NW_) hipLaunchKernelGGL((lin_kernel<FORM, V, NW_>), grid, dim3(256 * NW_), 0, s, jobs, gsq)
    if (vec) { if (nw == 4) LAY_GO(true, 4); else if (nw == 2) LAY_GO(true, 2); else LAY_GO(true, 1); }
    else { if (nw == 4) LAY_GO(false, 4); else if (nw == 2) LAY_GO(false, 2); else LAY_GO(false, 1); }
#undef LAY_GO
    HIPCHK(hipGetLastError());

    return 0;
}

// process_fn / recompute_advantage / collector inference: the layered counterpart of mlp_infer_kernel, same job numbering
static int lay_infer(fsrl_ctx* c, const InferArgs& ia, int jobs_y, hipStream_t s) {
    LayState* ls = c->lay;
    const LayModel& lm = ls->lm;
    const int N = ia.N, L = ls->L, C = ia.C;
    if (N <= 0) return 0;
    CHECK_ARG(jobs_y <= LAY_MAX_JOBS, "too many inference jobs");
    const size_t hm = (size_t)round_up(ls->hmax, 4);
    const size_t need = (size_t)jobs_y * N * (2 * hm + FSRL_MAX_ACT);
    if (need > ls->inf_floats) {
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(ls->mem.regrow(ls->inf_floats, need, need, {Mem::D(&ls->inf, need * 4)}));
    }
    float* bufs[2] = {ls->inf, ls->inf + (size_t)jobs_y * N * hm};
    float* outb = ls->inf + 2 * (size_t)jobs_y * N * hm;
    for (int l = 0; l <= L; ++l) {
        LinJobs jobs{};
        jobs.n = jobs_y;
        for (int job = 0; job < jobs_y; ++job) {
            const bool is_actor = (job == 2 * C);
            const int net = is_actor ? 0 : 1 + (C > 0 ? job % C : 0);
            const bool use_next = !is_actor && job >= C;
            const LayLayer& ll = lm.net[net].l[l];
            LinJob& jb = jobs.j[job];
            jb.A = (l == 0) ? (use_next ? ia.obs_next : ia.obs) : bufs[(l - 1) & 1] + (size_t)job * N * hm;
            jb.lda = ll.in;
            jb.B = c->P + ll.W; jb.ldb = ll.in;
            jb.aux = c->P + ll.b; jb.ldaux = 0; jb.bias_out = nullptr;
            jb.M = N; jb.N = ll.out; jb.K = ll.in;
            if (l < L) { jb.C = bufs[l & 1] + (size_t)job * N * hm; jb.ldc = ll.out; jb.relu = 1; }
            else { jb.C = outb + (size_t)job * N * FSRL_MAX_ACT; jb.ldc = FSRL_MAX_ACT; jb.relu = 0; }
        }
        int rc = lay_launch<LIN_F>(c, jobs, nullptr, s);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(lay_infer_out_kernel, dim3((N + 15) / 16, jobs_y), dim3(64), 0, s, outb, c->P, lm.net[0].sigma, lm.Da,
                       lm.unbounded, ia);
    HIPCHK(hipGetLastError());
    return 0;
}

// forward of the networks net0 .. net0 + ny - 1 (ny < 0: all) over the rows X[0 .. rows): hidden layers -> ls->act, heads -> ls->out
static int lay_fwd_k(fsrl_ctx* c, LayWork& k, const float* P, const float* X, int rows, int net0 = 0, int ny = -1, const float* const* Xn = nullptr) {
    LayWork* ls = &k;
    const LayModel& lm = ls->lm;
    const int L = ls->L;
    if (ny < 0) ny = lm.n_nets - net0;
    for (int l = 0; l <= L; ++l) {
        LinJobs jobs{};
        jobs.n = ny;
        for (int y = 0; y < ny; ++y) {
            const int net = net0 + y;
            const LayLayer& ll = lm.net[net].l[l];
            LinJob& jb = jobs.j[y];
            jb.A = (l == 0) ? (Xn ? Xn[y] : X) : ls->act[net][l - 1]; jb.lda = ll.in;      // Xn: one input matrix per network
            jb.B = P + ll.W; jb.ldb = ll.in;
            jb.aux = P + ll.b;
            jb.M = rows; jb.N = ll.out; jb.K = ll.in;
            if (l < L) { jb.C = ls->act[net][l]; jb.ldc = ll.out; jb.relu = 1; }
            else { jb.C = ls->out + (size_t)net * ls->mbp * FSRL_MAX_ACT; jb.ldc = FSRL_MAX_ACT; jb.relu = 0; }
        }
        int rc = lay_launch<LIN_F>(c, jobs, nullptr, c->compute);
        if (rc) return rc;
    }
    return 0;
}
static int lay_fwd(fsrl_ctx* c, const float* X, int rows, int net0 = 0, int ny = -1) { return lay_fwd_k(c, *c->lay, c->P, X, rows, net0, ny); }

// activation side of the backward pass from the head gradients in ls->dout: dZ_l = (dZ_{l+1} W_{l+1}) * relu'(Z_l) layer by layer
// dx_in: also the gradient with respect to the network INPUT (no relu below it), rows x in_dim per network at dx_in[y] -- the
// replay agents' dQ / da
static int lay_bwd_dz_k(fsrl_ctx* c, LayWork& k, const float* P, int rows, int net0 = 0, int ny = -1, float* const* dx_in = nullptr) {
    LayWork* ls = &k;
    const LayModel& lm = ls->lm;
    const int L = ls->L;
    if (ny < 0) ny = lm.n_nets - net0;
    for (int l = L - 1; l >= (dx_in ? -1 : 0); --l) {
        LinJobs jobs{};
        jobs.n = ny;
        for (int y = 0; y < ny; ++y) {
            const int net = net0 + y;
            const LayLayer& up = lm.net[net].l[l + 1];      // the Linear above hidden layer l (the head when l == L - 1)
            LinJob& jb = jobs.j[y];
            if (l == L - 1) { jb.A = ls->dout + (size_t)net * ls->mbp * FSRL_DOW; jb.lda = FSRL_DOW; jb.a_len = 16; }   // zeros past the head width
            else { jb.A = ls->dz[net][l + 1]; jb.lda = up.out; }
            jb.B = P + up.W; jb.ldb = up.in;
            if (l >= 0) { jb.C = ls->dz[net][l]; jb.ldc = up.in; jb.aux = ls->act[net][l]; jb.ldaux = up.in; }
            else { jb.C = dx_in[y]; jb.ldc = up.in; }                   // the input itself: nothing to mask
            jb.M = rows; jb.N = up.in; jb.K = up.out;
        }
        int rc = lay_launch<LIN_X>(c, jobs, nullptr, c->compute);
        if (rc) return rc;
    }
    return 0;
}
static int lay_bwd_dz(fsrl_ctx* c, int rows, int net0 = 0, int ny = -1) { return lay_bwd_dz_k(c, *c->lay, c->P, rows, net0, ny); }

// weight side: every weight / bias (/ sigma_param) gradient of the networks net0 .. net0 + ny - 1 in ONE launch into the
// parameter-layout vector `out`, each workgroup leaving its share of the squared norm in gsq (may be null).  Jobs are ordered
// actor layers, sigma_param, critic layers: the actor's shares come first.  rop: the R-operator form of the actor's products,
// R{dW_l} = R{dz_l}^T a_{l-1} + dz_l^T R{a_{l-1}} (second operand pair), R{db_l} = colsum R{dz_l}.
// split: (full-batch callers) cut the batch rows into ls->gparts ranges of >= 1 024 rows (at most 24), one partial per range at
// out + s * n_dev -- one fp32 chain over 20 000 rows is too long for conjugate gradients to digest, and one workgroup per
// output tile too few
// k-version: any LayWork; Xn: one input matrix per network (the replay agents' Q-networks all read [obs | act], the API allows
// different ones); rop_state: the R-operator buffers (on-policy actor only); split_stride > 0: split-K partials that far apart.
// The job table holds LAY_MAX_JOBS entries and a network is L + 1 jobs (+ sigma_param): four Q-networks of eight hidden layers
// (SAC-Lag, CVPO with double_critic) are 36.  So the jobs go out in launches of WHOLE networks, as many as fit the table.  Every
// job writes its own slice of `out` from its own operands, one accumulator per element over ascending batch rows whichever
// launch carries it: the split moves no result.  A launch with squared-norm slots or a fixed grid (the on-policy step: slots
// numbered by workgroup of ONE launch) is never split -- fsrl_ctx_create refuses an on-policy context whose table would not fit.
static_assert(FSRL_MAX_HIDDEN + 2 <= LAY_MAX_JOBS, "one network's weight-side jobs (every Linear + sigma_param) fit one launch");
static_assert(FSRL_MAX_NETS <= LAY_MAX_JOBS, "lay_fwd_k / lay_bwd_dz_k: one job per network in a launch");
static int lay_wgrad_k(fsrl_ctx* c, LayWork& k, const float* X, const float* const* Xn, int rows, int net0, int ny, float* out,
                       float* gsq, LayState* rs, int split_stride, int* gparts_out, const dim3* grid_fixed) {
    const LayModel& lm = k.lm;
    const int L = k.L;
    CHECK_ARG(net0 >= 0 && ny >= 1 && net0 + ny <= lm.n_nets && ny <= FSRL_MAX_NETS, "weight-side launch: networks %d .. %d of %d",
              net0, net0 + ny - 1, lm.n_nets);
    LinJobs jobs{};
    int gp = 1;
    if (split_stride > 0) {
        const int ks = std::max(1, std::min(LAY_KSPLIT_MAX, (rows + 1023) / 1024));
        jobs.ksplit = ks; jobs.kchunk = round_up((rows + ks - 1) / ks, 64); jobs.part_stride = split_stride;
        gp = ks;
    }
    if (gparts_out) *gparts_out = gp;
    int nj = 0;
    for (int y = 0; y < ny; ++y) {
        const int net = net0 + y;
        const float* X0 = Xn ? Xn[y] : X;
        const int need = L + 1 + (lm.net[net].sigma >= 0 ? 1 : 0);
        CHECK_ARG(need <= LAY_MAX_JOBS, "too many weight-side jobs: %d for one network (limit %d)", need, LAY_MAX_JOBS);
        if (nj + need > LAY_MAX_JOBS) {     // the table is full: launch the networks gathered so far
            CHECK_ARG(!gsq && !grid_fixed, "too many weight-side jobs for one launch with squared-norm slots (limit %d)", LAY_MAX_JOBS);
            jobs.n = nj;
            int rc = lay_launch<LIN_W>(c, jobs, nullptr, c->compute, nullptr);
            if (rc) return rc;
            for (int j = 0; j < nj; ++j) jobs.j[j] = LinJob{};
            nj = 0;
        }
        for (int l = 0; l <= L; ++l) {
            const LayLayer& ll = lm.net[net].l[l];
            LinJob& jb = jobs.j[nj++];
            const float* dz = (l < L) ? (rs ? rs->rdz[l] : k.dz[net][l]) : (rs ? rs->rdout : k.dout + (size_t)net * k.mbp * FSRL_DOW);
            jb.A = dz; jb.lda = (l < L) ? ll.out : FSRL_DOW; jb.a_len = (l < L) ? 0 : 16;
            jb.B = (l == 0) ? X0 : k.act[net][l - 1]; jb.ldb = ll.in;
            if (rs && l > 0) {
                jb.A2 = (l < L) ? k.dz[net][l] : k.dout + (size_t)net * k.mbp * FSRL_DOW;
                jb.B2 = rs->ract[l - 1];
            }
            jb.C = out + ll.W; jb.ldc = ll.in;
            jb.bias_out = out + ll.b;
            jb.M = ll.out; jb.N = ll.in; jb.K = rows;
        }
        if (lm.net[net].sigma >= 0) {   // d / d sigma_param: the column sums of the second half of the actor's head-gradient rows
            LinJob& jb = jobs.j[nj++];
            jb.A = (rs ? rs->rdout : k.dout + (size_t)net * k.mbp * FSRL_DOW) + 16; jb.lda = FSRL_DOW; jb.a_len = 16;
            jb.B = X0; jb.ldb = lm.net[net].l[0].in; jb.C = out; jb.ldc = 0;
            jb.bias_out = out + lm.net[net].sigma;
            jb.M = lm.Da; jb.N = 0; jb.K = rows;
        }
    }
    jobs.n = nj;
    return lay_launch<LIN_W>(c, jobs, gsq, c->compute, grid_fixed);
}
// the on-policy context's own networks.  rop: the R-operator form of the actor's products, R{dW_l} = R{dz_l}^T a_{l-1} +
// dz_l^T R{a_{l-1}} (second operand pair), R{db_l} = colsum R{dz_l}.  split: (full-batch callers) cut the batch rows into
// ls->gparts ranges of >= 1 024 rows (at most 24), one partial per range at out + s * n_dev -- one fp32 chain over 20 000 rows
// is too long for conjugate gradients to digest, and one workgroup per output tile too few
static int lay_wgrad(fsrl_ctx* c, const float* X, int rows, int net0, int ny, float* out, float* gsq, bool rop = false,
                     bool split = false) {
    LayState* ls = c->lay;
    const bool all = (net0 == 0 && ny == ls->lm.n_nets && !split);
    ls->gparts = 1;
    return lay_wgrad_k(c, *ls, X, nullptr, rows, net0, ny, out, gsq, rop ? ls : nullptr, split ? c->n_dev : 0, &ls->gparts,
                       all ? &ls->wgrid : nullptr);
}
static int lay_bwd(fsrl_ctx* c, const float* X, int rows) {
    int rc = lay_bwd_dz(c, rows);
    if (rc) return rc;
    return lay_wgrad(c, X, rows, 0, c->lay->lm.n_nets, c->G, c->lay->gsq);
}

// Hessian-vector product of the mean KL on the actor (cpo.py:169-182; the R-operator of fb_hvp_body, kernels_fb.hpp, layer by
// layer): tangent V (parameter layout) -> ls->gvec.  cached: ls->act / ls->out / ls->dz / ls->dout of network 0 already hold
// the forward pass and the first-order KL backward at the current theta, batch and old distribution.
static int lay_hvp(fsrl_ctx* c, const float* X, const float* rd, int rows, const float* V, float max_action, bool cached) {
    LayState* ls = c->lay;
    const LayModel& lm = ls->lm;
    const LayNet& an = lm.net[0];
    const int L = ls->L;
    hipStream_t s = c->compute;
    int rc;
    if (!cached) { rc = lay_fwd(c, X, rows, 0, 1); if (rc) return rc; }
    // ---- R-forward: R{z_l} = a_{l-1} V_l^T + v_b + R{a_{l-1}} W_l^T ; R{a_l} = R{z_l} * relu'(z_l) ; R{a_{-1}} = 0
    for (int l = 0; l <= L; ++l) {
        const LayLayer& ll = an.l[l];
        float* C = (l < L) ? ls->ract[l] : ls->rout;
        const int ldc = (l < L) ? ll.out : FSRL_MAX_ACT;
        const float* mask = (l < L) ? ls->act[0][l] : nullptr;
        {
            LinJobs jobs{}; jobs.n = 1;
            LinJob& jb = jobs.j[0];
            jb.A = (l == 0) ? X : ls->act[0][l - 1]; jb.lda = ll.in;
            jb.B = V + ll.W; jb.ldb = ll.in; jb.aux = V + ll.b;
            jb.C = C; jb.ldc = ldc; jb.M = rows; jb.N = ll.out; jb.K = ll.in;
            if (l == 0) { jb.mask = mask; jb.ldmask = ll.out; }
            rc = lay_launch<LIN_F>(c, jobs, nullptr, s);
            if (rc) return rc;
        }
        if (l > 0) {
            LinJobs jobs{}; jobs.n = 1;
            LinJob& jb = jobs.j[0];
            jb.A = ls->ract[l - 1]; jb.lda = ll.in;
            jb.B = c->P + ll.W; jb.ldb = ll.in;
            jb.acc = C; jb.ldacc = ldc; jb.mask = mask; jb.ldmask = ll.out;
            jb.C = C; jb.ldc = ldc; jb.M = rows; jb.N = ll.out; jb.K = ll.in;
            rc = lay_launch<LIN_F>(c, jobs, nullptr, s);
            if (rc) return rc;
        }
    }
    {
        LayHvpHeadArgs h{};
        h.out = ls->out; h.rout = ls->rout; h.dout = ls->dout; h.rdout = ls->rdout; h.rd = rd; h.P = c->P; h.V = V;
        h.sigma = an.sigma; h.Da = lm.Da; h.unbounded = lm.unbounded; h.N = rows; h.max_action = max_action;
        hipLaunchKernelGGL(lay_hvp_head_kernel, dim3((rows + 15) / 16), dim3(256), 0, s, h);
        HIPCHK(hipGetLastError());
    }
    if (!cached) { rc = lay_bwd_dz(c, rows, 0, 1); if (rc) return rc; }      // first-order dz_l of the KL (theta only)
    // ---- R-backward: R{dz_l} = (R{dz_{l+1}} W_{l+1} + dz_{l+1} V_{l+1}) * relu'(z_l)   (relu'' = 0)
    for (int l = L - 1; l >= 0; --l) {
        const LayLayer& up = an.l[l + 1];
        const bool top = (l == L - 1);
        {
            LinJobs jobs{}; jobs.n = 1;
            LinJob& jb = jobs.j[0];
            jb.A = top ? ls->rdout : ls->rdz[l + 1]; jb.lda = top ? FSRL_DOW : up.out; jb.a_len = top ? 16 : 0;
            jb.B = c->P + up.W; jb.ldb = up.in;
            jb.C = ls->rdz[l]; jb.ldc = up.in; jb.M = rows; jb.N = up.in; jb.K = up.out;
            rc = lay_launch<LIN_X>(c, jobs, nullptr, s);
            if (rc) return rc;
        }
        {
            LinJobs jobs{}; jobs.n = 1;
            LinJob& jb = jobs.j[0];
            jb.A = top ? ls->dout : ls->dz[0][l + 1]; jb.lda = top ? FSRL_DOW : up.out; jb.a_len = top ? 16 : 0;
            jb.B = V + up.W; jb.ldb = up.in;
            jb.acc = ls->rdz[l]; jb.ldacc = up.in; jb.aux = ls->act[0][l]; jb.ldaux = up.in;
            jb.C = ls->rdz[l]; jb.ldc = up.in; jb.M = rows; jb.N = up.in; jb.K = up.out;
            rc = lay_launch<LIN_X>(c, jobs, nullptr, s);
            if (rc) return rc;
        }
    }
    return lay_wgrad(c, X, rows, 0, 1, ls->gvec, nullptr, true, true);
}

// the minibatch steps of one pass (fsrl_ppo_pass after ppo_pass_prepare): ppo_lag.py:222-250 per minibatch
static int lay_ppo_steps(fsrl_ctx* c) {
    LayState* ls = c->lay;
    const LayModel& lm = ls->lm;
    const int nn = lm.n_nets, Do = lm.Do;
    hipStream_t s = c->compute;
    const int nmb = (int)c->mb_start.size();
    WgradPtrs wp{};
    wp.statp = c->statp; wp.stats = c->d_stats; wp.ctrl = c->ctrl; wp.P = c->P; wp.grad = c->G; wp.mbp_max = ls->mbp;
    PpoStepArgs sa = ppo_base_args(c);
    sa.fuse_adam = 0;
    sa.iters_in_pass = nmb;
    for (int mb = 0; mb < nmb; ++mb) {
        sa.mb_start = c->mb_start[mb]; sa.mb_size = c->mb_size[mb]; sa.mb_index = mb;
        sa.step = (int)c->n_steps + mb;
        sa.first_in_pass = (mb == 0); sa.last_in_pass = (mb == nmb - 1);
        c->adam_t += 1;
        const AdamStep as = adam_step(c->cfg.lr, c->cfg.beta1, c->cfg.beta2, c->adam_t);
        sa.step_size = as.step_size; sa.bc2_sqrt = as.bc2_sqrt;
        const int rows = sa.mb_size, tiles = (rows + 15) / 16;
        const float* X = c->obs_p + (size_t)sa.mb_start * Do;
        int rc = lay_fwd(c, X, rows);
        if (rc) return rc;
        {
            LayHeadArgs h{};
            h.out = ls->out; h.dout = ls->dout; h.rd = c->rd_p; h.statp = c->statp; h.P = c->P; h.sigma = lm.net[0].sigma;
            h.mbp = ls->mbp; h.n_nets = nn; h.Da = lm.Da; h.unbounded = lm.unbounded;
            hipLaunchKernelGGL(lay_ppo_head_kernel, dim3(tiles, nn), dim3(256), 0, s, h, sa);
            HIPCHK(hipGetLastError());
        }
        rc = lay_bwd(c, X, rows);
        if (rc) return rc;
        hipLaunchKernelGGL(ppo_stats_kernel, dim3(1), dim3(64), 0, s, c->md, wp, sa, tiles);
        hipLaunchKernelGGL(adam_clip_kernel, dim3((c->n_dev + 4 * ADAM_NT - 1) / (4 * ADAM_NT)), dim3(ADAM_NT), 0, s, c->P, c->M,
                           c->V, c->G, ls->gsq, ls->nparts, c->n_dev, sa, c->ctrl, c->md);
        HIPCHK(hipGetLastError());
    }
    return 0;
}
