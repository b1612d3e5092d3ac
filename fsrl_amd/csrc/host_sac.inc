// host_sac.inc -- SAC- / DDPG-Lagrangian on the replay store: fsrl_sac_* (part of fsrl_hip.hip).
// Included once by fsrl_hip.hip: same translation unit, so the static helpers and fsrl_ctx above are visible.
// ====================================================================================== SAC-Lagrangian
#include "kernels_sac.hpp"
#include "kernels_cvpo.hpp"
#include "kernels_layered_sac.hpp"

struct SacState {
    fsrl_sac_config cfg{};
    Mem mem;                                   // every block of this state, the alternate batch set, the CVPO fields and ka / kq's working sets
    ModelDesc mda{}, mdq{};
    std::vector<TensorMap> tmap_a, tmap_q;     // API order -> device offsets
    int na_api = 0, nq_api = 0, na_dev = 0, nq_dev = 0;
    float *PA = nullptr, *MA = nullptr, *VA = nullptr;          // gradients live in the split-K partial buffers
    float *PQ = nullptr, *PQT = nullptr, *MQ = nullptr, *VQ = nullptr;
    float* PAT = nullptr;                      // target actor (DDPG-Lag mode only)
    int n_q = 4;                               // Q-networks: 4 (two double critics) or 2 (DDPG-Lag)
    bool plan_nofold = false;                  // fsrl_sac_set_plan bit 4: sample + gather as ONE launch of their own (round 4) instead of inside the actors' forward launch
    bool plan_separate = false;                // fsrl_sac_set_plan bit 1: sample and gather as launches of their own
    bool plan_nstep_sep = false;               // fsrl_sac_set_plan bit 2: the n-step targets as a launch of their own
    bool ddpg = false;
    int mean_tanh = 0;          // the Gaussian actor's mean: 1 = max_action * tanh(head), 0 = the head (cfg.actor_mean / ccfg.actor_mean resolved)
    SacScalars* sc = nullptr;
    int64_t t_actor = 0, t_critic = 0;
    // per-batch buffers
    int cap_B = 0, n_tiles = 0;               // n_tiles = 16-row tiles of the batch
    bool q_rows4 = false, a_rows4 = false;    // 4-row tile variants for the Q / actor launches
    int *d_idx = nullptr, *d_chain = nullptr; uint8_t* d_end = nullptr;
    int *h_idx = nullptr, *h_chain = nullptr; uint8_t* h_end = nullptr;          // pinned
    float *XQ = nullptr, *OBS = nullptr, *OBSN = nullptr, *XN = nullptr, *XP = nullptr;
    float *eps_t = nullptr, *eps_p = nullptr, *h_eps = nullptr;                   // device / pinned
    // the NEXT update's sample: while update u runs, sample + gather of update u + 1 (same Philox counters it would use, same store)
    // run on the side stream into this second set of batch buffers; update u + 1 swaps the sets if nothing that determines the
    // sample changed in between (store contents, batch size, key, update count) and draws again otherwise.  Takes the 9 us
    // launch off the update's critical path and is bit-identical -- and was measured SLOWER (152.7 vs 147.3 us per update on the
    // same box: two event waits per update and a second stream's kernel among the update's cost more than the launch they
    // hide), so it is OFF unless fsrl_sac_set_plan bit 3 asks for it.
    struct Alt { int *d_idx = nullptr, *d_chain = nullptr; uint8_t* d_end = nullptr;
                 float *XQ = nullptr, *OBS = nullptr, *OBSN = nullptr, *XN = nullptr, *XP = nullptr, *eps_t = nullptr, *eps_p = nullptr; } alt;
    bool plan_prefetch = false, pre_valid = false;      // off by default: measured slower (152.7 vs 147.3 us per update, same box)
    // r6: the same second set is filled IN-STREAM by rider blocks of the actor's weight-gradient launch (100 workgroups on 256 CUs:
    // kernels_sample.hpp SgRider) -- no second stream, no events; the next update's first launch is then the actors' forward alone.
    // On by default where that launch is fb_wgrad_kernel (batches above 512 rows); fsrl_sac_set_plan bit 5 switches it off.
    bool plan_noxcd = false;                            // fsrl_sac_set_plan bit 6: the critics' weight-gradient launch in plain block order (A/B)
    bool plan_norider = false, pre_side = false;        // pre_side: the valid prefetch came from the side stream (wait for pre_done)
    uint64_t pre_store_version = 0, pre_key = 0; int64_t pre_counter = -1; int pre_B = 0;
    hipEvent_t pre_done = nullptr, upd_done = nullptr, book_done = nullptr;
    float *LPN = nullptr, *LP = nullptr, *QT = nullptr, *QP = nullptr, *Y = nullptr, *DA = nullptr;
    float *A1 = nullptr, *A2 = nullptr, *D1 = nullptr, *D2 = nullptr, *DO = nullptr;   // [4][Bpad]
    float *stq = nullptr, *stdin_ = nullptr, *stpi = nullptr;   // stdin_: per-tile scratch of the Q_DIN launch (unused sums)
    float* gsq_scratch = nullptr;             // per-block squared-norm slots ppo_wgrad_kernel writes (unused by the replay agents)
    bool wgrad_splitk = false;                // fsrl_sac_set_plan(ctx, 1): split-K weight gradients at every batch size (A/B, tests)
    float* d_stats = nullptr;                 // ring [SAC_RING][FSRL_SAC_NSTATS]: one row per update
    int64_t n_updates = 0, n_drained = 0;
    uint64_t key = 0x243F6A8885A308D3ull;     // Philox key of the library-RNG mode
    SacBook* d_book = nullptr; SacBook* h_book = nullptr;      // device / pinned sub-buffer bookkeeping
    uint64_t book_version = 0;
    int last_B = 0;
    int nstats = FSRL_SAC_NSTATS_K;           // floats per row of the statistics ring
    // ---- CVPO mode (fsrl_cvpo_init): Gaussian actor + actor_old (PAT), E-step / M-step state
    bool cvpo = false;
    fsrl_cvpo_config ccfg{};
    CvpoScalars* csc = nullptr;
    int n_tiles_k = 0; bool k_rows4 = false;  // tiles of the K*B particle launch
    float *MU_OLD = nullptr, *STD_OLD = nullptr, *XK = nullptr, *QK = nullptr, *q0 = nullptr, *q1 = nullptr;
    float *Wk = nullptr, *eps_k = nullptr, *h_epsk = nullptr, *stqk = nullptr;
    // ---- layered context (hidden_sizes of another depth / width, host_layered.inc): the actor and the Q-networks as LayWork sets,
    //      parameter-layout gradient vectors the weight-side launch fills, the Q-networks' input gradients
    bool layered = false;
    LayWork ka, kq;
    float *GA = nullptr, *GQ = nullptr, *DXQ = nullptr;
};
static constexpr int SAC_RING = 4096;

static SacState* sac_of(fsrl_ctx* c) { return reinterpret_cast<SacState*>(c->sac); }
static SacSampleArgs sac_sample_args(const fsrl_ctx* c, const SacState* s, int B, int n_step, int64_t stored, int64_t counter);
#include "host_per.inc"

// layered layout: dense tensors (no padded units, no W2 mirror), device order = the networks one after the other; the API orders
// are the fused layout's (actor: preprocess, mu head, sigma head; critics per DoubleCritic: pre1 pre2 last1 last2)
static void sac_layout_layered(fsrl_ctx* c, SacState* s) {
    const int Do = c->cfg.obs_dim, Da = c->cfg.act_dim, Din = Do + Da;
    const LayState* base = c->lay;
    const int L = base->L;
    auto init_work = [&](LayWork& k, int in_dim, int n_nets, int out) {
        k.L = L; k.hmax = base->hmax;
        for (int l = 0; l < L; ++l) k.w[l] = base->w[l];
        k.lm.Do = in_dim; k.lm.Da = Da; k.lm.n_nets = n_nets; k.lm.unbounded = 0;
        int dev = 0;
        for (int n = 0; n < n_nets; ++n) {
            LayNet& ln = k.lm.net[n];
            ln.sigma = -1; ln.nl = L + 1;
            int in = in_dim;
            for (int l = 0; l <= L; ++l) {
                const int o = (l < L) ? base->w[l] : out;
                ln.l[l].in = in; ln.l[l].out = o;
                ln.l[l].W = dev; dev = round_up(dev + o * in, 64);
                ln.l[l].b = dev; dev = round_up(dev + o, 64);
                in = o;
            }
        }
        return round_up(dev, 1024);
    };
    const int heads = s->ddpg ? 1 : 2;
    s->na_dev = init_work(s->ka, Do, 1, heads * Da);
    s->nq_dev = init_work(s->kq, Din, s->n_q, 1);
    // ModelDesc stubs for the shared Adam kernels: H = 0 -> no mirrors
    s->mda = ModelDesc{}; s->mda.Do = Do; s->mda.Da = Da; s->mda.H = 0; s->mda.n_nets = 1; s->mda.net[0].sigma = -1;
    s->mda.net[0].begin = 0; s->mda.net[0].end = s->na_dev; s->mda.net[0].out = heads * Da;
    s->mdq = ModelDesc{}; s->mdq.Do = Din; s->mdq.Da = Da; s->mdq.H = 0; s->mdq.n_nets = s->n_q;
    int api = 0;
    auto add = [&](std::vector<TensorMap>& tm, int dev_off, int rows, int cols) { tm.push_back(TensorMap{api, dev_off, rows, cols, cols}); api += rows * cols; };
    {
        const LayNet& an = s->ka.lm.net[0];
        for (int l = 0; l < L; ++l) { add(s->tmap_a, an.l[l].W, an.l[l].out, an.l[l].in); add(s->tmap_a, an.l[l].b, 1, an.l[l].out); }
        const LayLayer& hd = an.l[L];                 // device head = [Wmu ; Wsig], [bmu ; bsig]
        add(s->tmap_a, hd.W, Da, hd.in); add(s->tmap_a, hd.b, 1, Da);
        if (!s->ddpg) { add(s->tmap_a, hd.W + Da * hd.in, Da, hd.in); add(s->tmap_a, hd.b + Da, 1, Da); }
        s->na_api = api;
    }
    api = 0;
    auto pre = [&](const LayNet& ln) { for (int l = 0; l < L; ++l) { add(s->tmap_q, ln.l[l].W, ln.l[l].out, ln.l[l].in); add(s->tmap_q, ln.l[l].b, 1, ln.l[l].out); } };
    auto last = [&](const LayNet& ln) { add(s->tmap_q, ln.l[L].W, 1, ln.l[L].in); add(s->tmap_q, ln.l[L].b, 1, 1); };
    for (int i = 0; i < 2 && s->n_q == 4; ++i) {
        for (int j = 0; j < 2; ++j) pre(s->kq.lm.net[2 * i + j]);
        for (int j = 0; j < 2; ++j) last(s->kq.lm.net[2 * i + j]);
    }
    for (int i = 0; i < 2 && s->n_q == 2; ++i) { pre(s->kq.lm.net[i]); last(s->kq.lm.net[i]); }
    s->nq_api = api;
    for (int n = 0; n < s->n_q; ++n) {
        s->mdq.net[n].sigma = -1; s->mdq.net[n].out = 1;
        s->mdq.net[n].begin = s->kq.lm.net[n].l[0].W;
        s->mdq.net[n].end = (n + 1 < s->n_q) ? s->kq.lm.net[n + 1].l[0].W : s->nq_dev;
    }
    s->layered = true;
}

static void sac_layout(fsrl_ctx* c, SacState* s) {
    if (c->lay) { sac_layout_layered(c, s); return; }
    const int Do = c->cfg.obs_dim, Da = c->cfg.act_dim, H = c->cfg.hidden, Din = Do + Da;
    // ---- actor: device W3 = [Wmu ; Wsig], b3 = [bmu ; bsig]
    {
        ModelDesc& md = s->mda;
        md.Do = Do; md.Da = Da; md.H = H; md.n_nets = 1;
        int dev = 0, api = 0;
        auto place = [&](int n) { int o = dev; dev = round_up(dev + n, 64); return o; };
        NetOff& no = md.net[0];
        no.sigma = -1; no.out = 2 * Da; no.begin = 0;
        no.W1 = place(H * Do); no.b1 = place(H); no.W2 = place(H * H); no.b2 = place(H);
        const int heads = s->ddpg ? 1 : 2;                        // DDPG-Lag: the mean head only
        no.out = heads * Da;
        no.W3 = place(heads * Da * H); no.b3 = place(heads * Da);
        no.end = dev;
        const int h1 = c->h1, h2 = c->h2;                        // the caller's layer widths (zero-padded to H on the device)
        auto add = [&](int dev_off, int rows, int cols, int ld) { s->tmap_a.push_back(TensorMap{api, dev_off, rows, cols, ld}); api += rows * cols; };
        add(no.W1, h1, Do, Do); add(no.b1, 1, h1, H); add(no.W2, h2, h1, H); add(no.b2, 1, h2, H);
        add(no.W3, Da, h2, H); add(no.b3, 1, Da, Da);            // mu head
        if (!s->ddpg) { add(no.W3 + Da * H, Da, h2, H); add(no.b3 + Da, 1, Da, Da); }   // sigma head
        s->na_api = api; s->na_dev = round_up(dev, 1024);
        no.W2f = s->na_dev;                                       // forward-fragment mirror behind the main vector
    }
    // ---- four Q-nets: device order Qr1, Qr2, Qc1, Qc2 ; API order per DoubleCritic: pre1 pre2 last1 last2
    {
        ModelDesc& md = s->mdq;
        md.Do = Din; md.Da = Da; md.H = H; md.n_nets = s->n_q;
        int dev = 0;
        auto place = [&](int n) { int o = dev; dev = round_up(dev + n, 64); return o; };
        for (int n = 0; n < s->n_q; ++n) {
            NetOff& no = md.net[n];
            no.sigma = -1; no.out = 1; no.begin = dev;
            no.W1 = place(H * Din); no.b1 = place(H); no.W2 = place(H * H); no.b2 = place(H);
            no.W3 = place(H); no.b3 = place(1);
            no.end = dev;
        }
        int api = 0;
        const int h1 = c->h1, h2 = c->h2;
        auto add = [&](int dev_off, int rows, int cols, int ld) { s->tmap_q.push_back(TensorMap{api, dev_off, rows, cols, ld}); api += rows * cols; };
        auto pre = [&](const NetOff& no) { add(no.W1, h1, Din, Din); add(no.b1, 1, h1, H); add(no.W2, h2, h1, H); add(no.b2, 1, h2, H); };
        auto last = [&](const NetOff& no) { add(no.W3, 1, h2, H); add(no.b3, 1, 1, 1); };
        for (int i = 0; i < 2 && s->n_q == 4; ++i) {
            for (int j = 0; j < 2; ++j) pre(md.net[2 * i + j]);
            for (int j = 0; j < 2; ++j) last(md.net[2 * i + j]);
        }
        for (int i = 0; i < 2 && s->n_q == 2; ++i) {     // tianshou Critic / SingleCritic: preprocess MLP then the last layer
            pre(md.net[i]); last(md.net[i]);
        }
        s->nq_api = api; s->nq_dev = round_up(dev, 1024);
        for (int n = 0; n < s->n_q; ++n) md.net[n].W2f = s->nq_dev + n * H * H;
    }
}

// bytes of the actor's / the Q-networks' parameter store with its W2 mirrors (used in P only; none in a layered context: hidden = 0)
static size_t sac_actor_bytes(const fsrl_ctx* c, const SacState* s) { return ((size_t)s->na_dev + (size_t)c->cfg.hidden * c->cfg.hidden) * 4; }
static size_t sac_critic_bytes(const fsrl_ctx* c, const SacState* s) { return ((size_t)s->nq_dev + 4 * (size_t)c->cfg.hidden * c->cfg.hidden) * 4; }

// what fsrl_sac_init and fsrl_cvpo_init allocate alike once the kind (ddpg, n_q, nstats) is set: the layout, the parameter, target
// and Adam stores (zeroed on the compute stream: the caller waits for it), a layered context's gradient vectors, the scalars, the
// statistics ring and the sampler's books
static int sac_alloc_state(fsrl_ctx* c, SacState* s) {
    sac_layout(c, s);
    const size_t ab = sac_actor_bytes(c, s), qb = sac_critic_bytes(c, s);
    for (float** p : {&s->PA, &s->MA, &s->VA, &s->PAT}) { HIPCHK(s->mem.dev(p, ab)); HIPCHK(hipMemsetAsync(*p, 0, ab, c->compute)); }
    for (float** p : {&s->PQ, &s->PQT, &s->MQ, &s->VQ}) { HIPCHK(s->mem.dev(p, qb)); HIPCHK(hipMemsetAsync(*p, 0, qb, c->compute)); }
    if (s->layered) {           // parameter-layout gradient vectors of the layered weight-side launches
        HIPCHK(s->mem.dev(&s->GA, (size_t)s->na_dev * 4)); HIPCHK(hipMemsetAsync(s->GA, 0, (size_t)s->na_dev * 4, c->compute));
        HIPCHK(s->mem.dev(&s->GQ, (size_t)s->nq_dev * 4)); HIPCHK(hipMemsetAsync(s->GQ, 0, (size_t)s->nq_dev * 4, c->compute));
    }
    HIPCHK(s->mem.dev(&s->sc, sizeof(SacScalars)));
    HIPCHK(s->mem.dev(&s->d_stats, (size_t)SAC_RING * s->nstats * 4));
    HIPCHK(s->mem.dev(&s->d_book, (size_t)c->cfg.env_num * sizeof(SacBook)));
    HIPCHK(s->mem.pinned(&s->h_book, (size_t)c->cfg.env_num * sizeof(SacBook)));
    return 0;
}

extern "C" int fsrl_sac_init(fsrl_ctx* c, const fsrl_sac_config* cfg) {
    CHECK_ARG(c && cfg, "null argument");
    CHECK_ARG(c->cfg.algo == FSRL_ALGO_SAC_LAG, "context was not created with FSRL_ALGO_SAC_LAG");
    CHECK_ARG(cfg->deterministic ? c->cfg.act_dim <= 16 : c->cfg.act_dim <= 8,
              "the actor head has at most 16 outputs (act_dim <= 8 for SAC, <= 16 for DDPG)");
    CHECK_ARG(c->cfg.obs_dim + c->cfg.act_dim <= FSRL_MAX_OBS, "obs_dim + act_dim too large");
    CHECK_ARG(cfg->n_step >= 1 && cfg->n_step <= 8, "n_step must be in [1, 8]");
    CHECK_ARG(cfg->tau >= 0.0f && cfg->tau <= 1.0f, "tau should be in [0, 1]");
    CHECK_ARG(cfg->actor_mean >= FSRL_ACTOR_MEAN_DEFAULT && cfg->actor_mean <= FSRL_ACTOR_MEAN_TANH,
              "actor_mean must be 0 (default), 1 (unbounded) or 2 (max_action * tanh), got %d", cfg->actor_mean);
    CHECK_ARG(!(cfg->deterministic && cfg->actor_mean != FSRL_ACTOR_MEAN_DEFAULT),
              "actor_mean %d: the deterministic (DDPG-Lagrangian) actor has no such option, pass 0", cfg->actor_mean);
    ENTER_DEV(c);
    if (c->sac) sac_free(c);
    SacState* s = new SacState();
    c->sac = s;
    s->cfg = *cfg;
    s->ddpg = cfg->deterministic != 0;
    s->mean_tanh = cfg->actor_mean == FSRL_ACTOR_MEAN_TANH ? 1 : 0;       // SAC-Lag's default: the unbounded mean
    s->n_q = s->ddpg ? 2 : 4;
    if (s->ddpg) { s->cfg.auto_alpha = 0; s->cfg.alpha = 0.0f; }      // no entropy term anywhere
    const int rc = sac_alloc_state(c, s);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->compute));
    SacScalars init{cfg->auto_alpha ? 1.0f : cfg->alpha, 0.0f, 0.0f, 0.0f, 0, 0};
    HIPCHK(hipMemcpy(s->sc, &init, sizeof(init), hipMemcpyHostToDevice));
    return 0;
}

static void sac_free(fsrl_ctx* c) {
    SacState* s = sac_of(c);
    if (!s) return;
    s->mem.release_all();
    if (s->pre_done) (void)hipEventDestroy(s->pre_done);
    if (s->upd_done) (void)hipEventDestroy(s->upd_done);
    if (s->book_done) (void)hipEventDestroy(s->book_done);
    delete s;
    c->sac = nullptr;
}

extern "C" int64_t fsrl_sac_param_count(const fsrl_ctx* c, int32_t which) {
    if (!c || !c->sac) return 0;
    const SacState* s = reinterpret_cast<const SacState*>(c->sac);
    return which == 0 ? s->na_api : s->nq_api;
}

static int sac_copy(fsrl_ctx* c, const std::vector<TensorMap>& tm, const ModelDesc& md, int n_dev, float* dev,
                    const float* in, float* out) {
    const size_t n_alloc = (size_t)n_dev + (size_t)md.n_nets * md.H * md.H;
    std::vector<float> tmp(in ? n_alloc : (size_t)n_dev, 0.0f);
    HIPCHK(hipStreamSynchronize(c->compute));
    if (in) {
        for (const TensorMap& t : tm) t.to_dev(tmp.data(), in);
        fill_mirrors(md, tmp);
        HIPCHK(hipMemcpy(dev, tmp.data(), tmp.size() * 4, hipMemcpyHostToDevice));
    } else {
        HIPCHK(hipMemcpy(tmp.data(), dev, tmp.size() * 4, hipMemcpyDeviceToHost));
        for (const TensorMap& t : tm) t.to_api(out, tmp.data());
    }
    return 0;
}

extern "C" int fsrl_sac_params_set(fsrl_ctx* c, const float* actor, int64_t na, const float* critics, int64_t nc,
                                   float log_alpha) {
    CHECK_ARG(c && actor && critics, "null argument");
    SacState* s = sac_of(c);
    if (!s) return fail(FSRL_ESTATE, "fsrl_sac_init first");
    CHECK_ARG(na == s->na_api && nc == s->nq_api, "expected %d actor / %d critic parameters", s->na_api, s->nq_api);
    ENTER_DEV(c);
    int rc = sac_copy(c, s->tmap_a, s->mda, s->na_dev, s->PA, actor, nullptr);
    if (rc) return rc;
    rc = sac_copy(c, s->tmap_q, s->mdq, s->nq_dev, s->PQ, critics, nullptr);
    if (rc) return rc;
    HIPCHK(hipMemcpy(s->PQT, s->PQ, sac_critic_bytes(c, s), hipMemcpyDeviceToDevice));    // critics_old = deepcopy (with the W2 mirrors)
    HIPCHK(hipMemcpy(s->PAT, s->PA, sac_actor_bytes(c, s), hipMemcpyDeviceToDevice));     // actor_old = deepcopy (DDPG-Lag)
    for (float* p : {s->MA, s->VA}) HIPCHK(hipMemsetAsync(p, 0, (size_t)s->na_dev * 4, c->compute));
    for (float* p : {s->MQ, s->VQ}) HIPCHK(hipMemsetAsync(p, 0, (size_t)s->nq_dev * 4, c->compute));
    HIPCHK(hipStreamSynchronize(c->compute));
    s->t_actor = s->t_critic = 0;
    SacScalars init{s->cfg.auto_alpha ? std::exp(log_alpha) : s->cfg.alpha, log_alpha, 0.0f, 0.0f, 0, 0};
    HIPCHK(hipMemcpy(s->sc, &init, sizeof(init), hipMemcpyHostToDevice));
    return 0;
}

// Overwrite ONE parameter set (checkpoint load): which = 0 actor, 1 critics, 2 critics_old, 3 actor_old.
// Unlike fsrl_sac_params_set nothing else changes (targets, Adam moments, step counts stay).
extern "C" int fsrl_sac_params_put(fsrl_ctx* c, int32_t which, const float* in, int64_t n) {
    CHECK_ARG(c && in, "null argument");
    SacState* s = sac_of(c);
    if (!s) return fail(FSRL_ESTATE, "fsrl_sac_init first");
    CHECK_ARG(which >= 0 && which <= 3, "which must be 0..3");
    CHECK_ARG(which != 3 || s->ddpg || s->cvpo, "actor_old exists in the DDPG-Lagrangian and CVPO modes only");
    ENTER_DEV(c);
    if (which == 0 || which == 3) {
        CHECK_ARG(n == s->na_api, "expected %d actor parameters", s->na_api);
        return sac_copy(c, s->tmap_a, s->mda, s->na_dev, which == 0 ? s->PA : s->PAT, in, nullptr);
    }
    CHECK_ARG(n == s->nq_api, "expected %d critic parameters", s->nq_api);
    return sac_copy(c, s->tmap_q, s->mdq, s->nq_dev, which == 1 ? s->PQ : s->PQT, in, nullptr);
}

extern "C" int fsrl_sac_params_get(fsrl_ctx* c, int32_t which, float* out, int64_t n, float* alpha_out) {
    CHECK_ARG(c && out, "null argument");
    SacState* s = sac_of(c);
    if (!s) return fail(FSRL_ESTATE, "fsrl_sac_init first");
    ENTER_DEV(c);
    int rc;
    if (which == 0 || which == 3) {
        CHECK_ARG(n == s->na_api, "bad size");
        rc = sac_copy(c, s->tmap_a, s->mda, s->na_dev, which == 0 ? s->PA : s->PAT, nullptr, out);
    }
    else { CHECK_ARG(n == s->nq_api, "bad size"); rc = sac_copy(c, s->tmap_q, s->mdq, s->nq_dev, which == 1 ? s->PQ : s->PQT, nullptr, out); }
    if (rc) return rc;
    if (alpha_out) {
        SacScalars sc;
        HIPCHK(hipMemcpy(&sc, s->sc, sizeof(sc), hipMemcpyDeviceToHost));
        *alpha_out = s->cfg.auto_alpha ? sc.alpha : s->cfg.alpha;
    }
    return 0;
}

static int sac_alloc_batch(fsrl_ctx* c, SacState* s, int B) {
    s->n_tiles = (B + 15) / 16;
    s->q_rows4 = !s->layered && 4 * s->n_tiles * s->n_q <= c->n_cus && !c->probe_tile16;
    s->a_rows4 = !s->layered && 4 * s->n_tiles <= c->n_cus && !c->probe_tile16;
    if (s->cvpo) {
        s->n_tiles_k = (B * s->ccfg.sample_act_num + 15) / 16;
        s->k_rows4 = !s->layered && 4 * s->n_tiles_k * s->n_q <= c->n_cus && !c->probe_tile16;
    }
    if (B <= s->cap_B) return 0;
    HIPCHK(hipStreamSynchronize(c->compute));
    HIPCHK(hipStreamSynchronize(c->side));
    s->pre_valid = false;
    if (!s->pre_done) { HIPCHK(hipEventCreateWithFlags(&s->pre_done, hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&s->upd_done, hipEventDisableTiming));
                        HIPCHK(hipEventCreateWithFlags(&s->book_done, hipEventDisableTiming)); }
    const int Do = c->cfg.obs_dim, Da = c->cfg.act_dim, Din = Do + Da, H = c->cfg.hidden, ns = s->cfg.n_step;
    const size_t Bp = (size_t)s->n_tiles * 16 + 64;
    s->cap_B = 0;               // until the whole set stands: also over the layered working sets and DXQ
    if (s->layered) {
        int rc = lay_work_ensure(c, s->mem, s->ka, (int)Bp);
        if (rc) return rc;
        rc = lay_work_ensure(c, s->mem, s->kq, s->cvpo ? (int)(Bp * s->ccfg.sample_act_num) : (int)Bp);      // CVPO: the K x B particle rows of the E-step
        if (rc) return rc;
        HIPCHK(s->mem.release(&s->DXQ));
        HIPCHK(s->mem.dev(&s->DXQ, (size_t)s->n_q * s->kq.mbp * Din * 4));
    }
    // device buffers are zero-filled below; at least 16 bytes: a layered context has no tile-kernel slabs (H = 0).  on = false: not in this mode
    auto d = [](auto** p, size_t bytes, bool on = true) { return Mem::D(p, on ? std::max<size_t>(bytes, 16) : 0); };
    const bool cv = s->cvpo;
    const size_t K = cv ? (size_t)s->ccfg.sample_act_num : 0, KB = K * Bp;
    const std::initializer_list<Mem::Req> set = {
        d(&s->d_idx, Bp * 4), d(&s->d_chain, Bp * ns * 4), d(&s->d_end, Bp * ns),
        Mem::H(&s->h_idx, Bp * 4), Mem::H(&s->h_chain, Bp * ns * 4), Mem::H(&s->h_end, Bp * ns), Mem::H(&s->h_eps, Bp * Da * 4 * 2),
        d(&s->XQ, Bp * Din * 4), d(&s->XN, Bp * Din * 4), d(&s->XP, Bp * Din * 4), d(&s->OBS, Bp * Do * 4), d(&s->OBSN, Bp * Do * 4),
        d(&s->eps_t, Bp * Da * 4), d(&s->eps_p, Bp * Da * 4),
        d(&s->alt.d_idx, Bp * 4, !cv), d(&s->alt.d_chain, Bp * ns * 4, !cv), d(&s->alt.d_end, Bp * ns, !cv),
        d(&s->alt.XQ, Bp * Din * 4, !cv), d(&s->alt.XN, Bp * Din * 4, !cv), d(&s->alt.XP, Bp * Din * 4, !cv),
        d(&s->alt.OBS, Bp * Do * 4, !cv), d(&s->alt.OBSN, Bp * Do * 4, !cv), d(&s->alt.eps_t, Bp * Da * 4, !cv), d(&s->alt.eps_p, Bp * Da * 4, !cv),
        d(&s->LPN, Bp * 4), d(&s->LP, Bp * 4), d(&s->QT, 4 * Bp * 4), d(&s->QP, 4 * Bp * 4), d(&s->Y, 2 * Bp * 4), d(&s->DA, 4 * Bp * Da * 4),
        d(&s->A1, 4 * Bp * H * 4), d(&s->A2, 4 * Bp * H * 4), d(&s->D1, 4 * Bp * H * 4), d(&s->D2, 4 * Bp * H * 4), d(&s->DO, 4 * Bp * FSRL_DOW * 4),
        // per-tile partial statistics: room for 4-row tiles (4 x the 16-row tile count); stpi: two batches in the merged forward launch
        d(&s->stq, (size_t)(4 * s->n_tiles + 4) * 4 * FB_NSTAT * 4), d(&s->stdin_, (size_t)(4 * s->n_tiles + 4) * 4 * FB_NSTAT * 4),
        d(&s->stpi, (size_t)(8 * s->n_tiles + 8) * FB_NSTAT * 4),
        d(&s->MU_OLD, Bp * Da * 4, cv), d(&s->STD_OLD, Bp * Da * 4, cv), d(&s->XK, KB * Din * 4, cv), d(&s->QK, 4 * KB * 4, cv),
        d(&s->q0, KB * 4, cv), d(&s->q1, KB * 4, cv), d(&s->Wk, KB * 4, cv), d(&s->eps_k, KB * Da * 4, cv), Mem::H(&s->h_epsk, KB * Da * 4),
        d(&s->stqk, (size_t)(4 * ((KB + 15) / 16) + 4) * 4 * FB_NSTAT * 4, cv)};
    HIPCHK(s->mem.regrow(s->cap_B, B, B, set));
    for (const Mem::Req& r : set) if (!r.pin && r.bytes) HIPCHK(hipMemsetAsync(*r.field, 0, r.bytes, c->compute));
    return 0;
}

// tianshou ReplayBuffer.next inside the owning sub-buffer
static inline int64_t store_next(const fsrl_ctx* c, int64_t idx) {
    const int64_t e = idx / c->sub_size, local = idx % c->sub_size;
    const EnvBook& eb = c->env[(size_t)e];
    const bool end = c->h_flags[(size_t)idx] != 0 || local == eb.last_index;
    if (end || eb.size == 0) return idx;
    return e * c->sub_size + (local + 1) % eb.size;
}
static inline bool store_end_flag(const fsrl_ctx* c, int64_t idx) {
    if (c->h_flags[(size_t)idx] != 0) return true;
    const int64_t e = idx / c->sub_size, local = idx % c->sub_size;
    const EnvBook& eb = c->env[(size_t)e];
    return eb.size > 0 && local == (eb.index - 1 + eb.size) % eb.size;   // unfinished tail
}

// ---- the arguments of one update's launches.  fsrl_sac_update, fsrl_cvpo_update and the grouped updates (host_sac_group.inc,
//      host_cvpo_group.inc) all form them here, so a member of a group cannot be handed anything its own update would not be.
// library RNG: the sample of update `counter`
static SacSampleArgs sac_sample_args(const fsrl_ctx* c, const SacState* s, int B, int n_step, int64_t stored, int64_t counter) {
    SacSampleArgs sa{};
    sa.book = s->d_book; sa.flags = c->st.flags; sa.idx = s->d_idx; sa.chain = s->d_chain; sa.endbits = s->d_end;
    sa.eps_t = s->eps_t; sa.eps_p = s->eps_p; sa.env_num = c->cfg.env_num; sa.sub_size = (int)c->sub_size; sa.B = B;
    sa.n_step = n_step; sa.Da = c->cfg.act_dim; sa.stored = (unsigned long long)stored; sa.key = s->key;
    sa.counter = (unsigned long long)counter;
    return sa;
}
static SacGatherArgs sac_gather_args(const fsrl_ctx* c, const SacState* s, int B, int n_step) {
    SacGatherArgs ga{};
    ga.st = c->st; ga.idx = s->d_idx; ga.term = s->d_chain + (size_t)(n_step - 1) * B; ga.XQ = s->XQ; ga.OBS = s->OBS;
    ga.OBSN = s->OBSN; ga.XN = s->XN; ga.XP = s->XP; ga.B = B; ga.Do = c->cfg.obs_dim; ga.Da = c->cfg.act_dim;
    return ga;
}
// what the actor's forward and backward launches share; the caller adds the second batch, tiles_half and the folded sample
static SacActorArgs sac_actor_args(const fsrl_ctx* c, const SacState* s, int B, int mode, const float* obs, const float* eps, float* X,
                                   float* lp, float resc, float lam, int deterministic, int probe) {
    SacActorArgs aa{};
    aa.deterministic = deterministic; aa.max_action = c->cfg.max_action; aa.mean_tanh = s->mean_tanh;
    aa.obs = obs; aa.eps = eps; aa.X = X; aa.lp_out = lp; aa.DA = s->DA; aa.QP = s->QP; aa.sc = s->sc; aa.A1 = s->A1; aa.A2 = s->A2;
    aa.cr = -resc; aa.cc = s->cfg.use_lagrangian ? resc * lam : 0.0f;
    aa.D1 = s->D1; aa.D2 = s->D2; aa.DO = s->DO; aa.statp = s->stpi; aa.B = B; aa.mode = mode; aa.rescale = resc;
    aa.auto_alpha = s->cfg.auto_alpha; aa.alpha_fixed = s->cfg.alpha;
    aa.probe = probe;
    return aa;
}
// the head of a layered actor pass (lay_sac_actor_head_kernel behind lay_fwd_k): sac_actor_args' selections
static LaySacActorArgs lay_sac_actor_head_args(const fsrl_ctx* c, const SacState* s, int B, int mode, const float* eps, float* X,
                                               float* lp, float resc, float lam) {
    LaySacActorArgs h{};
    h.out = s->ka.out; h.dout = s->ka.dout; h.eps = eps; h.X = X; h.lp = lp; h.DXQ = s->DXQ; h.QP = s->QP; h.sc = s->sc;
    h.statp = s->stpi; h.B = B; h.Bq = s->kq.mbp; h.Do = c->cfg.obs_dim; h.Da = c->cfg.act_dim; h.mode = mode;
    h.deterministic = s->ddpg ? 1 : 0; h.auto_alpha = s->cfg.auto_alpha; h.max_action = c->cfg.max_action; h.mean_tanh = s->mean_tanh;
    h.cr = -resc; h.cc = s->cfg.use_lagrangian ? resc * lam : 0.0f; h.rescale = resc; h.alpha_fixed = s->cfg.alpha;
    return h;
}
static SacNstepArgs sac_nstep_args(const fsrl_ctx* c, const SacState* s, int B) {
    SacNstepArgs na{};
    na.QT = s->QT; na.lpn = s->LPN; na.chain = s->d_chain; na.endbits = s->d_end; na.rew = c->st.rew; na.cost = c->st.cost;
    na.flags = c->st.flags; na.sc = s->sc; na.Y = s->Y; na.B = B; na.n_step = s->cfg.n_step; na.gamma = c->cfg.gamma;
    na.auto_alpha = s->cfg.auto_alpha; na.alpha_fixed = s->cfg.alpha; na.single = s->ddpg ? 1 : 0;
    return na;
}
// the logged-row block of the actor's Adam pass; n_tiles_q / n_tiles_pi: the tiles whose partial statistics it adds up
static SacFinalArgs sac_final_args(const fsrl_ctx* c, const SacState* s, int B, float resc, float lam, int n_tiles_q, int n_tiles_pi,
                                   float* stats_row) {
    SacFinalArgs fa{};
    fa.statp_q = s->stq; fa.statp_pi = s->stpi; fa.sc = s->sc; fa.stats = stats_row;
    fa.n_tiles_q = n_tiles_q; fa.n_tiles_pi = n_tiles_pi; fa.B = B; fa.rescale = resc; fa.lam = lam;
    fa.target_entropy = s->cfg.target_entropy;
    fa.alpha_lr = s->cfg.alpha_lr; fa.beta1 = c->cfg.beta1; fa.beta2 = c->cfg.beta2; fa.adam_eps = c->cfg.adam_eps;
    fa.alpha_fixed = s->cfg.alpha; fa.auto_alpha = s->cfg.auto_alpha; fa.use_lagrangian = s->cfg.use_lagrangian;
    fa.n_q = s->n_q;
    return fa;
}

// the sampler's sub-buffer books (size, index, last_index per environment): uploaded again once the store has changed.  The
// pre_valid / book_done steps belong to the SAC contexts' prefetched samples.  On a CVPO context pre_valid is never set (only
// fsrl_sac_update sets it, and it refuses CVPO contexts), so the wait and the reset do nothing there, and book_done, which only
// the side-stream prefetch waits on, is not recorded.
static int sac_upload_book(fsrl_ctx* c, SacState* s) {
    if (s->book_version == c->store_version) return 0;
    hipStream_t st = c->compute;
    HIPCHK(hipStreamSynchronize(st));           // h_book may still be in flight
    if (s->pre_valid && s->pre_side) HIPCHK(hipEventSynchronize(s->pre_done));   // a prefetched sample still reads d_book
    s->pre_valid = false;                       // (rider blocks ran on `st`: done)
    for (int e = 0; e < c->cfg.env_num; ++e) {
        const EnvBook& eb = c->env[(size_t)e];
        s->h_book[e] = SacBook{(int)eb.size, (int)eb.index, (int)eb.last_index, 0};
    }
    HIPCHK(hipMemcpyAsync(s->d_book, s->h_book, (size_t)c->cfg.env_num * sizeof(SacBook), hipMemcpyHostToDevice, st));
    if (s->book_done && s->plan_prefetch && !s->cvpo) HIPCHK(hipEventRecord(s->book_done, st));
    s->book_version = c->store_version;
    return 0;
}

// caller-provided sample (parity mode): the index chains on the host, staged through pinned memory with the target noise; behind
// them the update's second noise block, n2 floats through its pinned buffer h2 to d2 (SAC: the policy's, behind the target's in
// h_eps, to eps_p; CVPO: the particles', through h_epsk to eps_k)
static int sac_stage_indices(fsrl_ctx* c, SacState* s, int B, const int64_t* indices, const float* eps_target, const float* eps2,
                             size_t n2, float* h2, float* d2) {
    hipStream_t st = c->compute;
    const int Da = c->cfg.act_dim, ns = s->cfg.n_step;
    HIPCHK(hipStreamSynchronize(st));      // pinned staging of the previous update has landed
    for (int b = 0; b < B; ++b) {
        const int64_t idx = indices[b];
        CHECK_ARG(idx >= 0 && idx < c->maxsize, "index %lld out of range", (long long)idx);
        s->h_idx[b] = (int)idx;
        int64_t cur = idx;
        for (int n = 0; n < ns; ++n) {      // indices[n] = buffer.next(indices[n-1])
            if (n > 0) cur = store_next(c, cur);
            s->h_chain[(size_t)n * B + b] = (int)cur;
            s->h_end[(size_t)n * B + b] = store_end_flag(c, cur) ? 1 : 0;
        }
    }
    memcpy(s->h_eps, eps_target, (size_t)B * Da * 4);
    HIPCHK(hipMemcpyAsync(s->d_idx, s->h_idx, (size_t)B * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(s->d_chain, s->h_chain, (size_t)B * ns * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(s->d_end, s->h_end, (size_t)B * ns, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(s->eps_t, s->h_eps, (size_t)B * Da * 4, hipMemcpyHostToDevice, st));
    memcpy(h2, eps2, n2 * 4);
    HIPCHK(hipMemcpyAsync(d2, h2, n2 * 4, hipMemcpyHostToDevice, st));
    return 0;
}

// where a Q-network launch leaves its values: the target networks' forward in QT, every other launch in QP, unless the caller names
// the place (the K * B particle rows of CVPO's E-step: QK)
static float* sac_q_out(const SacState* s, const float* params, int mode, float* qout_override) {
    return qout_override ? qout_override : ((mode == FB_MODE_Q_FWD && params == s->PQT) ? s->QT : s->QP);
}
// the arguments of a Q-network tile launch of n_tiles 16-row groups (sac_q_launch; the grouped updates)
static FbArgs sac_q_args(const fsrl_ctx* c, const SacState* s, const float* params, const float* X, int mode, float cr, float cc,
                         float* statp, int B, float* qout_override, int n_tiles, const SacNstepArgs* ns) {
    FbArgs a{};
    a.obs = X; a.rd = nullptr; a.A1 = s->A1; a.A2 = s->A2; a.D1 = s->D1; a.D2 = s->D2; a.DO = s->DO; a.statp = statp;
    a.N = B; a.rows_pad = n_tiles * 16; a.mode = mode; a.net0 = 0; a.cr = cr; a.cc = cc; a.max_action = 1.0f;
    a.tgt = s->Y; a.qout = sac_q_out(s, params, mode, qout_override); a.qin = s->QP; a.da_out = s->DA;
    a.act_cols = c->cfg.act_dim; a.pair_shift = s->n_q == 2 ? 0 : 1;
    if (ns) { a.ns_on = 1; a.ns = *ns; }          // Q_TRAIN: the tile launch computes its n-step targets itself
    if (c->per && mode == FB_MODE_Q_TRAIN) a.wgt = c->per->w;      // prioritised replay: the rows' importance weights
    return a;
}
// the head of a layered Q-network pass (lay_sac_q_head_kernel behind lay_fwd_k over the B rows of `params`' networks)
static LaySacQArgs lay_sac_q_head_args(const fsrl_ctx* c, const SacState* s, int mode, float* statp, int B, float* qout_override,
                                       const float* params) {
    LaySacQArgs qa{};
    qa.out = s->kq.out; qa.dout = s->kq.dout; qa.tgt = s->Y; qa.statp = statp; qa.B = B; qa.mbp = s->kq.mbp; qa.n_q = s->n_q;
    qa.mode = mode; qa.pair_shift = s->n_q == 2 ? 0 : 1;
    qa.qout = sac_q_out(s, params, mode, qout_override);
    if (c->per && mode == FB_MODE_Q_TRAIN) qa.wgt = c->per->w;
    return qa;
}

// qout_override / n_tiles / rows4: the K*B particle launch of CVPO's E-step (forward only) reuses the Q-net kernel
static int sac_q_launch(fsrl_ctx* c, SacState* s, const float* params, const float* X, int mode, float cr, float cc,
                        float* statp, int B, float* qout_override = nullptr, int n_tiles = -1, int rows4 = -1,
                        const SacNstepArgs* ns = nullptr) {
    if (s->layered) {
        // forward of every Q-network on X, the Q head of the mode, and for the training / input-gradient modes the activation
        // side of the backward pass (Q_DIN: down to the input, dQ / d[obs | act] per network in s->DXQ)
        int rc = lay_fwd_k(c, s->kq, params, X, B);
        if (rc) return rc;
        const LaySacQArgs qa = lay_sac_q_head_args(c, s, mode, statp, B, qout_override, params);
        hipLaunchKernelGGL(lay_sac_q_head_kernel, dim3((B + 15) / 16, s->n_q), dim3(64), 0, c->compute, qa);
        HIPCHK(hipGetLastError());
        if (mode == FB_MODE_Q_FWD) return 0;
        if (mode == FB_MODE_Q_TRAIN) return lay_bwd_dz_k(c, s->kq, params, B);
        float* dx[FSRL_MAX_NETS];
        for (int n = 0; n < s->n_q; ++n) dx[n] = s->DXQ + (size_t)n * s->kq.mbp * (c->cfg.obs_dim + c->cfg.act_dim);
        return lay_bwd_dz_k(c, s->kq, params, B, 0, -1, dx);
    }
    if (n_tiles < 0) n_tiles = s->n_tiles;
    const bool r4 = rows4 < 0 ? s->q_rows4 : rows4 != 0;
    FbArgs a = sac_q_args(c, s, params, X, mode, cr, cc, statp, B, qout_override, n_tiles, ns);
#ifdef FSRL_PROBES
    { static const char* e = getenv("FSRL_QTILE_PROBE"); if (e) a.eta = (float)atoi(e); }      // kernels_fb.hpp FBT_PROBE (results invalid)
#endif
    return dispatch_H(c->cfg.hidden, [&](auto hc) {
        constexpr int H = decltype(hc)::value;
        // 4-row tiles while they still fit the chip in one round (batch <= 256 for the four Q-nets)
        if (r4) hipLaunchKernelGGL((fb_tile_kernel<H, 4>), dim3(4 * n_tiles, s->n_q), dim3(4 * H), 0, c->compute, params, s->mdq, a);
        else hipLaunchKernelGGL((fb_tile_kernel<H, 16>), dim3(n_tiles, s->n_q), dim3(4 * H), 0, c->compute, params, s->mdq, a);
        HIPCHK(hipGetLastError());
        return 0;
    });
}

// the split-K weight-gradient operands of the first `ny` networks behind a tile launch over X (sac_wgrad; the grouped updates)
static FbWgradArgs sac_wgrad_args(const fsrl_ctx* c, const SacState* s, int ny, const float* X, int B) {
    FbWgradArgs wa{};
    const size_t rp = (size_t)s->n_tiles * 16;
    wgrad_fill_nets(wa, ny, 0, (size_t)c->cfg.hidden, rp, s->A1, s->A2, s->D1, s->D2, s->DO);
    wa.obs = X; wa.rows = (int)rp; wa.N = B;
    return wa;
}
// ... and of batches of up to 512 padded rows (rp), where ppo_wgrad_body writes the final gradient into G (no `stats`: the extra
// block only reduces db3)
static WgradPtrs sac_wgrad_small_args(const SacState* s, int rp, const float* X, float* G) {
    WgradPtrs w{};
    w.A1 = s->A1; w.A2 = s->A2; w.D1 = s->D1; w.D2 = s->D2; w.DO = s->DO; w.X = X; w.grad = G;
    w.gsq_part = s->gsq_scratch; w.mbp_max = rp;
    return w;
}

// weight gradients of `ny` networks of `md` as split-K partials in c->wg_parts (stride = n_dev)
static int sac_wgrad(fsrl_ctx* c, SacState* s, const ModelDesc& md, int ny, const float* X, int n_dev, int B, int* nsplit,
                     SgRider* rider = nullptr, bool* rode = nullptr) {
    if (rode) *rode = false;
    if (s->layered) {           // one launch writes the finished gradient of the actor / of all Q-networks
        const bool actor = (&md == &s->mda);
        LayWork& k = actor ? s->ka : s->kq;
        float* G = actor ? s->GA : s->GQ;
        int rc = lay_wgrad_k(c, k, X, nullptr, B, 0, ny, G, nullptr, nullptr, 0, nullptr, nullptr);
        if (rc) return rc;
        c->wg_parts = G;
        *nsplit = 1;
        return 0;
    }
    const size_t rp = (size_t)s->n_tiles * 16;
    if (rp <= 512 && !s->wgrad_splitk) {
        // Batches of up to 512 rows (the replay agents' default 256): the PPO step's weight-gradient kernel -- one workgroup per
        // 32 x 32 output tile, all rows, 16-way split-K over its waves -- writes the FINAL gradient where the Adam kernels expect
        // the first (only) partial.  One launch of ~7 us instead of split-K over workgroups (12-15 us at these sizes) and
        // nothing for the Adam kernel to add up.
        int rc = ensure_parts(c, n_dev, 1);
        if (rc) return rc;
        if (!s->gsq_scratch) HIPCHK(s->mem.dev(&s->gsq_scratch, (size_t)wg_grid(256, FSRL_MAX_NETS) * 4));
        const WgradPtrs wp = sac_wgrad_small_args(s, (int)rp, X, c->wg_parts);
        *nsplit = 1;
        const PpoStepArgs none{};
        ModelDesc mdy = md;
        mdy.n_nets = ny;                                          // the launch covers the first ny networks of `md`
        return dispatch_H(c->cfg.hidden, [&](auto hc) {
            constexpr int HH = decltype(hc)::value;
            hipLaunchKernelGGL((ppo_wgrad_kernel<HH, false, false>), dim3(wg_grid(HH, ny)), dim3(1024), 0, c->compute, mdy, wp, (int)rp, none, 0);
            HIPCHK(hipGetLastError());
            return 0;
        });
    }
    FbWgradArgs wa = sac_wgrad_args(c, s, ny, X, B);
    // the critics' launch (four networks x 25 blocks x 2 splits) in XCD-aware block order: the blocks of one (network, split) -- which
    // stream the same rows -- behind one L2.  Same sums, same time (127.6 / 127.9 us per update), 46 -> 20 MB of memory-side traffic per launch;
    // the actor's launch keeps the 3-D grid its rider blocks extend
    return wgrad_launch<false>(c, md, wa, ny, n_dev, nsplit, rider, rode, (ny > 1 && !rider && !s->plan_noxcd) ? 1 : -1);
}
extern "C" int fsrl_sac_set_plan(fsrl_ctx* c, int32_t plan) {
    CHECK_ARG(c, "null ctx");
    CHECK_ARG(plan >= 0 && plan <= 127, "plan: bit 0 = split-K weight gradients at every batch size, bit 1 = separate sample / gather launches, bit 2 = separate n-step launch, bit 3 = prefetch the next update's sample on the side stream, bit 4 = sample + gather as a launch of their own, bit 5 = no rider blocks (the next update's sample inside the actor's weight-gradient launch), bit 6 = the critics' weight-gradient launch in plain block order");
    if (!c->sac) return fail(FSRL_ESTATE, "fsrl_sac_init / fsrl_cvpo_init first");
    sac_of(c)->wgrad_splitk = (plan & 1) != 0;
    sac_of(c)->plan_separate = (plan & 2) != 0;
    sac_of(c)->plan_nstep_sep = (plan & 4) != 0;
    sac_of(c)->plan_prefetch = (plan & 8) != 0;
    sac_of(c)->plan_nofold = (plan & 16) != 0;
    sac_of(c)->plan_norider = (plan & 32) != 0;
    sac_of(c)->plan_noxcd = (plan & 64) != 0;
    sac_of(c)->pre_valid = false;
    ENTER_DEV(c);
    HIPCHK(hipStreamSynchronize(c->compute));      // the events of the side-stream plan are only recorded while it is on: start it from an idle stream
    return 0;
}

// Adam with the gradient read as the z-ordered sum of `nparts` split-K partials
// tgt != NULL: the Polyak update of the target copy rides on the same pass (target <- tau * new + (1 - tau) * target)
static void adam_launch(fsrl_ctx* c, const ModelDesc& md, float* P, float* M, float* V, const float* G, int n, float lr,
                        int64_t t, int nparts, int stride, float* tgt = nullptr, float tau = 0.0f) {
    const double b1 = c->cfg.beta1, b2 = c->cfg.beta2;
    const AdamStep as = adam_step(lr, c->cfg.beta1, c->cfg.beta2, t);
    hipLaunchKernelGGL(adam_range_kernel, dim3((n + 255) / 256), dim3(256), 0, c->compute, P, M, V, G, 0, n, 0.0f,
                       (float)(1.0 - b1), c->cfg.beta2, (float)(1.0 - b2), as.step_size,
                       as.bc2_sqrt, c->cfg.adam_eps, nparts, stride, md, (const float*)nullptr, 0, 0.0f,
                       (float*)nullptr, tgt, tau, (float)(1.0 - (double)tau));
}

// the update's LAST Adam pass, with the logged-row block riding along (adam_final_kernel)
template <class FinalArgs, void (*FINAL)(const FinalArgs&, int)>
static void adam_final_launch(fsrl_ctx* c, const ModelDesc& md, float* P, float* M, float* V, const float* G, int n, float lr,
                              int64_t t, int nparts, int stride, float* tgt, float tau, const FinalArgs& fa) {
    const double b1 = c->cfg.beta1, b2 = c->cfg.beta2;
    const AdamStep as = adam_step(lr, c->cfg.beta1, c->cfg.beta2, t);
    hipLaunchKernelGGL((adam_final_kernel<FinalArgs, FINAL>), dim3((n + 255) / 256 + 1), dim3(256), 0, c->compute, P, M, V, G, n,
                       (float)(1.0 - b1), c->cfg.beta2, (float)(1.0 - b2), as.step_size, as.bc2_sqrt,
                       c->cfg.adam_eps, nparts, stride, md, tgt, tau, (float)(1.0 - (double)tau), fa);
}

// the layered actor pass of a SAC-Lag / DDPG-Lag context, layer by layer: the forward and the actor head of the mode; `both`: then,
// as the fused launch's second batch, the current actor on (OBS, eps_p) -> XP, LP; SAC_A_BWD: also the activation side of the
// backward pass
static int lay_sac_actor_pass(fsrl_ctx* c, SacState* s, int B, int mode, const float* PAx, const float* obs, const float* eps, float* X,
                              float* lp, float resc, float lam, bool both) {
    auto one = [&](const float* Pn, const float* obs_, const float* eps_, float* X_, float* lp_) -> int {
        int rc = lay_fwd_k(c, s->ka, Pn, obs_, B);
        if (rc) return rc;
        const LaySacActorArgs h = lay_sac_actor_head_args(c, s, B, mode, eps_, X_, lp_, resc, lam);
        hipLaunchKernelGGL(lay_sac_actor_head_kernel, dim3((B + 15) / 16), dim3(256), 0, c->compute, h);
        HIPCHK(hipGetLastError());
        return 0;
    };
    int rc = one(PAx, obs, eps, X, lp);
    if (rc) return rc;
    if (both) { rc = one(s->PA, s->OBS, s->eps_p, s->XP, s->LP); if (rc) return rc; }
    return mode == SAC_A_BWD ? lay_bwd_dz_k(c, s->ka, PAx, B) : 0;
}

// ---- the frame of one solo replay update, the same for fsrl_sac_update and fsrl_cvpo_update (host_cvpo.inc), beside the grouped
//      frame of host_sac_group.inc: replay_join, the key (replay_seed_key), the caller's sample (sac_stage_indices) or the books
//      (sac_upload_book), the update's own first actor launch, replay_critic_half, the update's own actor side up to its last Adam
//      pass (which writes replay_stats_row), replay_finish.
// the context before an update: its resident actor ends, its pushes land, its batch buffers hold B rows (rgroup_join: a member's)
static int replay_join(fsrl_ctx* c, SacState* s, int B) {
    ENTER_DEV(c);
    const int rc = join_store(c);
    return rc ? rc : sac_alloc_batch(c, s, B);
}
// the Philox key of the library-RNG mode is a hash of the last non-zero seed; a zero seed keeps the key
static void replay_seed_key(SacState* s, uint64_t seed) { if (seed) s->key = seed * 0x9E3779B97F4A7C15ull + 0x243F6A8885A308D3ull; }
// the critic half: target Q-networks on (s_{t+n}, a') -> the float64 n-step return -> the critics' forward + backward -> their weight
// gradients -> one Adam of all Q-networks.  na: the update's n-step arguments (sac_nstep_args / cvpo_nstep_args)
static int replay_critic_half(fsrl_ctx* c, SacState* s, int B, const SacNstepArgs& na, float lr, float tau, int* nsplit) {
    int rc = sac_q_launch(c, s, s->PQT, s->XN, FB_MODE_Q_FWD, 0.f, 0.f, s->stq, B);
    if (rc) return rc;
    // the critics' tile launch computes its float64 targets itself and leaves them in Y for the logged row; the layered Q head reads
    // them from the stand-alone launch, which fsrl_sac_set_plan bit 2 keeps for fused contexts too
    // (a prioritised update keeps the stand-alone launch as well: per_update_kernel reads the targets from Y)
    const bool ns_fold = !s->layered && !s->plan_nstep_sep && !c->per;
    if (!ns_fold) {
        hipLaunchKernelGGL(sac_nstep_kernel, dim3((B + 255) / 256), dim3(256), 0, c->compute, na);
        HIPCHK(hipGetLastError());
    }
    rc = sac_q_launch(c, s, s->PQ, s->XQ, FB_MODE_Q_TRAIN, 0.f, 0.f, s->stq, B, nullptr, -1, -1, ns_fold ? &na : nullptr);
    if (rc) return rc;
    if (c->per) {           // the sampled rows' new priorities from the Q values and targets that launch just used
        rc = per_update_launch(c, s, B);
        if (rc) return rc;
    }
    rc = sac_wgrad(c, s, s->mdq, s->n_q, s->XQ, s->nq_dev, B, nsplit);
    if (rc) return rc;
    s->t_critic += 1;
    // sync_weight (sac_lag.py:132-134, cvpo.py:202-204) is folded into this pass: the critics do not change again within the update
    adam_launch(c, s->mdq, s->PQ, s->MQ, s->VQ, c->wg_parts, s->nq_dev, lr, s->t_critic, *nsplit, s->nq_dev, s->PQT, tau);
    return 0;
}
// the ring row the update's last Adam pass writes
static float* replay_stats_row(const SacState* s) { return s->d_stats + (size_t)(s->n_updates % SAC_RING) * s->nstats; }
// the update is issued: count it, and with stats_out read its row back (n_floats of it) synchronously and mark it drained
static int replay_finish(fsrl_ctx* c, SacState* s, const float* stats_row, float* stats_out, size_t n_floats) {
    s->n_updates += 1;
    if (stats_out) {
        HIPCHK(hipMemcpyAsync(stats_out, stats_row, n_floats * 4, hipMemcpyDeviceToHost, c->compute));
        HIPCHK(hipStreamSynchronize(c->compute));
        s->n_drained = s->n_updates;
    }
    return 0;
}

// the two sets of batch buffers change places (SacState::alt): a prefetched sample becomes this update's
static void sac_swap_sets(SacState* s) {
    std::swap(s->d_idx, s->alt.d_idx); std::swap(s->d_chain, s->alt.d_chain); std::swap(s->d_end, s->alt.d_end);
    std::swap(s->XQ, s->alt.XQ); std::swap(s->OBS, s->alt.OBS); std::swap(s->OBSN, s->alt.OBSN); std::swap(s->XN, s->alt.XN);
    std::swap(s->XP, s->alt.XP); std::swap(s->eps_t, s->alt.eps_t); std::swap(s->eps_p, s->alt.eps_p);
}
// the sample + gather arguments of update n_updates + 1 into the other set, which the builders address through the usual members
static void sac_next_sample_args(const fsrl_ctx* c, SacState* s, int B, int64_t stored, SacSampleArgs& sa, SacGatherArgs& ga) {
    sac_swap_sets(s);
    sa = sac_sample_args(c, s, B, s->cfg.n_step, stored, s->n_updates + 1);
    ga = sac_gather_args(c, s, B, s->cfg.n_step);
    sac_swap_sets(s);                                         // this update's set is back
}
// that sample sits in the other set, drawn on the side stream or by rider blocks; update n_updates + 1 takes it if batch size, store
// version, key and count are still these
static void sac_mark_prefetched(const fsrl_ctx* c, SacState* s, int B, bool side) {
    s->pre_valid = true; s->pre_side = side; s->pre_B = B; s->pre_store_version = c->store_version; s->pre_key = s->key;
    s->pre_counter = s->n_updates + 1;
}

extern "C" int fsrl_sac_update(fsrl_ctx* c, int32_t B, const int64_t* indices, const float* eps_target,
                               const float* eps_pi, uint64_t seed, const double* lagrangians, double rescaling,
                               float* stats_out) {
    CHECK_ARG(c, "null ctx");
    SacState* s = sac_of(c);
    if (!s) return fail(FSRL_ESTATE, "fsrl_sac_init first");
    CHECK_ARG(B >= 1, "batch_size must be >= 1");
    if (s->cvpo) return fail(FSRL_ESTATE, "this context runs CVPO: call fsrl_cvpo_update");
    const int64_t stored = fsrl_store_len(c);
    CHECK_ARG(stored > 0, "empty replay store");
    CHECK_ARG((indices != nullptr) == (eps_target != nullptr) && (indices != nullptr) == (eps_pi != nullptr),
              "indices, eps_target and eps_pi are given together (caller RNG) or all NULL (library RNG)");
    int rc = replay_join(c, s, B);
    if (rc) return rc;
    hipStream_t st = c->compute;
    const int Do = c->cfg.obs_dim, Da = c->cfg.act_dim, ns = s->cfg.n_step;
    replay_seed_key(s, seed);
    bool fused_gather = false;
    bool want_rider = false;                           // r6: the NEXT update's sample + gather inside this update's actor weight-gradient launch
                                                       // (never with prioritised replay: the next sample depends on this update's priorities)
    bool fold = false;                                // r5: sample + gather inside the actors' forward launch
    SacSampleArgs fold_sa{}; SacGatherArgs fold_ga{};
    if (indices) {
        // ---- caller-provided sample (parity mode): the policy's noise goes behind the target's in the pinned block
        rc = sac_stage_indices(c, s, B, indices, eps_target, eps_pi, (size_t)B * Da, s->h_eps + (size_t)B * Da, s->eps_p);
        if (rc) return rc;
        if (c->per) rc = per_sample_launch(c, s, B, false, stored);      // the importance weights of the caller's rows
        if (rc) return rc;
    } else if (c->per) {
        // ---- prioritised replay: the descent of the sum tree, then the plain gather below.  The rider blocks and the side-stream
        // prefetch (want_rider, can_prefetch) draw the NEXT update's sample while this one runs, but the next prioritised sample
        // depends on the priorities this update writes; the fold into the actors' forward launch (fold) draws tile by tile, and
        // weight_norm needs the maximum over the whole batch before the first weight is used.  All three stay off.
        rc = sac_upload_book(c, s);
        if (rc) return rc;
        rc = per_sample_launch(c, s, B, true, stored);
        if (rc) return rc;
        s->pre_valid = false;
    } else {
        // ---- library RNG: everything on the device, nothing to wait for
        rc = sac_upload_book(c, s);
        if (rc) return rc;
        // sample + gather as ONE launch (plan 0); fsrl_sac_set_plan bit 1 keeps the two launches for A/B
        fused_gather = !s->plan_separate;
        const bool can_prefetch = fused_gather && s->plan_prefetch && !s->cvpo;
        want_rider = fused_gather && !can_prefetch && !s->plan_norider && !s->plan_nofold && !s->layered && !s->cvpo && !c->wgrad_xcd;
        const bool hit = fused_gather && s->pre_valid && s->pre_B == B && s->pre_store_version == c->store_version &&
                         s->pre_key == s->key && s->pre_counter == s->n_updates && (s->pre_side ? can_prefetch : want_rider);
        if (hit) {                                            // this update's sample is already in the other buffer set
            sac_swap_sets(s);
            if (s->pre_side) HIPCHK(hipStreamWaitEvent(st, s->pre_done, 0));      // (the riders ran on this stream)
        } else {
            const SacSampleArgs sa = sac_sample_args(c, s, B, ns, stored, s->n_updates);
            const SacGatherArgs ga = sac_gather_args(c, s, B, ns);
            // r5: the fused kernels' forward launch of both actors draws and gathers its own rows (9 launches per update)
            fold = fused_gather && !can_prefetch && !s->plan_nofold && !s->layered && !s->cvpo;
            if (fold) { fold_sa = sa; fold_ga = ga; }
            else if (fused_gather) hipLaunchKernelGGL(sac_sample_gather_kernel, dim3((B + SG_ROWS - 1) / SG_ROWS), dim3(256), 0, st, sa, ga);
            else hipLaunchKernelGGL(sac_sample_kernel, dim3((B + 255) / 256), dim3(256), 0, st, sa);
            HIPCHK(hipGetLastError());
        }
        s->pre_valid = false;
        if (can_prefetch) {
            // the next update's sample into the set this update does NOT use (its last readers: the previous update, whose end
            // upd_done marks), on the side stream -- behind every store flush issued so far, concurrent with this update's kernels
            SacSampleArgs sa{}; SacGatherArgs ga{};
            sac_next_sample_args(c, s, B, stored, sa, ga);
            HIPCHK(hipStreamWaitEvent(c->side, s->upd_done, 0));
            HIPCHK(hipStreamWaitEvent(c->side, s->book_done, 0));     // the sub-buffer bookkeeping this sample reads has landed
            hipLaunchKernelGGL(sac_sample_gather_kernel, dim3((B + SG_ROWS - 1) / SG_ROWS), dim3(256), 0, c->side, sa, ga);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(s->pre_done, c->side));
            sac_mark_prefetched(c, s, B, true);
        }
    }
    s->last_B = B;
    const float lam = (s->cfg.use_lagrangian && lagrangians) ? (float)lagrangians[0] : 0.0f;
    const float resc = (float)rescaling;
    // ---- gather (the caller's indices, or the two-launch plan)
    if (!fused_gather) {
        const SacGatherArgs ga = sac_gather_args(c, s, B, ns);
        hipLaunchKernelGGL(sac_gather_kernel, dim3(std::min(1024, (B * (Do + Da) + 255) / 256)), dim3(256), 0, st, ga);
        HIPCHK(hipGetLastError());
    }
    // ---- target: a', log pi' at s_{t+n} (the target Q-nets and the float64 n-step return: replay_critic_half)
    // `both`: the forward launch also evaluates the current actor on (OBS, eps_p) -> XP, LP as its second batch
    auto actor_launch = [&](const float* obs, const float* eps, float* X, float* lp, int mode, const float* PAx, bool both = false) {
        if (s->layered) return lay_sac_actor_pass(c, s, B, mode, PAx, obs, eps, X, lp, resc, lam, both);
        // probe: c->probe_phase is 0 outside probe builds
        SacActorArgs aa = sac_actor_args(c, s, B, mode, obs, eps, X, lp, resc, lam, s->ddpg ? 1 : 0, c->probe_phase);
        // 4-row tiles while the launch fits the chip in one round; the two-batch forward is twice as many workgroups
        const bool r4 = s->a_rows4 && (!both || 8 * s->n_tiles <= c->n_cus);
        const int tiles = r4 ? 4 * s->n_tiles : s->n_tiles;
        if (both) { aa.P2 = s->PA; aa.obs2 = s->OBS; aa.eps2 = s->eps_p; aa.X2 = s->XP; aa.lp2 = s->LP; aa.tiles_half = tiles; }
        if (both && fold) { aa.sg_on = 1; aa.sa = fold_sa; aa.ga = fold_ga; }
        const int grid = both ? 2 * tiles : tiles;
        return dispatch_H(c->cfg.hidden, [&](auto hc) {
            constexpr int H = decltype(hc)::value;
            if (r4) hipLaunchKernelGGL((sac_actor_tile_kernel<H, 4>), dim3(grid), dim3(4 * H), 0, st, PAx, s->mda, aa);
            else hipLaunchKernelGGL((sac_actor_tile_kernel<H, 16>), dim3(grid), dim3(4 * H), 0, st, PAx, s->mda, aa);
            HIPCHK(hipGetLastError());
            return 0;
        });
    };
    // one launch for both actor forwards of the update: a' ~ pi(s_{t+n}) (DDPG: the target actor) and a ~ pi(s_t) -- the
    // second does not depend on the critic step in between
    rc = actor_launch(s->OBSN, s->eps_t, s->XN, s->LPN, SAC_A_FWD, s->ddpg ? s->PAT : s->PA, true);
    if (rc) return rc;
    // ---- critic step (all four Q-nets, one Adam)
    int nsplit = 1;
    rc = replay_critic_half(c, s, B, sac_nstep_args(c, s, B), s->cfg.critic_lr, s->cfg.tau, &nsplit);
    if (rc) return rc;
    // ---- actor step: a ~ pi(s), Q(s, a) with the UPDATED critics, dL/da, actor backward
    rc = sac_q_launch(c, s, s->PQ, s->XP, FB_MODE_Q_DIN, 0.f, 0.f, s->stdin_, B);   // Q values + unit-seed dQ/da
    if (rc) return rc;
    rc = actor_launch(s->OBS, s->eps_p, s->XP, s->LP, SAC_A_BWD, s->PA);
    if (rc) return rc;
    {
        SgRider rd{};
        bool rode = false;
        if (want_rider) sac_next_sample_args(c, s, B, stored, rd.sa, rd.ga);      // the other set, the next update's Philox counter
        rc = sac_wgrad(c, s, s->mda, 1, s->OBS, s->na_dev, B, &nsplit, want_rider ? &rd : nullptr, &rode);
        if (rc) return rc;
        if (rode) sac_mark_prefetched(c, s, B, false);
    }
    s->t_actor += 1;
    // ---- actor Adam; its extra block does the alpha step + logged stats (reads only what earlier launches wrote)
    float* stats_row = replay_stats_row(s);
    const SacFinalArgs fa = sac_final_args(c, s, B, resc, lam, s->q_rows4 ? 4 * s->n_tiles : s->n_tiles,
                                           s->a_rows4 ? 4 * s->n_tiles : s->n_tiles, stats_row);
    // DDPG-Lag: actor_old <- tau * actor + (1 - tau) * actor_old in the same pass (ddpg_lag.py:120-123)
    adam_final_launch<SacFinalArgs, sac_finalize_row>(c, s->mda, s->PA, s->MA, s->VA, c->wg_parts, s->na_dev, s->cfg.actor_lr,
                                                      s->t_actor, nsplit, s->na_dev, s->ddpg ? s->PAT : nullptr, s->cfg.tau, fa);
    HIPCHK(hipGetLastError());
    if (s->upd_done && s->plan_prefetch) HIPCHK(hipEventRecord(s->upd_done, st));      // side-stream prefetch only: the batch buffers of this update are free from here on
    return replay_finish(c, s, stats_row, stats_out, FSRL_SAC_NSTATS_K);
}
