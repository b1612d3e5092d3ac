// host_train_state.inc -- the full training state of a context as bytes: fsrl_train_state_size / _export / _import / _copy (part of
// fsrl_hip.hip).  Included once by fsrl_hip.hip, last: same translation unit, so every context struct above is visible.
// The byte format, its writer and everything that is checked about a blob live in train_state.hpp (HIP-free, driven by
// tests/host/train_state_sim.cpp); here: WHAT the state of a context is -- one section table -- and the copies.
// ====================================================================================== training state
#include "train_state.hpp"

// One entry per section: (tag, pointer, bytes).  Export, import and copy walk the SAME table -- device entries as D2H, H2D and D2D
// copies, host entries as memcpy from / to a TsHostBuf that ts_gather fills from the context and ts_scatter writes back into it.
// A store column's `bytes` is its row width: its length follows from the sub-buffer books (ts_ranges).
enum TsKind { TS_HOST, TS_DEV, TS_STORE_HOST, TS_STORE_COL };
struct TsSection { uint32_t tag; void* ptr; int64_t bytes; TsKind kind; };
struct TsHostBuf {
    tstate::HostSlots host;
    int64_t geom[2] = {0, 0};                  // sub_size, buffer_num
    std::vector<tstate::BookRow> book;         // [cfg.env_num]
};
static bool ts_is_store(TsKind k) { return k == TS_STORE_HOST || k == TS_STORE_COL; }

static int ts_fingerprint(fsrl_ctx* c, tstate::Fingerprint& fp) {
    using namespace tstate;
    fp = Fingerprint{};
    const SacState* s = sac_of(c);
    if (ctx_is_replay(c) && !s) return fail(FSRL_ESTATE, "training state of a replay context before fsrl_sac_init / fsrl_cvpo_init");
    if (c->cfg.algo == FSRL_ALGO_FOCOPS && !c->foc) return fail(FSRL_ESTATE, "training state of a FOCOPS context before fsrl_focops_init");
    fp.v[F_ALGO] = c->cfg.algo;
    fp.v[F_MODE] = !s ? MODE_ONPOLICY : s->cvpo ? MODE_CVPO : s->ddpg ? MODE_DDPG : MODE_SAC;
    fp.v[F_LAYERED] = c->lay ? 1 : 0;
    fp.v[F_OBS_DIM] = c->cfg.obs_dim; fp.v[F_ACT_DIM] = c->cfg.act_dim; fp.v[F_HIDDEN_PAD] = c->cfg.hidden;
    if (c->lay) {
        fp.v[F_N_HIDDEN] = c->lay->L;
        for (int l = 0; l < c->lay->L && l < MAX_HIDDEN; ++l) fp.v[F_W0 + l] = c->lay->w[l];
    } else {
        fp.v[F_N_HIDDEN] = 2; fp.v[F_W0] = c->h1; fp.v[F_W1] = c->h2;
    }
    fp.v[F_N_CRITICS] = c->cfg.n_critics; fp.v[F_ENV_NUM] = c->cfg.env_num; fp.v[F_STORE_ROWS] = c->alloc_rows;
    fp.v[F_REW_NORM] = c->d_rms ? 1 : 0;
    fp.v[F_N_Q] = s ? s->n_q : 0;
    return 0;
}

// the section table of a context whose fingerprint ts_fingerprint accepted; hb backs the host entries
static void ts_table(fsrl_ctx* c, TsHostBuf& hb, bool with_store, std::vector<TsSection>& t) {
    using namespace tstate;
    t.clear();
    hb.book.resize((size_t)c->cfg.env_num);
    t.push_back({T_HOST, hb.host.s, HOST_BYTES, TS_HOST});
    if (SacState* s = sac_of(c)) {
        const int64_t HH = (int64_t)c->cfg.hidden * c->cfg.hidden;
        const int64_t ab = ((int64_t)s->na_dev + HH) * 4, qb = ((int64_t)s->nq_dev + 4 * HH) * 4;      // parameters with their W2 mirrors
        t.push_back({T_PA, s->PA, ab, TS_DEV}); t.push_back({T_MA, s->MA, (int64_t)s->na_dev * 4, TS_DEV});
        t.push_back({T_VA, s->VA, (int64_t)s->na_dev * 4, TS_DEV}); t.push_back({T_PAT, s->PAT, ab, TS_DEV});
        t.push_back({T_PQ, s->PQ, qb, TS_DEV}); t.push_back({T_PQT, s->PQT, qb, TS_DEV});
        t.push_back({T_MQ, s->MQ, (int64_t)s->nq_dev * 4, TS_DEV}); t.push_back({T_VQ, s->VQ, (int64_t)s->nq_dev * 4, TS_DEV});
        t.push_back({T_SACS, s->sc, (int64_t)sizeof(SacScalars), TS_DEV});
        if (s->cvpo) t.push_back({T_CVPS, s->csc, (int64_t)sizeof(CvpoScalars), TS_DEV});
    } else {                                    // fused and layered on-policy contexts keep the same three vectors
        t.push_back({T_P, c->P, (int64_t)c->n_alloc * 4, TS_DEV});
        t.push_back({T_M, c->M, (int64_t)c->n_dev * 4, TS_DEV}); t.push_back({T_V, c->V, (int64_t)c->n_dev * 4, TS_DEV});
        if (c->d_rms) t.push_back({T_RMS, c->d_rms, (int64_t)(3 * FSRL_MAX_CRITICS * sizeof(double)), TS_DEV});
    }
    if (!with_store) return;
    const int64_t Do = c->cfg.obs_dim, Da = c->cfg.act_dim;
    t.push_back({T_GEOM, hb.geom, 16, TS_STORE_HOST});
    t.push_back({T_BOOK, hb.book.data(), BOOK_ROW_BYTES * (int64_t)c->cfg.env_num, TS_STORE_HOST});
    t.push_back({T_SOBS, c->st.obs, 4 * Do, TS_STORE_COL}); t.push_back({T_SNXT, c->st.obs_next, 4 * Do, TS_STORE_COL});
    t.push_back({T_SACT, c->st.act, 4 * Da, TS_STORE_COL}); t.push_back({T_SREW, c->st.rew, 8, TS_STORE_COL});
    t.push_back({T_SCST, c->st.cost, 8, TS_STORE_COL}); t.push_back({T_SFLG, c->st.flags, 1, TS_STORE_COL});
}

// context -> hb (host work only)
static void ts_gather(fsrl_ctx* c, TsHostBuf& hb) {
    using namespace tstate;
    HostSlots& h = hb.host;
    h = HostSlots{};
    h.put_i(H_ADAM_T, c->adam_t);
    for (int i = 0; i < 4; ++i) { h.s[H_RNG + i] = c->rng[i]; h.s[H_SHUFFLE + i] = c->shuffle_rng[i]; }
    for (int g = 0; g < 3; ++g) h.put_d(H_LR0 + g, (double)std::max(0.0f, fsrl_get_lr(c, g)));       // < 0: the context has no such group
    h.put_i(H_TR_CRITIC_T, tr_critic_steps_taken(c));
    if (const FocState* f = c->foc) {
        h.put_d(H_FOC_NU, f->nu); h.put_d(H_FOC_NU_LOSS, f->nu_loss); h.put_i(H_FOC_T_ACTOR, f->t_actor); h.put_i(H_FOC_T_CRITIC, f->t_critic);
    }
    if (const SacState* s = sac_of(c)) {
        h.put_i(H_SAC_T_ACTOR, s->t_actor); h.put_i(H_SAC_T_CRITIC, s->t_critic); h.put_i(H_SAC_N_UPDATES, s->n_updates);
        h.s[H_SAC_KEY] = s->key;
    }
    hb.geom[0] = c->sub_size; hb.geom[1] = c->active_envs;
    hb.book.resize((size_t)c->cfg.env_num);
    for (size_t e = 0; e < hb.book.size(); ++e) {
        const EnvBook& eb = c->env[e];
        hb.book[e] = BookRow{eb.index, eb.size, eb.last_index, eb.ep_idx, eb.ep_rew, (int64_t)eb.ep_len};
    }
}

// hb -> context (host work only; the blob behind hb has been validated)
static void ts_scatter(fsrl_ctx* c, const TsHostBuf& hb, bool with_store) {
    using namespace tstate;
    const HostSlots& h = hb.host;
    c->adam_t = h.get_i(H_ADAM_T);
    for (int i = 0; i < 4; ++i) { c->rng[i] = h.s[H_RNG + i]; c->shuffle_rng[i] = h.s[H_SHUFFLE + i]; }
    if (c->cfg.algo == FSRL_ALGO_CPO || c->cfg.algo == FSRL_ALGO_TRPO_LAG) tr_of(c)->critic_t = h.get_i(H_TR_CRITIC_T);
    for (int g = 0; g < 3; ++g)
        if (fsrl_get_lr(c, g) >= 0.0f) (void)fsrl_set_lr(c, g, (float)h.get_d(H_LR0 + g));
    if (FocState* f = c->foc) {
        f->nu = h.get_d(H_FOC_NU); f->nu_loss = h.get_d(H_FOC_NU_LOSS); f->t_actor = h.get_i(H_FOC_T_ACTOR); f->t_critic = h.get_i(H_FOC_T_CRITIC);
    }
    if (SacState* s = sac_of(c)) {
        s->t_actor = h.get_i(H_SAC_T_ACTOR); s->t_critic = h.get_i(H_SAC_T_CRITIC); s->n_updates = h.get_i(H_SAC_N_UPDATES);
        s->key = h.s[H_SAC_KEY];
    }
    if (!with_store) return;
    c->sub_size = hb.geom[0]; c->active_envs = (int)hb.geom[1]; c->maxsize = c->sub_size * c->active_envs;
    for (size_t e = 0; e < hb.book.size(); ++e) {
        const BookRow& r = hb.book[e];
        EnvBook eb;
        eb.index = r.index; eb.size = r.size; eb.last_index = r.last_index; eb.ep_idx = r.ep_idx; eb.ep_rew = r.ep_rew; eb.ep_len = (int32_t)r.ep_len;
        c->env[e] = eb;
    }
}

// the live slots of the store, as (first row, rows) runs: sub-buffer e holds [e * sub, e * sub + size_e); neighbours that touch merge
// (a full store is ONE run, so one copy per column)
struct TsRun { int64_t row0, rows; };
static std::vector<TsRun> ts_ranges(const TsHostBuf& hb) {
    std::vector<TsRun> runs;
    for (size_t e = 0; e < hb.book.size(); ++e) {
        const int64_t row0 = (int64_t)e * hb.geom[0], rows = hb.book[e].size;
        if (rows == 0) continue;
        if (!runs.empty() && runs.back().row0 + runs.back().rows == row0) runs.back().rows += rows;
        else runs.push_back({row0, rows});
    }
    return runs;
}
static int64_t ts_live_rows(const TsHostBuf& hb) {
    int64_t n = 0;
    for (const tstate::BookRow& r : hb.book) n += r.size;
    return n;
}

// prioritised replay (section T_PER, only while it is on): the options and the two scalars, and with the store the leaves -- the
// tree above them is rebuilt on import.  A context without it writes no such section: its blob is what it always was.
static int64_t ts_per_bytes(const fsrl_ctx* c, bool with_store) { return tstate::per_bytes(with_store ? c->per->slots : 0); }
static int ts_per_export(fsrl_ctx* c, uint8_t* p, bool with_store) {
    const PerState* ps = c->per;
    double sc[3];
    HIPCHK(hipMemcpy(sc, ps->sc, sizeof(sc), hipMemcpyDeviceToHost));
    const tstate::PerHead h{ps->alpha, ps->beta, (int64_t)ps->weight_norm, sc[0], sc[1], with_store ? (int64_t)ps->slots : 0};
    memcpy(p, &h, (size_t)tstate::PER_HEAD_BYTES);
    if (with_store && ps->slots > 0)
        HIPCHK(hipMemcpy(p + tstate::PER_HEAD_BYTES, ps->tree + ps->bound, (size_t)ps->slots * 8, hipMemcpyDeviceToHost));
    return 0;
}
// ... into the context, whose store (geometry included) is already the blob's
static int ts_per_import(fsrl_ctx* c, const uint8_t* p) {
    tstate::PerHead h;
    memcpy(&h, p, (size_t)tstate::PER_HEAD_BYTES);
    PerState* ps = c->per;
    ps->alpha = h.alpha; ps->beta = h.beta; ps->weight_norm = (int)h.weight_norm;
    if (h.slots == 0) return 0;                 // a blob without the store: the tree stays this context's own, like its rows
    std::vector<double> leaves((size_t)h.slots);
    memcpy(leaves.data(), p + tstate::PER_HEAD_BYTES, (size_t)h.slots * 8);
    return per_load(c, leaves.data(), h.max_prio, h.min_prio);
}

static int ts_idle(const fsrl_ctx* c, const char* what) {
    if (c->in_update || c->verdict_pending) return fail(FSRL_ESTATE, "%s inside an update (between fsrl_ppo_begin and fsrl_ppo_end)", what);
    return 0;
}
// everything the context has enqueued has finished: the copies below are plain blocking hipMemcpys
static int ts_quiesce(fsrl_ctx* c) {
    HIPCHK(hipStreamSynchronize(c->side));
    HIPCHK(hipStreamSynchronize(c->compute));            // a grouped member: the group's stream; a replay group's call: its fan-out event
    if (c->tr && c->tr->cstream) HIPCHK(hipStreamSynchronize(c->tr->cstream));
    return 0;
}
// what is NOT state and was derived from the state that just changed
static void ts_invalidate(fsrl_ctx* c) {
    c->batch_ready = false; c->verdict_pending = false; c->snap_valid = false;
    c->theta_version += 1;
    c->store_version += 1;                               // device copies of the sub-buffer books
    if (TrState* t = c->tr) { t->hvp_valid = false; t->pad_valid = false; t->rd_version = 0; }
    if (SacState* s = sac_of(c)) { s->pre_valid = false; s->book_version = 0; s->n_drained = s->n_updates; }    // the ring's undrained tail is dropped
}

extern "C" int64_t fsrl_train_state_size(fsrl_ctx* c, int32_t with_store) {
    if (!c) return fail(FSRL_EINVAL, "null ctx");
    tstate::Fingerprint fp;
    int rc = ts_fingerprint(c, fp);
    if (rc) return rc;
    TsHostBuf hb;
    std::vector<TsSection> tab;
    ts_table(c, hb, with_store != 0, tab);
    ts_gather(c, hb);
    const int64_t live = ts_live_rows(hb);
    std::vector<int64_t> lens;
    for (const TsSection& s : tab) lens.push_back(s.kind == TS_STORE_COL ? live * s.bytes : s.bytes);
    if (c->per) lens.push_back(ts_per_bytes(c, with_store != 0));
    return tstate::blob_bytes(lens.data(), (int)lens.size());
}

extern "C" int fsrl_train_state_export(fsrl_ctx* c, int32_t with_store, void* out, int64_t cap, int64_t* written) {
    CHECK_ARG(c && out && written, "null argument");
    int rc = ts_idle(c, "fsrl_train_state_export");
    if (rc) return rc;
    tstate::Fingerprint fp;
    rc = ts_fingerprint(c, fp);
    if (rc) return rc;
    const int64_t need = fsrl_train_state_size(c, with_store);
    if (need < 0) return (int)need;
    CHECK_ARG(cap >= need, "a buffer of %lld bytes, the training state needs %lld (fsrl_train_state_size)", (long long)cap, (long long)need);
    ENTER_DEV(c);
    rc = join_store(c);                                  // the staging window lands first
    if (rc) return rc;
    rc = ts_quiesce(c);
    if (rc) return rc;
    TsHostBuf hb;
    std::vector<TsSection> tab;
    ts_table(c, hb, with_store != 0, tab);
    ts_gather(c, hb);
    const std::vector<TsRun> runs = ts_ranges(hb);
    const int64_t live = ts_live_rows(hb);
    tstate::Writer w(out, cap);
    w.header(fp, with_store ? tstate::FLAG_STORE : 0u, (uint32_t)tab.size() + (c->per ? 1u : 0u));
    for (const TsSection& s : tab) {
        const int64_t len = s.kind == TS_STORE_COL ? live * s.bytes : s.bytes;
        uint8_t* p = w.section(s.tag, len);
        if (!p) return fail(FSRL_EINVAL, "the training state does not fit %lld bytes", (long long)cap);
        if (s.kind == TS_HOST || s.kind == TS_STORE_HOST) memcpy(p, s.ptr, (size_t)len);
        else if (s.kind == TS_DEV) HIPCHK(hipMemcpy(p, s.ptr, (size_t)len, hipMemcpyDeviceToHost));
        else
            for (const TsRun& r : runs) {
                HIPCHK(hipMemcpy(p, (const char*)s.ptr + r.row0 * s.bytes, (size_t)(r.rows * s.bytes), hipMemcpyDeviceToHost));
                p += r.rows * s.bytes;
            }
    }
    if (c->per) {
        uint8_t* p = w.section(tstate::T_PER, ts_per_bytes(c, with_store != 0));
        if (!p) return fail(FSRL_EINVAL, "the training state does not fit %lld bytes", (long long)cap);
        rc = ts_per_export(c, p, with_store != 0);
        if (rc) return rc;
    }
    const int64_t n = w.finish();
    if (n != need) return fail(FSRL_ESTATE, "the training state took %lld bytes, not the %lld announced", (long long)n, (long long)need);
    *written = n;
    return 0;
}

extern "C" int fsrl_train_state_import(fsrl_ctx* c, const void* blob, int64_t n) {
    CHECK_ARG(c && blob, "null argument");
    int rc = ts_idle(c, "fsrl_train_state_import");
    if (rc) return rc;
    tstate::Fingerprint fp;
    rc = ts_fingerprint(c, fp);
    if (rc) return rc;
    // ---- everything that can refuse the blob, before the first write
    TsHostBuf hb;
    std::vector<TsSection> tab;
    ts_table(c, hb, true, tab);
    std::vector<tstate::SectionSpec> specs;
    for (const TsSection& s : tab) specs.push_back({s.tag, s.kind == TS_STORE_COL ? -1 : s.bytes, ts_is_store(s.kind)});
    specs.push_back({tstate::T_PER, -1, false, c->per == nullptr});      // behind the table's: found[tab.size()]
    std::vector<tstate::Found> found(specs.size());
    const uint8_t* b = (const uint8_t*)blob;
    uint32_t flags = 0;
    std::string err;
    if (tstate::validate(b, n, fp, specs.data(), (int)specs.size(), found.data(), &flags, err)) return fail(FSRL_EINVAL, "%s", err.c_str());
    const bool with_store = (flags & tstate::FLAG_STORE) != 0;
    const uint8_t *geom = nullptr, *book = nullptr, *flag_col = nullptr;
    int64_t col_len[6] = {0, 0, 0, 0, 0, 0};
    int ncol = 0;
    for (size_t i = 0; i < tab.size(); ++i) {
        if (found[i].off < 0) continue;
        const uint8_t* p = b + found[i].off;
        if (tab[i].tag == tstate::T_HOST && tstate::validate_host(p, err)) return fail(FSRL_EINVAL, "%s", err.c_str());
        if (tab[i].tag == tstate::T_GEOM) geom = p;
        if (tab[i].tag == tstate::T_BOOK) book = p;
        if (tab[i].tag == tstate::T_SFLG) flag_col = p;
        if (tab[i].kind == TS_STORE_COL) col_len[ncol++] = found[i].len;
    }
    if (with_store) {
        const tstate::StoreDims d{c->cfg.env_num, c->alloc_rows, c->cfg.obs_dim, c->cfg.act_dim};
        if (tstate::validate_store(geom, book, col_len, d, err)) return fail(FSRL_EINVAL, "%s", err.c_str());
    }
    const tstate::Found per_found = found[tab.size()];
    if (per_found.off >= 0) {                            // (present exactly when this context has prioritised replay on: validate)
        int64_t want_slots = 0;
        if (with_store) { int64_t g[2]; memcpy(g, geom, 16); want_slots = g[0] * g[1]; }
        if (tstate::validate_per(b + per_found.off, per_found.len, want_slots, err)) return fail(FSRL_EINVAL, "%s", err.c_str());
    }
    // ---- writes
    ENTER_DEV(c);                                        // a resident actor holds the old weights in registers: it ends here
    if (with_store) { rc = flush_stage(c); if (rc) return rc; }     // rows still in the window land first (and are then overwritten)
    rc = ts_quiesce(c);
    if (rc) return rc;
    for (size_t i = 0; i < tab.size(); ++i) {
        if (found[i].off < 0) continue;
        const TsSection& s = tab[i];
        if (s.kind == TS_HOST || s.kind == TS_STORE_HOST) memcpy(s.ptr, b + found[i].off, (size_t)found[i].len);
        else if (s.kind == TS_DEV) HIPCHK(hipMemcpy(s.ptr, b + found[i].off, (size_t)found[i].len, hipMemcpyHostToDevice));
    }
    ts_scatter(c, hb, with_store);
    if (with_store) {
        const std::vector<TsRun> runs = ts_ranges(hb);
        for (size_t i = 0; i < tab.size(); ++i) {
            const TsSection& s = tab[i];
            if (s.kind != TS_STORE_COL) continue;
            const uint8_t* p = b + found[i].off;
            for (const TsRun& r : runs) {
                HIPCHK(hipMemcpy((char*)s.ptr + r.row0 * s.bytes, p, (size_t)(r.rows * s.bytes), hipMemcpyHostToDevice));
                p += r.rows * s.bytes;
            }
        }
        std::fill(c->h_flags.begin(), c->h_flags.end(), (uint8_t)0);          // the host mirror of the flags, rebuilt
        const uint8_t* p = flag_col;
        for (const TsRun& r : runs) { memcpy(c->h_flags.data() + r.row0, p, (size_t)r.rows); p += r.rows; }
    }
    if (per_found.off >= 0) { rc = ts_per_import(c, b + per_found.off); if (rc) return rc; }
    ts_invalidate(c);
    return 0;
}

extern "C" int fsrl_train_state_copy(fsrl_ctx* dst, fsrl_ctx* src, int32_t with_store) {
    CHECK_ARG(dst && src, "null argument");
    CHECK_ARG(dst != src, "fsrl_train_state_copy of a context onto itself");
    CHECK_ARG(dst->device == src->device, "fsrl_train_state_copy: contexts on devices %d and %d (device-to-device on ONE device)", dst->device,
              src->device);
    int rc = ts_idle(dst, "fsrl_train_state_copy");
    if (!rc) rc = ts_idle(src, "fsrl_train_state_copy");
    if (rc) return rc;
    tstate::Fingerprint fd, fs;
    rc = ts_fingerprint(dst, fd);
    if (!rc) rc = ts_fingerprint(src, fs);
    if (rc) return rc;
    const int d = tstate::fingerprint_diff(fs, fd);
    CHECK_ARG(d < 0, "training state: %s differs: the source has %lld, the destination %lld", tstate::FIELD_NAMES[d], (long long)fs.v[d],
              (long long)fd.v[d]);
    CHECK_ARG((dst->per != nullptr) == (src->per != nullptr), "training state: prioritised replay is %s in the source and %s in the "
              "destination (fsrl_per_enable on both, or on neither)", src->per ? "on" : "off", dst->per ? "on" : "off");
    ENTER_DEV(src);
    rc = join_store(src);
    if (rc) return rc;
    rc = ts_quiesce(src);
    if (rc) return rc;
    pactor_release(dst);
    if (with_store) { rc = flush_stage(dst); if (rc) return rc; }
    rc = ts_quiesce(dst);
    if (rc) return rc;
    TsHostBuf hs, hd;
    std::vector<TsSection> ts, td;
    ts_table(src, hs, with_store != 0, ts);
    ts_table(dst, hd, with_store != 0, td);
    ts_gather(src, hs);
    const std::vector<TsRun> runs = ts_ranges(hs);
    for (size_t i = 0; i < ts.size(); ++i) {
        const TsSection &a = ts[i], &b = td[i];          // equal fingerprints: the same tags and sizes in the same order
        if (a.kind == TS_DEV) HIPCHK(hipMemcpyAsync(b.ptr, a.ptr, (size_t)a.bytes, hipMemcpyDeviceToDevice, dst->compute));
        else if (a.kind == TS_STORE_COL)
            for (const TsRun& r : runs)
                HIPCHK(hipMemcpyAsync((char*)b.ptr + r.row0 * a.bytes, (const char*)a.ptr + r.row0 * a.bytes, (size_t)(r.rows * a.bytes),
                                      hipMemcpyDeviceToDevice, dst->compute));
    }
    HIPCHK(hipStreamSynchronize(dst->compute));          // the source may change again as soon as this call returns
    ts_scatter(dst, hs, with_store != 0);
    if (with_store) dst->h_flags = src->h_flags;
    if (src->per) {                                      // the options always; with the store its tree and scalars, node for node
        PerState *ps = src->per, *pd = dst->per;
        pd->alpha = ps->alpha; pd->beta = ps->beta; pd->weight_norm = ps->weight_norm;
        if (with_store) {
            pd->slots = ps->slots; pd->bound = ps->bound;
            HIPCHK(hipMemcpy(pd->tree, ps->tree, (size_t)2 * ps->bound * 8, hipMemcpyDeviceToDevice));
            HIPCHK(hipMemcpy(pd->sc, ps->sc, 3 * 8, hipMemcpyDeviceToDevice));
        }
    }
    ts_invalidate(dst);
    return 0;
}
