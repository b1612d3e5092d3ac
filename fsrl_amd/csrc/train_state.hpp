// train_state.hpp -- the byte format of an exported training state (fsrl_train_state_export / _import, include/fsrl_hip.h): its
// writer, its reader and everything that is checked about a blob before the library writes a single byte of a context.
// Standard library only (no HIP), so tests/host/train_state_sim.cpp drives it as a plain program (tests/test_train_state_host.py).
// The blob comes from a file: this is the code that has to survive hostile input, so every offset is checked against the length
// before it is used and nothing here trusts a length field.
//
//   header    magic u64 | version u32 | flags u32 (bit 0: the store is inside) | n_fields u32 | n_sections u32 | fingerprint i64[n_fields]
//   sections  tag u32 | zero u32 | length i64 | payload, zero-padded to a multiple of 8 bytes
//   trailer   checksum u64 over every byte before it
// Little-endian, as the machine writes it.  A blob is a pure function of the state it was taken from.
#pragma once
#include <stdint.h>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>

namespace tstate {

static constexpr uint64_t MAGIC = 0x0153544c52534600ull;      // "\0FSRLTS\1"
static constexpr uint32_t VERSION = 1;
static constexpr uint32_t FLAG_STORE = 1u;
static constexpr int MAX_HIDDEN = 8;                          // FSRL_MAX_HIDDEN

// ---- the fingerprint: everything the section sizes and the meaning of their bytes depend on
enum Field {
    F_ALGO, F_MODE, F_LAYERED, F_OBS_DIM, F_ACT_DIM, F_HIDDEN_PAD, F_N_HIDDEN,
    F_W0, F_W1, F_W2, F_W3, F_W4, F_W5, F_W6, F_W7,
    F_N_CRITICS, F_ENV_NUM, F_STORE_ROWS, F_REW_NORM, F_N_Q, F_N
};
static const char* const FIELD_NAMES[F_N] = {
    "algo", "mode", "layered", "obs_dim", "act_dim", "hidden_pad", "n_hidden",
    "hidden_sizes[0]", "hidden_sizes[1]", "hidden_sizes[2]", "hidden_sizes[3]", "hidden_sizes[4]", "hidden_sizes[5]",
    "hidden_sizes[6]", "hidden_sizes[7]",
    "n_critics", "env_num", "store_rows", "rew_norm", "n_q"};
struct Fingerprint { int64_t v[F_N] = {0}; };
// modes of a context (F_MODE)
enum Mode { MODE_ONPOLICY = 0, MODE_SAC = 1, MODE_DDPG = 2, MODE_CVPO = 3 };

// first field in which two fingerprints differ, -1: none
static inline int fingerprint_diff(const Fingerprint& a, const Fingerprint& b) {
    for (int i = 0; i < F_N; ++i) if (a.v[i] != b.v[i]) return i;
    return -1;
}

// ---- section tags
static constexpr uint32_t fourcc(char a, char b, char c, char d) {
    return (uint32_t)(uint8_t)a | ((uint32_t)(uint8_t)b << 8) | ((uint32_t)(uint8_t)c << 16) | ((uint32_t)(uint8_t)d << 24);
}
static constexpr uint32_t T_HOST = fourcc('H', 'O', 'S', 'T');      // HostSlots: counters, streams, rates
static constexpr uint32_t T_P = fourcc('P', ' ', ' ', ' '), T_M = fourcc('M', ' ', ' ', ' '), T_V = fourcc('V', ' ', ' ', ' ');
static constexpr uint32_t T_RMS = fourcc('R', 'M', 'S', ' ');
static constexpr uint32_t T_PA = fourcc('P', 'A', ' ', ' '), T_MA = fourcc('M', 'A', ' ', ' '), T_VA = fourcc('V', 'A', ' ', ' ');
static constexpr uint32_t T_PAT = fourcc('P', 'A', 'T', ' ');
static constexpr uint32_t T_PQ = fourcc('P', 'Q', ' ', ' '), T_PQT = fourcc('P', 'Q', 'T', ' ');
static constexpr uint32_t T_MQ = fourcc('M', 'Q', ' ', ' '), T_VQ = fourcc('V', 'Q', ' ', ' ');
static constexpr uint32_t T_SACS = fourcc('S', 'A', 'C', 'S'), T_CVPS = fourcc('C', 'V', 'P', 'S');
static constexpr uint32_t T_GEOM = fourcc('G', 'E', 'O', 'M'), T_BOOK = fourcc('B', 'O', 'O', 'K');
static constexpr uint32_t T_SOBS = fourcc('S', 'O', 'B', 'S'), T_SNXT = fourcc('S', 'N', 'X', 'T'), T_SACT = fourcc('S', 'A', 'C', 'T');
static constexpr uint32_t T_SREW = fourcc('S', 'R', 'E', 'W'), T_SCST = fourcc('S', 'C', 'S', 'T'), T_SFLG = fourcc('S', 'F', 'L', 'G');
static constexpr uint32_t T_PER = fourcc('P', 'E', 'R', ' ');       // prioritised replay (PerHead, then the leaves): only when it is on

static inline std::string tag_name(uint32_t t) {
    char s[5];
    for (int i = 0; i < 4; ++i) { const char ch = (char)((t >> (8 * i)) & 0xff); s[i] = (ch >= 33 && ch < 127) ? ch : (ch == ' ' ? '_' : '?'); }
    s[4] = 0;
    return s;
}

// what a context expects of one section.  bytes < 0: the length is the blob's to state (the store's columns: their rows follow
// from the sub-buffer books, validate_store checks them); store: the section exists exactly in blobs with FLAG_STORE; absent: the
// section belongs to an option this context has OFF (prioritised replay), so a blob that carries it is refused by name
struct SectionSpec { uint32_t tag; int64_t bytes; bool store; bool absent = false; };
struct Found { int64_t off = -1, len = 0; };          // a section's payload inside the blob

static constexpr int64_t HEADER_BYTES = 24 + 8 * (int64_t)F_N;
static constexpr int64_t SECTION_HEAD = 16;
static inline int64_t pad8(int64_t n) { return (n + 7) / 8 * 8; }

// ---- checksum: h <- mix(h ^ word) over 64-bit words, mix = multiply by an odd constant, then xor-shift.  Every step is a bijection
//      of h for a fixed word and of the word for a fixed h, so two inputs of one length that differ in any one word differ in the
//      sum.  Four interleaved lanes (word i goes to lane i mod 4) keep the multiplies independent -- a store of 320 MB is 40 M
//      words -- and are folded the same way at the end; the length is mixed in last, so a blob followed by its own sum does not
//      sum to zero.  n is a multiple of 8.
static inline uint64_t checksum_mix(uint64_t h) {
    h *= 0x100000001b3ull;
    return h ^ (h >> 29);
}
static inline uint64_t checksum(const uint8_t* p, int64_t n) {
    uint64_t h[4] = {0xcbf29ce484222325ull, 0x9e3779b97f4a7c15ull, 0xbf58476d1ce4e5b9ull, 0x94d049bb133111ebull};
    int64_t i = 0;
    for (; i + 32 <= n; i += 32) {
        uint64_t w[4];
        memcpy(w, p + i, 32);
        for (int l = 0; l < 4; ++l) h[l] = checksum_mix(h[l] ^ w[l]);
    }
    for (int l = 0; i + 8 <= n; i += 8, ++l) {
        uint64_t w;
        memcpy(&w, p + i, 8);
        h[l] = checksum_mix(h[l] ^ w);
    }
    uint64_t f = 0x2545f4914f6cdd1dull;
    for (int l = 0; l < 4; ++l) f = checksum_mix(f ^ h[l]);
    return checksum_mix(f ^ (uint64_t)n);
}

// bytes of a blob whose sections have these payload lengths
static inline int64_t blob_bytes(const int64_t* lens, int n) {
    int64_t total = HEADER_BYTES + 8;
    for (int i = 0; i < n; ++i) total += SECTION_HEAD + pad8(lens[i]);
    return total;
}

// ---- writer: header(), then section() per section (the caller fills the returned payload), then finish()
struct Writer {
    uint8_t* p = nullptr;
    int64_t cap = 0, off = 0;
    bool ok = true;
    Writer(void* out, int64_t cap_) : p((uint8_t*)out), cap(cap_) {}
    void header(const Fingerprint& fp, uint32_t flags, uint32_t n_sections) {
        if (cap < HEADER_BYTES) { ok = false; return; }
        const uint32_t ver = VERSION, nf = F_N;
        memcpy(p, &MAGIC, 8); memcpy(p + 8, &ver, 4); memcpy(p + 12, &flags, 4); memcpy(p + 16, &nf, 4); memcpy(p + 20, &n_sections, 4);
        memcpy(p + 24, fp.v, 8 * (size_t)F_N);
        off = HEADER_BYTES;
    }
    // -> where the payload goes (len bytes; the padding behind it is zeroed here), nullptr once the buffer is too small
    uint8_t* section(uint32_t tag, int64_t len) {
        if (!ok || len < 0 || len > cap - off - SECTION_HEAD || pad8(len) > cap - off - SECTION_HEAD) { ok = false; return nullptr; }
        const uint32_t zero = 0;
        memcpy(p + off, &tag, 4); memcpy(p + off + 4, &zero, 4); memcpy(p + off + 8, &len, 8);
        uint8_t* payload = p + off + SECTION_HEAD;
        if (pad8(len) > len) memset(payload + len, 0, (size_t)(pad8(len) - len));
        off += SECTION_HEAD + pad8(len);
        return payload;
    }
    // -> total bytes, -1 if anything did not fit
    int64_t finish() {
        if (!ok || cap - off < 8) return -1;
        const uint64_t h = checksum(p, off);
        memcpy(p + off, &h, 8);
        off += 8;
        return off;
    }
};

static inline int refuse(std::string& err, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
static inline int refuse(std::string& err, const char* fmt, ...) {
    char buf[384];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    err = buf;
    return -1;
}

// ---- validator.  0: the blob is well formed, belongs to a context of fingerprint `want` and holds exactly the sections `specs`
//      asks for (the store's only with FLAG_STORE), each of its expected length; found[i] then locates specs[i]'s payload
//      (off < 0: a store section of a blob without the store).  -1: refused, `err` says why.  Nothing is written anywhere else.
static inline int validate(const uint8_t* b, int64_t n, const Fingerprint& want, const SectionSpec* specs, int nspecs, Found* found,
                           uint32_t* flags_out, std::string& err) {
    if (!b || n < HEADER_BYTES + 8) return refuse(err, "training state: %lld bytes are too few for a header", (long long)n);
    if (n % 8 != 0) return refuse(err, "training state: a length of %lld bytes is no multiple of 8 (truncated?)", (long long)n);
    uint64_t magic; uint32_t ver, flags, nf, nsec;
    memcpy(&magic, b, 8); memcpy(&ver, b + 8, 4); memcpy(&flags, b + 12, 4); memcpy(&nf, b + 16, 4); memcpy(&nsec, b + 20, 4);
    if (magic != MAGIC) return refuse(err, "training state: bad magic (not an exported training state)");
    if (ver != VERSION) return refuse(err, "training state: format version %u, this library reads version %u", ver, VERSION);
    uint64_t sum;
    memcpy(&sum, b + n - 8, 8);
    if (sum != checksum(b, n - 8)) return refuse(err, "training state: checksum mismatch (corrupt or truncated)");
    if (nf != (uint32_t)F_N) return refuse(err, "training state: %u fingerprint fields, expected %d", nf, (int)F_N);
    if (flags & ~FLAG_STORE) return refuse(err, "training state: unknown flags 0x%x", flags);
    Fingerprint got;
    memcpy(got.v, b + 24, 8 * (size_t)F_N);
    const int d = fingerprint_diff(got, want);
    if (d >= 0)
        return refuse(err, "training state: %s differs: the blob has %lld, this context %lld", FIELD_NAMES[d], (long long)got.v[d],
                      (long long)want.v[d]);
    const bool with_store = (flags & FLAG_STORE) != 0;
    for (int i = 0; i < nspecs; ++i) found[i] = Found{};
    const int64_t end = n - 8;
    int64_t pos = HEADER_BYTES;
    uint32_t seen = 0;
    while (pos < end) {
        if (end - pos < SECTION_HEAD) return refuse(err, "training state: %lld stray bytes behind the last section", (long long)(end - pos));
        uint32_t tag, zero; int64_t len;
        memcpy(&tag, b + pos, 4); memcpy(&zero, b + pos + 4, 4); memcpy(&len, b + pos + 8, 8);
        pos += SECTION_HEAD;
        if (zero != 0) return refuse(err, "training state: section %s: reserved word is not zero", tag_name(tag).c_str());
        if (len < 0) return refuse(err, "training state: section %s has the negative length %lld", tag_name(tag).c_str(), (long long)len);
        if (len > end - pos || pad8(len) > end - pos)
            return refuse(err, "training state: section %s of %lld bytes runs past the end (%lld left)", tag_name(tag).c_str(),
                          (long long)len, (long long)(end - pos));
        int k = -1;
        for (int i = 0; i < nspecs; ++i) if (specs[i].tag == tag) { k = i; break; }
        if (k < 0) return refuse(err, "training state: unknown section %s", tag_name(tag).c_str());
        if (specs[k].absent)
            return refuse(err, "training state: section %s: the blob carries %s state and this context has it off", tag_name(tag).c_str(),
                          tag == T_PER ? "prioritised-replay" : "optional");
        if (specs[k].store && !with_store) return refuse(err, "training state: store section %s in a blob without the store", tag_name(tag).c_str());
        if (found[k].off >= 0) return refuse(err, "training state: duplicate section %s", tag_name(tag).c_str());
        if (specs[k].bytes >= 0 && len != specs[k].bytes)
            return refuse(err, "training state: section %s has %lld bytes, this context's is %lld", tag_name(tag).c_str(), (long long)len,
                          (long long)specs[k].bytes);
        for (int64_t i = len; i < pad8(len); ++i)
            if (b[pos + i] != 0) return refuse(err, "training state: section %s: padding is not zero", tag_name(tag).c_str());
        found[k].off = pos; found[k].len = len;
        pos += pad8(len);
        seen += 1;
    }
    if (seen != nsec) return refuse(err, "training state: the header counts %u sections, %u are there", nsec, seen);
    for (int i = 0; i < nspecs; ++i)
        if (found[i].off < 0 && !specs[i].absent && (!specs[i].store || with_store))
            return refuse(err, "training state: missing section %s%s", tag_name(specs[i].tag).c_str(),
                          specs[i].tag == T_PER ? ": this context has prioritised replay on and the blob was taken from one without it" : "");
    if (flags_out) *flags_out = flags;
    return 0;
}

// ---- the host's scalars (section T_HOST): 32 slots of 8 bytes, unused ones zero.  Doubles travel as their bit patterns.
enum HostSlot {
    H_ADAM_T = 0, H_RNG = 1 /* .. 4 */, H_SHUFFLE = 5 /* .. 8 */, H_LR0 = 9, H_LR1 = 10, H_LR2 = 11, H_TR_CRITIC_T = 12,
    H_FOC_NU = 13, H_FOC_NU_LOSS = 14, H_FOC_T_ACTOR = 15, H_FOC_T_CRITIC = 16,
    H_SAC_T_ACTOR = 17, H_SAC_T_CRITIC = 18, H_SAC_N_UPDATES = 19, H_SAC_KEY = 20, H_SLOTS = 32
};
static constexpr int64_t HOST_BYTES = 8 * (int64_t)H_SLOTS;
struct HostSlots {
    uint64_t s[H_SLOTS] = {0};
    void put_i(int k, int64_t v) { s[k] = (uint64_t)v; }
    void put_d(int k, double v) { memcpy(&s[k], &v, 8); }
    int64_t get_i(int k) const { return (int64_t)s[k]; }
    double get_d(int k) const { double v; memcpy(&v, &s[k], 8); return v; }
};
// counters index device rows (the statistics ring) and feed Adam's bias correction: none may be negative; rates are finite, >= 0
static inline int validate_host(const uint8_t* payload, std::string& err) {
    HostSlots h;
    memcpy(h.s, payload, (size_t)HOST_BYTES);
    const int counters[] = {H_ADAM_T, H_TR_CRITIC_T, H_FOC_T_ACTOR, H_FOC_T_CRITIC, H_SAC_T_ACTOR, H_SAC_T_CRITIC, H_SAC_N_UPDATES};
    for (int k : counters)
        if (h.get_i(k) < 0) return refuse(err, "training state: host slot %d (a step counter) is negative: %lld", k, (long long)h.get_i(k));
    for (int k : {(int)H_LR0, (int)H_LR1, (int)H_LR2}) {
        const double lr = h.get_d(k);
        if (!(std::isfinite(lr) && lr >= 0.0)) return refuse(err, "training state: host slot %d (a learning rate) is not finite and >= 0", k);
    }
    for (int k = H_SAC_KEY + 1; k < H_SLOTS; ++k)
        if (h.s[k] != 0) return refuse(err, "training state: unused host slot %d is not zero", k);
    return 0;
}

// ---- the store.  T_GEOM: sub_size i64 | buffer_num i64.  T_BOOK: per sub-buffer of the CONTEXT (env_num of them, the ones past
//      buffer_num empty) BookRow.  The six columns hold, sub-buffer after sub-buffer, the slots [0, size) of each -- the only slots a
//      sub-buffer of `size` rows has ever written or will read.
struct BookRow { int64_t index, size, last_index, ep_idx; double ep_rew; int64_t ep_len; };
static constexpr int64_t BOOK_ROW_BYTES = 48;
static_assert(sizeof(BookRow) == BOOK_ROW_BYTES, "BookRow is six 8-byte fields");
struct StoreDims { int64_t env_num, alloc_rows, obs_dim, act_dim; };
// bytes per row of column k (obs, obs_next, act, rew, cost, flags)
static inline int64_t column_width(const StoreDims& d, int k) { return k < 2 ? 4 * d.obs_dim : k == 2 ? 4 * d.act_dim : k < 5 ? 8 : 1; }

// geometry fits the allocation; every book is one a sequence of pushes can have produced; the columns hold exactly the live rows
static inline int validate_store(const uint8_t* geom, const uint8_t* book, const int64_t col_len[6], const StoreDims& d, std::string& err) {
    int64_t sub, num;
    memcpy(&sub, geom, 8); memcpy(&num, geom + 8, 8);
    if (num < 1 || num > d.env_num) return refuse(err, "training state: store of %lld sub-buffers, this context has %lld", (long long)num, (long long)d.env_num);
    if (sub < 1 || sub > d.alloc_rows || sub > d.alloc_rows / num)
        return refuse(err, "training state: store of %lld x %lld rows does not fit the %lld rows of this context", (long long)sub, (long long)num,
                      (long long)d.alloc_rows);
    int64_t rows = 0;
    for (int64_t e = 0; e < d.env_num; ++e) {
        BookRow r;
        memcpy(&r, book + e * BOOK_ROW_BYTES, (size_t)BOOK_ROW_BYTES);
        const bool ok_range = r.size >= 0 && r.size <= sub && r.index >= 0 && r.index < sub && r.last_index >= 0 && r.last_index < sub &&
                              r.ep_idx >= 0 && r.ep_idx < sub && r.ep_len >= 0 && r.ep_len <= INT32_MAX;
        if (!ok_range) return refuse(err, "training state: sub-buffer %lld: bookkeeping outside its %lld rows", (long long)e, (long long)sub);
        if (e >= num && (r.size != 0 || r.index != 0)) return refuse(err, "training state: sub-buffer %lld is past the store's %lld and not empty", (long long)e, (long long)num);
        if (r.size < sub && r.index != r.size % sub) return refuse(err, "training state: sub-buffer %lld: index %lld does not follow from size %lld", (long long)e, (long long)r.index, (long long)r.size);
        if (r.size > 0 && r.last_index != (r.index - 1 + sub) % sub)
            return refuse(err, "training state: sub-buffer %lld: last_index %lld does not precede index %lld", (long long)e, (long long)r.last_index, (long long)r.index);
        if (r.size == 0 && r.last_index != 0) return refuse(err, "training state: sub-buffer %lld is empty with last_index %lld", (long long)e, (long long)r.last_index);
        rows += r.size;
    }
    static const char* const names[6] = {"obs", "obs_next", "act", "rew", "cost", "flags"};
    for (int k = 0; k < 6; ++k)
        if (col_len[k] != rows * column_width(d, k))
            return refuse(err, "training state: store column %s has %lld bytes, %lld live rows need %lld", names[k], (long long)col_len[k],
                          (long long)rows, (long long)(rows * column_width(d, k)));
    return 0;
}

// ---- prioritised replay (section T_PER, present exactly when the exporting context has it on).  PerHead, then `slots` float64
//      leaves in slot order; slots = sub_size * buffer_num in a blob with the store, 0 in one without (the leaves describe the
//      store's rows: without them only the options travel).  The tree above the leaves is rebuilt on import.
struct PerHead { double alpha, beta; int64_t weight_norm; double max_prio, min_prio; int64_t slots; };
static constexpr int64_t PER_HEAD_BYTES = 48;
static_assert(sizeof(PerHead) == PER_HEAD_BYTES, "PerHead is six 8-byte fields");
static inline int64_t per_bytes(int64_t slots) { return PER_HEAD_BYTES + 8 * slots; }
// want_slots: sub_size * buffer_num of the geometry the blob brings (validate_store has accepted it), 0 for a blob without the store
static inline int validate_per(const uint8_t* payload, int64_t len, int64_t want_slots, std::string& err) {
    if (len < PER_HEAD_BYTES) return refuse(err, "training state: section PER_ of %lld bytes is shorter than its head", (long long)len);
    PerHead h;
    memcpy(&h, payload, (size_t)PER_HEAD_BYTES);
    if (!(std::isfinite(h.alpha) && h.alpha >= 0.0 && std::isfinite(h.beta) && h.beta >= 0.0))
        return refuse(err, "training state: prioritised replay: alpha and beta must be finite and >= 0");
    if (h.weight_norm != 0 && h.weight_norm != 1) return refuse(err, "training state: prioritised replay: weight_norm is %lld", (long long)h.weight_norm);
    if (!(std::isfinite(h.max_prio) && std::isfinite(h.min_prio) && h.min_prio > 0.0 && h.min_prio <= h.max_prio))
        return refuse(err, "training state: prioritised replay: max_prio and min_prio must be finite with 0 < min_prio <= max_prio");
    if (h.slots != want_slots)
        return refuse(err, "training state: prioritised replay: leaves for %lld slots, the blob's store has %lld", (long long)h.slots,
                      (long long)want_slots);
    if (h.slots < 0 || h.slots > (INT64_MAX - PER_HEAD_BYTES) / 8 || len != per_bytes(h.slots))
        return refuse(err, "training state: section PER_ has %lld bytes, %lld slots need %lld", (long long)len, (long long)h.slots,
                      (long long)(h.slots < 0 || h.slots > (INT64_MAX - PER_HEAD_BYTES) / 8 ? -1 : per_bytes(h.slots)));
    for (int64_t i = 0; i < h.slots; ++i) {
        double v;
        memcpy(&v, payload + PER_HEAD_BYTES + 8 * i, 8);
        if (!(std::isfinite(v) && v >= 0.0)) return refuse(err, "training state: prioritised replay: leaf %lld is not finite and >= 0", (long long)i);
    }
    return 0;
}

}  // namespace tstate
