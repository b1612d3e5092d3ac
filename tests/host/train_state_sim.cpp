// train_state_sim.cpp -- fsrl_amd/csrc/train_state.hpp (the byte format of an exported training state) as a stand-alone program:
// tests/test_train_state_host.py builds it with the address / undefined-behaviour sanitizers and runs it in its own process.
// It writes a small blob with the header's writer and hands the validator everything a damaged or foreign file can hold.
// Every check prints one "ok <name> ..." line; the first failure prints "FAIL ..." and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "train_state.hpp"

using namespace tstate;

static void fail_now(const char* what, const std::string& detail) {
    printf("FAIL %s: %s\n", what, detail.c_str());
    exit(1);
}
#define EXPECT(cond, what, detail) do { if (!(cond)) fail_now(what, detail); } while (0)

// a context of 3 sub-buffers x 5 rows (15 allocated + 3 slack), obs 3, act 2
static const StoreDims DIMS{3, 18, 3, 2};
static Fingerprint make_fp() {
    Fingerprint fp;
    for (int i = 0; i < F_N; ++i) fp.v[i] = 100 + 7 * i;
    return fp;
}
static const uint32_t COLS[6] = {T_SOBS, T_SNXT, T_SACT, T_SREW, T_SCST, T_SFLG};
static std::vector<SectionSpec> make_specs() {
    std::vector<SectionSpec> s = {{T_HOST, HOST_BYTES, false}, {T_P, 100, false}, {T_M, 64, false}, {T_RMS, 7, false},
                                  {T_GEOM, 16, true}, {T_BOOK, BOOK_ROW_BYTES * 3, true}};
    for (uint32_t t : COLS) s.push_back({t, -1, true});
    return s;
}
// sub-buffer 0 wrapped (full, index 2), 1 empty, 2 holds 3 rows of an episode in progress
static std::vector<BookRow> make_book() {
    return {BookRow{2, 5, 1, 4, 1.5, 3}, BookRow{0, 0, 0, 0, 0.0, 0}, BookRow{3, 3, 2, 1, -2.25, 2}};
}
static const int64_t LIVE = 8;

struct Payloads {
    HostSlots host;
    std::vector<uint8_t> p, m, rms;
    int64_t geom[2] = {5, 3};
    std::vector<BookRow> book = make_book();
    std::vector<uint8_t> col[6];
};
static Payloads make_payloads() {
    Payloads x;
    x.host.put_i(H_ADAM_T, 12); x.host.put_d(H_LR0, 5e-4); x.host.put_d(H_LR1, 1e-3); x.host.put_i(H_SAC_N_UPDATES, 9);
    x.host.s[H_RNG] = 0x123456789abcdef0ull; x.host.s[H_SAC_KEY] = 0xfeedfacecafebeefull;
    x.p.resize(100); x.m.resize(64); x.rms.resize(7);
    for (size_t i = 0; i < x.p.size(); ++i) x.p[i] = (uint8_t)(i * 3 + 1);
    for (size_t i = 0; i < x.m.size(); ++i) x.m[i] = (uint8_t)(i * 5 + 2);
    for (size_t i = 0; i < x.rms.size(); ++i) x.rms[i] = (uint8_t)(0xa0 + i);
    for (int k = 0; k < 6; ++k) {
        x.col[k].resize((size_t)(LIVE * column_width(DIMS, k)));
        for (size_t i = 0; i < x.col[k].size(); ++i) x.col[k][i] = (uint8_t)(17 * k + i);
    }
    return x;
}

// order: the tags to write, in this order (so that a test can drop, repeat or add one)
static std::vector<uint8_t> write_blob(const Fingerprint& fp, const Payloads& x, bool with_store, const std::vector<uint32_t>& order) {
    std::vector<uint8_t> buf(4096, 0xEE);               // 0xEE: padding the writer forgets to zero would show
    Writer w(buf.data(), (int64_t)buf.size());
    w.header(fp, with_store ? FLAG_STORE : 0u, (uint32_t)order.size());
    for (uint32_t tag : order) {
        const void* src = nullptr; int64_t len = 0;
        if (tag == T_HOST) { src = x.host.s; len = HOST_BYTES; }
        else if (tag == T_P) { src = x.p.data(); len = (int64_t)x.p.size(); }
        else if (tag == T_M) { src = x.m.data(); len = (int64_t)x.m.size(); }
        else if (tag == T_RMS) { src = x.rms.data(); len = (int64_t)x.rms.size(); }
        else if (tag == T_GEOM) { src = x.geom; len = 16; }
        else if (tag == T_BOOK) { src = x.book.data(); len = BOOK_ROW_BYTES * (int64_t)x.book.size(); }
        else {
            int k = -1;
            for (int i = 0; i < 6; ++i) if (COLS[i] == tag) k = i;
            if (k >= 0) { src = x.col[k].data(); len = (int64_t)x.col[k].size(); }
            else { src = x.m.data(); len = 8; }         // a tag no context knows
        }
        uint8_t* p = w.section(tag, len);
        EXPECT(p != nullptr, "writer", "section did not fit");
        memcpy(p, src, (size_t)len);
    }
    const int64_t n = w.finish();
    EXPECT(n > 0, "writer", "finish failed");
    buf.resize((size_t)n);
    return buf;
}
static std::vector<uint32_t> full_order(bool with_store) {
    std::vector<uint32_t> o = {T_HOST, T_P, T_M, T_RMS};
    if (with_store) { o.push_back(T_GEOM); o.push_back(T_BOOK); for (uint32_t t : COLS) o.push_back(t); }
    return o;
}

struct Verdict { int rc; std::string err; std::vector<Found> found; uint32_t flags; };
static Verdict check(const std::vector<uint8_t>& b, int64_t n, const Fingerprint& want) {
    const std::vector<SectionSpec> specs = make_specs();
    Verdict v;
    v.found.resize(specs.size());
    v.flags = 0;
    // the validator must not read past n: hand it an exact-size copy so that the address sanitizer sees an overrun
    std::vector<uint8_t> exact(b.begin(), b.begin() + n);
    v.rc = validate(exact.data(), n, want, specs.data(), (int)specs.size(), v.found.data(), &v.flags, v.err);
    return v;
}
static void reseal(std::vector<uint8_t>& b) {            // a tampered blob with a VALID checksum: the field checks must catch it
    const uint64_t h = checksum(b.data(), (int64_t)b.size() - 8);
    memcpy(b.data() + b.size() - 8, &h, 8);
}
static bool has(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

int main() {
    const Fingerprint fp = make_fp();
    const Payloads x = make_payloads();
    const std::vector<SectionSpec> specs = make_specs();
    const std::vector<uint8_t> blob = write_blob(fp, x, true, full_order(true));
    const int64_t n = (int64_t)blob.size();

    // ---- round trip: every payload comes back, a second write of what was read is the same bytes
    {
        Verdict v = check(blob, n, fp);
        EXPECT(v.rc == 0, "round_trip", v.err);
        EXPECT(v.flags == FLAG_STORE, "round_trip", "flags");
        std::vector<int64_t> lens;
        for (size_t i = 0; i < specs.size(); ++i) { EXPECT(v.found[i].off >= 0, "round_trip", "section not found"); lens.push_back(v.found[i].len); }
        EXPECT(blob_bytes(lens.data(), (int)lens.size()) == n, "round_trip", "blob_bytes disagrees with the writer");
        Payloads y;
        memcpy(y.host.s, blob.data() + v.found[0].off, (size_t)HOST_BYTES);
        y.p.assign(blob.begin() + v.found[1].off, blob.begin() + v.found[1].off + v.found[1].len);
        y.m.assign(blob.begin() + v.found[2].off, blob.begin() + v.found[2].off + v.found[2].len);
        y.rms.assign(blob.begin() + v.found[3].off, blob.begin() + v.found[3].off + v.found[3].len);
        memcpy(y.geom, blob.data() + v.found[4].off, 16);
        memcpy(y.book.data(), blob.data() + v.found[5].off, (size_t)v.found[5].len);
        int64_t col_len[6];
        for (int k = 0; k < 6; ++k) {
            const Found& f = v.found[6 + (size_t)k];
            y.col[k].assign(blob.begin() + f.off, blob.begin() + f.off + f.len);
            col_len[k] = f.len;
        }
        EXPECT(y.p == x.p && y.m == x.m && y.rms == x.rms && memcmp(y.host.s, x.host.s, (size_t)HOST_BYTES) == 0, "round_trip", "payload differs");
        std::string err;
        EXPECT(validate_host(blob.data() + v.found[0].off, err) == 0, "round_trip", err);
        EXPECT(validate_store(blob.data() + v.found[4].off, blob.data() + v.found[5].off, col_len, DIMS, err) == 0, "round_trip", err);
        EXPECT(write_blob(fp, y, true, full_order(true)) == blob, "round_trip", "export(import(b)) != b");
        const std::vector<uint8_t> bare = write_blob(fp, x, false, full_order(false));
        Verdict w = check(bare, (int64_t)bare.size(), fp);
        EXPECT(w.rc == 0 && w.flags == 0 && w.found[4].off < 0 && w.found[11].off < 0, "round_trip", "blob without the store: " + w.err);
        printf("ok round_trip bytes=%lld sections=%zu\n", (long long)n, specs.size());
    }
    // ---- every prefix is refused
    {
        for (int64_t k = 0; k < n; ++k) {
            Verdict v = check(blob, k, fp);
            EXPECT(v.rc != 0 && !v.err.empty(), "prefixes", "a prefix of " + std::to_string(k) + " bytes was accepted");
        }
        printf("ok prefixes refused=%lld\n", (long long)n);
    }
    // ---- a flipped bit at every byte position is refused (every bit of the byte in turn)
    {
        int64_t flips = 0;
        for (int64_t k = 0; k < n; ++k)
            for (int bit = 0; bit < 8; ++bit) {
                std::vector<uint8_t> t = blob;
                t[(size_t)k] ^= (uint8_t)(1u << bit);
                Verdict v = check(t, n, fp);
                EXPECT(v.rc != 0, "bit_flips", "bit " + std::to_string(bit) + " of byte " + std::to_string(k) + " went unnoticed");
                flips += 1;
            }
        printf("ok bit_flips refused=%lld\n", (long long)flips);
    }
    // ---- section lengths: larger than the remainder, negative, and other than the context's (all behind a valid checksum)
    {
        Verdict v0 = check(blob, n, fp);
        const int64_t len_at = v0.found[1].off - 8;     // the length field of section P
        for (int64_t bad : {(int64_t)n, (int64_t)1 << 62, (int64_t)INT64_MAX, (int64_t)-1, (int64_t)INT64_MIN, (int64_t)-8}) {
            std::vector<uint8_t> t = blob;
            memcpy(t.data() + len_at, &bad, 8);
            reseal(t);
            Verdict v = check(t, n, fp);
            EXPECT(v.rc != 0 && (has(v.err, "negative length") || has(v.err, "runs past the end")), "lengths", "length " + std::to_string(bad) + ": " + v.err);
            EXPECT((bad < 0) == has(v.err, "negative length"), "lengths", v.err);
        }
        std::vector<uint8_t> t = blob;
        const int64_t other = 96;
        memcpy(t.data() + len_at, &other, 8);
        reseal(t);
        Verdict v = check(t, n, fp);
        EXPECT(v.rc != 0, "lengths", "a section of another length was accepted");
        // the last section's length one past what is left
        const Found& last = v0.found[specs.size() - 1];
        t = blob;
        const int64_t past = (n - 8 - last.off) + 1;
        memcpy(t.data() + last.off - 8, &past, 8);
        reseal(t);
        v = check(t, n, fp);
        EXPECT(v.rc != 0 && has(v.err, "runs past the end"), "lengths", v.err);
        printf("ok lengths\n");
    }
    // ---- tags: unknown, duplicate, missing, a store section in a blob that says it has none
    {
        std::vector<uint32_t> o = full_order(true);
        o.push_back(fourcc('X', 'Y', 'Z', 'W'));
        std::vector<uint8_t> t = write_blob(fp, x, true, o);
        Verdict v = check(t, (int64_t)t.size(), fp);
        EXPECT(v.rc != 0 && has(v.err, "unknown section XYZW"), "tags", v.err);
        o = full_order(true); o.push_back(T_M);
        t = write_blob(fp, x, true, o);
        v = check(t, (int64_t)t.size(), fp);
        EXPECT(v.rc != 0 && has(v.err, "duplicate section M"), "tags", v.err);
        for (size_t drop = 0; drop < full_order(true).size(); ++drop) {
            o = full_order(true);
            const uint32_t gone = o[drop];
            o.erase(o.begin() + (long)drop);
            t = write_blob(fp, x, true, o);
            v = check(t, (int64_t)t.size(), fp);
            EXPECT(v.rc != 0 && has(v.err, ("missing section " + tag_name(gone)).c_str()), "tags", v.err);
        }
        o = full_order(false); o.push_back(T_GEOM);
        t = write_blob(fp, x, false, o);
        v = check(t, (int64_t)t.size(), fp);
        EXPECT(v.rc != 0 && has(v.err, "blob without the store"), "tags", v.err);
        // the header's section count
        t = blob;
        uint32_t cnt; memcpy(&cnt, t.data() + 20, 4); cnt += 1; memcpy(t.data() + 20, &cnt, 4);
        reseal(t);
        v = check(t, n, fp);
        EXPECT(v.rc != 0 && has(v.err, "counts"), "tags", v.err);
        printf("ok tags\n");
    }
    // ---- header: magic, version, flags, non-zero padding -- behind a valid checksum
    {
        std::vector<uint8_t> t = blob;
        t[0] ^= 1; reseal(t);
        Verdict v = check(t, n, fp);
        EXPECT(v.rc != 0 && has(v.err, "magic"), "header", v.err);
        t = blob; t[8] = 2; reseal(t);
        v = check(t, n, fp);
        EXPECT(v.rc != 0 && has(v.err, "version 2"), "header", v.err);
        t = blob; t[12] |= 4; reseal(t);
        v = check(t, n, fp);
        EXPECT(v.rc != 0 && has(v.err, "flags"), "header", v.err);
        Verdict v0 = check(blob, n, fp);
        t = blob; t[(size_t)(v0.found[3].off + 7)] = 1; reseal(t);       // RMS: 7 bytes + 1 of padding
        v = check(t, n, fp);
        EXPECT(v.rc != 0 && has(v.err, "padding"), "header", v.err);
        // a valid blob with words appended: the sum covers the length, so zeros (or a second sum) behind it do not pass
        for (int extra = 1; extra <= 3; ++extra) {
            t = blob;
            t.resize(blob.size() + 8 * (size_t)extra, 0);
            v = check(t, (int64_t)t.size(), fp);
            EXPECT(v.rc != 0 && has(v.err, "checksum"), "header", v.err);
        }
        printf("ok header\n");
    }
    // ---- every fingerprint field in turn: refused, the message names the field and both values
    {
        for (int f = 0; f < F_N; ++f) {
            Fingerprint other = fp;
            other.v[f] += 1;
            const std::vector<uint8_t> t = write_blob(other, x, true, full_order(true));
            Verdict v = check(t, (int64_t)t.size(), fp);
            const std::string want = std::string(FIELD_NAMES[f]) + " differs: the blob has " + std::to_string(other.v[f]) + ", this context " +
                                     std::to_string(fp.v[f]);
            EXPECT(v.rc != 0 && has(v.err, want.c_str()), "fingerprint", std::string(FIELD_NAMES[f]) + ": " + v.err);
            for (int g = 0; g < F_N; ++g)
                EXPECT(g == f || !has(v.err, (std::string(" ") + FIELD_NAMES[g] + " differs").c_str()), "fingerprint", "names another field: " + v.err);
        }
        printf("ok fingerprint fields=%d\n", (int)F_N);
    }
    // ---- the store's bookkeeping and the host's scalars
    {
        std::string err;
        int64_t col_len[6];
        for (int k = 0; k < 6; ++k) col_len[k] = LIVE * column_width(DIMS, k);
        auto store_rc = [&](const int64_t* geom, const std::vector<BookRow>& book, const int64_t* cl) {
            err.clear();
            return validate_store((const uint8_t*)geom, (const uint8_t*)book.data(), cl, DIMS, err);
        };
        EXPECT(store_rc(x.geom, x.book, col_len) == 0, "store", err);
        int refused = 0;
        const int64_t geoms[][2] = {{5, 4}, {5, 0}, {0, 3}, {7, 3}, {INT64_MAX, 3}, {-5, 3}, {5, -1}};
        for (auto& g : geoms) { EXPECT(store_rc(g, x.book, col_len) != 0, "store", "geometry accepted"); refused += 1; }
        const BookRow bad_rows[] = {{2, 6, 1, 4, 0, 0}, {5, 5, 4, 0, 0, 0}, {-1, 5, 1, 0, 0, 0}, {2, 3, 1, 0, 0, 0}, {3, 3, 1, 0, 0, 0},
                                    {3, 3, 2, 5, 0, 0}, {3, 3, 2, 0, 0, -1}, {3, 3, 2, 0, 0, (int64_t)1 << 40}, {0, 0, 3, 0, 0, 0},
                                    {2, -5, 1, 0, 0, 0}, {2, INT64_MAX, 1, 0, 0, 0}};
        for (const BookRow& r : bad_rows) {
            std::vector<BookRow> book = x.book;
            book[2] = r;
            int64_t cl[6];
            const int64_t rows = 5 + (r.size > 0 && r.size <= 5 ? r.size : 0);
            for (int k = 0; k < 6; ++k) cl[k] = rows * column_width(DIMS, k);
            EXPECT(store_rc(x.geom, book, cl) != 0, "store", "a book no sequence of pushes produces was accepted");
            refused += 1;
        }
        const int64_t two[2] = {5, 2};                  // sub-buffer 2 is past the store's two and not empty
        EXPECT(store_rc(two, x.book, col_len) != 0 && has(err, "past the store"), "store", err);
        for (int k = 0; k < 6; ++k) {
            int64_t cl[6];
            memcpy(cl, col_len, sizeof(cl));
            cl[k] += column_width(DIMS, k);
            EXPECT(store_rc(x.geom, x.book, cl) != 0 && has(err, "live rows"), "store", err);
            refused += 1;
        }
        HostSlots h = x.host;
        EXPECT(validate_host((const uint8_t*)h.s, err) == 0, "host", err);
        h.put_i(H_SAC_N_UPDATES, -1);
        EXPECT(validate_host((const uint8_t*)h.s, err) != 0, "host", "a negative update counter was accepted");
        h = x.host; h.put_d(H_LR1, NAN);
        EXPECT(validate_host((const uint8_t*)h.s, err) != 0, "host", "a NaN rate was accepted");
        h = x.host; h.put_d(H_LR0, -1.0);
        EXPECT(validate_host((const uint8_t*)h.s, err) != 0, "host", "a negative rate was accepted");
        h = x.host; h.s[H_SLOTS - 1] = 1;
        EXPECT(validate_host((const uint8_t*)h.s, err) != 0, "host", "a used spare slot was accepted");
        printf("ok store_and_host refused=%d\n", refused + 5);
    }
    // ---- the writer refuses a buffer that is too small, at every size
    {
        for (int64_t cap = 0; cap < n; cap += 1) {
            std::vector<uint8_t> buf((size_t)cap);
            Writer w(buf.data(), cap);
            w.header(fp, 0, 1);
            uint8_t* p = w.ok ? w.section(T_P, n - HEADER_BYTES - SECTION_HEAD - 8 - 4) : nullptr;
            EXPECT(p == nullptr || w.finish() < 0 || cap >= n, "writer_bounds", "wrote past a buffer of " + std::to_string(cap));
        }
        printf("ok writer_bounds\n");
    }
    return 0;
}
