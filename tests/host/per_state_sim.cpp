// per_state_sim.cpp -- the prioritised-replay section of an exported training state (fsrl_amd/csrc/train_state.hpp: T_PER, PerHead,
// validate_per, SectionSpec::absent) as a stand-alone program: a blob with the section against a context that has prioritised replay
// off, a blob without it against one that has it on, and every way the section's own bytes can be wrong.  Prints "ok <case>" per
// case; exits non-zero at the first expectation that fails (tests/test_per_model.py).
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "train_state.hpp"

using namespace tstate;

#define EXPECT(cond, name, why)                                                                   \
    do {                                                                                          \
        if (!(cond)) { printf("FAIL %s: %s (line %d)\n", name, std::string(why).c_str(), __LINE__); return 1; } \
    } while (0)

static Fingerprint make_fp() {
    Fingerprint fp;
    for (int i = 0; i < F_N; ++i) fp.v[i] = 3 + i;
    return fp;
}

static std::vector<uint8_t> per_payload(const PerHead& h, const std::vector<double>& leaves) {
    std::vector<uint8_t> p((size_t)PER_HEAD_BYTES + 8 * leaves.size());
    memcpy(p.data(), &h, (size_t)PER_HEAD_BYTES);
    if (!leaves.empty()) memcpy(p.data() + PER_HEAD_BYTES, leaves.data(), 8 * leaves.size());
    return p;
}

// a blob of T_HOST and, when per != nullptr, T_PER
static std::vector<uint8_t> write_blob(const Fingerprint& fp, const std::vector<uint8_t>* per) {
    const int64_t lens[2] = {HOST_BYTES, per ? (int64_t)per->size() : 0};
    std::vector<uint8_t> out((size_t)blob_bytes(lens, per ? 2 : 1));
    Writer w(out.data(), (int64_t)out.size());
    w.header(fp, 0u, per ? 2u : 1u);
    HostSlots hs;
    hs.put_d(H_LR0, 1e-3);
    memcpy(w.section(T_HOST, HOST_BYTES), hs.s, (size_t)HOST_BYTES);
    if (per) memcpy(w.section(T_PER, (int64_t)per->size()), per->data(), per->size());
    const int64_t n = w.finish();
    if (n != (int64_t)out.size()) { printf("FAIL writer: %lld bytes, %zu announced\n", (long long)n, out.size()); exit(1); }
    return out;
}

struct Verdict { int rc; std::string err; Found found[2]; };
static Verdict check(const std::vector<uint8_t>& blob, const Fingerprint& fp, bool ctx_has_per) {
    const SectionSpec specs[2] = {{T_HOST, HOST_BYTES, false}, {T_PER, -1, false, !ctx_has_per}};       // three initialisers: absent = false
    Verdict v;
    uint32_t flags = 7;
    v.rc = validate(blob.data(), (int64_t)blob.size(), fp, specs, 2, v.found, &flags, v.err);
    return v;
}
static bool has(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

int main() {
    const Fingerprint fp = make_fp();
    const std::vector<double> leaves = {1.0, 0.0, 2.5, 0.125, 0.0, 3.0};
    const PerHead good{0.6, 0.4, 1, 3.0, 0.125, (int64_t)leaves.size()};
    const std::vector<uint8_t> pay = per_payload(good, leaves);
    const std::vector<uint8_t> with = write_blob(fp, &pay), without = write_blob(fp, nullptr);
    std::string err;

    {   // both sides agree
        Verdict v = check(with, fp, true);
        EXPECT(v.rc == 0 && v.found[1].off >= 0 && v.found[1].len == per_bytes(6), "agree", v.err);
        EXPECT(validate_per(with.data() + v.found[1].off, v.found[1].len, 6, err) == 0, "agree", err);
        PerHead back;
        memcpy(&back, with.data() + v.found[1].off, (size_t)PER_HEAD_BYTES);
        EXPECT(back.alpha == 0.6 && back.beta == 0.4 && back.weight_norm == 1 && back.max_prio == 3.0 && back.min_prio == 0.125 && back.slots == 6,
               "agree", "head differs");
        EXPECT(memcmp(with.data() + v.found[1].off + PER_HEAD_BYTES, leaves.data(), 48) == 0, "agree", "leaves differ");
        Verdict w = check(without, fp, false);
        EXPECT(w.rc == 0 && w.found[1].off < 0, "agree", w.err);
        // a blob without the store: the head alone, slots = 0
        PerHead bare = good;
        bare.slots = 0;
        const std::vector<uint8_t> p0 = per_payload(bare, {});
        EXPECT(validate_per(p0.data(), (int64_t)p0.size(), 0, err) == 0, "agree", err);
        printf("ok agree bytes=%zu\n", with.size());
    }
    {   // the blob has the section, the context has prioritised replay off
        Verdict v = check(with, fp, false);
        EXPECT(v.rc != 0 && has(v.err, "PER_") && has(v.err, "prioritised-replay") && has(v.err, "has it off"), "blob_has_context_has_not", v.err);
        printf("ok blob_has_context_has_not\n");
    }
    {   // the context has it on, the blob does not carry the section
        Verdict v = check(without, fp, true);
        EXPECT(v.rc != 0 && has(v.err, "missing section PER_") && has(v.err, "prioritised replay on"), "context_has_blob_has_not", v.err);
        printf("ok context_has_blob_has_not\n");
    }
    {   // the section's own bytes
        int refused = 0;
        auto bad = [&](PerHead h, std::vector<double> l, int64_t want, const char* what) {
            const std::vector<uint8_t> p = per_payload(h, l);
            std::string e;
            const int rc = validate_per(p.data(), (int64_t)p.size(), want, e);
            if (rc == 0 || !has(e, what)) { printf("FAIL section: expected a refusal naming '%s', got rc %d '%s'\n", what, rc, e.c_str()); exit(1); }
            refused += 1;
        };
        const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
        PerHead h = good;
        h.alpha = -0.1; bad(h, leaves, 6, "alpha and beta");
        h = good; h.alpha = nan; bad(h, leaves, 6, "alpha and beta");
        h = good; h.beta = inf; bad(h, leaves, 6, "alpha and beta");
        h = good; h.weight_norm = 2; bad(h, leaves, 6, "weight_norm");
        h = good; h.min_prio = 0.0; bad(h, leaves, 6, "min_prio");
        h = good; h.min_prio = 4.0; bad(h, leaves, 6, "min_prio");
        h = good; h.max_prio = inf; bad(h, leaves, 6, "max_prio");
        bad(good, leaves, 8, "leaves for 6 slots, the blob's store has 8");       // another geometry
        bad(good, leaves, 0, "leaves for 6 slots");                               // leaves in a blob without the store
        h = good; h.slots = 5; bad(h, leaves, 5, "bytes");                        // the head counts fewer leaves than follow
        h = good; h.slots = 7; bad(h, leaves, 7, "bytes");                        // ... and more: nothing past the end is read
        h = good; h.slots = -1; bad(h, leaves, -1, "bytes");
        h = good; h.slots = std::numeric_limits<int64_t>::max(); bad(h, leaves, h.slots, "bytes");
        std::vector<double> l = leaves;
        l[3] = -1e-300; bad(good, l, 6, "leaf 3");
        l = leaves; l[5] = nan; bad(good, l, 6, "leaf 5");
        l = leaves; l[0] = inf; bad(good, l, 6, "leaf 0");
        for (int64_t n = 0; n < PER_HEAD_BYTES; ++n) {                              // every prefix of the head
            std::string e;
            EXPECT(validate_per(pay.data(), n, 6, e) != 0 && has(e, "shorter than its head"), "section", e);
            refused += 1;
        }
        printf("ok section refused=%d\n", refused);
    }
    return 0;
}
