// dev_mem_sim.cpp -- fsrl_amd/csrc/dev_mem.hpp over a checking malloc backend (tests/test_dev_mem_host.py builds this with the address /
// undefined-behaviour sanitizers and runs it as its own process).  The backend counts live blocks and bytes per kind at the choke point
// (what HipMem::live is in the library) AND keeps the set of blocks it handed out; it poisons a block before it takes it back, aborts
// on a block it did not hand out or already took back, fails the n-th allocation on request, and can hand a freed address out again.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <vector>

#include "dev_mem.hpp"

struct SimMem {
    using Err = int;
    static constexpr Err ok = 0, bad = 22;
    struct Blk { size_t bytes; bool pin; };
    static inline std::map<void*, Blk> out;                 // every block handed out and not taken back
    static inline std::vector<std::pair<void*, size_t>> kept;   // recycle mode: freed blocks, handed out again first
    static inline long live[4] = {0, 0, 0, 0};              // device blocks, device bytes, pinned blocks, pinned bytes
    static inline long n_alloc = 0, n_free = 0, fail_at = -1;   // fail_at: allocations from now until the one that fails (0 = the next)
    static inline bool recycle = false;
    static Err alloc(void** p, size_t n, bool pin) {
        if (fail_at >= 0 && fail_at-- == 0) return 2;
        void* q = nullptr;
        for (size_t i = 0; i < kept.size() && !q; ++i)
            if (kept[i].second >= n) { q = kept[i].first; kept.erase(kept.begin() + (long)i); }
        if (!q) q = malloc(n);
        if (!q) return 2;
        if (out.count(q)) { fprintf(stderr, "backend handed %p out twice\n", q); abort(); }
        out[q] = Blk{n, pin};
        live[pin ? 2 : 0] += 1; live[pin ? 3 : 1] += (long)n;
        n_alloc += 1;
        *p = q;
        return ok;
    }
    static Err release(void* p, size_t n, bool pin) {
        auto it = out.find(p);
        if (it == out.end()) { fprintf(stderr, "free of %p: not handed out, or already taken back\n", p); abort(); }
        if (it->second.bytes != n || it->second.pin != pin) { fprintf(stderr, "free of %p with the wrong size or kind\n", p); abort(); }
        memset(p, 0xDD, n);
        out.erase(it);
        live[pin ? 2 : 0] -= 1; live[pin ? 3 : 1] -= (long)n;
        n_free += 1;
        if (recycle) kept.emplace_back(p, n); else free(p);
        return ok;
    }
    static Err dev_alloc(void** p, size_t n) { return alloc(p, n, false); }
    static Err host_alloc(void** p, size_t n) { return alloc(p, n, true); }
    static Err dev_free(void* p, size_t n) { return release(p, n, false); }
    static Err host_free(void* p, size_t n) { return release(p, n, true); }
    static bool empty() { return out.empty() && !live[0] && !live[1] && !live[2] && !live[3]; }
    static bool holds(const void* p, size_t n) { auto it = out.find(const_cast<void*>(p)); return it != out.end() && it->second.bytes == n; }
};
using Own = MemOwner<SimMem>;

#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: REQUIRE(%s) failed\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

static void case_release_all() {
    std::mt19937 rng(7);
    Own m;
    std::vector<float*> f(200, nullptr);
    std::vector<int> order(200);
    for (int i = 0; i < 200; ++i) order[(size_t)i] = i;
    std::shuffle(order.begin(), order.end(), rng);
    long bytes[2] = {0, 0}, blocks[2] = {0, 0};
    for (int i : order) {
        const size_t n = 1 + rng() % 5000;
        const bool pin = rng() & 1;
        REQUIRE((pin ? m.pinned(&f[(size_t)i], n) : m.dev(&f[(size_t)i], n)) == SimMem::ok);
        memset(f[(size_t)i], 1, n);
        bytes[pin] += (long)n; blocks[pin] += 1;
    }
    REQUIRE(SimMem::live[0] == blocks[0] && SimMem::live[1] == bytes[0] && SimMem::live[2] == blocks[1] && SimMem::live[3] == bytes[1]);
    REQUIRE(SimMem::out.size() == 200);
    m.release_all();
    REQUIRE(SimMem::empty());
    m.release_all();                                    // nothing left: nothing freed twice
    REQUIRE(SimMem::empty());
    puts("ok release_all");
}

static void case_release() {
    Own m, other;
    int* a = nullptr;
    const long frees = SimMem::n_free;
    REQUIRE(m.release(&a) == SimMem::ok && SimMem::n_free == frees);     // a null field
    double* theirs = nullptr;
    REQUIRE(other.dev(&theirs, 64) == SimMem::ok);
    double* alias = theirs;
    REQUIRE(m.release(&alias) == SimMem::bad);                           // a pointer this owner does not hold: refused ...
    REQUIRE(alias == theirs && SimMem::n_free == frees && SimMem::holds(theirs, 64));    // ... and not freed
    theirs[7] = 1.0;
    REQUIRE(m.pinned(&a, 40) == SimMem::ok && a);
    int* interior = a + 1;
    REQUIRE(m.release(&interior) == SimMem::bad);                        // an alias into an own block is not the block
    REQUIRE(m.release(&a) == SimMem::ok && a == nullptr && SimMem::n_free == frees + 1);
    REQUIRE(m.release(&a) == SimMem::ok && SimMem::n_free == frees + 1); // released: null, and again a no-op
    other.release_all();
    REQUIRE(SimMem::empty());
    puts("ok release");
}

static void case_regrow() {
    Own m;
    int cap = 0;
    float *x = nullptr, *y = nullptr; char* h = nullptr;
    auto grow = [&](int need, int to) { return m.regrow(cap, need, to, {Own::D(&x, (size_t)to * 4), Own::D(&y, (size_t)to * 8), Own::H(&h, (size_t)to)}); };
    REQUIRE(grow(10, 16) == SimMem::ok && cap == 16);
    REQUIRE(SimMem::holds(x, 64) && SimMem::holds(y, 128) && SimMem::holds(h, 16) && SimMem::out.size() == 3);
    float *x0 = x, *y0 = y; char* h0 = h;
    const long allocs = SimMem::n_alloc, frees = SimMem::n_free;
    REQUIRE(grow(16, 99) == SimMem::ok && grow(3, 99) == SimMem::ok);    // need <= cap: nothing happens
    REQUIRE(SimMem::n_alloc == allocs && SimMem::n_free == frees && cap == 16 && x == x0 && y == y0 && h == h0);
    REQUIRE(grow(17, 40) == SimMem::ok && cap == 40);
    REQUIRE(SimMem::n_free == frees + 3 && SimMem::n_alloc == allocs + 3);   // every old block freed exactly once (the backend aborts on twice)
    REQUIRE(!SimMem::out.count(x0) && !SimMem::out.count(y0) && !SimMem::out.count(h0));
    REQUIRE(SimMem::holds(x, 160) && SimMem::holds(y, 320) && SimMem::holds(h, 40) && SimMem::out.size() == 3);
    bool flag = false;                                                       // a bool capacity ("the tangent buffers exist")
    float* r = nullptr;
    REQUIRE(m.regrow(flag, true, true, {Own::D(&r, 8)}) == SimMem::ok && flag && SimMem::holds(r, 8));
    float* z = nullptr;                                                      // bytes == 0: the member stays null
    size_t cz = 0;
    REQUIRE(m.regrow(cz, (size_t)1, (size_t)1, {Own::D(&z, 0), Own::D(&r, 24)}) == SimMem::ok && z == nullptr && SimMem::holds(r, 24));
    m.release_all();
    REQUIRE(SimMem::empty());
    puts("ok regrow");
}

// a set of `nset` buffers at capacity 64; the regrow to 128 fails at allocation `at`; then a call that needs LESS than the old capacity
static void regrow_fails_one(int nset, int at) {
    Own m;
    int cap = 0;
    std::vector<float*> f((size_t)nset, nullptr);
    auto grow = [&](int need) {
        // the largest set of the library's named regrows: ensure_ppo_buffers' seven; lay_work_ensure's is one
        const size_t b = (size_t)need * 4;
        if (nset == 1) return m.regrow(cap, need, need, {Own::D(&f[0], b)});
        return m.regrow(cap, need, need, {Own::D(&f[0], b), Own::D(&f[1], b), Own::D(&f[2], b), Own::D(&f[3], b), Own::D(&f[4], b + 4),
                                          Own::H(&f[5], b + 8), Own::D(&f[6], b + 12)});
    };
    auto size_of = [&](int i, int need) { return (size_t)need * 4 + (nset == 1 ? 0 : i == 4 ? 4 : i == 5 ? 8 : i == 6 ? 12 : 0); };
    REQUIRE(grow(64) == SimMem::ok && cap == 64 && (int)SimMem::out.size() == nset);
    SimMem::fail_at = at;
    REQUIRE(grow(128) != SimMem::ok);
    REQUIRE(SimMem::fail_at < 0);                                        // the injected failure was the one that ended the call
    REQUIRE(cap == 0);
    int named = 0;
    for (int i = 0; i < nset; ++i)
        if (f[(size_t)i]) { REQUIRE(SimMem::holds(f[(size_t)i], size_of(i, 128))); named += 1; }
    REQUIRE(named == at && (int)SimMem::out.size() == named);           // the backend holds exactly the blocks the fields name
    REQUIRE(grow(32) == SimMem::ok && cap == 32);                        // smaller than the OLD capacity: allocates again
    for (int i = 0; i < nset; ++i) { REQUIRE(SimMem::holds(f[(size_t)i], size_of(i, 32))); memset(f[(size_t)i], 0, size_of(i, 32)); }
    REQUIRE((int)SimMem::out.size() == nset);
    m.release_all();
    REQUIRE(SimMem::empty());
}
static void case_regrow_fails() {
    for (int at = 0; at < 7; ++at) regrow_fails_one(7, at);
    regrow_fails_one(1, 0);
    puts("ok regrow_fails");
}

static void case_reuse() {
    SimMem::recycle = true;
    Own a, b;
    float *pa = nullptr, *pb = nullptr;
    REQUIRE(a.dev(&pa, 256) == SimMem::ok);
    float* first = pa;
    REQUIRE(a.release(&pa) == SimMem::ok);
    REQUIRE(b.dev(&pb, 256) == SimMem::ok && pb == first);               // the same address, now b's
    float* stale = first;
    REQUIRE(a.release(&stale) == SimMem::bad && SimMem::holds(pb, 256)); // a forgot it: it does not free b's block
    REQUIRE(a.dev(&pa, 256) == SimMem::ok && pa != pb);
    a.release_all();
    REQUIRE(SimMem::holds(pb, 256) && SimMem::out.size() == 1);
    float* gone = pa;
    REQUIRE(b.release(&gone) == SimMem::bad);                            // nor does b free a's
    b.release_all();
    REQUIRE(SimMem::empty());
    SimMem::recycle = false;
    for (auto& k : SimMem::kept) free(k.first);
    SimMem::kept.clear();
    puts("ok reuse");
}

int main() {
    case_release_all();
    case_release();
    case_regrow();
    case_regrow_fails();
    case_reuse();
    return 0;
}
