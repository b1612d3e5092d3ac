// collect_release_sim.cpp -- the release hook of a collect group (rr_release_guarded, resident_ring.hpp; collect_group_actor_release,
// host_collect_group.inc) under threads, against a kernel made of host threads.  The members of a collect group of on-policy seeds
// run their updates on host threads of their own, and every library entry point of every member releases the SAME ring.  Here 8
// threads hammer that hook while the main thread alternates request and release as a collect step does: the group's mutex held from
// the request to its answer, the hook's mark (`reorder`) read and cleared under it.  The kernel is resident_ring_sim.cpp's: one host
// thread per workgroup that polls the bell, serves a request, ends on EXIT.
// Passes when: it exits 0; every live generation hears exactly one EXIT (a generation launched at bell value s hears its request
// at s + 1 and its EXIT at s + 2, the next launch is told s + 2, and the bell ends at 2 per cycle); `seq` never repeats (every bell
// value a workgroup hears is above the one before); the mark is set whenever a release came since the last request.
//   g++ -std=c++17 -O1 -g -pthread -fsanitize=thread -I fsrl_amd/csrc tests/host/collect_release_sim.cpp
// -DUNGUARDED builds the hook as it was before the mutex (rr_release and a plain store): the thread sanitizer then reports the race
// on `live` / `seq` / the mark.  That build is for showing the race, not part of the test.
#include "resident_ring.hpp"

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <random>
#include <thread>
#include <vector>

#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

static constexpr int MAX_WG = 8;

struct Group {
    ResidentRing r;
    std::mutex mu;
    bool reorder = true;
    // the "pinned" memory
    unsigned long long bell = 0;
    unsigned k_m[RR_MAX_MEMBERS] = {}, done[MAX_WG] = {}, state[MAX_WG] = {};
    unsigned obs[MAX_WG * 16] = {}, out[MAX_WG * 16] = {};
    int wg_member[MAX_WG] = {}, wg_tile[MAX_WG] = {};
    std::atomic<int> running{0};
    std::atomic<long> bad_order{0}, bad_exit{0}, exits_heard{0}, bad_last_seq{0};
    unsigned expect_last = 0;                   // what the next launch must be told: the bell after the last generation's one EXIT
    std::vector<std::thread> threads;

    explicit Group(std::vector<int> tiles) {
        r.n = (int)tiles.size();
        for (int i = 0, b = 0; i < r.n; ++i) {
            r.base[i] = b; r.tiles[i] = tiles[(size_t)i];
            for (int t = 0; t < tiles[(size_t)i]; ++t, ++b) { wg_member[b] = i; wg_tile[b] = t; }
            r.blocks = b;
        }
        r.bell = &bell; r.done = done; r.state = state;
        r.launch = launch; r.query = query; r.owner = this;
        r.idle_us = 60.0e6;                     // no idle timeout here: every end is an EXIT
    }
    void join() { for (auto& t : threads) t.join(); threads.clear(); }

    static unsigned answer(unsigned x, unsigned seq) { return x * 2654435761u + seq; }

    void workgroup(int b, unsigned gen, unsigned last) {
        const int mem = wg_member[b], tile = wg_tile[b];
        const unsigned told = last;                              // the bell at launch: the request follows at + 1, the one EXIT at + 2
        for (;;) {
            unsigned long long v;
            for (;;) {
                v = __atomic_load_n(&bell, __ATOMIC_ACQUIRE);
                if ((unsigned)v != last) break;
                std::this_thread::yield();
            }
            const unsigned cmd = (unsigned)(v >> 32), seq = (unsigned)v;
            if (seq <= last) bad_order += 1;                     // (no wrap in this program's few thousand rings)
            last = seq;
            if (cmd == RR_EXIT) {
                // one EXIT per generation: the very next sequence number behind the request this generation was launched for (a
                // workgroup without rows may hear the EXIT without having looked at the request's doorbell)
                exits_heard += 1;
                if (seq != told + 2u) bad_exit += 1;
                break;
            }
            if (seq != told + 1u) bad_exit += 1;
            const unsigned k = __atomic_load_n(k_m + mem, __ATOMIC_RELAXED);
            const int n_valid = std::min(16, (int)k - tile * 16);
            if (n_valid > 0) {
                for (int i = 0; i < n_valid; ++i) out[b * 16 + i] = answer(__atomic_load_n(obs + b * 16 + i, __ATOMIC_RELAXED), seq);
                __atomic_store_n(done + b, seq, __ATOMIC_RELEASE);
            }
        }
        __atomic_store_n(state + b, gen, __ATOMIC_RELEASE);
        running -= 1;
    }

    static int launch(void* owner, ResidentRing& r, unsigned last_seq) {
        Group& g = *(Group*)owner;
        if (last_seq != g.expect_last) g.bad_last_seq += 1;
        g.join();
        g.running += r.blocks;
        for (int b = 0; b < r.blocks; ++b) g.threads.emplace_back(&Group::workgroup, &g, b, r.gen, last_seq);
        return 0;
    }
    static int query(void* owner) { return ((Group*)owner)->running.load() > 0 ? RR_STREAM_BUSY : RR_STREAM_IDLE; }

    // collect_group_actor_release
    void hook() {
#ifdef UNGUARDED
        rr_release(r); reorder = true;
#else
        rr_release_guarded(r, mu, [this]() { reorder = true; });
#endif
    }
};

int main() {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    Group g({1, 2, 4});
    std::mt19937 rng(11);
    std::atomic<bool> stop{false};
    std::atomic<long> hooks{0};
    std::vector<std::thread> members;
    for (int t = 0; t < 8; ++t)
        members.emplace_back([&]() {
            while (!stop.load()) { g.hook(); hooks += 1; }
        });
    const int cycles = 600;
    for (int it = 0; it < cycles; ++it) {
        std::vector<int> k((size_t)g.r.n);
        {
            std::unique_lock<std::mutex> held(g.mu);             // a step: from the request to its answer
            REQUIRE(g.reorder);                                  // a release came since the last request (the main thread's own, at least)
            g.reorder = false;
            int total = 0;
            while (total == 0)
                for (int i = 0; i < g.r.n; ++i) total += k[(size_t)i] = (int)(rng() % (unsigned)(16 * g.r.tiles[i] + 1));
            for (int i = 0; i < g.r.n; ++i) {
                for (int j = 0; j < k[(size_t)i]; ++j) __atomic_store_n(g.obs + g.r.base[i] * 16 + j, (unsigned)rng() | 1u, __ATOMIC_RELAXED);
                __atomic_store_n(g.k_m + i, (unsigned)k[(size_t)i], __ATOMIC_RELAXED);
                g.r.k[i] = k[(size_t)i];
            }
            REQUIRE(rr_request(g.r, 1u) == RR_OK);
            REQUIRE(rr_wait(g.r) == RR_OK);
            for (int i = 0; i < g.r.n; ++i)
                for (int j = 0; j < k[(size_t)i]; ++j)
                    REQUIRE(g.out[g.r.base[i] * 16 + j] == Group::answer(g.obs[g.r.base[i] * 16 + j], g.r.seq));
            // exactly one launch and one ring for this request, and the one EXIT that follows takes the next number
            REQUIRE(g.r.launches == it + 1 && g.r.requests == it + 1 && g.r.seq == 2u * (unsigned)it + 1u && g.r.live);
            g.expect_last = g.r.seq + 1u;
        }
        g.hook();                                                // the collect is over / a member's entry point on this thread
        {
            std::lock_guard<std::mutex> lock(g.mu);
            REQUIRE(!g.r.live && g.r.seq == 2u * (unsigned)it + 2u && (unsigned)g.bell == g.r.seq && (unsigned)(g.bell >> 32) == RR_EXIT);
        }
    }
    stop = true;
    for (auto& t : members) t.join();
    g.join();
    printf("%d cycles, %ld hook calls on 8 threads, %ld EXITs heard by %d workgroups\n", cycles, hooks.load(), g.exits_heard.load(), g.r.blocks);
    REQUIRE(g.r.seq == 2u * (unsigned)cycles && g.r.launches == cycles && g.r.requests == cycles);
    REQUIRE(g.exits_heard.load() == (long)cycles * g.r.blocks);
    REQUIRE(g.bad_order.load() == 0 && g.bad_exit.load() == 0 && g.bad_last_seq.load() == 0);
    REQUIRE(hooks.load() > cycles);
    printf("ok  one EXIT per live generation, seq never repeats\n");
    return 0;
}
