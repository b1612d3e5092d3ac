// resident_ring_sim.cpp -- resident_ring.hpp (the host protocol of the resident actor kernels) against a kernel made of host threads.
// One thread per workgroup repeats the device loop of actor_resident_kernel / actor_group_resident_kernel on plain memory: poll the
// bell against the last sequence number seen, give up after the idle timeout and store the generation in state[b], serve a request
// by writing its rows' answers tagged with the request's sequence number and then done[b] = seq, end on EXIT.  The fake stream is
// busy while a thread of any generation runs.  Every branch of the protocol that cannot be provoked on a GPU runs here, under the
// thread sanitizer and under the address / undefined-behaviour sanitizers (tests/test_resident_ring.py builds and runs both).
//   g++ -std=c++17 -O1 -g -pthread -fsanitize=thread -I fsrl_amd/csrc tests/host/resident_ring_sim.cpp
#include "resident_ring.hpp"

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <thread>
#include <vector>

static constexpr int MAX_WG = 16;
enum Mode { NORMAL, MUTE /* never answers, still ends on EXIT and on its idle timeout */, VANISH /* ends at once, stores nothing */ };

struct Fake {
    ResidentRing r;
    // the "pinned" memory
    unsigned long long bell = 0;
    unsigned k_m[RR_MAX_MEMBERS] = {}, done[MAX_WG] = {}, state[MAX_WG] = {};
    unsigned obs[MAX_WG * 16] = {}, out[MAX_WG * 16] = {};      // one word per row
    bool group_style = false;                   // rows from k_m[member] (the group kernel) or from the command word (the solo kernel)
    int wg_member[MAX_WG] = {}, wg_tile[MAX_WG] = {};
    std::atomic<int> running{0}, started{0}, mode{NORMAL}, query_override{-1};
    std::atomic<unsigned> cur_gen{0};
    std::vector<unsigned> served[MAX_WG];       // the tags workgroup b answered with, in order (its threads' own; read after join)
    std::atomic<long> heard_by_old_gen{0}, launched_early{0}, bad_last_seq{0};
    double exit_delay_us = 0.0;                 // between the EXIT command and the state word
    bool expect_ended = true;                   // the launch hook checks that the last generation has stored every state word
    std::vector<std::thread> threads;
    // what the test itself saw go out: the bell's sequence number after its last call, and whether that call left a kernel live
    // (the ring then sends an EXIT of its own before it launches).  The launch hook checks last_seq against these.
    unsigned sent = 0;
    bool told_live = false;
    // scenario (b)'s clock is simulated, so that nothing there depends on how long this machine takes to start or schedule a
    // thread: the workgroups read it for their idle timers, pass() moves it.  Workgroup b gives up 2 b us later than workgroup 0
    // (on the GPU they do not start to poll at the same instant either), so that a gap can fall between two ends.
    bool simulated = false;
    std::atomic<long long> sim_us{0};
    std::atomic<long long> deadline[MAX_WG];    // simulated time at which workgroup b gives up; published when it starts to poll ...
    std::atomic<unsigned> polling[MAX_WG];      // ... for a sequence number other than this one
    double now() const { return simulated ? (double)sim_us.load() : rr_now_us(); }

    Fake(bool group, std::vector<int> tiles) : group_style(group) {
        r.n = (int)tiles.size();
        for (int i = 0, b = 0; i < r.n; ++i) {
            r.base[i] = b; r.tiles[i] = tiles[(size_t)i];
            for (int t = 0; t < tiles[(size_t)i]; ++t, ++b) { wg_member[b] = i; wg_tile[b] = t; }
            r.blocks = b;
        }
        r.bell = &bell; r.done = done; r.state = state;
        r.launch = launch; r.query = query; r.owner = this;
        r.idle_us = 1.0e6;
        for (int b = 0; b < MAX_WG; ++b) { deadline[b] = 0; polling[b] = 0; }
    }
    ~Fake() { release(); join(); }
    void join() { for (auto& t : threads) t.join(); threads.clear(); }

    static unsigned answer(unsigned x, unsigned seq) { return x * 2654435761u + seq; }

    void workgroup(int b, unsigned gen, unsigned last, double timeout_us) {
        const int mem = wg_member[b], tile = wg_tile[b];
        // the workgroups of one launch start together (a thread takes longer to start than the shortest idle timeout used here)
        for (started += 1; started.load() < r.blocks;) std::this_thread::yield();
        const double limit = timeout_us + (simulated ? 2.0 * b : 0.0);
        while (mode.load() != VANISH) {
            const double t0 = now();
            deadline[b] = (long long)(t0 + limit); polling[b] = last;
            unsigned long long v;
            for (;;) {
                // (the kernel: a relaxed load and an acquire fence behind the loop; the thread sanitizer does not model fences)
                v = __atomic_load_n(&bell, __ATOMIC_ACQUIRE);
                if ((unsigned)v != last) break;
                if (now() - t0 > limit) { v = (unsigned long long)RR_EXIT << 32; break; }
                std::this_thread::yield();
            }
            const unsigned cmd = (unsigned)(v >> 32), seq = (unsigned)v;
            last = seq;
            if (cmd == RR_EXIT) break;
            if (gen != cur_gen.load()) heard_by_old_gen += 1;    // a request doorbell is only ever heard by the current generation
            if (mode.load() == MUTE) continue;
            const unsigned k = group_style ? __atomic_load_n(k_m + mem, __ATOMIC_RELAXED) : cmd;
            const int n_valid = std::min(16, (int)k - tile * 16);
            if (n_valid <= 0) continue;
            for (int i = 0; i < n_valid; ++i) out[b * 16 + i] = answer(__atomic_load_n(obs + b * 16 + i, __ATOMIC_RELAXED), seq);
            served[b].push_back(seq);
            __atomic_store_n(done + b, seq, __ATOMIC_RELEASE);
        }
        if (mode.load() != VANISH) {
            if (exit_delay_us > 0.0) std::this_thread::sleep_for(std::chrono::microseconds((long)exit_delay_us));
            __atomic_store_n(state + b, gen, __ATOMIC_RELEASE);
        }
        running -= 1;
    }

    static int launch(void* owner, ResidentRing& r, unsigned last_seq) {
        Fake& f = *(Fake*)owner;
        const unsigned prev = f.cur_gen.load();
        if (f.expect_ended && prev)
            for (int b = 0; b < r.blocks; ++b) f.launched_early += __atomic_load_n(f.state + b, __ATOMIC_ACQUIRE) != prev;
        const unsigned expect = f.told_live ? (f.sent == 0xFFFFFFFFu ? 1u : f.sent + 1u) : f.sent;
        if ((f.expect_ended && last_seq != expect) || r.gen == 0) f.bad_last_seq += 1;
        f.join();                                                // (they are on their way out, or gone)
        f.cur_gen = r.gen;
        f.running += r.blocks; f.started = 0;
        for (int b = 0; b < r.blocks; ++b) f.threads.emplace_back(&Fake::workgroup, &f, b, r.gen, last_seq, r.idle_us);
        return 0;
    }
    static int query(void* owner) {
        Fake& f = *(Fake*)owner;
        const int o = f.query_override.load();
        return o >= 0 ? o : f.running.load() > 0 ? RR_STREAM_BUSY : RR_STREAM_IDLE;
    }

    // what pactor_post / gactor_post do: the rows, the row counts, the request.  The kernels read both with relaxed atomic loads,
    // and the group kernel may do so late: a workgroup WITHOUT rows in request s answers to nobody, so nothing orders its read of
    // k_m behind the host's later writes.  It can then take a later request's rows for s's, and answers them with the tag s, which the
    // host never waits for, before it answers that request properly.  (The solo kernel's row count is in the command word itself.)
    int post(const std::vector<int>& k, std::mt19937& rng) {
        for (int i = 0; i < r.n; ++i) {
            for (int j = 0; j < k[(size_t)i]; ++j) __atomic_store_n(obs + r.base[i] * 16 + j, (unsigned)rng() | 1u, __ATOMIC_RELAXED);
            __atomic_store_n(k_m + i, (unsigned)k[(size_t)i], __ATOMIC_RELAXED);
            r.k[i] = k[(size_t)i];
        }
        const int rc = rr_request(r, group_style ? 1u : (unsigned)k[0]);
        sent = (unsigned)bell; told_live = r.live;
        return rc;
    }
    int wait() {
        const int rc = rr_wait(r);
        sent = (unsigned)bell; told_live = r.live;
        return rc;
    }
    void release() { rr_release(r); sent = (unsigned)bell; told_live = false; }
    // `us` of simulated time pass.  First, what takes no time has happened: every workgroup still there has seen the last command and
    // polls again.  settle: what the time brings has happened too -- a workgroup whose idle timeout has run out has ended.  Without
    // it the next doorbell races those ends, as on the GPU a doorbell rung around the timeout does.
    void pass(long long us, bool settle) {
        const unsigned gen = cur_gen.load();
        auto ended = [&](int b) { return __atomic_load_n(state + b, __ATOMIC_ACQUIRE) == gen; };
        for (int b = 0; b < r.blocks; ++b)
            while (polling[b].load() != r.seq && !ended(b)) std::this_thread::yield();
        sim_us += us;
        for (int b = 0; settle && b < r.blocks; ++b)
            while (sim_us.load() > deadline[b].load() && !ended(b)) std::this_thread::yield();
    }
    // every row of the request in flight carries this request's tag
    bool answered(const std::vector<int>& k) const {
        for (int i = 0; i < r.n; ++i)
            for (int j = 0; j < k[(size_t)i]; ++j)
                if (out[r.base[i] * 16 + j] != answer(obs[r.base[i] * 16 + j], r.seq)) return false;
        return true;
    }
    bool clean() const { return heard_by_old_gen == 0 && launched_early == 0 && bad_last_seq == 0; }
};

#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

static std::vector<int> random_rows(const Fake& f, std::mt19937& rng) {
    std::vector<int> k((size_t)f.r.n);
    int total = 0;
    while (total == 0) {                                         // a request has rows; a member of a group may have none
        total = 0;
        for (int i = 0; i < f.r.n; ++i) total += k[(size_t)i] = (int)(rng() % (unsigned)(16 * f.r.tiles[i] + 1));
    }
    return k;
}

// (a) every request is answered once, with its own tag, by the workgroups that have rows and no others
static void scenario_a(bool group, std::vector<int> tiles) {
    Fake f(group, tiles);
    std::mt19937 rng(1);
    const int n_req = 3000;
    std::vector<std::vector<char>> rows((size_t)n_req + 1, std::vector<char>(MAX_WG, 0));      // [seq][b]: b had rows in request seq
    for (int it = 0; it < n_req; ++it) {
        const std::vector<int> k = random_rows(f, rng);
        REQUIRE(f.post(k, rng) == RR_OK && f.wait() == RR_OK && f.answered(k) && f.r.seq == (unsigned)it + 1u);
        for (int i = 0; i < f.r.n; ++i)
            for (int t = 0; t < (k[(size_t)i] + 15) / 16; ++t) rows[f.r.seq][(size_t)(f.r.base[i] + t)] = 1;
    }
    f.release(); f.join();
    for (int b = 0; b < f.r.blocks; ++b) {
        std::vector<int> count((size_t)n_req + 2, 0);
        for (unsigned tag : f.served[b]) { REQUIRE(tag >= 1 && tag <= (unsigned)n_req); count[tag] += 1; }
        for (int s = 1; s <= n_req; ++s)        // once where it had rows; elsewhere never, but for the group kernel's late read (Fake::post)
            REQUIRE(count[(size_t)s] == rows[(size_t)s][(size_t)b] || (group && !rows[(size_t)s][(size_t)b] && count[(size_t)s] == 1));
    }
    int64_t st[3];
    rr_stats(f.r, st);
    REQUIRE(st[0] == 1 && st[1] == n_req && st[2] == 0 && f.clean());
}

// (b) calls spaced 0.6 .. 1.4 idle timeouts apart, on the simulated clock: every request answered, those after a short gap by the
//     kernel that was still there, those after a long gap by a new one, and every fourth long gap racing the workgroups' ends
static void scenario_b() {
    Fake f(false, {2});
    std::mt19937 rng(2);
    f.simulated = true;
    REQUIRE(rr_set_resident(f.r, 1, 50.0) == RR_OK);
    const int n_req = 1000;
    long settled = 0, raced = 0;
    for (int it = 0; it < n_req; ++it) {
        const std::vector<int> k = {1 + (int)(rng() % 32u)};
        REQUIRE(f.post(k, rng) == RR_OK && f.wait() == RR_OK && f.answered(k));
        const long long gap = 30 + (long long)(rng() % 41u);    // 30 .. 70 us; workgroup 0 gives up after more than 50, workgroup 1 after 52
        const bool race = gap > 50 && it % 4 == 3;
        f.pass(gap, !race);
        if (it + 1 < n_req) { settled += gap > 50 && !race; raced += race; }
    }
    printf("    b: %lld launches for %lld requests (%ld gaps past the timeout, %ld more racing it)\n", f.r.launches, f.r.requests, settled, raced);
    // the first launch, one for every gap that outlasted a workgroup, at most one for a gap that raced one
    REQUIRE(f.r.requests == n_req && f.r.launches >= 1 + settled && f.r.launches <= 1 + settled + raced);
    REQUIRE(settled > 0 && f.r.launches > 1 && f.r.launches < n_req && f.clean());
}

// (c) release, then a request at once: the launch waits for every state word of the generation that was told to end
static void scenario_c() {
    Fake f(true, {1, 2, 4});
    std::mt19937 rng(3);
    f.exit_delay_us = 20000.0;
    for (int it = 0; it < 5; ++it) {
        const std::vector<int> k = random_rows(f, rng);
        REQUIRE(f.post(k, rng) == RR_OK && f.wait() == RR_OK && f.answered(k));
        f.release();
        REQUIRE(!f.r.live && rr_ended_count(f.r) < f.r.blocks);  // release never waits: the workgroups are still on their way out
    }
    REQUIRE(f.r.launches == 5 && f.clean());
}

// (d) the stream reports an error while a request is pending; (e) nothing answers and the stream stays busy: the bound
static void scenario_d_e() {
    for (int e = 0; e < 2; ++e) {
        Fake f(false, {4});
        std::mt19937 rng(4);
        f.mode = MUTE;
        f.r.give_up_us = 0.25e6;
        if (!e) f.query_override = RR_STREAM_ERROR;
        const double t0 = rr_now_us();
        REQUIRE(f.post({40}, rng) == RR_OK);
        const int rc = f.wait();
        const double dt = rr_now_us() - t0;
        if (!e) REQUIRE(rc == RR_ERROR && dt < 0.2e6);
        else REQUIRE(rc == RR_NO_ANSWER && dt >= 0.25e6 && dt < 2.0e6);
    }
}

// (f) the stream goes idle without an answer (the kernel is gone and has stored nothing): relaunch, ring again
static void scenario_f() {
    Fake f(true, {2, 1});
    std::mt19937 rng(5);
    f.expect_ended = false;
    f.mode = VANISH;
    const std::vector<int> k = {20, 3};
    REQUIRE(f.post(k, rng) == RR_OK);
    while (f.running.load() > 0) std::this_thread::yield();
    f.mode = NORMAL;
    REQUIRE(f.wait() == RR_OK && f.answered(k) && f.r.launches == 2 && f.r.requests == 1 && f.r.live);
}

// (g) both numbers across their wrap, with relaunches: neither is ever 0, and tiles that were never served (done == 0) get their
//     first rows in the very request whose sequence number follows 0xFFFFFFFF
static void scenario_g() {
    Fake f(false, {4});
    std::mt19937 rng(6);
    f.r.seq = 0xFFFFFFF0u; f.bell = f.sent = 0xFFFFFFF0u;
    f.r.gen = 0xFFFFFFFEu; f.cur_gen = 0xFFFFFFFEu;
    for (auto& s : f.state) s = 0xFFFFFFFEu;                     // that generation has ended
    REQUIRE(rr_next(0xFFFFFFFFu) == 1u && rr_next(0u) == 1u);
    bool wrapped = false;
    for (int it = 0; it < 60; ++it) {
        const bool at_wrap = f.r.seq == 0xFFFFFFFFu;
        const std::vector<int> k = {at_wrap || wrapped ? 64 : 5};
        REQUIRE(f.post(k, rng) == RR_OK && f.r.seq != 0 && f.r.gen != 0);
        REQUIRE(f.wait() == RR_OK && f.answered(k));
        wrapped = wrapped || at_wrap;
        if (it % 3 == 2 && (wrapped || f.r.seq < 0xFFFFFFF8u)) { f.release(); REQUIRE(f.r.seq != 0); }
    }
    REQUIRE(wrapped && f.r.seq < 100u && f.r.gen < 100u && f.r.launches > 10 && f.clean());
}

int main() {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    struct { const char* name; void (*run)(); } all[] = {
        {"a: 1 member x 4 tiles", [] { scenario_a(false, {4}); }}, {"a: 3 members x {1, 2, 4} tiles", [] { scenario_a(true, {1, 2, 4}); }},
        {"b: calls around the idle timeout", scenario_b}, {"c: release then request", scenario_c},
        {"d, e: stream error / no answer", scenario_d_e}, {"f: idle stream without an answer", scenario_f},
        {"g: sequence and generation wrap", scenario_g}};
    for (auto& s : all) {
        const double t0 = rr_now_us();
        s.run();
        printf("ok  %-36s %.2f s\n", s.name, (rr_now_us() - t0) * 1e-6);
    }
    return 0;
}
