// resident_ring.hpp -- the host half of the protocol of a resident actor kernel (actor_resident_kernel and
// actor_group_resident_kernel, kernels_mlp.hpp), once, for every owner: a context's own kernel (fsrl_hip.hip), an on-policy group's
// (host_group_collect.inc) and a collect group's (host_collect_group.inc).  No HIP in here: the owner supplies the three
// protocol words in its pinned memory and two hooks -- launch a generation, and ask the kernel's stream -- so the same code runs
// against a kernel made of host threads (tests/host/resident_ring_sim.cpp).
//   request: [wait until every workgroup of the last generation has stored its end] -> launch generation g if none is live -> ring
//            the doorbell (hi << 32 | seq, one release store behind the request's rows);
//   wait:    poll `done[b] == seq` of the request's tiles; if a `state[b] == g` shows up instead (a workgroup ended by its idle
//            timeout just before the doorbell), tell the rest to end, wait for them, launch generation g + 1 and ring again;
//   release: doorbell = EXIT; nothing is waited for (the stream orders what follows behind the kernel).
// A doorbell is only ever rung when generation `gen` is the one kernel that can hear it.
#pragma once
#include <stdint.h>
#include <chrono>
#include <mutex>

#define RR_MAX_MEMBERS 16
#define RR_EXIT 0xFFFFFFFFu                     // the command word that ends the kernel
// The functions return 0, a launch hook's own (negative) error, or one of these.  RR_IDLE (rr_poll only): the stream is idle, so every
// workgroup has ended and nothing else is queued.
enum { RR_OK = 0, RR_IDLE = 1,
       RR_ERROR = 2,                            // the query hook reported an error (and recorded its text)
       RR_NO_ANSWER = 3,                        // nothing for `give_up_us`
       RR_BAD_TIMEOUT = 4 };                    // rr_set_resident: idle_timeout_us above one second
enum { RR_STREAM_IDLE = 0, RR_STREAM_BUSY = 1, RR_STREAM_ERROR = 2 };      // the query hook's answers

struct ResidentRing {
    bool on = true;                             // *_actor_set_resident
    bool live = false;                          // a kernel of generation gen was launched and not told to end
    unsigned gen = 0, seq = 0, hi = 0;          // hi: the command word of the request in flight (a re-ring repeats it)
    double idle_us = 2000.0, give_up_us = 20.0e6;
    int n = 0;                                  // members (a context's own ring: one, with base 0)
    int blocks = 0;                             // workgroups of every launch: sum of tiles
    int base[RR_MAX_MEMBERS] = {}, tiles[RR_MAX_MEMBERS] = {};   // member m: workgroups base[m] .. + tiles[m] - 1
    int k[RR_MAX_MEMBERS] = {};                 // rows of each member in the request in flight
    unsigned long long* bell = nullptr;         // pinned, the owner's: (hi << 32) | seq
    unsigned* done = nullptr;                   // pinned [blocks]: seq of the last request workgroup b served; starts at 0
    unsigned* state = nullptr;                  // pinned [blocks]: generation of the last kernel whose workgroup b ended; starts at 0
    long long launches = 0, requests = 0;       // *_actor_resident_stats
    int (*launch)(void* owner, ResidentRing& r, unsigned last_seq) = nullptr;   // launches generation r.gen: 0 or the owner's error
    int (*query)(void* owner) = nullptr;        // RR_STREAM_* of the stream the kernel runs on
    void* owner = nullptr;
};

// sequence and generation numbers skip 0, where the pinned words start: a tile never served must not look served
static inline unsigned rr_next(unsigned v) { return v + 1u ? v + 1u : 1u; }

static inline void rr_command(ResidentRing& r, unsigned hi) {
    r.seq = rr_next(r.seq);
    __atomic_store_n(r.bell, ((unsigned long long)hi << 32) | r.seq, __ATOMIC_RELEASE);
}

// release never waits
static inline void rr_release(ResidentRing& r) {
    if (!r.live) return;
    rr_command(r, RR_EXIT);
    r.live = false;
}

// Release from any number of host threads at once (a collect group's hook, host_collect_group.inc: its members' entry points run on
// threads of their own and every one of them releases the SAME ring).  Under the owner's mutex one thread tests `live`, rings EXIT and
// clears `live`, so a live generation hears exactly one EXIT and `seq` never repeats; `also()` runs under the same lock (the owner's
// own mark).  A host lock only: nothing waits for the kernel.  The owner takes the same mutex around its requests and waits.
template <class F>
static inline void rr_release_guarded(ResidentRing& r, std::mutex& mu, F&& also) {
    std::lock_guard<std::mutex> lock(mu);
    rr_release(r);
    also();
}

// how many workgroups of generation gen have ended
static inline int rr_ended_count(const ResidentRing& r) {
    int n = 0;
    for (int b = 0; b < r.blocks; ++b) n += __atomic_load_n(r.state + b, __ATOMIC_ACQUIRE) == r.gen;
    return n;
}

static inline double rr_now_us() {
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Bounded wait: `ready()` polled; every 2 ms without it the stream is asked.  An error there -> RR_ERROR; an idle stream -> RR_IDLE;
// give_up_us -> RR_NO_ANSWER.  0 once `ready()` holds.
template <typename F>
static inline int rr_poll(ResidentRing& r, F&& ready) {
    const double t0 = rr_now_us();
    double next_query = t0 + 2000.0;
    for (long spins = 0;; ++spins) {
        if (ready()) return RR_OK;
        if ((spins & 255) == 255) {
            const double t = rr_now_us();
            if (t >= next_query) {
                next_query = t + 2000.0;
                const int q = r.query(r.owner);
                if (q == RR_STREAM_IDLE) return ready() ? RR_OK : RR_IDLE;
                if (q != RR_STREAM_BUSY) return RR_ERROR;
            }
            if (t - t0 > r.give_up_us) return RR_NO_ANSWER;
        }
        __builtin_ia32_pause();
    }
}

// ring the doorbell for the request already in place (launching a kernel first if none can hear it)
static inline int rr_ring(ResidentRing& r) {
    if (r.live && rr_ended_count(r) > 0) rr_release(r);         // (some of) it ended by its idle timeout: the rest follows
    if (!r.live) {
        // generation gen was told to end: wait for a kernel on its way out (at once if none was launched; an idle stream: it is gone)
        const int rc = r.gen == 0 ? RR_OK : rr_poll(r, [&]() { return rr_ended_count(r) == r.blocks; });
        if (rc != RR_OK && rc != RR_IDLE) return rc;
        // the next generation through the owner's launch: its number first, the bookkeeping after a launch that went out.  The last
        // sequence number, which the kernel must not take for a command, is the one in the bell -- not seq - 1 (seq skips 0)
        r.gen = rr_next(r.gen);
        const int rl = r.launch(r.owner, r, (unsigned)__atomic_load_n(r.bell, __ATOMIC_RELAXED));
        if (rl) return rl;
        r.live = true; r.launches += 1;
    }
    rr_command(r, r.hi);
    return RR_OK;
}

// a new request: rows (k[]) and their data are in place; `hi` is the command word's high half -- what the owner's kernel reads there
static inline int rr_request(ResidentRing& r, unsigned hi) {
    r.hi = hi;
    const int rc = rr_ring(r);
    if (rc) return rc;
    r.requests += 1;
    return RR_OK;
}

static inline bool rr_served(const ResidentRing& r) {
    for (int i = 0; i < r.n; ++i)
        for (int t = 0; t < (r.k[i] + 15) / 16; ++t)
            if (__atomic_load_n(r.done + r.base[i] + t, __ATOMIC_ACQUIRE) != r.seq) return false;
    return true;
}

// every tile of the request in flight has answered
static inline int rr_wait(ResidentRing& r) {
    const double t0 = rr_now_us();
    for (;;) {
        // a workgroup gone before it served the request (idle timeout just before the doorbell): end the rest, relaunch, ring again
        const int rc = rr_poll(r, [&]() { return rr_served(r) || rr_ended_count(r) > 0; });
        if (rc != RR_OK && rc != RR_IDLE) return rc;
        if (rr_served(r)) return RR_OK;
        if (rr_now_us() - t0 > r.give_up_us) return RR_NO_ANSWER;
        if (rc == RR_IDLE) r.live = false;      // the stream is idle: every workgroup has ended
        const int rr = rr_ring(r);
        if (rr) return rr;
    }
}

// *_actor_set_resident / *_actor_resident_stats of every owner
static inline int rr_set_resident(ResidentRing& r, int on, double idle_timeout_us) {
    if (!(idle_timeout_us <= 1.0e6)) return RR_BAD_TIMEOUT;
    rr_release(r);
    r.on = on != 0;
    if (idle_timeout_us > 0.0) r.idle_us = idle_timeout_us;
    return RR_OK;
}
// out3 = {kernel launches, requests served through the doorbell, 1 if the resident kernel is live now}
static inline void rr_stats(const ResidentRing& r, int64_t* out3) { out3[0] = r.launches; out3[1] = r.requests; out3[2] = r.live ? 1 : 0; }
