// dev_mem.hpp -- the one place that allocates and frees device and pinned memory.  Plain C++17 over a backend B that supplies
//   using Err; static constexpr Err ok, bad;  dev_alloc / host_alloc(void**, size_t) -> Err;  dev_free / host_free(void*, size_t) -> Err
// (the library: HipMem below; tests/host/dev_mem_sim.cpp: a checking malloc backend).  A MemOwner remembers the VALUE, size and
// kind of every block it handed out: the fields stay raw pointers (they go by value into kernel-argument structs, sit in arrays,
// get copied), a state's teardown is release_all(), and a new buffer is a field plus one dev() / pinned() call.  Aliases into a
// block, and pointers another owner holds, are never registered.  Nothing is cached, pooled or deferred.
#pragma once
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <vector>

template <class B>
class MemOwner {
public:
    using Err = typename B::Err;
    struct Req { void** field; size_t bytes; bool pin; };      // one buffer of a regrow set; bytes == 0: the field stays null
    template <class T> static Req D(T** f, size_t bytes) { return Req{reinterpret_cast<void**>(f), bytes, false}; }
    template <class T> static Req H(T** f, size_t bytes) { return Req{reinterpret_cast<void**>(f), bytes, true}; }
    template <class T> struct Same { using type = T; };

    MemOwner() = default;
    MemOwner(const MemOwner&) = delete;
    MemOwner& operator=(const MemOwner&) = delete;

    template <class T> Err dev(T** f, size_t bytes) { return alloc(D(f, bytes)); }
    template <class T> Err pinned(T** f, size_t bytes) { return alloc(H(f, bytes)); }
    // free one block and null its field; a null field is a no-op, a pointer this owner does not hold is refused (and not freed)
    template <class T> Err release(T** f) {
        if (!*f) return B::ok;
        for (Block& b : held_)
            if (b.p == (const void*)*f) {
                const Block gone = b;
                b = held_.back(); held_.pop_back();
                *f = nullptr;
                return gone.pin ? B::host_free(gone.p, gone.bytes) : B::dev_free(gone.p, gone.bytes);
            }
        return B::bad;
    }
    // A set of buffers behind one capacity.  The capacity reads 0 from the first free until every allocation succeeded: after a
    // failure every field of the set is null or valid at the new size, and the next call -- whatever it needs -- tries again.
    template <class Cap>
    Err regrow(Cap& cap, typename Same<Cap>::type need, typename Same<Cap>::type grow_to, std::initializer_list<Req> set) {
        if (need <= cap) return B::ok;
        cap = Cap{};
        Err e = B::ok;
        for (const Req& r : set) { const Err e1 = release(r.field); if (e == B::ok) e = e1; }
        for (const Req& r : set) { if (e != B::ok) return e; e = alloc(r); }
        if (e == B::ok) cap = grow_to;
        return e;
    }
    void release_all() {
        for (const Block& b : held_) (void)(b.pin ? B::host_free(b.p, b.bytes) : B::dev_free(b.p, b.bytes));
        held_.clear();
    }

private:
    struct Block { void* p; size_t bytes; bool pin; };
    std::vector<Block> held_;
    Err alloc(const Req& r) {
        *r.field = nullptr;
        if (!r.bytes) return B::ok;
        void* p = nullptr;
        const Err e = r.pin ? B::host_alloc(&p, r.bytes) : B::dev_alloc(&p, r.bytes);
        if (e != B::ok) return e;
        held_.push_back(Block{p, r.bytes, r.pin});
        *r.field = p;
        return B::ok;
    }
};

#ifdef __HIPCC__     // the library's backend; the includer has <hip/hip_runtime.h>.  live: what fsrl_mem_live reports
#include <atomic>
struct HipMem {
    using Err = hipError_t;
    static constexpr Err ok = hipSuccess, bad = hipErrorInvalidValue;
    static inline std::atomic<int64_t> live[4];      // device blocks, device bytes, pinned blocks, pinned bytes
    static Err count(Err e, int k, int sign, size_t n) { if (e == ok) { live[k] += sign; live[k + 1] += sign * (int64_t)n; } return e; }
    static Err dev_alloc(void** p, size_t n) { return count(hipMalloc(p, n), 0, 1, n); }
    static Err host_alloc(void** p, size_t n) { return count(hipHostMalloc(p, n), 2, 1, n); }
    static Err dev_free(void* p, size_t n) { return count(hipFree(p), 0, -1, n); }
    static Err host_free(void* p, size_t n) { return count(hipHostFree(p), 2, -1, n); }
};
using Mem = MemOwner<HipMem>;
#endif
