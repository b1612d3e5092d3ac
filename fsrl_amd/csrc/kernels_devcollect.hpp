// kernels_devcollect.hpp -- FastCollector.collect(n_episode) as ONE workgroup that loops on the device (fsrl_collect_device).
//
// collect_device_body<H, Env, HEAD>, a workgroup of collect_device_group_kernel: 4 * H threads, staged like actor_resident_kernel<H, false> -- the W2 fragment in registers and the small
// parameters in LDS, loaded once per launch, the same tile_forward and the same head, so a deterministic collect computes the actions
// of the existing collectors bit for bit.  Per vector step, over the live envs in position order:
//   1. per tile of 16 rows (at most 4): the rows' observations (device memory) -> sm.xT, tile_forward, then
//      a = mu (+ exp(sigma_param) * eps, eps from the action stream of device_env.hpp) and map_action -- into LDS
//   2. a thread per live env: Env::step, the time limit, rew / cost / flags into the store slot, one log row for the host
//   3. all threads: obs, obs_next, act of the rows into their store slots
//   4. a thread per live env: reset where the episode ended (the ordinal advances, dropped or not), else obs := obs_next
//   5. thread 0: the surplus rule and the end of the collect (devcollect_plan.hpp)
// The loop has a fixed upper trip count (max_steps <= DC_MAX_STEPS), waits on nothing but its own workgroup's barriers and touches
// device memory only.  What must survive a launch -- live set, episode count, write indices -- is in DcState; env state is in the
// env's own arrays.
// Registers.  At H = 256 the workgroup has 1024 threads, i.e. 128 VGPRs per lane, 64 of them the W2 fragment: nothing else may stay
// live across tile_forward.  Hence (a) the arguments come through a pointer (held by value they filled the scalar file, and scalar
// spills live in vector registers), (b) every vector step and the epilogue take a fresh, opaque copy of the thread id, so that no
// per-lane address arithmetic of the phases is hoisted out of the loop, (c) the live count is read into a scalar register, and (d) the
// two divisions by run-time constants are multiply-highs with host-made magics (a hoisted reciprocal is a long-lived VGPR).  No
// instantiation spills (tests/test_code_object.py).
//
// HEAD: whose actor this is.  DC_HEAD_ONPOLICY is the kernel above.  The replay agents' fused actors (P / md are what
// sac_actor_resident_args returns, staged as actor_resident_kernel<H, true> stages them) leave the RAW head row in sm.out, and phase 1
// does in float32, every operation rounded on its own, what sac_actor_finish + actor_draw do on the host:
//   DC_HEAD_GAUSS (SAC-Lag, CVPO; 2 * Da raw columns, Da <= 8):  m = mean_tanh ? max_action * tanhf(raw[d]) : raw[d],
//       sigma = expf(clamp(raw[Da + d], -20, 2)), u = m (+ sigma * eps), a = squash ? tanhf(u) : u      (squash: SAC-Lag only)
//   DC_HEAD_DDPG (DDPG-Lag; Da raw columns, Da <= 16):            m = max_action * tanhf(raw[d]), a = m (+ exploration_sigma * eps)
// eps is the same draw of the action stream as above.  These instantiations also write every row's slot next to the log (a.slots,
// when the context has prioritised replay on) for per_slots_kernel behind the launch.  Phases 2 - 5 are the same code.
#pragma once
#include "kernels_mlp.hpp"
#include "device_env.hpp"

struct DevCollectArgs {
    DevEnvParams ep;
    DevEnvArrays ea;
    uint32_t k0, k1;
    StorePtrs st;
    int64_t sub_size;
    DcState* state;
    DcLogRow* log;          // [max_steps][env_num]
    int max_steps;
    int deterministic, bound_method, scaled;
    float low[FSRL_MAX_ACT], high[FSRL_MAX_ACT];
    float max_action;
    unsigned magic_per, magic_da;   // div_magic(2 * Do + Da), div_magic(Da): no integer division in the loop
    // the replay heads only
    int mean_tanh, squash;
    float exploration_sigma;
    int32_t* slots;         // [max_steps][env_num] or NULL: the store slot of every log row (prioritised replay)
};
#define DC_HEAD_ONPOLICY 0
#define DC_HEAD_GAUSS 1
#define DC_HEAD_DDPG 2

struct DevCollectSmem {
    int32_t live[DC_MAX_ENVS], index[DC_MAX_ENVS], slot[DC_MAX_ENVS];
    uint8_t done[DC_MAX_ENVS];
    int32_t n_live, episodes, finished;
    float act[DC_MAX_ENVS * FSRL_MAX_ACT];      // the policy's actions (what the store holds)
    float eact[DC_MAX_ENVS * FSRL_MAX_ACT];     // mapped into the env's range
};

// ---- the phases of one vector step as functions: collect_device_body below and the layered loop (kernels_devcollect_layered.hpp)
// are the same calls around their own phase 1.  Every one takes this step's opaque thread id (Registers above).
// what a launch starts from / leaves behind in DcState
template <bool STORE>
__device__ __forceinline__ void dc_state_load(const DevCollectArgs& a, DevCollectSmem& sh, const int tid) {
    if (tid < DC_MAX_ENVS) {
        sh.live[tid] = a.state->live[tid];
        if constexpr (STORE) sh.index[tid] = a.state->index[tid];
    }
    if (tid == 0) { sh.n_live = a.state->n_live; sh.episodes = a.state->episodes; sh.finished = a.state->finished; }
}
template <bool STORE>
__device__ __forceinline__ void dc_state_save(const DevCollectArgs& a, DevCollectSmem& sh, const int step, const int log_rows) {
    int te = threadIdx.x;
    asm volatile("" : "+v"(te));
    if (te < DC_MAX_ENVS) {
        a.state->live[te] = sh.live[te];
        if constexpr (STORE) a.state->index[te] = sh.index[te];
    }
    if (te == 0) {
        a.state->n_live = sh.n_live; a.state->episodes = sh.episodes; a.state->finished = sh.finished;
        a.state->steps = step; a.state->log_rows = log_rows;
    }
}
// phase 1's tail for component d of the row at live position p: the head arithmetic, the draw and map_action.  `raw` is the row's raw
// head outputs (raw[d]; DC_HEAD_GAUSS: the log sigma head at raw[Da + d]), `sig` the actor's sigma_param (DC_HEAD_ONPOLICY); both are
// read only where the mode needs them.
template <int HEAD>
__device__ __forceinline__ void dc_head(const DevCollectArgs& a, DevCollectSmem& sh, const float* raw, const float* sig, const int unbounded,
                                        const int Da, const int p, const int d) {
#pragma clang fp contract(off)
    const int e = sh.live[p];
    const float x = raw[d];
    float act;
    if constexpr (HEAD == DC_HEAD_ONPOLICY) {
        act = unbounded ? x : a.max_action * tanhf(x);
        if (!a.deterministic) {
            const DevRng g{a.k0, a.k1, (uint32_t)e, (uint32_t)(a.ea.ordinal[e] - 1)};
            const float eps = devenv_normal(g, (uint32_t)a.ea.t[e], DEVENV_STREAM_ACT, d);
            act = act + expf(sig[d]) * eps;
        }
    } else {                             // the replay agents: the raw head row -> (m, sigma) -> the draw
        float sg;
        if constexpr (HEAD == DC_HEAD_GAUSS) {
            act = a.mean_tanh ? a.max_action * tanhf(x) : x;
            sg = expf(fminf(fmaxf(raw[Da + d], -20.0f), 2.0f));
        } else {
            act = a.max_action * tanhf(x);
            sg = a.exploration_sigma;
        }
        if (!a.deterministic) {
            const DevRng g{a.k0, a.k1, (uint32_t)e, (uint32_t)(a.ea.ordinal[e] - 1)};
            const float eps = devenv_normal(g, (uint32_t)a.ea.t[e], DEVENV_STREAM_ACT, d);
            act = act + sg * eps;
        }
        if (HEAD == DC_HEAD_GAUSS && a.squash) act = tanhf(act);
    }
    sh.act[p * FSRL_MAX_ACT + d] = act;
    sh.eact[p * FSRL_MAX_ACT + d] = devenv_map_action(act, a.bound_method, a.scaled != 0, a.low[d], a.high[d]);
}
// phase 2: env step, scalars of the row, log
template <class Env, int HEAD, bool STORE>
__device__ __forceinline__ void dc_env_step(const DevCollectArgs& a, DevCollectSmem& sh, const int lt, const int n_live, const int log_rows,
                                            const int Do) {
    if (lt < n_live) {
        const int e = sh.live[lt];
        const DevRng g{a.k0, a.k1, (uint32_t)e, (uint32_t)(a.ea.ordinal[e] - 1)};
        const int32_t t = a.ea.t[e];
        double rew, cost;
        bool term;
        Env::step(a.ep, a.ea.state + (size_t)e * DEVENV_STATE, &sh.eact[lt * FSRL_MAX_ACT], g, (uint32_t)t,
                  a.ea.nxt + (size_t)e * Do, rew, cost, term);
        a.ea.t[e] = t + 1;
        const uint32_t fl = dc_flags(term, dc_truncated(t + 1, a.ep.max_steps));
        [[maybe_unused]] int64_t slot = 0;
        if constexpr (STORE) {
            slot = dc_slot(e, a.sub_size, sh.index[e]);
            sh.index[e] = dc_next_index(sh.index[e], a.sub_size);
            sh.slot[lt] = (int32_t)slot;
        }
        sh.done[lt] = fl != 0u;
        if constexpr (STORE) { a.st.rew[slot] = rew; a.st.cost[slot] = cost; a.st.flags[slot] = (uint8_t)fl; }
        DcLogRow lr;
        lr.env = e; lr.flags = fl; lr.rew = rew; lr.cost = cost;
        a.log[log_rows + lt] = lr;
        if constexpr (STORE && HEAD != DC_HEAD_ONPOLICY) { if (a.slots) a.slots[log_rows + lt] = (int32_t)slot; }
    }
}
// phase 3: the rows' vectors into the store, nt threads
__device__ __forceinline__ void dc_store_rows(const DevCollectArgs& a, DevCollectSmem& sh, const int lt, const int nt, const int n_live,
                                              const int Do, const int Da) {
    const int per = 2 * Do + Da;
    for (int x = lt; x < n_live * per; x += nt) {
        const int p = div_by_magic((unsigned)x, a.magic_per), f = x - p * per, e = sh.live[p];
        const size_t slot = (size_t)sh.slot[p];
        if (f < Do) a.st.obs[slot * Do + f] = a.ea.obs[(size_t)e * Do + f];
        else if (f < 2 * Do) a.st.obs_next[slot * Do + (f - Do)] = a.ea.nxt[(size_t)e * Do + (f - Do)];
        else a.st.act[slot * Da + (f - 2 * Do)] = sh.act[p * FSRL_MAX_ACT + (f - 2 * Do)];
    }
}
// phase 4: the next observation: a reset where the episode ended
template <class Env>
__device__ __forceinline__ void dc_next_obs(const DevCollectArgs& a, DevCollectSmem& sh, const int lt, const int n_live, const int Do) {
    if (lt < n_live) {
        const int e = sh.live[lt];
        if (sh.done[lt]) {
            const DevRng g{a.k0, a.k1, (uint32_t)e, (uint32_t)a.ea.ordinal[e]};
            Env::reset(a.ep, a.ea.state + (size_t)e * DEVENV_STATE, g, a.ea.obs + (size_t)e * Do);
            a.ea.t[e] = 0;
            a.ea.ordinal[e] += 1;
        } else {
            for (int j = 0; j < Do; ++j) a.ea.obs[(size_t)e * Do + j] = a.ea.nxt[(size_t)e * Do + j];
        }
    }
}
// phase 5: who goes on (thread 0)
__device__ __forceinline__ void dc_who_goes_on(DevCollectSmem& sh, const int lt, const int n_live, const int n_episode) {
    if (lt == 0) {
        int32_t ep = sh.episodes;
        sh.n_live = dc_episode_end(sh.live, n_live, sh.done, n_episode, &ep);
        sh.episodes = ep;
        sh.finished = dc_complete(ep, n_episode) ? 1 : 0;
    }
}

// The collect of ONE workgroup: the whole loop above over (P, md, ap), which the kernels below read from their member's row of the
// table; nothing in it knows whose they are.
// STORE = false is the evaluation (fsrl_evaluate_device): the same loop with nothing stored -- no slot, no write index, no phase 3 and
// its barrier; phases 1, 4 and 5 and the log are the code above, so an evaluated step is a collected step.
template <int H, class Env, int HEAD, bool STORE = true>
__device__ __forceinline__ void collect_device_body(const float* __restrict__ P, const ModelDesc& md, const DevCollectArgs* __restrict__ ap,
                                                    TileSmem<H>& sm, DevCollectSmem& sh) {
    const DevCollectArgs& a = *ap;
    constexpr int NT = TileGeom<H>::NT;
    constexpr int NX = TileStage<H>::NX;
    const int tid = threadIdx.x;
    const NetOff no = md.net[0];
    const int Do = md.Do, Da = md.Da;
    const unsigned magic = div_magic(Do);
    TileStage<H> stg;
    stg.issue(P, no, Do, Da, P, nullptr, 0, tid);             // the small parameters; no rows (n_valid = 0 masks the x loads)
    FwdW2Frag<H> wf;
    wf.load(P + no.W2f, tid >> 6, tid & 63);
    stg.commit(sm, no, Do, tid);
    dc_state_load<STORE>(a, sh, tid);
    const int n_episode = a.state->n_episode;
    int step = 0, log_rows = 0;
    for (; step < a.max_steps; ++step) {
        __syncthreads();
        if (__builtin_amdgcn_readfirstlane(sh.finished)) break;
        const int n_live = __builtin_amdgcn_readfirstlane(sh.n_live);      // workgroup-uniform: scalar registers
        int lt = threadIdx.x;
        asm volatile("" : "+v"(lt));           // this step's thread id, opaque: see Registers above
        // ---- 1. actor, noise, map_action
        for (int row0 = 0; row0 < n_live; row0 += 16) {
            const int n_valid = min(16, n_live - row0);
#pragma unroll
            for (int u = 0; u < NX; ++u) {
                const int e = lt + u * NT;
                if (e < 16 * Do) {
                    const int i = div_by_magic((unsigned)e, magic), k = e - i * Do;
                    sm.xT[k * 16 + i] = (i < n_valid) ? a.ea.obs[(size_t)sh.live[row0 + i] * Do + k] : 0.0f;
                }
            }
            __syncthreads();
            tile_forward<H>(sm, P, no, Do, lt, wf);
            if (lt < n_valid * Da) {
                const int i = div_by_magic((unsigned)lt, a.magic_da), d = lt - i * Da;
                dc_head<HEAD>(a, sh, &sm.out[i * FSRL_MAX_ACT], sm.sig, md.unbounded, Da, row0 + i, d);
            }
            __syncthreads();
        }
        // ---- 2. env step, scalars of the row, log
        dc_env_step<Env, HEAD, STORE>(a, sh, lt, n_live, log_rows, Do);
        __syncthreads();
        if constexpr (STORE) {
            // ---- 3. the rows' vectors into the store
            dc_store_rows(a, sh, lt, NT, n_live, Do, Da);
            __syncthreads();
        }
        // ---- 4. the next observation: a reset where the episode ended
        dc_next_obs<Env>(a, sh, lt, n_live, Do);
        log_rows += n_live;
        __syncthreads();
        // ---- 5. who goes on
        dc_who_goes_on(sh, lt, n_live, n_episode);
    }
    __syncthreads();
    dc_state_save<STORE>(a, sh, step, log_rows);
}

// ---- k collects in one launch (fsrl_collect_device_group; fsrl_collect_device is its one-member case): grid k, workgroup b runs
// member b's collect, the loop above.
// The members share nothing -- each has its own store, env arrays, DcState and log -- and the workgroups do not communicate: no
// flags, no waits on another block's data; a member that is finished breaks at the loop's first test and reports 0 steps, 0 rows.
// Per-member inputs come from a table in device memory (by value they would fill the scalar file: Registers above); md is member 0's,
// the host checks that the members agree on what it describes.  blockIdx.x and the two pointers are workgroup-uniform: scalar registers.
#ifndef FSRL_MAX_GROUP
#define FSRL_MAX_GROUP 16
#endif
struct DevCollectGroupTable {
    const float* P[FSRL_MAX_GROUP];
    const DevCollectArgs* a[FSRL_MAX_GROUP];
};
// A pointer read from memory is a flat pointer to the compiler, and a flat load never becomes a scalar load.  AS = 1 says that it is
// global; AS = 4 that what it points to is constant for the length of the kernel (the arguments: nothing writes them while a launch
// runs), which is what `const __restrict__` says of a kernel argument: the fields are read with scalar loads, whenever they are
// needed, and none of them has to stay in a vector register across tile_forward.
template <int AS, class T>
__device__ __forceinline__ const T* dc_uniform_ptr(const T* p) {
    const unsigned long long v = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    typedef const T __attribute__((address_space(AS))) * SpacePtr;
    return (const T*)(SpacePtr)(((unsigned long long)hi << 32) | lo);
}
template <int H, class Env, int HEAD = DC_HEAD_ONPOLICY>
__global__ __launch_bounds__(4 * H) void collect_device_group_kernel(const ModelDesc md, const DevCollectGroupTable* __restrict__ tab) {
    const int b = __builtin_amdgcn_readfirstlane((int)blockIdx.x);
    const float* P = dc_uniform_ptr<1>(tab->P[b]);
    const DevCollectArgs* ap = dc_uniform_ptr<4>(tab->a[b]);
    __shared__ TileSmem<H> sm;
    __shared__ DevCollectSmem sh;
    collect_device_body<H, Env, HEAD>(P, md, ap, sm, sh);
}

// ---- k evaluations in one launch (fsrl_evaluate_device_group; fsrl_evaluate_device is its one-member case): the table-driven launch
// above over the store-less loop.  The members' stores, write indices and slot arrays are not arguments of this form: a.st, a.sub_size
// and a.slots are never read.
template <int H, class Env, int HEAD = DC_HEAD_ONPOLICY>
__global__ __launch_bounds__(4 * H) void evaluate_device_group_kernel(const ModelDesc md, const DevCollectGroupTable* __restrict__ tab) {
    const int b = __builtin_amdgcn_readfirstlane((int)blockIdx.x);
    const float* P = dc_uniform_ptr<1>(tab->P[b]);
    const DevCollectArgs* ap = dc_uniform_ptr<4>(tab->a[b]);
    __shared__ TileSmem<H> sm;
    __shared__ DevCollectSmem sh;
    collect_device_body<H, Env, HEAD, false>(P, md, ap, sm, sh);
}
