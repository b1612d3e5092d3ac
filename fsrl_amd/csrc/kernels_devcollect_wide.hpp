// kernels_devcollect_wide.hpp -- device collects over 65 .. 4096 envs (fsrl_collect_device_wide): ONE LAUNCH PER VECTOR STEP, one
// workgroup per 16-row tile of the live list.
//
// The looping collect (kernels_devcollect.hpp) is one workgroup because the surplus rule needs the whole vector's episode ends at
// every step.  Here the kernel boundary is that synchronisation: launch t runs phases 1 - 4 of vector step t on its tile and leaves
// the tile's episode-end flags in device memory; phase 5 of step t is done at the START of launch t + 1, by every workgroup,
// redundantly, from the same flags -- every workgroup arrives at the same live list and takes its own 16 positions of it.  No
// workgroup reads a word that another workgroup of the same launch writes: the scalar state, the flags and the live list are held
// twice, by the parity of t (DcwState, devcollect_plan.hpp), and everything else a step touches -- an env's state, observation, t,
// ordinal, write index, store slot, log row -- belongs to one position, i.e. one thread.  No atomics, fences, flags or waits.
//
// wide_collect_step_kernel<H, Env, HEAD>, grid ceil(first_live / 16) x 4 * H threads:
//   0. the small parameters and the W2 fragment are issued (the loads stream in under what follows)
//   5'. the deferred phase 5 (dcw_settle): the state of side t & 1 with scalar loads; if a step is pending, its flags -- a dword of
//      four positions per thread, 4096 positions in one trip of a 1024-thread block -- counted with four wave ballots and one LDS pass
//      over the wave totals.  No episode end: nothing changes (the common step).  Ends but no surplus: the episode count alone.  A
//      surplus: the stable compaction of dc_wide_leaves / dc_wide_new_pos, a position's rank from mbcnt over the ballots plus the
//      totals of the waves in front; the tile keeps the env ids that land in its 16 positions, workgroup 0 also writes the new list
//      into the OTHER half of live[] (so the common step copies nothing).  Workgroup 0 writes the next state.
//      Workgroups whose tile lies beyond the live count, and every workgroup of a launch behind a finished collect, exit here.
//   1 - 4. the tile's step: the phases of collect_device_body on 16 rows -- same staging, tile_forward and dc_head, the draws keyed by
//      (env id, ordinal, t), so nothing depends on the tiling -- with a phase 2 of its own (the write index by env id in device
//      memory, the log row at log_rows + position, the flag into the other side's done[]).
// settle = 1 (one workgroup, behind every batch of launches): 5' alone, clearing `pending`, so that what the host reads is settled.
// first = 1 (a batch's first launch): the batch's log and step counters start at zero.
// Registers: the rules of kernels_devcollect.hpp -- arguments through a pointer and read with scalar loads, opaque thread ids, magic
// divisions; 5' holds nothing across tile_forward.  No instantiation spills (tests/test_devcollect_wide_host.py).
#pragma once
#include "kernels_devcollect.hpp"

// The grouped kernels are compiled without the packed-fp32 instructions (v_pk_add / mul / fma_f32), as wide_layered_step_kernel is.
// Not for register fit: with them the 256-wide forms take 128 / 126 VGPRs and do not spill.  The one-lane forms round identically
// (the bits are the solo kernels'), and the rate is the same with and without to the measurement's last stable digit (DESIGN.md
// 3.4.1), so the attribute is free and keeps the new kernels independent of how the two-lane forms behave.
#if defined(__HIP_DEVICE_COMPILE__)
#define DCW_NO_PK __attribute__((target("no-packed-fp32-ops")))
#else
#define DCW_NO_PK           // the host pass does not know the feature
#endif

struct WideCollectArgs {
    DevCollectArgs a;       // a.state and a.max_steps are not read
    DcwState* ws;
    int log_cap;            // rows the log holds: a step that would not fit is not taken (the host reports the batch that made no step)
};

// bytes of a flags dword as predicates: position 4 i + k of the dword at i is a finished one
__device__ __forceinline__ bool dcw_flag(const uint32_t w, const int k) { return ((w >> (8 * k)) & 0xFFu) != 0u; }

// The deferred phase 5.  In: the state of this launch's side (s, scalar).  Out: the state the step runs on; sh.live[0 .. 16) = the env
// ids of positions tile0 .. tile0 + 15 of the live list; `writer` also leaves a compacted list in the other half of ws->live.
// wtot: 16 ints of LDS.  Every thread of the workgroup calls it (barriers).
template <int NT>
__device__ __forceinline__ DcwScalars dcw_settle(DcwState* __restrict__ ws, DcwScalars s, const int side, const int n_episode, const int tile0,
                                                 int32_t* sh_live, int32_t* wtot, const bool writer) {
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63;
    int n_done = 0, surplus = 0;
    const int n_live = s.n_live;
    const uint32_t* __restrict__ done = ws->done[side];
    const int n4 = (n_live + 3) >> 2, trips = (n4 + NT - 1) / NT;           // n4 <= 1024: at most 16 waves' worth of dwords
    if (s.pending && !s.finished) {
        for (int it = 0; it < trips; ++it) {
            const int i = it * NT + tid;
            uint32_t w = i < n4 ? done[i] : 0u;
            if (4 * i + 4 > n_live) w &= 4 * i >= n_live ? 0u : (0xFFFFFFFFu >> (8 * (4 * i + 4 - n_live)));      // flags of an earlier, longer list
            int cnt = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) cnt += __popcll(__ballot(dcw_flag(w, k)));
            if (lane == 0) wtot[i >> 6] = cnt;
        }
        __syncthreads();
        const int nw = (n4 + 63) >> 6;
        for (int w = 0; w < nw; ++w) n_done += wtot[w];
        n_done = __builtin_amdgcn_readfirstlane(n_done);
        s.episodes += n_done;
        surplus = dc_wide_surplus(n_live, n_done, n_episode, s.episodes);
    }
    if (surplus == 0) {          // the common step: the list stays where it is
        if (tid < 16 && tile0 + tid < n_live) sh_live[tid] = ws->live[s.lpar][tile0 + tid];
    } else {
        const int32_t* __restrict__ src = ws->live[s.lpar];
        int32_t* __restrict__ dst = ws->live[s.lpar ^ 1];
        for (int it = 0; it < trips; ++it) {
            const int i = it * NT + tid;
            uint32_t w = i < n4 ? done[i] : 0u;
            if (4 * i + 4 > n_live) w &= 4 * i >= n_live ? 0u : (0xFFFFFFFFu >> (8 * (4 * i + 4 - n_live)));
            int rank = 0;
            for (int v = 0; v < (i >> 6); ++v) rank += wtot[v];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned long long b = __ballot(dcw_flag(w, k));
                rank += (int)__builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int p = 4 * i + k;
                const bool d = dcw_flag(w, k);
                if (p < n_live && !dc_wide_leaves(d, rank, surplus)) {
                    const int q = dc_wide_new_pos(p, rank, surplus);
                    const int32_t e = src[p];
                    if (q >= tile0 && q < tile0 + 16) sh_live[q - tile0] = e;
                    if (writer) dst[q] = e;
                }
                rank += d ? 1 : 0;
            }
        }
        s.n_live = dc_wide_n_live(n_live, n_done, surplus);
        s.lpar ^= 1;
    }
    s.finished = (s.finished || dc_complete(s.episodes, n_episode)) ? 1 : 0;
    s.pending = 0;
    return s;
}

// phase 2 of a wide step, a thread per row of the tile: dc_env_step with the write index by env id in device memory, the log row at
// the row's position in the whole list and the flag into the next launch's side of done[] (a byte store; the byte is this thread's)
template <class Env, int HEAD>
__device__ __forceinline__ void dcw_env_step(const DevCollectArgs& a, DevCollectSmem& sh, DcwState* __restrict__ ws, const int lt, const int n_valid,
                                             const int tile0, const int log0, const int nside, const int Do) {
    if (lt < n_valid) {
        const int e = sh.live[lt];
        const DevRng g{a.k0, a.k1, (uint32_t)e, (uint32_t)(a.ea.ordinal[e] - 1)};
        const int32_t t = a.ea.t[e];
        double rew, cost;
        bool term;
        Env::step(a.ep, a.ea.state + (size_t)e * DEVENV_STATE, &sh.eact[lt * FSRL_MAX_ACT], g, (uint32_t)t, a.ea.nxt + (size_t)e * Do, rew, cost, term);
        a.ea.t[e] = t + 1;
        const uint32_t fl = dc_flags(term, dc_truncated(t + 1, a.ep.max_steps));
        const int32_t index = ws->index[e];
        const int64_t slot = dc_slot(e, a.sub_size, index);
        ws->index[e] = dc_next_index(index, a.sub_size);
        sh.slot[lt] = (int32_t)slot;
        sh.done[lt] = fl != 0u;
        reinterpret_cast<uint8_t*>(ws->done[nside])[tile0 + lt] = fl != 0u;
        a.st.rew[slot] = rew; a.st.cost[slot] = cost; a.st.flags[slot] = (uint8_t)fl;
        DcLogRow lr;
        lr.env = e; lr.flags = fl; lr.rew = rew; lr.cost = cost;
        a.log[log0 + lt] = lr;
    }
}

// One workgroup's launch: a tile of ONE collect, whoever launched it.  wp: the collect's arguments, a uniform pointer into constant memory
// (dc_uniform_ptr<4>); t: the collect's own launch ordinal; tile: the tile's number in that collect's live list, uniform.  `settled`
// (uniform, or null): where the writer also leaves the state it hands on -- the grouped settle launch gathers the members' there.
// wide_collect_step_kernel and wide_collect_group_step_kernel are this function behind two ways of finding (wp, P, t, tile).
template <int H, class Env, int HEAD>
__device__ __forceinline__ void wide_collect_step_body(const ModelDesc& md, const float* __restrict__ P, const WideCollectArgs* wp, const int t, const int first,
                                                       const int settle, const int tile, DcwScalars* settled) {
    __shared__ TileSmem<H> sm;
    __shared__ DevCollectSmem sh;
    __shared__ int32_t wtot[16];
    constexpr int NT = TileGeom<H>::NT;
    constexpr int NX = TileStage<H>::NX;
    const DevCollectArgs& a = wp->a;
    DcwState* ws = wp->ws;
    const int side = t & 1, nside = side ^ 1;
    const int tile0 = 16 * tile;
    const bool writer = tile0 == 0;
    const int tid = threadIdx.x;
    const NetOff no = md.net[0];
    const int Do = md.Do, Da = md.Da;
    TileStage<H> stg;
    FwdW2Frag<H> wf;
    if (!settle) {
        stg.issue(P, no, Do, Da, P, nullptr, 0, tid);
        wf.load(P + no.W2f, tid >> 6, tid & 63);
    }
    // ---- 5'. the state of this side, uniform; the step before is settled
    DcwScalars s = *dc_uniform_ptr<4>(&ws->s[side]);
    const int n_episode = *dc_uniform_ptr<4>(&ws->n_episode);
    if (first) { s.log_rows = 0; s.steps = 0; }
    s = dcw_settle<NT>(ws, s, side, n_episode, tile0, sh.live, wtot, writer);
    const bool go = !settle && !s.finished && s.log_rows + s.n_live <= wp->log_cap;
    if (writer && tid == 0) {
        DcwScalars nx = s;
        if (go) { nx.log_rows = s.log_rows + s.n_live; nx.steps = s.steps + 1; nx.pending = 1; }
        ws->s[nside] = nx;
        if (settled) *settled = nx;
    }
    if (!go || tile0 >= s.n_live) return;
    const int n_valid = min(16, s.n_live - tile0);
    stg.commit(sm, no, Do, tid);
    __syncthreads();
    int lt = threadIdx.x;
    asm volatile("" : "+v"(lt));
    // ---- 1. actor, noise, map_action
    const unsigned magic = div_magic(Do);
#pragma unroll
    for (int u = 0; u < NX; ++u) {
        const int e = lt + u * NT;
        if (e < 16 * Do) {
            const int i = div_by_magic((unsigned)e, magic), k = e - i * Do;
            sm.xT[k * 16 + i] = (i < n_valid) ? a.ea.obs[(size_t)sh.live[i] * Do + k] : 0.0f;
        }
    }
    __syncthreads();
    tile_forward<H>(sm, P, no, Do, lt, wf);
    if (lt < n_valid * Da) {
        const int i = div_by_magic((unsigned)lt, a.magic_da), d = lt - i * Da;
        dc_head<HEAD>(a, sh, &sm.out[i * FSRL_MAX_ACT], sm.sig, md.unbounded, Da, i, d);
    }
    __syncthreads();
    // ---- 2. env step, scalars of the row, log, flag
    dcw_env_step<Env, HEAD>(a, sh, ws, lt, n_valid, tile0, s.log_rows + tile0, nside, Do);
    __syncthreads();
    // ---- 3. the rows' vectors into the store; 4. the next observation
    dc_store_rows(a, sh, lt, NT, n_valid, Do, Da);
    __syncthreads();
    dc_next_obs<Env>(a, sh, lt, n_valid, Do);
}

template <int H, class Env, int HEAD>
__global__ __launch_bounds__(4 * H) void wide_collect_step_kernel(const ModelDesc md, const float* __restrict__ P, const WideCollectArgs* __restrict__ wap,
                                                                  const int t, const int first, const int settle) {
    wide_collect_step_body<H, Env, HEAD>(md, P, dc_uniform_ptr<4>(wap), t, first, settle, __builtin_amdgcn_readfirstlane((int)blockIdx.x), nullptr);
}

// ---- k wide collects in one launch per vector step (fsrl_collect_device_wide_group, host_devcollect_wide_group.inc).
// The grid is the members' tiles laid end to end -- sum over members of ceil(first_live_m / 16) workgroups, fixed for the collect --
// not a k x max-tiles rectangle: members may differ in env_num by two orders of magnitude (17 envs beside 4096 would launch 512
// workgroups for 258 tiles).  A workgroup finds (member, tile) from the prefix of tile counts with scalar loads and fifteen scalar
// comparisons (dc_wgroup_member, devcollect_plan.hpp), reads its member's row with scalar loads and runs wide_collect_step_body on
// that member's pointers: its own WideCollectArgs (store, env arrays, log, DcwState, log_cap), parameters and launch ordinal
// t_m = par0[m] + j (only the parity of an ordinal is ever read) -- every env counts its own launches (fsrl_devenv::wide_t), members arrive with different parities, and all of
// them advance by one per launch of the call.  Phase 5' runs over the member's flags and live list in each of its workgroups, the
// writer is the member's tile 0, a finished member's workgroups and tiles beyond its live count exit at the first test.  Nothing is
// shared between members, so the launch has the solo launch's property between ALL its workgroups: no word one of them writes is
// read by another, no atomics, fences or waits.
// The settle launch (settle = 1) is k workgroups, workgroup m the tile 0 of member m; it also leaves the settled scalars of member
// m in settled[m], so that the host reads every member's back with one copy.
// md is member 0's: the host checks that the members agree on what it describes, as for collect_device_group_kernel.  The row is
// read through constant address space, whenever a field is needed: nothing of it has to live in a vector register.
struct WideGroupTable {
    int32_t prefix[DCWG_MAX_MEMBERS + 1];       // tiles in front of member m; from k on: the grid
    int32_t par0[DCWG_MAX_MEMBERS];             // the PARITY of the member's launch ordinal at the call's first launch
    const WideCollectArgs* wa[DCWG_MAX_MEMBERS];
    const float* P[DCWG_MAX_MEMBERS];           // fused members: the actor's parameters
    const struct WideLayActor* la[DCWG_MAX_MEMBERS];   // layered members: the actor's row (kernels_devcollect_wide_layered.hpp)
};
static_assert(DCWG_MAX_MEMBERS == FSRL_MAX_GROUP, "the plan's member count is the group's");
// (member, tile) of this workgroup, both in scalar registers
__device__ __forceinline__ void dcwg_find(const WideGroupTable* tb, const int settle, int& m, int& tile) {
    const int b = __builtin_amdgcn_readfirstlane((int)blockIdx.x);
    m = settle ? b : __builtin_amdgcn_readfirstlane(dc_wgroup_member(tb->prefix, b));
    tile = settle ? 0 : b - tb->prefix[m];
}
template <int H, class Env, int HEAD>
__global__ __launch_bounds__(4 * H) DCW_NO_PK void wide_collect_group_step_kernel(const ModelDesc md, const WideGroupTable* __restrict__ tab,
                                                                                  DcwScalars* __restrict__ settled, const int j, const int first,
                                                                                  const int settle) {
    const WideGroupTable* tb = dc_uniform_ptr<4>(tab);
    int m, tile;
    dcwg_find(tb, settle, m, tile);
    wide_collect_step_body<H, Env, HEAD>(md, dc_uniform_ptr<1>(tb->P[m]), dc_uniform_ptr<4>(tb->wa[m]), tb->par0[m] + j, first, settle, tile,
                                         settle ? settled + m : nullptr);
}
