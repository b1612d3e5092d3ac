// kernels_deveval_wide.hpp -- device EVALUATIONS over 1 .. 4096 envs (fsrl_evaluate_device_wide / _wide_layered): the launch scheme of
// kernels_devcollect_wide.hpp -- one launch per vector step, one workgroup per 16-row tile of the live list, phase 5 of a step settled
// at the start of the next launch by every workgroup -- with the EPISODE, not the step row, as the unit that leaves the GPU.
//
// A storing wide collect writes a 24-byte DcLogRow per env per step, and the host reads the rows back and replays them one by one.
// An evaluation stores nothing, so nothing needs the rows: it needs n_episode episode records in the collector's order.  Here
//   2.  the row's thread (phase 2, dcw_eval_env_step) adds the step's reward and cost (double) and 1 to the running episode of its env,
//       held by env id in device memory (DcwEval, devcollect_plan.hpp) as the write index of a collect is, touched by this thread
//       alone.  On an episode end it parks {return, cost, length, flags} at park[nside][position] and zeroes the running episode.
//       Parked by POSITION and PARITY, never by env id: with one-step episodes an env ends again in the next launch, maybe in another
//       tile, while its old tile still reads the record of the step before.  No slot, no write index, no store write, no log row;
//       phase 3 (dc_store_rows) and its barrier are gone.
//   5'. the settle of the next launch (dcw_eval_settle) counts the flags as dcw_settle does, and whenever n_done > 0 -- not only under
//       a surplus -- takes every finished position's rank (mbcnt over the ballots plus the totals of the waves in front).  The
//       workgroup that ran old position p's tile, tile p / 16 of the fixed grid, copies park[side][p] to row
//       episodes_before + rank(p) of the episode log (dc_wide_episode_row): step-major, position order inside a step, the order in
//       which devcollect_replay meets the ending rows.  A workgroup whose tile lies beyond the shrunken live count writes its rows
//       before it exits; the one-workgroup settle launch behind a batch writes the rows of ALL positions of the last pending step.
//       Compaction, sh_live, the other half of live[] and the handed-on scalars are dcw_settle's.
// What a launch shares is unchanged in kind: no word one workgroup writes is read by another workgroup of the same launch (park[] and
// done[] are held twice by the parity of the launch ordinal, a log row has one writer and no reader on the device), no atomics,
// fences or waits.  The host reads 32 bytes of settled scalars per batch and n_episode rows once at the end (host_deveval_wide.inc).
//
// wide_eval_step_kernel<H, Env, HEAD>: fused contexts, TileStage / tile_forward / dc_head / dc_next_obs as wide_collect_step_kernel
// uses them; wide_eval_layered_step_kernel<Env, HEAD, DEVWS>: layered contexts, around wl_prefetch / wl_tile_actor.  Both are their
// body functions (wide_eval_step_body / wide_eval_layered_step_body) behind the kernel's own arguments and blockIdx; the grouped
// kernels (kernels_deveval_wide_group.hpp) call the same bodies with a member's row.  The actions, the
// env steps and the draws (keyed by env id, ordinal, t) are the collect's, so an evaluation leaves the env where a collect leaves it.
// Registers: the rules of kernels_devcollect.hpp; the settle copies a record as three 8-byte words, one in flight at a time, and holds
// nothing across the actor.  No instantiation spills or uses scratch, and none takes more LDS than its collect counterpart
// (tests/test_deveval_wide_host.py).
#pragma once
#include "kernels_devcollect_wide.hpp"
#include "kernels_devcollect_wide_layered.hpp"

struct WideEvalArgs {
    DevCollectArgs a;       // a.state, a.log, a.st, a.slots and a.max_steps are not read
    DcwState* ws;           // index[] is not read
    DcwEval* ev;
    DcEpisodeRow* ep_log;   // [n_episode]
};

// The deferred phase 5 of an evaluation: dcw_settle, and the episode rows of the step before.  all_rows: the settle launch (every
// finished position's row); else the rows of this workgroup's own 16 old positions.  park: the side this launch reads.
template <int NT>
__device__ __forceinline__ DcwScalars dcw_eval_settle(DcwState* __restrict__ ws, DcwScalars s, const int side, const int n_episode, const int tile,
                                                      int32_t* sh_live, int32_t* wtot, const bool writer, const bool all_rows,
                                                      const DcEpisodeRow* __restrict__ park, DcEpisodeRow* __restrict__ ep_log) {
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, tile0 = 16 * tile;
    int n_done = 0, surplus = 0;
    const int n_live = s.n_live, ep0 = s.episodes;
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
    if (n_done > 0) {            // ranks: the episode rows, and under a surplus the stable compaction
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
            const bool mine = dc_wide_row_owner(4 * i, tile, all_rows);       // a dword's four positions lie in one tile
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int p = 4 * i + k;
                const bool d = dcw_flag(w, k);          // masked: d implies p < n_live
                if (mine) {
                    const int row = dc_wide_episode_row(d, ep0, rank, n_episode);
                    if (row >= 0) {
                        const double* __restrict__ from = reinterpret_cast<const double*>(park + p);
                        double* __restrict__ to = reinterpret_cast<double*>(ep_log + row);
#pragma unroll
                        for (int x = 0; x < 3; ++x) to[x] = from[x];
                    }
                }
                if (surplus > 0 && p < n_live && !dc_wide_leaves(d, rank, surplus)) {
                    const int q = dc_wide_new_pos(p, rank, surplus);
                    const int32_t e = src[p];
                    if (q >= tile0 && q < tile0 + 16) sh_live[q - tile0] = e;
                    if (writer) dst[q] = e;
                }
                rank += d ? 1 : 0;
            }
        }
    }
    if (surplus == 0) {          // the list stays where it is
        if (tid < 16 && tile0 + tid < n_live) sh_live[tid] = ws->live[s.lpar][tile0 + tid];
    } else {
        s.n_live = dc_wide_n_live(n_live, n_done, surplus);
        s.lpar ^= 1;
    }
    s.finished = (s.finished || dc_complete(s.episodes, n_episode)) ? 1 : 0;
    s.pending = 0;
    return s;
}
static_assert(sizeof(DcEpisodeRow) == 24, "a record is three 8-byte words");

// phase 2 of an evaluation's step, a thread per row of the tile: Env::step and t + 1 as dcw_env_step does them, the running episode of
// the env (its own thread's alone), the parked record of an ended episode and the flag, both into the next launch's side
template <class Env>
__device__ __forceinline__ void dcw_eval_env_step(const DevCollectArgs& a, DevCollectSmem& sh, DcwState* __restrict__ ws, DcwEval* __restrict__ ev,
                                                  const int lt, const int n_valid, const int tile0, const int nside, const int Do) {
    if (lt < n_valid) {
        const int e = sh.live[lt];
        const DevRng g{a.k0, a.k1, (uint32_t)e, (uint32_t)(a.ea.ordinal[e] - 1)};
        const int32_t t = a.ea.t[e];
        double rew, cost;
        bool term;
        Env::step(a.ep, a.ea.state + (size_t)e * DEVENV_STATE, &sh.eact[lt * FSRL_MAX_ACT], g, (uint32_t)t, a.ea.nxt + (size_t)e * Do, rew, cost, term);
        a.ea.t[e] = t + 1;
        const uint32_t fl = dc_flags(term, dc_truncated(t + 1, a.ep.max_steps));
        sh.done[lt] = fl != 0u;
        reinterpret_cast<uint8_t*>(ws->done[nside])[tile0 + lt] = fl != 0u;
        double er = ev->rew[e] + rew, ec = ev->cost[e] + cost;          // 0.0 + the first step: the additions of dc_eval_row, in its order
        int32_t el = ev->len[e] + 1;
        if (fl != 0u) {
            DcEpisodeRow r;
            r.rew = er; r.cost = ec; r.len = el; r.flags = fl;
            ev->park[nside][tile0 + lt] = r;
            er = 0.0; ec = 0.0; el = 0;
        }
        ev->rew[e] = er; ev->cost[e] = ec; ev->len[e] = el;
    }
}

// the state hand-over of every wide launch, by the writer's thread 0: log_rows counts the batch's env steps (there is no log to cap)
__device__ __forceinline__ void dcw_eval_hand_on(DcwState* __restrict__ ws, const DcwScalars& s, const bool go, const int nside) {
    DcwScalars nx = s;
    if (go) { nx.log_rows = s.log_rows + s.n_live; nx.steps = s.steps + 1; nx.pending = 1; }
    ws->s[nside] = nx;
}

// One workgroup's launch: a tile of ONE evaluation, whoever launched it (wide_collect_step_body's contract).  wp: the evaluation's
// arguments, a uniform pointer into constant memory; t: the env's own launch ordinal; tile: the tile's number in THAT evaluation's
// fixed grid, uniform -- the row owner of old position p is tile p / 16 of the member, not of the launch.  `settled` (uniform, or
// null; given by a settle launch alone): where the writer also leaves the settled scalars -- the grouped settle launch gathers the
// members' there.  wide_eval_step_kernel and wide_eval_group_step_kernel (kernels_deveval_wide_group.hpp) are this function behind
// two ways of finding (wp, P, t, tile).
template <int H, class Env, int HEAD>
__device__ __forceinline__ void wide_eval_step_body(const ModelDesc& md, const float* __restrict__ P, const WideEvalArgs* wp, const int t, const int first,
                                                    const int settle, const int tile, DcwScalars* settled) {
    __shared__ TileSmem<H> sm;
    __shared__ DevCollectSmem sh;
    __shared__ int32_t wtot[16];
    constexpr int NT = TileGeom<H>::NT;
    constexpr int NX = TileStage<H>::NX;
    const DevCollectArgs& a = wp->a;
    DcwState* ws = wp->ws;
    DcwEval* ev = wp->ev;
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
    // ---- 5'. the state of this side, uniform; the step before is settled, its episodes are rows of the log
    DcwScalars s = *dc_uniform_ptr<4>(&ws->s[side]);
    const int n_episode = *dc_uniform_ptr<4>(&ws->n_episode);
    if (first) { s.log_rows = 0; s.steps = 0; }
    s = dcw_eval_settle<NT>(ws, s, side, n_episode, tile, sh.live, wtot, writer, settle != 0, ev->park[side], wp->ep_log);
    const bool go = !settle && !s.finished;
    if (writer && tid == 0) {
        dcw_eval_hand_on(ws, s, go, nside);
        if (settled) *settled = s;          // a settle launch makes no step: what it hands on is s
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
    // ---- 2. env step, the running episode, the parked record, the flag; 4. the next observation (the row's own thread: no barrier)
    dcw_eval_env_step<Env>(a, sh, ws, ev, lt, n_valid, tile0, nside, Do);
    dc_next_obs<Env>(a, sh, lt, n_valid, Do);
}

template <int H, class Env, int HEAD>
__global__ __launch_bounds__(4 * H) DCW_NO_PK void wide_eval_step_kernel(const ModelDesc md, const float* __restrict__ P, const WideEvalArgs* __restrict__ wap,
                                                                         const int t, const int first, const int settle) {
    wide_eval_step_body<H, Env, HEAD>(md, P, dc_uniform_ptr<4>(wap), t, first, settle, __builtin_amdgcn_readfirstlane((int)blockIdx.x), nullptr);
}

// The layered form of wide_eval_step_body (wide_layered_step_body's arguments): both pointers are uniform and point into constant
// memory.  wide_eval_layered_step_kernel and wide_eval_layered_group_step_kernel call it.
template <class Env, int HEAD, bool DEVWS>
__device__ __forceinline__ void wide_eval_layered_step_body(const WideEvalArgs* __restrict__ wap, const WideLayActor* __restrict__ lap, const int t,
                                                            const int first, const int settle, const int tile, DcwScalars* settled, float* wl_lds,
                                                            DevCollectSmem& sh, float* raw, int32_t* wtot) {
    const WideEvalArgs* wp = dc_uniform_ptr<4>(wap);
    const WideLayActor& la = *dc_uniform_ptr<4>(lap);
    const DevCollectArgs& a = wp->a;
    DcwState* ws = wp->ws;
    DcwEval* ev = wp->ev;
    const float* P = dc_uniform_ptr<1>(la.P);
    const int side = t & 1, nside = side ^ 1;
    const int tile0 = 16 * tile;
    const bool writer = tile0 == 0;
    const int Do = a.ep.Do, Da = a.ep.Da;
    f32x4 b0[4], b1[4];
    wl_prefetch(b0, la, P, settle);
    // ---- 5'. as above
    DcwScalars s = *dc_uniform_ptr<4>(&ws->s[side]);
    const int n_episode = *dc_uniform_ptr<4>(&ws->n_episode);
    if (first) { s.log_rows = 0; s.steps = 0; }
    s = dcw_eval_settle<WL_NT>(ws, s, side, n_episode, tile, sh.live, wtot, writer, settle != 0, ev->park[side], wp->ep_log);
    const bool go = !settle && !s.finished;
    if (writer && threadIdx.x == 0) {
        dcw_eval_hand_on(ws, s, go, nside);
        if (settled) *settled = s;
    }
    if (!go || tile0 >= s.n_live) return;
    const int n_valid = min(16, s.n_live - tile0);
    __syncthreads();
    int lt = threadIdx.x;
    asm volatile("" : "+v"(lt));
    // ---- 0. / 1. the layered tile actor, the head
    wl_tile_actor<DEVWS>(a, la, P, sh, wl_lds, raw, b0, b1, lt, tile, n_valid);
    if (lt < n_valid * Da) {
        const int i = div_by_magic((unsigned)lt, a.magic_da), d = lt - i * Da;
        dc_head<HEAD>(a, sh, &raw[i * FSRL_MAX_ACT], P + la.net.sigma, la.unbounded, Da, i, d);
    }
    __syncthreads();
    // ---- 2. / 4.
    dcw_eval_env_step<Env>(a, sh, ws, ev, lt, n_valid, tile0, nside, Do);
    dc_next_obs<Env>(a, sh, lt, n_valid, Do);
}

template <class Env, int HEAD, bool DEVWS>
__global__ __launch_bounds__(WL_NT) WL_NO_PK void wide_eval_layered_step_kernel(const WideEvalArgs* __restrict__ wap, const WideLayActor* __restrict__ lap,
                                                                                const int t, const int first, const int settle) {
    extern __shared__ __align__(16) float wl_lds[];             // !DEVWS: [2][16][ldp]
    __shared__ DevCollectSmem sh;                               // the tile uses its first 16 rows
    __shared__ float raw[16 * FSRL_MAX_ACT];                    // the head's raw rows
    __shared__ int32_t wtot[16];
    wide_eval_layered_step_body<Env, HEAD, DEVWS>(wap, lap, t, first, settle, __builtin_amdgcn_readfirstlane((int)blockIdx.x), nullptr, wl_lds, sh, raw, wtot);
}
