// kernels_devcollect_wide_layered.hpp -- wide device collects for LAYERED contexts (fsrl_collect_device_wide_layered): the launch
// scheme of kernels_devcollect_wide.hpp -- one launch per vector step, one workgroup per 16-row tile of the live list, phase 5 of a
// step settled at the start of the next launch -- around an actor of any depth and width (LayNet, kernels_layered.hpp).
//
// wide_layered_step_kernel<Env, HEAD, DEVWS>, grid ceil(first_live / 16) x WL_NT threads; nothing is instantiated per shape:
//   5'. dcw_settle<WL_NT>, the state hand-over, the `first` / `settle` arguments and the early exits of wide_collect_step_kernel, as
//       they are.  Every wave has the first 64 k of its first weight row of layer 0 in flight before it.
//   0.  the tile's live rows' observations -> the half of the activation buffer layer 0 reads
//   1.  the actor on the tile's 16 rows, layer by layer, Z_l = relu(Z_{l-1} W_l^T + b_l).  A layer's jobs are its ceil(N / 16)
//       column tiles, taken round the waves; a wave accumulates one 16 x 16 output tile at a time.
//       A operand: the 16 x K activations, shared by every wave, in 16-byte reads at row li, k = k0 + 16 u + 4 q.  The buffer is two
//       halves of 16 rows; layer l reads half (l + 1) & 1 and writes half l & 1 (bias, relu) directly -- no staging round trip, ONE
//       barrier per layer.
//       B operand: the weight rows from L2 as layc_tile loads them (straight-line, 64 k per round trip, addresses clamped into the
//       row, zero-fill by select, four dword loads where K & 3).  A layer's weights do not depend on the layer before it, so the
//       loads run ONE UNIT AHEAD of the MFMAs in a second set of 16 registers: the next 64 k of the row, else the first 64 k of the
//       wave's next column tile, else the first 64 k of its first column tile of layer l + 1 -- issued before the barrier that ends
//       layer l, so that the barrier and the epilogue hide an L2 round trip.
//       The head's raw rows go to a 16 x FSRL_MAX_ACT LDS array and through dc_head<HEAD>.
//   2 - 4. dcw_env_step, dc_store_rows, dc_next_obs, unchanged.
// Where the activations live.  DEVWS = false: dynamic LDS, 2 x 16 x ldp floats sized to the shape at launch (dc_wl_stride,
// devcollect_plan.hpp): a 64x48x32 net takes 8.5 KB and several tiles share a CU, a 1024-wide one 128.5 KB.  The row stride ldp is
// the first multiple of 4 at or above ld with ldp / 4 ODD: lane (li, q) of a wave reads the 16 bytes at float li * ldp + 4 q + const,
// i.e. the four-bank group (li * (ldp / 4) + q) mod 16 of the 64 banks, and with an odd multiplier the sixteen rows of one q group
// land in sixteen different groups -- every 16-lane pass of a ds_read_b128 touches each bank once, whichever k the chunk is at
// (ldp = ld, a multiple of 64 at the widths that matter, would put all sixteen rows in ONE group: a 16-way conflict).  The epilogue's
// stores are a float per lane along a row: conflict-free at any stride.
// DEVWS = true (a layer wider than DCWL_LDS_WIDTH: the halves do not fit next to the static arrays): the same code over the tile's
// slice of a device-memory workspace the env owns, [tiles][2][16][ld]; the writes of a layer are visible to the workgroup's other
// waves behind the same barrier (as in lay_collect_kernel).  The MFMA sequence is the same in both forms, and so are the bits.
// Bits.  Every output element is accumulated in ONE accumulator by the MFMA sequence of lin_body<LIN_F> / layc_tile: sub-chunks of
// 16 k issued while their first k < K, s = 0..3 inside, lane (i, q) feeding k = 16 kc + 4 q + s, zeros past K, then bias, then relu.
// A row's action is the action lay_collect_kernel and fsrl_collect_step compute for it; draws are keyed by (env id, ordinal, t).
// Rows of the tile beyond the live count read the tile's last live row (MFMA rows are independent) and are not written.
// Registers: the rules of kernels_devcollect.hpp -- arguments through pointers and scalar loads, opaque thread ids, magic divisions.
// 512 threads: two waves per SIMD, 256 VGPRs a lane; no instantiation spills (tests/test_devcollect_wide_layered_host.py).
#pragma once
#include "kernels_devcollect_wide.hpp"
#include "kernels_devcollect_layered.hpp"

#define WL_NT 512
#define WL_NW (WL_NT / 64)

// whose actor a wide layered launch runs (device memory, next to the env's WideCollectArgs; constant for the length of a launch)
struct WideLayActor {
    const float* P;             // on-policy: the context's parameters; replay: SacState::PA
    float* ws;                  // DEVWS: [tiles][2][16][ldp]; else null
    int ld, ldp;                // round_up(max(widest hidden layer, obs_dim), 4); the row stride (DEVWS: ld itself)
    int unbounded;              // on-policy: the mean is the head itself
    LayNet net;
};

// 64 k of a weight row from k0 on, as layc_tile loads them: lane q's four dwordx4 (or sixteen dwords), clamped into the row
__device__ __forceinline__ void wl_load_w(f32x4 (&bv)[4], const float* wrow, const int K, const int k0, const int q) {
    if ((K & 3) == 0) {         // one branch for the sixteen loads
#pragma unroll
        for (int u = 0; u < 4; ++u) bv[u] = *reinterpret_cast<const f32x4*>(wrow + min(k0 + 16 * u + 4 * q, K - 4));
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int e = 0; e < 4; ++e) bv[u][e] = wrow[min(k0 + 16 * u + 4 * q + e, K - 1)];
        }
    }
}
// one unit of a column tile: 64 k from k0 on.  `ahead`: the unit behind it is issued into `bn` first, then this one's A operand is read
// and its MFMAs run on `bv` -- no register copies between the two sets, so the loads have a whole unit to land
__device__ __forceinline__ f32x4 wl_unit(f32x4 acc, f32x4 (&bv)[4], f32x4 (&bn)[4], const float* in, const int K, const int ka, const int k0, const int q,
                                         const bool ahead, const float* wn, const int Kn, const int kn) {
    f32x4 av[4];
    if (ahead) wl_load_w(bn, wn, Kn, kn, q);
#pragma unroll
    for (int u = 0; u < 4; ++u) av[u] = *reinterpret_cast<const f32x4*>(in + min(k0 + 16 * u + 4 * q, ka));
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int k = k0 + 16 * u + 4 * q;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            av[u][e] = (k + e < K) ? av[u][e] : 0.0f;
            bv[u][e] = (k + e < K) ? bv[u][e] : 0.0f;
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        if (k0 + 16 * u < K) {          // uniform; the rest of the chunk is zeros
#pragma unroll
            for (int sx = 0; sx < 4; ++sx) acc = mfma_16x16x4(av[u][sx], bv[u][sx], acc);
        }
    }
    return acc;
}
__device__ __forceinline__ const float* wl_wrow(const float* P, const LayLayer& ll, const int ct, const int li) {
    return P + ll.W + (size_t)min(16 * ct + li, ll.out - 1) * ll.in;
}

// Every wave's first 64 k of its first weight row of layer 0, issued before the settle (not in a settle launch: it runs no actor)
__device__ __forceinline__ void wl_prefetch(f32x4 (&b0)[4], const WideLayActor& la, const float* P, const int settle) {
    int t0 = threadIdx.x;
    asm volatile("" : "+v"(t0));
    const int wave = __builtin_amdgcn_readfirstlane(t0 >> 6), li = t0 & 15, q = (t0 & 63) >> 4;
    const LayLayer l0 = la.net.l[0];
    if (!settle && wave < ((l0.out + 15) >> 4)) wl_load_w(b0, wl_wrow(P, l0, wave, li), l0.in, 0, q);
}
// Phases 0 and 1 of a tile's step, the layered tile actor: the live rows' observations, then the layers; the head's raw rows are left in
// `raw` behind the last layer's barrier.  b0: what wl_prefetch issued.  Every thread of the workgroup calls it (barriers).
// wide_layered_step_body and the evaluation's body (kernels_deveval_wide.hpp) are this function between their own settle and phase 2.
template <bool DEVWS>
__device__ __forceinline__ void wl_tile_actor(const DevCollectArgs& a, const WideLayActor& la, const float* P, DevCollectSmem& sh, float* wl_lds, float* raw,
                                              f32x4 (&b0)[4], f32x4 (&b1)[4], const int lt, const int tile, const int n_valid) {
    const int Do = a.ep.Do, ldp = la.ldp, nl = la.net.nl;
    int par = 0;
    float* act;
    if constexpr (DEVWS) act = const_cast<float*>(dc_uniform_ptr<1>((const float*)la.ws)) + (size_t)tile * 32 * ldp;
    else act = wl_lds;
    // ---- 0. the tile's observations, in position order, into the half layer 0 reads
    {
        const unsigned magic_do = div_magic(Do);
        for (int x = lt; x < n_valid * Do; x += WL_NT) {
            const int p = div_by_magic((unsigned)x, magic_do), k = x - p * Do;
            act[(16 + p) * ldp + k] = a.ea.obs[(size_t)sh.live[p] * Do + k];
        }
    }
    __syncthreads();
    // ---- 1. the actor, layer by layer; layer l reads half (l + 1) & 1 and writes half l & 1
    {
        const int wave = __builtin_amdgcn_readfirstlane(lt >> 6), lane = lt & 63, li = lane & 15, q = lane >> 4;
        const int arow = min(li, n_valid - 1) * ldp;
        for (int l = 0; l < nl; ++l) {
            const LayLayer ll = la.net.l[l];
            const int K = ll.in, N = ll.out, CT = (N + 15) >> 4;
            const float* in = act + ((l + 1) & 1) * 16 * ldp + arow;
            float* out = act + (l & 1) * 16 * ldp;
            const bool head = l == nl - 1;
            const int ka = ((K + 3) & ~3) - 4;          // the last 16 bytes of an A row that hold a k < K
            const LayLayer ln = la.net.l[head ? l : l + 1];
            const bool more = !head && wave < ((ln.out + 15) >> 4);        // this wave has a column tile in the next layer
            if (wave >= CT && more) {           // idle in this layer: straight on
                if (par) wl_load_w(b1, wl_wrow(P, ln, wave, li), ln.in, 0, q);
                else wl_load_w(b0, wl_wrow(P, ln, wave, li), ln.in, 0, q);
            }
            for (int ct = wave; ct < CT; ct += WL_NW) {
                const float* wrow = wl_wrow(P, ll, ct, li);
                f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
                for (int k0 = 0; k0 < K; k0 += 64) {
                    // the unit behind this one: its weights are issued before this one's MFMAs
                    const float* wn = wrow;
                    int Kn = K, kn = k0 + 64;
                    bool ahead = true;
                    if (kn >= K) {
                        kn = 0;
                        if (ct + WL_NW < CT) wn = wl_wrow(P, ll, ct + WL_NW, li);
                        else if (more) { wn = wl_wrow(P, ln, wave, li); Kn = ln.in; }
                        else ahead = false;
                    }
                    if (par) acc = wl_unit(acc, b1, b0, in, K, ka, k0, q, ahead, wn, Kn, kn);
                    else acc = wl_unit(acc, b0, b1, in, K, ka, k0, q, ahead, wn, Kn, kn);
                    par ^= 1;
                }
                const int n = 16 * ct + li;
                if (n < N) {
                    const float bias = P[ll.b + n];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int m = 4 * q + r;
                        if (m < n_valid) {
                            const float v = acc[r] + bias;
                            if (head) raw[m * FSRL_MAX_ACT + n] = v;
                            else out[m * ldp + n] = fmaxf(v, 0.0f);
                        }
                    }
                }
            }
            __syncthreads();
        }
    }
}

// Compiled without the packed-fp32 instructions (v_pk_add / mul / fma_f32): the arithmetic outside the MFMAs is a few dozen
// operations a step, the one-lane forms round identically, and the kernel does not depend on how the two-lane forms behave.
#if defined(__HIP_DEVICE_COMPILE__)
#define WL_NO_PK __attribute__((target("no-packed-fp32-ops")))
#else
#define WL_NO_PK            // the host pass does not know the feature
#endif
// One workgroup's launch: a tile of ONE collect (wide_collect_step_body's arguments, the actor's row in the place of (md, P)); both
// pointers are uniform and point into constant memory (read through dc_uniform_ptr<4> here).  wide_layered_step_kernel and wide_layered_group_step_kernel call it.
template <class Env, int HEAD, bool DEVWS>
__device__ __forceinline__ void wide_layered_step_body(const WideCollectArgs* __restrict__ wap, const WideLayActor* __restrict__ lap, const int t, const int first,
                                                       const int settle, const int tile, DcwScalars* settled, float* wl_lds, DevCollectSmem& sh,
                                                       float* raw, int32_t* wtot) {
    const WideCollectArgs* wp = dc_uniform_ptr<4>(wap);
    const WideLayActor& la = *dc_uniform_ptr<4>(lap);
    const DevCollectArgs& a = wp->a;
    DcwState* ws = wp->ws;
    const float* P = dc_uniform_ptr<1>(la.P);
    const int side = t & 1, nside = side ^ 1;
    const int tile0 = 16 * tile;
    const bool writer = tile0 == 0;
    const int Do = a.ep.Do, Da = a.ep.Da;
    f32x4 b0[4], b1[4];         // the weights of this unit and of the one behind it: b0 holds the current unit's while par == 0
    wl_prefetch(b0, la, P, settle);
    // ---- 5'. the state of this side, uniform; the step before is settled
    DcwScalars s = *dc_uniform_ptr<4>(&ws->s[side]);
    const int n_episode = *dc_uniform_ptr<4>(&ws->n_episode);
    if (first) { s.log_rows = 0; s.steps = 0; }
    s = dcw_settle<WL_NT>(ws, s, side, n_episode, tile0, sh.live, wtot, writer);
    const bool go = !settle && !s.finished && s.log_rows + s.n_live <= wp->log_cap;
    if (writer && threadIdx.x == 0) {
        DcwScalars nx = s;
        if (go) { nx.log_rows = s.log_rows + s.n_live; nx.steps = s.steps + 1; nx.pending = 1; }
        ws->s[nside] = nx;
        if (settled) *settled = nx;
    }
    if (!go || tile0 >= s.n_live) return;
    const int n_valid = min(16, s.n_live - tile0);
    __syncthreads();
    int lt = threadIdx.x;
    asm volatile("" : "+v"(lt));
    wl_tile_actor<DEVWS>(a, la, P, sh, wl_lds, raw, b0, b1, lt, tile, n_valid);
    if (lt < n_valid * Da) {
        const int i = div_by_magic((unsigned)lt, a.magic_da), d = lt - i * Da;
        dc_head<HEAD>(a, sh, &raw[i * FSRL_MAX_ACT], P + la.net.sigma, la.unbounded, Da, i, d);
    }
    __syncthreads();
    // ---- 2. env step, scalars of the row, log, flag
    dcw_env_step<Env, HEAD>(a, sh, ws, lt, n_valid, tile0, s.log_rows + tile0, nside, Do);
    __syncthreads();
    // ---- 3. the rows' vectors into the store; 4. the next observation
    dc_store_rows(a, sh, lt, WL_NT, n_valid, Do, Da);
    __syncthreads();
    dc_next_obs<Env>(a, sh, lt, n_valid, Do);
}

template <class Env, int HEAD, bool DEVWS>
__global__ __launch_bounds__(WL_NT) WL_NO_PK void wide_layered_step_kernel(const WideCollectArgs* __restrict__ wap, const WideLayActor* __restrict__ lap,
                                                                           const int t, const int first, const int settle) {
    extern __shared__ __align__(16) float wl_lds[];             // !DEVWS: [2][16][ldp]
    __shared__ DevCollectSmem sh;                               // the tile uses its first 16 rows
    __shared__ float raw[16 * FSRL_MAX_ACT];                    // the head's raw rows
    __shared__ int32_t wtot[16];
    wide_layered_step_body<Env, HEAD, DEVWS>(wap, lap, t, first, settle, __builtin_amdgcn_readfirstlane((int)blockIdx.x), nullptr, wl_lds, sh, raw, wtot);
}

// ---- k wide layered collects in one launch per vector step: the grid, the member table and the settle launch of
// wide_collect_group_step_kernel (kernels_devcollect_wide.hpp) around wide_layered_step_body.  A member's row names its own
// WideLayActor -- parameters, LayNet, and in the DEVWS form its own workspace, indexed by the tile's number in THAT member's list.
// The members share hidden_sizes (the host checks it), so one dynamic LDS size and one form serve the whole launch.
template <class Env, int HEAD, bool DEVWS>
__global__ __launch_bounds__(WL_NT) WL_NO_PK void wide_layered_group_step_kernel(const WideGroupTable* __restrict__ tab, DcwScalars* __restrict__ settled,
                                                                                 const int j, const int first, const int settle) {
    extern __shared__ __align__(16) float wl_lds[];             // !DEVWS: [2][16][ldp]
    __shared__ DevCollectSmem sh;                               // the tile uses its first 16 rows
    __shared__ float raw[16 * FSRL_MAX_ACT];                    // the head's raw rows
    __shared__ int32_t wtot[16];
    const WideGroupTable* tb = dc_uniform_ptr<4>(tab);
    int m, tile;
    dcwg_find(tb, settle, m, tile);
    wide_layered_step_body<Env, HEAD, DEVWS>(tb->wa[m], tb->la[m], tb->par0[m] + j, first, settle, tile,
                                             settle ? settled + m : nullptr, wl_lds, sh, raw, wtot);
}
