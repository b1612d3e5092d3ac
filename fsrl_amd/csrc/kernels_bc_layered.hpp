// kernels_bc_layered.hpp -- behaviour cloning for LAYERED contexts (fsrl_bc_update_layered, host_bc_layered.inc): an actor of any
// depth and width (LayNet, kernels_layered.hpp) regressed onto stored actions in TWO launches per update, whatever the depth.
//
//   bc_lay_fwd_bwd_kernel<HEAD, DEVWS>   grid ceil(B / 16) x BCL_NT threads, one 16-row tile of the minibatch per workgroup.  The tile
//       walks 2 nl - 1 STAGES behind one another: the nl forward layers (the scheme of wl_tile_actor, kernels_devcollect_wide_layered.hpp),
//       the loss head, then the nl - 1 backward products dZ_{l-1} = (dZ_l W_l) * (Z_{l-1} > 0) from the head down to layer 1 (no dX of
//       layer 0).  A stage's jobs are its ceil(N / 16) output column tiles, taken round the 8 waves, one 16 x 16 accumulator per job.
//       A operand: the 16 x K rows the stage before left (activations going up, dZ coming down), 16-byte reads at row li.
//       B operand: straight from L2, 64 k per unit, addresses clamped, zero-fill by select.  Forward: lane (li, q) walks weight row
//       n0 + li along k (wl_load_w).  Backward: W_l is read K-MAJOR, lane (li, q) takes W_l[k0 + 16 u + 4 q + e][j0 + li] -- 16 lanes on
//       16 consecutive floats of one weight row.  No stage's weights depend on anything computed, so the loads run ONE UNIT AHEAD of
//       the MFMAs in a second register set, across job and stage boundaries: the next stage's first unit is issued before the barrier
//       that ends a stage, and the head's first backward unit before the loss head.  One barrier per stage (two round the loss head).
//       Epilogues: relu(Z_l) goes to the side buffer act[l] in HBM (the backward masks and the weight-gradient launch read it there),
//       dZ_{l-1} to dz[l-1]; the head's raw rows and the loss head's dout rows (zeros past the head width, FSRL_DOW wide) live in LDS,
//       dout goes to HBM as well, the tile's loss sum to a slot of its own.
//       Where the operand rows live.  DEVWS = false: dynamic LDS, two halves of 16 x ldp floats (dc_wl_stride: ldp / 4 odd, conflict-free
//       ds_read_b128); stage t reads half (t + 1) & 1 and writes half t & 1.  DEVWS = true (a layer wider than DCWL_LDS_WIDTH): the
//       same code with the A operand read from the tile's own rows of act[l - 1] / dz[l] in HBM -- written by this workgroup, visible
//       behind the stage's barrier (the rule lay_collect_kernel relies on); only the gathered obs rows stay in LDS.  The MFMA sequence is
//       the same in both forms, and so are the bits.  Rows past B read the tile's last valid slot, their dout is zero, so their dZ is.
//       MFMA rows are independent: a row's result does not depend on which rows share its tile.
//   bc_lay_wgrad_kernel   ONE launch for every layer: a workgroup of 4 waves per 16 x 16 output tile of some dW_l, found in a prefix
//       table over the layers with scalar arithmetic before the first operand load.  The body is bc_wgrad_body's (kernels_bc.hpp): the
//       waves split the minibatch rows four ways (MFMA 16x16x4 f32 over k = batch row, operands from dz[l] / act[l - 1]; layer 0: the
//       store's obs rows by index; the head: dout), partial tiles added through LDS in a fixed order, Adam in place (adam_element, dense
//       layout, no mirror), the gradient written to the context's vector.  Bias sums ride on the first column block's tiles; on-policy
//       dsigma_param and the update's mean loss have a workgroup each.  No atomics.
// Nothing is instantiated per shape.  Registers: the rules of kernels_devcollect.hpp (uniform arguments, opaque thread ids, magic
// divisions); no instantiation spills (tests/test_bc_layered_host.py).
#pragma once
#include "kernels_bc.hpp"
#include "kernels_devcollect_wide_layered.hpp"      // wl_load_w, WL_NO_PK

#define BCL_NT 512
#define BCL_NW (BCL_NT / 64)

struct BcLayArgs {
    const float* P;                                  // the actor's parameters (dense layered layout)
    const float* obs; const float* act;              // the store's columns
    const int* idx;                                  // [B] the minibatch's slots
    float* actb[FSRL_MAX_HIDDEN];                    // relu(Z_l), [rows_pad][round_up(w_l, 4)]
    float* dzb[FSRL_MAX_HIDDEN];                     // dL/dZ_l, the same shape
    float* dout;                                     // [rows_pad][FSRL_DOW]
    float* lossp;                                    // [tiles]
    int B, loss, mean_tanh, Do, Da, ldp;             // ldp: row stride of the LDS halves (DEVWS: of the obs rows)
    float max_action;
    LayNet net;
};

// one operand stream of a stage: output columns n < N, reduction k < K over the weight matrix W (row stride ldw)
struct BclOp { const float* W; int ldw, K, N, km; };      // km: k-major (backward), W[k][n]; else W[n][k]
__device__ __forceinline__ BclOp bcl_op(const BcLayArgs& a, const int t) {
    const int nl = a.net.nl, fwd = t < nl;
    const LayLayer ll = a.net.l[fwd ? t : 2 * nl - 1 - t];
    BclOp o;
    o.W = a.P + ll.W; o.ldw = ll.in; o.km = !fwd;
    o.K = fwd ? ll.in : ll.out; o.N = fwd ? ll.out : ll.in;
    return o;
}
// `b` where `second`, else `a`, field by field: a select between two structs by address would keep both in memory
__device__ __forceinline__ BclOp bcl_pick(const bool second, const BclOp& a, const BclOp& b) {
    BclOp o;
    o.W = second ? b.W : a.W; o.ldw = second ? b.ldw : a.ldw; o.K = second ? b.K : a.K; o.N = second ? b.N : a.N; o.km = second ? b.km : a.km;
    return o;
}
// 64 k of column tile ct from k0 on, for lane (li, q): straight-line, clamped into the matrix
__device__ __forceinline__ void bcl_load(f32x4 (&bv)[4], const BclOp& o, const int ct, const int k0, const int li, const int q) {
    const int n = min(16 * ct + li, o.N - 1);
    if (!o.km) wl_load_w(bv, o.W + (size_t)n * o.ldw, o.K, k0, q);
    else {
        const float* col = o.W + n;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int e = 0; e < 4; ++e) bv[u][e] = col[(size_t)min(k0 + 16 * u + 4 * q + e, o.K - 1) * o.ldw];
        }
    }
}
// one unit: the unit behind it is issued into `bn` first, then this one's A operand is read and its MFMAs run on `bv` (wl_unit's order)
__device__ __forceinline__ f32x4 bcl_unit(f32x4 acc, f32x4 (&bv)[4], f32x4 (&bn)[4], const float* in, const int K, const int k0, const int li, const int q,
                                          const bool ahead, const BclOp on, const int ctn, const int kn) {
    f32x4 av[4];
    const int ka = ((K + 3) & ~3) - 4;              // the last 16 bytes of an A row that hold a k < K
    if (ahead) bcl_load(bn, on, ctn, kn, li, q);
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

template <int HEAD, bool DEVWS>
__global__ __launch_bounds__(BCL_NT) WL_NO_PK void bc_lay_fwd_bwd_kernel(const BcLayArgs a) {
    extern __shared__ __align__(16) float bcl_lds[];            // !DEVWS: [2][16][ldp]; DEVWS: [16][ldp], the obs rows
    __shared__ __align__(16) float raw[16 * FSRL_MAX_ACT];      // the head's raw rows
    __shared__ __align__(16) float dsm[16 * FSRL_DOW];          // the tile's dout rows
    __shared__ float acts[16 * FSRL_MAX_ACT];                   // the stored actions
    __shared__ float rowl[16];
    int lt = threadIdx.x;
    asm volatile("" : "+v"(lt));
    const int wave = __builtin_amdgcn_readfirstlane(lt >> 6), lane = lt & 63, li = lane & 15, q = lane >> 4;
    const int tile = __builtin_amdgcn_readfirstlane((int)blockIdx.x), row0 = 16 * tile;
    const int nl = a.net.nl, T = 2 * nl - 1, Do = a.Do, Da = a.Da, ldp = a.ldp;
    const int n_valid = min(16, a.B - row0);                    // >= 1: the grid is ceil(B / 16)
    f32x4 b0[4], b1[4];             // the weights of this unit and of the one behind it: b0 holds the current unit's while par == 0
    int par = 0;
    BclOp op = bcl_op(a, 0);
    if (wave < ((op.N + 15) >> 4)) bcl_load(b0, op, wave, 0, li, q);
    // ---- prologue: the tile's obs rows into the half stage 0 reads, the stored actions, a clean dout tile
    {
        float* x = bcl_lds + (DEVWS ? 0 : 16 * ldp);
        const unsigned magic_do = div_magic(Do);
        for (int e = lt; e < 16 * Do; e += BCL_NT) {
            const int i = div_by_magic((unsigned)e, magic_do), k = e - i * Do;
            x[i * ldp + k] = a.obs[(size_t)a.idx[row0 + min(i, n_valid - 1)] * Do + k];
        }
        if (lt < 16 * FSRL_MAX_ACT) {
            const int i = lt >> 4, d = lt & 15;
            acts[lt] = a.act[(size_t)a.idx[row0 + min(i, n_valid - 1)] * Da + min(d, Da - 1)];
        }
        dsm[lt] = 0.0f;             // 16 * FSRL_DOW == BCL_NT
    }
    __syncthreads();
    for (int t = 0; t < T; ++t) {
        const bool fwd = t < nl, head = t == nl - 1;
        const int l = fwd ? t : 2 * nl - 1 - t;                 // forward: layer l; backward: the product through W_l, giving dZ_{l-1}
        const int K = op.K, N = op.N, CT = (N + 15) >> 4;
        // the stage's A rows, and where its epilogue leaves its own (sw: row stride of a side buffer)
        const float* in; int ldin;
        if (t == 0) { in = bcl_lds + (DEVWS ? 0 : 16 * ldp); ldin = ldp; }
        else if (t == nl) { in = dsm; ldin = FSRL_DOW; }
        else if (DEVWS) {
            const int lw = fwd ? l - 1 : l;
            ldin = (a.net.l[lw].out + 3) & ~3;
            in = (fwd ? a.actb[lw] : a.dzb[lw]) + (size_t)row0 * ldin;
        } else { in = bcl_lds + ((t + 1) & 1) * 16 * ldp; ldin = ldp; }
        in += li * ldin;
        float* half = bcl_lds + (t & 1) * 16 * ldp;
        const int lo = fwd ? l : l - 1, sw = (N + 3) & ~3;      // the hidden layer whose rows this stage produces (the head: none)
        float* side = head ? nullptr : (fwd ? a.actb[lo] : a.dzb[lo]) + (size_t)row0 * sw;
        const float* mask = fwd ? nullptr : a.actb[lo] + (size_t)row0 * sw;
        const int bias_off = a.net.l[l].b;
        const BclOp on = bcl_op(a, min(t + 1, T - 1));
        const bool more = t + 1 < T && wave < ((on.N + 15) >> 4);      // this wave has a column tile in the next stage
        if (wave >= CT && more) {           // idle in this stage: straight on
            if (par) bcl_load(b1, on, wave, 0, li, q);
            else bcl_load(b0, on, wave, 0, li, q);
        }
        for (int ct = wave; ct < CT; ct += BCL_NW) {
            f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int k0 = 0; k0 < K; k0 += 64) {
                // the unit behind this one: its weights are issued before this one's MFMAs
                int kn = k0 + 64, ctn = ct;
                bool ahead = true, nxt = false;
                if (kn >= K) {
                    kn = 0;
                    if (ct + BCL_NW < CT) ctn = ct + BCL_NW;
                    else if (more) { ctn = wave; nxt = true; }
                    else ahead = false;
                }
                const BclOp ob = bcl_pick(nxt, op, on);
                if (par) acc = bcl_unit(acc, b1, b0, in, K, k0, li, q, ahead, ob, ctn, kn);
                else acc = bcl_unit(acc, b0, b1, in, K, k0, li, q, ahead, ob, ctn, kn);
                par ^= 1;
            }
            const int n = 16 * ct + li;
            if (n < N) {
                const float bias = fwd ? a.P[bias_off + n] : 0.0f;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int m = 4 * q + r;
                    float v = acc[r] + bias;
                    if (head) { raw[m * FSRL_MAX_ACT + n] = v; continue; }
                    if (fwd) v = fmaxf(v, 0.0f);
                    else v = (mask[m * sw + n] > 0.0f) ? v : 0.0f;
                    side[m * sw + n] = v;
                    if (!DEVWS) half[m * ldp + n] = v;
                }
            }
        }
        if (head) {
            // ---- loss head: thread (row i = lt >> 4, dim d = lt & 15), the arithmetic of bc_fwd_bwd_body's
            __syncthreads();
            if (lt < 256) {
#pragma clang fp contract(off)
                const int i = lt >> 4, d = lt & 15;
                const float invB = 1.0f / (float)a.B;
                float ls_sum = 0.0f;
                if (i < n_valid && d < Da) {
                    const float x = raw[i * FSRL_MAX_ACT + d];
                    float m = x, dm = 1.0f;
                    if (HEAD == DC_HEAD_DDPG || a.mean_tanh) {
                        const float th = tanhf(x);
                        m = a.max_action * th; dm = a.max_action * (1.0f - th * th);
                    }
                    const float df = m - acts[i * FSRL_MAX_ACT + d];
                    if (HEAD == DC_HEAD_DDPG || a.loss == BC_LOSS_MSE) {
                        ls_sum = df * df;
                        dsm[i * FSRL_DOW + d] = (2.0f * df * invB) * dm;
                    } else {
                        float ls, pass = 1.0f;
                        if constexpr (HEAD == DC_HEAD_ONPOLICY) ls = a.P[a.net.sigma + d];
                        else {
                            const float lraw = raw[i * FSRL_MAX_ACT + Da + d];
                            pass = (lraw >= BC_LOG_SIG_MIN && lraw <= BC_LOG_SIG_MAX) ? 1.0f : 0.0f;      // clamp's gradient, bounds included
                            ls = fminf(fmaxf(lraw, BC_LOG_SIG_MIN), BC_LOG_SIG_MAX);
                        }
                        const float sg = expf(ls), var = sg * sg;
                        ls_sum = (df * df) / (2.0f * var) + ls;
                        dsm[i * FSRL_DOW + d] = ((df / var) * invB) * dm;
                        dsm[i * FSRL_DOW + (HEAD == DC_HEAD_ONPOLICY ? 16 : Da) + d] = ((1.0f - (df * df) / var) * invB) * pass;
                    }
                }
                float rl = 0.0f;                                // the row's dims in ascending order
                for (int dd = 0; dd < Da; ++dd) rl += __shfl(ls_sum, (lane & 48) + dd, 64);
                if (d == 0) rowl[i] = rl;                       // rows past the batch: 0
            }
        }
        __syncthreads();
        if (head) {
            a.dout[(size_t)row0 * FSRL_DOW + lt] = dsm[lt];
            if (lt == 0) {                                      // rows in ascending order (fixed => deterministic)
                float s = 0.0f;
                for (int i = 0; i < 16; ++i) s += rowl[i];
                a.lossp[tile] = s;
            }
        }
        op = on;
    }
}

// ------------------------------------------------------------------------------ weight gradients + Adam, every layer in one launch
struct BcLayWgradArgs {
    const float* obs; const int* idx;
    const float* actb[FSRL_MAX_HIDDEN]; const float* dzb[FSRL_MAX_HIDDEN]; const float* dout;
    float* P; float* M; float* V; float* G;
    const float* lossp; float* loss_out; int tiles;      // loss_out[0] = sum(lossp) / B
    int B, rows_pad, sigma_job, sigma_zero, Do, Da;      // as BcWgradArgs
    float one_minus_b1, beta2, one_minus_b2, step_size, bc2_sqrt, eps;
    int pre[FSRL_MAX_HIDDEN + 2];                        // pre[l]: the first workgroup of layer l's tiles; pre[nl]: the extra jobs
    unsigned mag[FSRL_MAX_HIDDEN + 1];                   // div_magic(column tiles of layer l)
    LayNet net;
};
// the table of a shape, built once per call -> workgroups of a launch
static inline int bc_lay_wg_table(BcLayWgradArgs& w) {
    int n = 0;
    for (int l = 0; l < w.net.nl; ++l) {
        const int kt = (w.net.l[l].in + 15) / 16;
        w.pre[l] = n; w.mag[l] = div_magic(kt);
        n += ((w.net.l[l].out + 15) / 16) * kt;
    }
    w.pre[w.net.nl] = n;
    return n + (w.sigma_job ? 1 : 0) + 1;
}

__global__ __launch_bounds__(256) void bc_lay_wgrad_kernel(const BcLayWgradArgs a) {
    __shared__ float part[4][256];
    __shared__ float partb[4][16];
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, q = lane >> 4;
    const int b = __builtin_amdgcn_readfirstlane((int)blockIdx.x), nb = (int)gridDim.x;
    const int nl = a.net.nl, Da = a.Da;
    if (b == nb - 1) {                                       // the update's mean loss: tiles in ascending order
        if (tid == 0) {
            float t = 0.0f;
            for (int i = 0; i < a.tiles; ++i) t += a.lossp[i];
            a.loss_out[0] = t / (float)a.B;
        }
        if (a.sigma_zero && tid < Da) a.G[a.net.sigma + tid] = 0.0f;
        return;
    }
    // job (bc_wgrad_body's): Y[rows][ldy] (columns n0 .., valid below nlim) x X[rows][ldx] (columns k0 .., valid below klim) -> W[n][k]
    const float *Y, *X = nullptr;
    int ldy, ldx = 0, n0, k0 = 0, nlim, klim = 0, wbase = 0, ldw = 0, bbase = 0;
    bool gather = false, bias_only = false, has_bias = true;
    if (b < a.pre[nl]) {
        int l = 0;
        while (b >= a.pre[l + 1]) ++l;                       // uniform: scalar loads and compares
        const LayLayer ll = a.net.l[l];
        const int bt = b - a.pre[l], kt = (ll.in + 15) >> 4, rt = div_by_magic((unsigned)bt, a.mag[l]);
        n0 = 16 * rt; k0 = 16 * (bt - rt * kt);
        if (l == nl - 1) { Y = a.dout; ldy = FSRL_DOW; } else { Y = a.dzb[l]; ldy = (ll.out + 3) & ~3; }
        if (l == 0) { X = a.obs; ldx = a.Do; gather = true; } else { X = a.actb[l - 1]; ldx = (ll.in + 3) & ~3; }
        nlim = ll.out; klim = ll.in; wbase = ll.W; ldw = ll.in; bbase = ll.b; has_bias = k0 == 0;
    } else {                                                 // on-policy nll: dsigma_param = the column sums of dout[:, 16 + d]
        n0 = 16; Y = a.dout; X = a.dout; ldy = FSRL_DOW; nlim = 16 + Da; bbase = a.net.sigma - 16; bias_only = true;
    }
    const bool yon = n0 + li < nlim, xon = !bias_only && k0 + li < klim;
    const float* __restrict__ yp = Y + n0 + (yon ? li : 0);
    const float* __restrict__ xp = X + k0 + (xon ? li : 0);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f}, accb = {0.f, 0.f, 0.f, 0.f};
    // wave w takes the 4-row chunks w, w + 4, ...; rows past the batch hold zeros in dz / dout and finite activations
    constexpr int U = 4;
    for (int c0 = wave; c0 < a.rows_pad / 4; c0 += 4 * U) {
        float yv[U], xv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int r = 4 * (c0 + 4 * u) + q;
            const bool in = r < a.rows_pad;
            const int rc = in ? r : 0;
            yv[u] = (in && yon) ? yp[(size_t)rc * ldy] : 0.0f;
            float x = 0.0f;
            if (in && xon) {
                if (gather) { if (r < a.B) x = xp[(size_t)a.idx[r] * ldx]; }
                else x = xp[(size_t)rc * ldx];
            }
            xv[u] = x;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!bias_only) acc = mfma_16x16x4(yv[u], xv[u], acc);
            if (has_bias) accb = mfma_16x16x4(yv[u], 1.0f, accb);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        part[wave][(4 * q + r) * 16 + li] = acc[r];
        if (li == 0) partb[wave][4 * q + r] = accb[r];
    }
    __syncthreads();
    ModelDesc none{};                                        // dense layered layout: no W2 mirror to keep
    const int nn = tid >> 4, kk = tid & 15;
    if (!bias_only && n0 + nn < nlim && k0 + kk < klim) {
        const float g = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
        const int i = wbase + (n0 + nn) * ldw + k0 + kk;
        a.G[i] = g;
        adam_element(a.P, a.M, a.V, i, a.P[i], g, 1.0f, 0.0f, a.one_minus_b1, a.beta2, a.one_minus_b2, a.step_size, a.bc2_sqrt, a.eps, none,
                     nullptr, 0.0f, 0.0f);
    }
    if (has_bias && tid < 16 && n0 + tid < nlim) {
        const float g = (partb[0][tid] + partb[1][tid]) + (partb[2][tid] + partb[3][tid]);
        const int i = bbase + n0 + tid;
        a.G[i] = g;
        adam_element(a.P, a.M, a.V, i, a.P[i], g, 1.0f, 0.0f, a.one_minus_b1, a.beta2, a.one_minus_b2, a.step_size, a.bc2_sqrt, a.eps, none,
                     nullptr, 0.0f, 0.0f);
    }
}
