// kernels_bc.hpp -- behaviour cloning on the device: the fused actors regressed onto stored actions (fsrl_bc_update, host_bc.inc).
//
// One update is TWO launches, no atomics, no waits between workgroups:
//   bc_fwd_bwd_kernel<H, HEAD>   one workgroup (4 * H threads) per 16-row tile of the minibatch: gathers the tile's obs / act rows from
//                                the store by index, runs the actor forward (TileStage / tile_forward, the collectors' own), evaluates
//                                the supervised loss head on 16 * Da lanes, forms dz3 and walks back dz3 -> dz2 -> dz1 (tile_backward:
//                                MFMA 16x16x4 f32, ReLU masks off the forward activations in LDS).  h1, h2, dz1, dz2, dz3 of its rows go to
//                                side buffers, the tile's loss sum to a slot of its own.
//   bc_wgrad_kernel<H>           one workgroup (4 waves) per 16 x 16 OUTPUT tile of dW2 / dW1 / dW3: the waves split the minibatch's rows
//                                four ways (MFMA 16x16x4 f32, operands straight from the side buffers), add their partial tiles through
//                                LDS in a fixed order and step the tile's 256 parameters with Adam at once -- a gradient element is final
//                                the moment its workgroup has reduced it (no clip: nothing global stands between it and the step).  The
//                                bias sums ride on the tiles of the first column block; on-policy dsigma_param and the update's mean
//                                loss have a workgroup each.
//
// The backward W2 fragment (lane (li, q) of wave w: W2[16 jc + 4 q + s][16 w + li], H / 4 registers per lane) is NOT a second cold
// fetch behind the forward one: its first BcEarly<H>::JE row groups are issued in the prologue, right behind the forward burst, and stay in
// registers across the forward pass -- all of them at H = 64 / 128 (16 / 32 registers), 6 of 16 at H = 256, where the forward fragment
// alone is 64 of the 128 registers a 1024-thread workgroup's lanes have (8 row groups spill); the other 10 are issued the moment the forward fragment is
// dead and lands under the loss head, the activation spills and dz2 (two barriers), in front of the dz1 MFMAs that read it.
// LDS cannot hold it (256 KB at H = 256 against 160 KB), and tile_forward's trickle hook exists on its 4- / 8-row path only.
#pragma once
#include "kernels_mlp.hpp"
#include "kernels_fb.hpp"
#include "kernels_devcollect.hpp"      // DC_HEAD_*

#define BC_LOSS_MSE 0
#define BC_LOSS_NLL 1
#define BC_LOG_SIG_MIN (-20.0f)
#define BC_LOG_SIG_MAX 2.0f

template <int H> struct BcEarly { static constexpr int JE = H == 256 ? 6 : H / 16; };   // row groups of the backward fragment issued early

struct BcArgs {
    const float* obs; const float* act;      // the store's columns
    const int* idx;                          // [B] the minibatch's slots
    float* A1; float* A2; float* D1; float* D2; float* DO;      // [rows_pad][H] x 4, [rows_pad][FSRL_DOW]
    float* lossp;                            // [tiles] per-tile sums of the rows' losses
    int B, loss, mean_tanh;                  // mean_tanh: m = max_action * tanh(head) (always for DC_HEAD_DDPG), else m = head
    float max_action;
};

// The tile's whole pass.  bc_fwd_bwd_kernel runs it on its arguments, bc_fwd_bwd_group_kernel (kernels_bc_group.hpp) on the member's:
// ONE body, so a member's tile is the solo tile instruction for instruction.  `tile` is uniform (a scalar register).
template <int H, int HEAD>
__device__ __forceinline__ void bc_fwd_bwd_body(const float* __restrict__ P, const ModelDesc& md, const BcArgs& a, const int tile) {
    __shared__ TileSmem<H> sm;
    constexpr int NT = TileGeom<H>::NT;
    constexpr int KC = H / 16, JE = BcEarly<H>::JE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, q = lane >> 4;
    const int row0 = tile * 16;
    const NetOff no = md.net[0];
    const int Do = md.Do, Da = md.Da;
    const int n_valid = min(16, a.B - row0);           // >= 1: the grid is ceil(B / 16)
    const float invB = 1.0f / (float)a.B;

    // ---- prologue: the small parameters, the gathered rows (element e = row * Do + k, the stage's own mapping; rows past the batch
    //      read the tile's last valid slot and are masked), then the two W2 bursts behind them
    TileStage<H> stg;
    stg.issue_params(P, no, Do, Da, tid);
    {
        const int nx = n_valid * Do;
        const unsigned magic = div_magic(Do);
#pragma unroll
        for (int u = 0; u < TileStage<H>::NX; ++u) {
            const int e = tid + u * NT, ec = min(e, nx - 1);
            const int i = div_by_magic((unsigned)ec, magic), k = ec - i * Do;
            const float v = a.obs[(size_t)a.idx[row0 + i] * Do + k];
            stg.xv[u] = (e < nx) ? v : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < TileStage<H>::NR; ++u) {       // row data: the stored action in columns [0, Da)
            const int e = tid + u * NT, i = min(e / FSRL_RD, n_valid - 1), f = min(e % FSRL_RD, Da - 1);
            const float v = a.act[(size_t)a.idx[row0 + i] * Da + f];
            stg.rdv[u] = (e / FSRL_RD < n_valid && e % FSRL_RD < Da) ? v : 0.0f;
        }
    }
    FwdW2Frag<H> wf;
    wf.load(P + no.W2f, wave, lane);
    float wb[KC][4];
    const float* __restrict__ W2c = P + no.W2 + wave * 16 + li;
#pragma unroll
    for (int jc = 0; jc < JE; ++jc) {
#pragma unroll
        for (int s = 0; s < 4; ++s) wb[jc][s] = W2c[(size_t)(16 * jc + 4 * q + s) * H];
    }
    for (int e = tid; e < 16 * FSRL_DOW; e += NT) sm.dout[e] = 0.0f;
    stg.commit(sm, no, Do, tid);
    __syncthreads();
    tile_forward<H, 16, HEAD == DC_HEAD_GAUSS>(sm, P, no, Do, tid, wf);      // sm.out[i][0..Da) = mean head (DC_HEAD_GAUSS: [Da..2Da) raw log sigma)
#pragma unroll
    for (int jc = JE; jc < KC; ++jc) {
#pragma unroll
        for (int s = 0; s < 4; ++s) wb[jc][s] = W2c[(size_t)(16 * jc + 4 * q + s) * H];
    }

    // ---- loss head: thread (row i = tid >> 4, dim d = tid & 15), 16-lane shuffles per row
    if (tid < 256) {
#pragma clang fp contract(off)
        const int i = tid >> 4, d = tid & 15;
        float l = 0.0f;
        if (i < n_valid && d < Da) {
            const float x = sm.out[i * FSRL_MAX_ACT + d];
            float m = x, dm = 1.0f;
            if (HEAD == DC_HEAD_DDPG || a.mean_tanh) {
                const float th = tanhf(x);
                m = a.max_action * th; dm = a.max_action * (1.0f - th * th);
            }
            const float df = m - sm.rd[i * FSRL_RD + d];
            if (HEAD == DC_HEAD_DDPG || a.loss == BC_LOSS_MSE) {
                l = df * df;
                sm.dout[i * FSRL_DOW + d] = (2.0f * df * invB) * dm;
            } else {
                float ls, pass = 1.0f;
                if constexpr (HEAD == DC_HEAD_ONPOLICY) ls = sm.sig[d];
                else {
                    const float lraw = sm.out[i * FSRL_MAX_ACT + Da + d];
                    pass = (lraw >= BC_LOG_SIG_MIN && lraw <= BC_LOG_SIG_MAX) ? 1.0f : 0.0f;      // clamp's gradient, bounds included
                    ls = fminf(fmaxf(lraw, BC_LOG_SIG_MIN), BC_LOG_SIG_MAX);
                }
                const float sg = expf(ls), var = sg * sg;
                l = (df * df) / (2.0f * var) + ls;
                sm.dout[i * FSRL_DOW + d] = ((df / var) * invB) * dm;
                const float dls = ((1.0f - (df * df) / var) * invB) * pass;
                sm.dout[i * FSRL_DOW + (HEAD == DC_HEAD_ONPOLICY ? 16 : Da) + d] = dls;
            }
        }
        float rowl = 0.0f;                                   // the row's dims in ascending order
        for (int dd = 0; dd < Da; ++dd) rowl += __shfl(l, (lane & 48) + dd, 64);
        if (d == 0) sm.st[i * 4] = rowl;                     // rows past the batch: l = 0
    }
    __syncthreads();
    if (tid == 0) {                                          // rows in ascending order (fixed => deterministic)
        float t = 0.0f;
        for (int i = 0; i < 16; ++i) t += sm.st[i * 4];
        a.lossp[tile] = t;
    }
    tile_backward<H, 16>(sm, no, wb, a.A1 + (size_t)row0 * H, a.A2 + (size_t)row0 * H, a.D1 + (size_t)row0 * H,
                         a.D2 + (size_t)row0 * H, a.DO + (size_t)row0 * FSRL_DOW, tid, false);
}
template <int H, int HEAD>
__global__ __launch_bounds__(4 * H) void bc_fwd_bwd_kernel(const float* __restrict__ P, const ModelDesc md, const BcArgs a) {
    bc_fwd_bwd_body<H, HEAD>(P, md, a, (int)blockIdx.x);
}

// ------------------------------------------------------------------------------ weight gradients + Adam
struct BcWgradArgs {
    const float* A1; const float* A2; const float* D1; const float* D2; const float* DO;
    const float* obs; const int* idx;        // layer 1's input rows, gathered again by slot
    float* P; float* M; float* V;            // the actor's parameter store (W2 mirror behind it) and its Adam moments
    float* G;                                // the step's gradient, parameter layout
    const float* lossp; float* loss_out; int tiles;      // loss_out[0] = sum(lossp) / B
    int B, rows_pad, sigma_job;              // sigma_job: on-policy nll, dsigma_param = the column sums of DO[:, 16 + d]
    int sigma_zero;                          // on-policy mse: sigma_param takes no part, its slots of G are cleared (no Adam step)
    float one_minus_b1, beta2, one_minus_b2, step_size, bc2_sqrt, eps;
};
// workgroups of a launch: dW2 tiles | dW1 tiles | dW3 tiles | (dsigma_param) | the loss
__host__ __device__ constexpr int bc_wg_n2(int H) { return (H / 16) * (H / 16); }
__host__ __device__ inline int bc_wg_n1(int H, int Do) { return (H / 16) * ((Do + 15) / 16); }
__host__ __device__ inline int bc_wg_grid(int H, int Do, int sigma_job) { return bc_wg_n2(H) + bc_wg_n1(H, Do) + H / 16 + (sigma_job ? 1 : 0) + 1; }

// workgroup b of the nb = bc_wg_grid(...) of one update (the solo launch's grid; a member's share of the grouped launch's)
template <int H>
__device__ __forceinline__ void bc_wgrad_body(const ModelDesc& md, const BcWgradArgs& a, int b, const int nb) {
    __shared__ float part[4][256];
    __shared__ float partb[4][16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, q = lane >> 4;
    const NetOff no = md.net[0];
    const int Do = md.Do, Da = md.Da;
    constexpr int T = H / 16;
    const int n2 = bc_wg_n2(H), n1 = bc_wg_n1(H, Do);
    if (b == nb - 1) {                                       // the update's mean loss: tiles in ascending order
        if (tid == 0) {
            float t = 0.0f;
            for (int i = 0; i < a.tiles; ++i) t += a.lossp[i];
            a.loss_out[0] = t / (float)a.B;
        }
        if (a.sigma_zero && tid < Da) a.G[no.sigma + tid] = 0.0f;
        return;
    }
    // job: Y[rows][ldy] (columns n0 .. n0 + 16, valid below nlim) x X[rows][ldx] (columns k0 .., valid below klim) -> W[n][k] at
    // wbase + n * ldw + k; bias sums of Y's columns at bbase + n (has_bias: the tiles of the first column block)
    const float *Y, *X = nullptr;
    int ldy, ldx = 0, n0, k0 = 0, nlim, klim = 0, wbase = 0, ldw = 0, bbase = 0;
    bool gather = false, bias_only = false, has_bias = false;
    if (b < n2) {
        n0 = 16 * (b / T); k0 = 16 * (b % T);
        Y = a.D2; ldy = H; X = a.A1; ldx = H; nlim = H; klim = H; wbase = no.W2; ldw = H; bbase = no.b2; has_bias = k0 == 0;
    } else if (b < n2 + n1) {
        b -= n2;
        const int kt = (Do + 15) / 16;
        n0 = 16 * (b / kt); k0 = 16 * (b % kt);
        Y = a.D1; ldy = H; X = a.obs; ldx = Do; gather = true; nlim = H; klim = Do; wbase = no.W1; ldw = Do; bbase = no.b1; has_bias = k0 == 0;
    } else if (b < n2 + n1 + T) {
        b -= n2 + n1;
        n0 = 0; k0 = 16 * b;
        Y = a.DO; ldy = FSRL_DOW; X = a.A2; ldx = H; nlim = no.out; klim = H; wbase = no.W3; ldw = H; bbase = no.b3; has_bias = k0 == 0;
    } else {
        n0 = 16; Y = a.DO; X = a.DO; ldy = FSRL_DOW; nlim = 16 + Da; bbase = no.sigma - 16; bias_only = true; has_bias = true;
    }
    const bool yon = n0 + li < nlim, xon = !bias_only && k0 + li < klim;
    const float* __restrict__ yp = Y + n0 + (yon ? li : 0);
    const float* __restrict__ xp = X + k0 + (xon ? li : 0);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f}, accb = {0.f, 0.f, 0.f, 0.f};
    // wave w takes the 4-row chunks w, w + 4, ...: rows_pad is a multiple of 16, so every wave runs rows_pad / 16 steps; rows past the
    // batch hold zeros in D1 / D2 / DO (their dout is zero) and finite activations
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
    const int nn = tid >> 4, kk = tid & 15;
    if (!bias_only && n0 + nn < nlim && k0 + kk < klim) {
        const float g = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
        const int i = wbase + (n0 + nn) * ldw + k0 + kk;
        a.G[i] = g;
        adam_element(a.P, a.M, a.V, i, a.P[i], g, 1.0f, 0.0f, a.one_minus_b1, a.beta2, a.one_minus_b2, a.step_size, a.bc2_sqrt, a.eps, md,
                     nullptr, 0.0f, 0.0f);
    }
    if (has_bias && tid < 16 && n0 + tid < nlim) {
        const float g = (partb[0][tid] + partb[1][tid]) + (partb[2][tid] + partb[3][tid]);
        const int i = bbase + n0 + tid;
        a.G[i] = g;
        adam_element(a.P, a.M, a.V, i, a.P[i], g, 1.0f, 0.0f, a.one_minus_b1, a.beta2, a.one_minus_b2, a.step_size, a.bc2_sqrt, a.eps, md,
                     nullptr, 0.0f, 0.0f);
    }
}
template <int H>
__global__ __launch_bounds__(256) void bc_wgrad_kernel(const ModelDesc md, const BcWgradArgs a) {
    bc_wgrad_body<H>(md, a, (int)blockIdx.x, (int)gridDim.x);
}
