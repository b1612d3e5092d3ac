// kernels_devcollect_layered.hpp -- whole collects on the device for LAYERED contexts (fsrl_collect_device_layered,
// fsrl_evaluate_device_layered): the loop of kernels_devcollect.hpp around an actor of any depth and width.
//
// lay_collect_kernel<Env, HEAD, STORE>: grid k, workgroup b runs member b's whole collect, as collect_device_group_kernel does.  A
// layered actor cannot keep its weights in registers; the workgroup (LAYC_NT threads, 16 waves) streams them from L2 every vector
// step instead and keeps the loop on the device.  Phases 2 - 5, the head arithmetic and the DcState hand-over are the functions of
// kernels_devcollect.hpp; phase 1 is this file's:
//   0. all threads: the live rows' observations -> the workspace, one row of `ld` floats per live position
//   1. layer by layer, Z_l = relu(Z_{l-1} W_l^T + b_l), over ALL live rows at once (at most 64 = four 16-row tiles): the
//      (row tile, column tile) jobs of a layer go round the waves, a barrier between layers; activations ping-pong between the two
//      halves of the workspace (2 x 64 x ld floats of device memory the env owns: L2-resident, one code path for every shape up to
//      FSRL_MAX_WIDTH x FSRL_MAX_HIDDEN; LDS holds the head row only); the head's raw row goes to LDS and through dc_head.
//      Staging a layer's input through LDS (slabs of 256 k, a weight fragment shared by a wave's row tiles, 8 waves) was built and
//      MEASURED: 1.37 x at 256x256x256 with 64 envs, 0.94 x with 20, 0.71 - 0.77 x at 64x48x32 -- two more barriers and a staging
//      round trip per layer cost the small shapes more than the saved traffic gives the large one back.  Not kept.
// Bits.  Every output element is accumulated in ONE accumulator by the MFMA sequence of lin_body<LIN_F> (kernels_layered.hpp):
// sub-chunks of 16 k, issued while their first k < K; four v_mfma_f32_16x16x4_f32 inside each, s = 0..3, lane (i, q) feeding
// k = 16 kc + 4 q + s, zeros past K; then + bias, then relu on the hidden layers.  So a deterministic layered device collect computes
// the actions fsrl_collect_step computes on the same context, bit for bit.
// Loads follow lin_body's rule: straight-line (64 k of both operands in flight before the first MFMA of the chunk), addresses clamped
// into the row, zero-fill by select.  Workspace rows are 16-byte aligned by construction (ld is a multiple of 4): the A operand is
// always a dwordx4 load.  A weight row is 16-byte aligned when 4 | K (tensors start on 256 bytes); otherwise four dword loads.
// The workgroups share nothing and wait on nothing but their own barriers; a finished member breaks at the loop's first test.
#pragma once
#include "kernels_devcollect.hpp"
#include "kernels_layered.hpp"

#define LAYC_NT 1024
#define LAYC_NW (LAYC_NT / 64)

// one member's row of the table (device memory): next to its DevCollectArgs, whose actor this is and where its activations go
struct LayCollectMember {
    const float* P;             // on-policy: the context's parameters; replay: SacState::PA
    const DevCollectArgs* a;
    float* ws;                  // [2][DC_MAX_ENVS][ld]
    int ld;                     // >= round_up(max(widest hidden layer, obs_dim), 4), a multiple of 4
    int unbounded;              // on-policy: the mean is the head itself
    LayNet net;                 // the actor: net.l[0 .. nl - 2] hidden layers, net.l[nl - 1] the head; net.sigma: sigma_param (on-policy)
};
struct LayCollectTable { LayCollectMember m[FSRL_MAX_GROUP]; };

// one 16 x 16 output tile: lane (li, q) holds row `arow` of A and row `wrow` of W (both k-minor); returns acc[r] = C[4 q + r][li]
__device__ __forceinline__ f32x4 layc_tile(const float* arow, const float* wrow, const int K, const bool vecb, const int q) {
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    const int ka = ((K + 3) & ~3) - 4;          // the last dwordx4 of an A row that holds a k < K
    for (int k0 = 0; k0 < K; k0 += 64) {
        f32x4 av[4], bv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + 16 * u + 4 * q;
            av[u] = *reinterpret_cast<const f32x4*>(arow + min(k, ka));
            if (vecb) {
                bv[u] = *reinterpret_cast<const f32x4*>(wrow + min(k, K - 4));
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) bv[u][e] = wrow[min(k + e, K - 1)];
            }
        }
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
            if (k0 + 16 * u < K) {              // uniform; the rest of the chunk is zeros
#pragma unroll
                for (int s = 0; s < 4; ++s) acc = mfma_16x16x4(av[u][s], bv[u][s], acc);
            }
        }
    }
    return acc;
}

template <class Env, int HEAD, bool STORE>
__global__ __launch_bounds__(LAYC_NT) void lay_collect_kernel(const LayCollectTable* __restrict__ tab) {
    const int b = __builtin_amdgcn_readfirstlane((int)blockIdx.x);
    const LayCollectMember& mb = *dc_uniform_ptr<4>(&tab->m[b]);
    const float* P = dc_uniform_ptr<1>(mb.P);
    const DevCollectArgs& a = *dc_uniform_ptr<4>(mb.a);
    float* ws = const_cast<float*>(dc_uniform_ptr<1>((const float*)mb.ws));
    __shared__ DevCollectSmem sh;
    __shared__ float raw[DC_MAX_ENVS * FSRL_MAX_ACT];          // the head's raw rows
    const int tid = threadIdx.x;
    const int Do = a.ep.Do, Da = a.ep.Da, ld = mb.ld, nl = mb.net.nl;
    const unsigned magic_do = div_magic(Do);
    dc_state_load<STORE>(a, sh, tid);
    const int n_episode = a.state->n_episode;
    int step = 0, log_rows = 0;
    for (; step < a.max_steps; ++step) {
        __syncthreads();
        if (__builtin_amdgcn_readfirstlane(sh.finished)) break;
        const int n_live = __builtin_amdgcn_readfirstlane(sh.n_live);      // workgroup-uniform: scalar registers
        int lt = threadIdx.x;
        asm volatile("" : "+v"(lt));           // this step's thread id, opaque (kernels_devcollect.hpp, Registers)
        // ---- 0. the live rows' observations, in position order, into the half of the workspace layer 0 reads
        for (int x = lt; x < n_live * Do; x += LAYC_NT) {
            const int p = div_by_magic((unsigned)x, magic_do), k = x - p * Do;
            ws[(size_t)(DC_MAX_ENVS + p) * ld + k] = a.ea.obs[(size_t)sh.live[p] * Do + k];
        }
        __syncthreads();
        // ---- 1. the actor, layer by layer; layer l reads half (l + 1) & 1 and writes half l & 1
        {
            const int wave = __builtin_amdgcn_readfirstlane(lt >> 6), lane = lt & 63, li = lane & 15, q = lane >> 4;
            const int n_rt = (n_live + 15) >> 4;
            for (int l = 0; l < nl; ++l) {
                const LayLayer ll = mb.net.l[l];
                const int K = ll.in, N = ll.out;
                const float* in = ws + (size_t)((l + 1) & 1) * DC_MAX_ENVS * ld;
                float* out = ws + (size_t)(l & 1) * DC_MAX_ENVS * ld;
                const bool head = l == nl - 1, vecb = (K & 3) == 0;
                const int jobs = n_rt * ((N + 15) >> 4);
                for (int j = wave; j < jobs; j += LAYC_NW) {
                    // j = ct * n_rt + rt: the waves of one round share a column tile's weights
                    const int ct = n_rt == 1 ? j : n_rt == 2 ? j >> 1 : n_rt == 4 ? j >> 2 : (int)(((unsigned)j * 43691u) >> 17);
                    const int rt = j - ct * n_rt;
                    const float* arow = in + (size_t)min(16 * rt + li, n_live - 1) * ld;
                    const float* wrow = P + ll.W + (size_t)min(16 * ct + li, N - 1) * K;
                    const f32x4 acc = layc_tile(arow, wrow, K, vecb, q);
                    const int n = 16 * ct + li;
                    if (n < N) {
                        const float bias = P[ll.b + n];
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int m = 16 * rt + 4 * q + r;
                            if (m < n_live) {
                                float v = acc[r] + bias;
                                if (head) raw[m * FSRL_MAX_ACT + n] = v;
                                else out[(size_t)m * ld + n] = fmaxf(v, 0.0f);
                            }
                        }
                    }
                }
                __syncthreads();
            }
        }
        for (int x = lt; x < n_live * Da; x += LAYC_NT) {
            const int p = div_by_magic((unsigned)x, a.magic_da), d = x - p * Da;
            dc_head<HEAD>(a, sh, &raw[p * FSRL_MAX_ACT], P + mb.net.sigma, mb.unbounded, Da, p, d);
        }
        __syncthreads();
        // ---- 2. env step, scalars of the row, log
        dc_env_step<Env, HEAD, STORE>(a, sh, lt, n_live, log_rows, Do);
        __syncthreads();
        if constexpr (STORE) {
            // ---- 3. the rows' vectors into the store
            dc_store_rows(a, sh, lt, LAYC_NT, n_live, Do, Da);
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
