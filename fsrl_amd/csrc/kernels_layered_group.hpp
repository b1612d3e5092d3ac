// kernels_layered_group.hpp -- the layered PPO-Lagrangian minibatch step (kernels_layered.hpp) for a GROUP of contexts of one
// shape: every launch carries all members, so a step stays 2 L + 5 launches whatever the number of members.  The bodies are the
// single-context ones (lin_body, lay_ppo_head_body, ppo_stats_finalize, adam_clip_body), inlined: every output element is one
// accumulator over ascending k whatever the launch shape, and the one launch-shape-dependent sum -- a workgroup's share of the
// squared gradient norm, reduced over its NW column groups -- is kept by launching the weight side with the NW a member's own
// launch would have.  A member's grouped update is therefore bit-identical to its own fsrl_ppo_update.
// What changes per step (rows, the minibatch's offset in the pass-ordered batch) is read from the member's GroupStep row, as the
// fused group kernels do; the job tables are uploaded once per grouped update.
#pragma once
#include "kernels_layered.hpp"

#define LGJ_A_OBS 1     // operand A is "the minibatch's observation rows": A = the member's obs_p + mb_start * lda
#define LGJ_B_OBS 2     // ... operand B: B = obs_p + mb_start * ldb
struct LinGroupJob {
    LinJob j;           // the job with rows (M of LIN_F / LIN_X, K of LIN_W) left open: they are the step's mb_size
    int member;         // row of the member and step tables
    int first;          // index of the member's first job in this launch's table (squared-norm slots count from there)
    int flags;          // LGJ_*
    int pad;
    float* gsq;         // LIN_W: the member's own squared-norm partials, slot order of its own launch
};

// grid = (max column tiles, max row tiles, jobs of all members); the workgroup's job is read from device memory (uniform: scalar
// loads), then the member's step row.  Workgroups of a member that sits this step out return at once.
template <int FORM, bool VEC, int NW>
__global__ __launch_bounds__(256 * NW) void lin_group_kernel(const LinGroupJob* __restrict__ jobs, const GroupAgent* __restrict__ tab,
                                                            const GroupStep* __restrict__ steps) {
    const LinGroupJob gj = jobs[blockIdx.z];
    const int mb_size = steps[gj.member].mb_size, mb_start = steps[gj.member].mb_start;
    if (!steps[gj.member].active) return;
    LinJob jb = gj.j;
    if (FORM == LIN_W) jb.K = mb_size; else jb.M = mb_size;
    if (gj.flags & LGJ_A_OBS) jb.A = tab[gj.member].bp.obs_p + (size_t)mb_start * jb.lda;
    if (gj.flags & LGJ_B_OBS) jb.B = tab[gj.member].bp.obs_p + (size_t)mb_start * jb.ldb;
    lin_body<FORM, VEC, NW>(jb, blockIdx.y, FORM == LIN_W ? gj.gsq : nullptr,
                            ((blockIdx.z - gj.first) * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x);
}

// grid = (tiles of the largest minibatch of the step, n_nets, members); heads[member]: that member's buffers (kernels_layered.hpp)
__global__ __launch_bounds__(256) void lay_ppo_head_group_kernel(const LayHeadArgs* __restrict__ heads, const GroupAgent* __restrict__ tab,
                                                                const GroupStep* __restrict__ steps, const PpoStepArgs base) {
    const GroupStep st = steps[blockIdx.z];
    if (!st.active || (int)blockIdx.x * 16 >= st.mb_size) return;       // the member's own tile count
    const PpoStepArgs sa = group_step_args(base, tab[blockIdx.z], st);
    lay_ppo_head_body(heads[blockIdx.z], sa, blockIdx.x, blockIdx.y);
}

// the logged row of every member's step (ppo_stats_kernel per member): grid = members, 64 threads
__global__ __launch_bounds__(64) void ppo_stats_group_kernel(const ModelDesc md, const GroupAgent* __restrict__ tab,
                                                            const GroupStep* __restrict__ steps, const PpoStepArgs base) {
    const GroupStep st = steps[blockIdx.x];
    if (!st.active) return;
    const GroupAgent& a = tab[blockIdx.x];
    const PpoStepArgs sa = group_step_args(base, a, st);
    ppo_stats_finalize(md, a.wp, sa, (st.mb_size + 15) >> 4, (int)threadIdx.x);
}

// ---------------------------------------------------------------- lock-step collection: the tail of the members' actor forward
// grid = (tiles of the member with the most rows, members), 64 threads: lane r < 16 finishes row 16 blockIdx.x + r of member
// blockIdx.y from its head outputs (`out`: [member][cap][16], left there by lin_kernel<LIN_F> launches with one job per member)
// -> mu [member][cap][Da] and the member's sigma_param row [member][16], both in pinned host memory.  The completion word of the
// (member, tile) goes out behind a system-scope fence of the wave that stored (one wave per workgroup).
struct LayInferGroupArgs {
    const float* P[GACTOR_MAX_MEMBERS];
    int rows[GACTOR_MAX_MEMBERS];
    const float* out; float* mu; float* sp; unsigned* done;
    int cap, tiles_cap;         // rows / completion words reserved per member
    int sigma, Da, unbounded;
    float max_action;
    unsigned seq;
};
__global__ __launch_bounds__(64) void lay_infer_out_group_kernel(const LayInferGroupArgs a) {
    const int m = blockIdx.y, tid = threadIdx.x, rows = a.rows[m];
    if ((int)blockIdx.x * 16 >= rows) return;
    const float* P = a.P[m];
    const int r = blockIdx.x * 16 + tid;
    if (blockIdx.x == 0 && tid < a.Da) a.sp[(size_t)m * FSRL_MAX_ACT + tid] = P[a.sigma + tid];
    if (tid < 16 && r < rows) {
        const float* o = a.out + ((size_t)m * a.cap + r) * FSRL_MAX_ACT;
        for (int d = 0; d < a.Da; ++d) {
            const float x = o[d];
            a.mu[((size_t)m * a.cap + r) * a.Da + d] = a.unbounded ? x : a.max_action * tanhf(x);
        }
    }
    __threadfence_system();
    __syncthreads();
    if (tid == 0) __hip_atomic_store(a.done + (size_t)m * a.tiles_cap + blockIdx.x, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
