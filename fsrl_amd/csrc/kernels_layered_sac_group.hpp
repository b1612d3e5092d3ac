// kernels_layered_sac_group.hpp -- the layered SAC-Lagrangian / DDPG-Lagrangian update (host_sac.inc's layered branches) and the
// layered replay actor of the collector for a GROUP of contexts of one shape (host side: host_sac_group_layered.inc).  Every
// launch of the member's own update becomes one launch that carries all members, the member being one more grid coordinate; the
// bodies are the single-context ones (lin_body, lay_sac_actor_head_body, lay_sac_q_head_body, sac_sample_gather_block,
// sac_nstep_target), inlined.  lin_body gives every output element as one accumulator over ascending k whatever the launch
// shape, and the replay agents pass no squared-norm partials, so a member's grouped update is bit-identical to its own
// fsrl_sac_update at every group size and batch size.
// What changes per update -- whether the member still has updates to run, its Philox counter, its Adam step sizes, its row of
// the statistics ring -- is read from the member's SacGroupStep row (kernels_sac_group.hpp); everything else sits in device
// tables written once per grouped call.
#pragma once
#include "kernels_layered_group.hpp"
#include "kernels_layered_sac.hpp"     // (kernels_sac_group.hpp -- SacGroupStep -- comes before this file in fsrl_hip.hip)

// grid = (max column tiles, max row tiles, jobs of all members).  The jobs are complete (rows = the batch size of the call);
// workgroups of a member that sits this update out return at once.
template <int FORM, bool VEC, int NW>
__global__ __launch_bounds__(256 * NW) void lin_sac_group_kernel(const LinGroupJob* __restrict__ jobs, const SacGroupStep* __restrict__ steps) {
    const LinGroupJob gj = jobs[blockIdx.z];
    if (!steps[gj.member].active) return;
    lin_body<FORM, VEC, NW>(gj.j, blockIdx.y, nullptr, 0);
}

// grid = (tiles, members); heads[member]: the member's arguments of this launch of the update
__global__ __launch_bounds__(256) void lay_sac_actor_head_group_kernel(const LaySacActorArgs* __restrict__ heads,
                                                                      const SacGroupStep* __restrict__ steps) {
    if (!steps[blockIdx.y].active) return;
    lay_sac_actor_head_body(heads[blockIdx.y], (int)blockIdx.x);
}

// the CVPO actor head of a layered CVPO group (host_cvpo_group_layered.inc).  grid = (tiles, members).  The early return is
// uniform per workgroup, so the __syncthreads() of the body's MBWD branch stays legal.
__global__ __launch_bounds__(256) void lay_cvpo_actor_head_group_kernel(const LayCvpoActorArgs* __restrict__ heads,
                                                                       const SacGroupStep* __restrict__ steps) {
    if (steps[blockIdx.y].active == 0) return;
    lay_cvpo_actor_head_body(heads[blockIdx.y], (int)blockIdx.x);
}

// grid = (tiles, n_q, members)
__global__ __launch_bounds__(64) void lay_sac_q_head_group_kernel(const LaySacQArgs* __restrict__ heads, const SacGroupStep* __restrict__ steps) {
    if (!steps[blockIdx.z].active) return;
    lay_sac_q_head_body(heads[blockIdx.z], (int)blockIdx.x, (int)blockIdx.y);
}

// sample + gather of every member's update: its sample arguments with its Philox counter come from the step row.
// grid = (ceil(B / SG_ROWS), members)
__global__ __launch_bounds__(256) void sac_sample_gather_group_kernel(const SacGatherArgs* __restrict__ ga, const SacGroupStep* __restrict__ steps) {
    const SacGroupStep& st = steps[blockIdx.y];
    if (!st.active) return;
    sac_sample_gather_block(st.sa, ga[blockIdx.y], (int)blockIdx.x);
}

// the float64 n-step targets (sac_nstep_kernel per member).  grid = (ceil(B / 256), members), 256 threads
__global__ __launch_bounds__(256) void sac_nstep_group_kernel(const SacNstepArgs* __restrict__ na, const SacGroupStep* __restrict__ steps) {
    if (!steps[blockIdx.y].active) return;
    const SacNstepArgs& a = na[blockIdx.y];
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= a.B) return;
    a.Y[b] = sac_nstep_target(a, b, 0);
    a.Y[(size_t)a.B + b] = sac_nstep_target(a, b, 1);
}

// ---------------------------------------------------------------- lock-step collection: the tail of the members' actor forward
// grid = (tiles of the member with the most rows, members), 64 threads: thread (row = tid >> 2, column phase = tid & 3) copies
// the raw head row 16 blockIdx.x + row of member blockIdx.y (`out`: [member][cap][16], left there by lin_kernel<LIN_F> launches
// with one job per member) to raw [member][cap][cols] in pinned host memory.  The completion word of the (member, tile) goes out
// behind a system-scope fence of the wave that stored (one wave per workgroup).
struct LayRawGroupArgs {
    int rows[GACTOR_MAX_MEMBERS];
    const float* out; float* raw; unsigned* done;
    int cap, tiles_cap, cols;
    unsigned seq;
};
__global__ __launch_bounds__(64) void lay_raw_out_group_kernel(const LayRawGroupArgs a) {
    const int m = blockIdx.y, rows = a.rows[m];
    if ((int)blockIdx.x * 16 >= rows) return;
    const int r = blockIdx.x * 16 + (threadIdx.x >> 2);
    if (r < rows)
        for (int o = threadIdx.x & 3; o < a.cols; o += 4)
            a.raw[((size_t)m * a.cap + r) * a.cols + o] = a.out[((size_t)m * a.cap + r) * FSRL_MAX_ACT + o];
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(a.done + (size_t)m * a.tiles_cap + blockIdx.x, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
