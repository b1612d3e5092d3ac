// kernels_traj.hpp -- the device side of the trajectory archive (fsrl_traj_*, host_traj.inc): rows only ever MOVE here.
//   traj_stage_kernel   one launch per flushed staging window: the window's packed records -> the rows of the open-episode area the
//                       host assigned them (a scatter, record by record: the rows of one env are not adjacent in a window)
//   traj_move_kernel    one launch per commit batch / per compaction: a job table of row runs, contiguous at both ends, all seven
//                       columns of a run in the same launch
//   store_fill_kernel   one launch per fsrl_store_fill: a job table of row runs archive -> a context's store, contiguous at both
//                       ends; the action column goes through BasePolicy.map_action_inverse, the two flag columns become one byte
// HBM-bound copies: no LDS, grid-stride loops, 16-byte accesses where source and destination allow them.
#pragma once
#include "common.hpp"
#include "kernels_misc.hpp"

// the seven DSRL columns of `rows` rows (archive half, or a context's open-episode area)
struct TrajCols {
    float* obs;          // [rows][Do]
    float* obs_next;     // [rows][Do]
    float* act;          // [rows][Da]   the action the env received
    double* rew;         // [rows]
    double* cost;        // [rows]
    uint8_t* terminals;  // [rows]
    uint8_t* timeouts;   // [rows]
};
struct TrajJob { long long src, dst; int rows, pad; };     // = trajp::Job (traj_plan.hpp)

// Staging records (struct Staging: rew f64 | cost f64 | slot i32 | flags u32 | obs[Do] | obs_next[Do] | act[Da]) and, record for
// record, the tap's own: dst i32 (row of the open-episode area, or -1: not recorded) | env_act[Da].
__global__ void traj_stage_kernel(TrajCols open, const uint8_t* __restrict__ recs, const int rec, const uint8_t* __restrict__ taps,
                                  const int tap_rec, int k, int Do, int Da) {
    const int per = 2 * Do + Da + 1;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < k * per; e += gridDim.x * blockDim.x) {
        const int row = e / per, f = e - row * per;
        const uint8_t* t = taps + (size_t)row * tap_rec;
        const int d = *reinterpret_cast<const int*>(t);
        if (d < 0) continue;
        const size_t dst = (size_t)d;
        const uint8_t* r = recs + (size_t)row * rec;
        const float* x = reinterpret_cast<const float*>(r + 24);
        if (f < Do) open.obs[dst * Do + f] = x[f];
        else if (f < 2 * Do) open.obs_next[dst * Do + (f - Do)] = x[f];
        else if (f < 2 * Do + Da) open.act[dst * Da + (f - 2 * Do)] = reinterpret_cast<const float*>(t + 4)[f - 2 * Do];
        else {
            open.rew[dst] = *reinterpret_cast<const double*>(r);
            open.cost[dst] = *reinterpret_cast<const double*>(r + 8);
            const uint32_t fl = *reinterpret_cast<const uint32_t*>(r + 20);
            open.terminals[dst] = (uint8_t)(fl & 1);
            open.timeouts[dst] = (uint8_t)((fl >> 1) & 1);
        }
    }
}

// n bytes from s to d by the threads of one workgroup.  16 bytes per access over the part where both ends are 16-byte aligned (they
// are when s and d are congruent mod 16); the ragged head and tail, and runs whose ends are not congruent (obs_dim 5: rows of 20
// bytes), go in dwords; byte columns whose ends are not even dword-congruent go in bytes.
__device__ __forceinline__ void traj_copy_small(uint8_t* d, const uint8_t* s, size_t n) {
    if ((((uintptr_t)d | (uintptr_t)s | n) & 3) == 0) {
        for (size_t i = threadIdx.x; i < n / 4; i += blockDim.x)
            reinterpret_cast<uint32_t*>(d)[i] = reinterpret_cast<const uint32_t*>(s)[i];
    } else {
        for (size_t i = threadIdx.x; i < n; i += blockDim.x) d[i] = s[i];
    }
}
__device__ __forceinline__ void traj_copy_run(uint8_t* d, const uint8_t* s, size_t n) {
    if ((((uintptr_t)d ^ (uintptr_t)s) & 15) != 0 || n < 64) { traj_copy_small(d, s, n); return; }
    const size_t head = (16 - ((uintptr_t)d & 15)) & 15;      // < 16 <= n
    const size_t body = (n - head) / 16;
    traj_copy_small(d, s, head);
    const uint4* s4 = reinterpret_cast<const uint4*>(s + head);
    uint4* d4 = reinterpret_cast<uint4*>(d + head);
    for (size_t i = threadIdx.x; i < body; i += blockDim.x) d4[i] = s4[i];
    const size_t done = head + body * 16;
    traj_copy_small(d + done, s + done, n - done);
}

__global__ __launch_bounds__(256) void traj_move_kernel(TrajCols src, TrajCols dst, const TrajJob* __restrict__ jobs, int n_jobs,
                                                        int Do, int Da) {
    for (int j = blockIdx.x; j < n_jobs; j += gridDim.x) {
        const TrajJob jb = jobs[j];
        const size_t s = (size_t)jb.src, d = (size_t)jb.dst, n = (size_t)jb.rows;
        traj_copy_run((uint8_t*)(dst.obs + d * Do), (const uint8_t*)(src.obs + s * Do), n * Do * 4);
        traj_copy_run((uint8_t*)(dst.obs_next + d * Do), (const uint8_t*)(src.obs_next + s * Do), n * Do * 4);
        traj_copy_run((uint8_t*)(dst.act + d * Da), (const uint8_t*)(src.act + s * Da), n * Da * 4);
        traj_copy_run((uint8_t*)(dst.rew + d), (const uint8_t*)(src.rew + s), n * 8);
        traj_copy_run((uint8_t*)(dst.cost + d), (const uint8_t*)(src.cost + s), n * 8);
        traj_copy_run(dst.terminals + d, src.terminals + s, n);
        traj_copy_run(dst.timeouts + d, src.timeouts + s, n);
    }
}

// ---- fsrl_store_fill.  BasePolicy.map_action_inverse (base_policy.py:258-283) of one action element: the env's action back to the
// value a policy stores.  The rescale is the reference's float32 expression in its operation order, every step rounded on its own
// (the _rn intrinsics keep the compiler from contracting any two of them); `scale` is high - low with float32 eps added where it
// is below eps, prepared by the host.  tanh: the input is clamped to +-(1 - 2^-24) first (at +-1 the reference returns +-inf, and a
// recorded, saturated tanh action is exactly +-1); the two logarithms are taken in float64 and the result is rounded once.
__device__ __forceinline__ float traj_action_inverse(float a, bool scaled, float low, float scale, int bound_method) {
    if (scaled) a = __fsub_rn(__fdiv_rn(__fmul_rn(__fsub_rn(a, low), 2.0f), scale), 1.0f);
    if (bound_method == 2) {
        const float lim = 0.99999994f;      // 1 - 2^-24
        a = fminf(fmaxf(a, -lim), lim);
        a = (float)((log(1.0 + (double)a) - log(1.0 - (double)a)) * 0.5);
    }
    return a;
}

// One workgroup per job, grid-stride over the table.  obs / obs_next / rew / cost are plain copies under traj_copy_run's rule
// (16-byte accesses where both ends are congruent mod 16, dwords for the ragged parts and for rows such as obs_dim 5's 20 bytes);
// act is mapped element-wise; terminals / timeouts become the store's flags byte.  The host (store_fill_plan.hpp) guarantees that
// no slot appears in two jobs and that every run lies inside the archive and inside the store.  map = [low[Da] | scale[Da]], or
// null when actions are not rescaled.
__global__ __launch_bounds__(256) void store_fill_kernel(TrajCols src, StorePtrs dst, const TrajJob* __restrict__ jobs, int n_jobs,
                                                         int Do, int Da, int bound_method, const float* __restrict__ map) {
    for (int j = blockIdx.x; j < n_jobs; j += gridDim.x) {
        const TrajJob jb = jobs[j];
        const size_t s = (size_t)jb.src, d = (size_t)jb.dst, n = (size_t)jb.rows;
        traj_copy_run((uint8_t*)(dst.obs + d * Do), (const uint8_t*)(src.obs + s * Do), n * Do * 4);
        traj_copy_run((uint8_t*)(dst.obs_next + d * Do), (const uint8_t*)(src.obs_next + s * Do), n * Do * 4);
        traj_copy_run((uint8_t*)(dst.rew + d), (const uint8_t*)(src.rew + s), n * 8);
        traj_copy_run((uint8_t*)(dst.cost + d), (const uint8_t*)(src.cost + s), n * 8);
        const float* sa = src.act + s * Da;
        float* da = dst.act + d * Da;
        for (int i = threadIdx.x; i < (int)n * Da; i += blockDim.x) {
            const int k = i % Da;
            da[i] = traj_action_inverse(sa[i], map != nullptr, map ? map[k] : 0.0f, map ? map[Da + k] : 1.0f, bound_method);
        }
        for (int i = threadIdx.x; i < (int)n; i += blockDim.x)
            dst.flags[d + i] = (uint8_t)((src.terminals[s + i] ? 1 : 0) | (src.timeouts[s + i] ? 2 : 0));
    }
}
