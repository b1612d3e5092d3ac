// Cost of the gradient-norm exchange INSIDE the PPO weight-gradient launch (wg_grid(256, 3) = 244 blocks x 1024 threads, one per CU,
// ppo_wgrad_kernel's LDS footprint), against the kernel boundary it would replace (a dependent adam_clip_kernel-shaped launch,
// 197 x 256 threads).  Unlike gridsync.hip's barriers nothing here maintains a cache and nothing is read-modify-written:
//   publish : every block stores ONE {float value, uint32 epoch} word to its own slot, a 64-bit relaxed agent-scope atomic store
//   gather  : threads 0..nblocks-1 of every block poll one slot each (relaxed agent-scope atomic loads, s_sleep between polls)
//             until its tag is the epoch, then one __syncthreads()
// Two slot arrays alternate by epoch parity: a block can publish epoch e + 2 only after every block has published e + 1, which a
// block does only after it has read all of e, so a slot is never overwritten before its last reader is through.
// Slots sit on their own 128-byte lines (stride 16 words) or packed (stride 1).  Every poll loop is bounded by wall_clock64():
// past the limit the block counts a failure and leaves, and every later poller of its slot runs into the same limit and leaves too.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)
typedef unsigned long long u64;
#define WG_LDS_BYTES (1024 * 9 * 4 + 16 * 4)     // ppo_wgrad_body: red[1024 * 9] + wsum[16]
#define MAX_BLOCKS 1024

template <int MODE>   // 0: the loop alone (one __syncthreads per iteration), 1: publish + gather
__global__ __launch_bounds__(1024) void k(u64* slots, int stride, int iters, long long limit_ticks, unsigned* fails, unsigned* bad) {
    extern __shared__ float lds[];
    __shared__ int quit;
    const int tid = threadIdx.x, nb = gridDim.x;
    if (tid == 0) quit = 0;
    if (tid == 4095) slots[0] = (u64)lds[0];                       // never true: keeps the LDS allocation alive
    __syncthreads();
    unsigned wrong = 0;
    for (int it = 1; it <= iters; ++it) {
        if (MODE == 1) {
            u64* arr = slots + (size_t)(it & 1) * MAX_BLOCKS * stride;
            if (tid == 0) {
                const float val = (float)(blockIdx.x + it);
                __hip_atomic_store(arr + (size_t)blockIdx.x * stride, ((u64)(unsigned)it << 32) | __float_as_uint(val), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            }
            if (tid < nb) {
                const long long t0 = wall_clock64();
                u64 w;
                while (true) {
                    w = __hip_atomic_load(arr + (size_t)tid * stride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if ((unsigned)(w >> 32) == (unsigned)it) break;
                    if (wall_clock64() - t0 > limit_ticks) { quit = 1; break; }
                    __builtin_amdgcn_s_sleep(1);
                }
                if ((unsigned)(w >> 32) == (unsigned)it && __uint_as_float((unsigned)w) != (float)(tid + it)) ++wrong;
            }
        }
        __syncthreads();
        if (MODE == 1 && quit) break;                              // block-uniform: read after the barrier, written before it
    }
    if (MODE == 1 && tid == 0 && quit) atomicAdd(fails, 1u);
    if (wrong) atomicAdd(bad, wrong);
}
template <int NT>
__global__ __launch_bounds__(NT) void floor_kernel(int* sink) {
    extern __shared__ float floor_lds[];
    if (sink && threadIdx.x == 4095) sink[0] = (int)floor_lds[0];
}

int main(int argc, char** argv) {
    const int blocks = argc > 1 ? atoi(argv[1]) : 244;              // wg_grid(256, 3)
    const int adam_blocks = argc > 2 ? atoi(argv[2]) : 197;         // ceil(n_dev / (4 * 256)) of the headline model
    const long long limit_ticks = argc > 3 ? atoll(argv[3]) : 100000;   // wall_clock64 runs at 100 MHz: 1 ms
    if (blocks < 1 || blocks > MAX_BLOCKS) { printf("1..%d blocks\n", MAX_BLOCKS); return 1; }
    hipDeviceProp_t prop; CHECK(hipGetDeviceProperties(&prop, 0));
    if (blocks > prop.multiProcessorCount) { printf("%d blocks need %d CUs, the device has %d\n", blocks, blocks, prop.multiProcessorCount); return 1; }
    u64* slots; unsigned *fails, *bad;
    const size_t slot_bytes = (size_t)2 * MAX_BLOCKS * 16 * sizeof(u64);
    CHECK(hipMalloc(&slots, slot_bytes)); CHECK(hipMalloc(&fails, 4)); CHECK(hipMalloc(&bad, 4));
    CHECK(hipFuncSetAttribute((const void*)k<0>, hipFuncAttributeMaxDynamicSharedMemorySize, WG_LDS_BYTES));
    CHECK(hipFuncSetAttribute((const void*)k<1>, hipFuncAttributeMaxDynamicSharedMemorySize, WG_LDS_BYTES));
    CHECK(hipFuncSetAttribute((const void*)floor_kernel<1024>, hipFuncAttributeMaxDynamicSharedMemorySize, WG_LDS_BYTES));
    hipEvent_t e0, e1; CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    const int iters = 2000, reps = 5;
    printf("%s, %d CUs; poll limit %lld ticks of wall_clock64 (100 MHz)\n", prop.name, prop.multiProcessorCount, limit_ticks);
    // ---- the exchange, per iteration of one resident launch
    for (int stride : {16, 1}) {
        for (int rep = 0; rep < reps; ++rep) {
            float us[2];
            unsigned f = 0, b = 0;
            for (int mode = 0; mode < 2; ++mode) {
                CHECK(hipMemset(slots, 0, slot_bytes)); CHECK(hipMemset(fails, 0, 4)); CHECK(hipMemset(bad, 0, 4));
                CHECK(hipDeviceSynchronize());
                CHECK(hipEventRecord(e0, 0));
                if (mode == 0) hipLaunchKernelGGL(k<0>, dim3(blocks), dim3(1024), WG_LDS_BYTES, 0, slots, stride, iters, limit_ticks, fails, bad);
                else hipLaunchKernelGGL(k<1>, dim3(blocks), dim3(1024), WG_LDS_BYTES, 0, slots, stride, iters, limit_ticks, fails, bad);
                CHECK(hipEventRecord(e1, 0)); CHECK(hipEventSynchronize(e1)); CHECK(hipGetLastError());
                float ms; CHECK(hipEventElapsedTime(&ms, e0, e1));
                us[mode] = ms * 1000.f / iters;
                if (mode == 1) { CHECK(hipMemcpy(&f, fails, 4, hipMemcpyDeviceToHost)); CHECK(hipMemcpy(&b, bad, 4, hipMemcpyDeviceToHost)); }
            }
            printf("exchange %d blocks x 1024 thr, slots %s: loop alone %.3f us/iter | publish + gather %.3f (+%.3f) | timed-out blocks %u | wrong values %u\n",
                   blocks, stride == 16 ? "on 128-B lines" : "packed        ", us[0], us[1], us[1] - us[0], f, b);
        }
    }
    // ---- the boundary it replaces: dependent empty launches on one stream (fsrl_launch_floors' method)
    const int chain = 2000;
    for (int rep = 0; rep < reps; ++rep) {
        float us[3];
        for (int m = 0; m < 3; ++m) {      // 0: weight-gradient grid alone, 1: adam grid alone, 2: the pair
            for (int w = 0; w < 8; ++w) {
                hipLaunchKernelGGL(floor_kernel<1024>, dim3(blocks), dim3(1024), WG_LDS_BYTES, 0, (int*)nullptr);
                hipLaunchKernelGGL(floor_kernel<256>, dim3(adam_blocks), dim3(256), 0, 0, (int*)nullptr);
            }
            CHECK(hipDeviceSynchronize());
            CHECK(hipEventRecord(e0, 0));
            for (int i = 0; i < chain; ++i) {
                if (m != 1) hipLaunchKernelGGL(floor_kernel<1024>, dim3(blocks), dim3(1024), WG_LDS_BYTES, 0, (int*)nullptr);
                if (m != 0) hipLaunchKernelGGL(floor_kernel<256>, dim3(adam_blocks), dim3(256), 0, 0, (int*)nullptr);
            }
            CHECK(hipEventRecord(e1, 0)); CHECK(hipEventSynchronize(e1)); CHECK(hipGetLastError());
            float ms; CHECK(hipEventElapsedTime(&ms, e0, e1));
            us[m] = ms * 1000.f / chain;
        }
        printf("empty dependent launches: %d x 1024 thr %.3f us | %d x 256 thr %.3f us | the pair %.3f us (the second launch adds %.3f)\n",
               blocks, us[0], adam_blocks, us[1], us[2], us[2] - us[0]);
    }
    return 0;
}
