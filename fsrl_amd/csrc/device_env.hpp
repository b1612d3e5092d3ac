// device_env.hpp -- environments as device functions (fsrl_devenv_*, include/fsrl_hip.h).
//
// A device env is a struct of static __device__ functions over one env's state row (DEVENV_STATE floats in device memory):
//     observe(P, state, obs)                                        obs[Do] of the state
//     reset  (P, state, rng, obs)                                   draws a start state, writes its observation
//     step   (P, state, env_act, rng, t, obs_next, rew, cost, terminated)
// One thread runs one env.  `t` is the number of steps the episode has taken so far; the time limit (truncation) is NOT the env's
// business: the kernels cut the episode (devcollect_plan.hpp dc_truncated).  obs_next is a row of its own -- an env may write it while
// it still reads its state.  The small kernels behind fsrl_devenv_reset / _step and the collect kernel (kernels_devcollect.hpp) are
// templated over the env type and inline the SAME functions, so a device env stepped from the host and one stepped inside the collect
// kernel compute the same bits.
//
// Arithmetic.  Every *, +, - and / below is rounded on its own (contraction is switched off in each function) and sqrt is the
// correctly rounded one: a float32 restatement in numpy computes the same bits wherever no transcendental is involved
// (tests/devenv_model.py).
//
// Random numbers.  One Philox4x32-10 block per
//     counter = (env id, ordinal, t, stream << 28 | block),   key = seed * 0x9E3779B97F4A7C15 + 0x243F6A8885A308D3
// where `ordinal` counts the resets of this env since creation / fsrl_devenv_seed -- the reset that STARTS an episode has the
// ordinal the episode's step and action draws use, too -- and t is the step inside the episode (0 for the reset's own draws).
// A block gives four uniforms (word >> 8, 24 bits) or four normals (kernels_sample.hpp box_muller on words (0, 1) and (2, 3));
// dimension d of a stream is element d & 3 of block d >> 2.  Nothing else enters a draw: not the launch, not n_episode, not the
// other envs.
//
// Adding an env: write the struct, give it a FSRL_DEVENV_* value in include/fsrl_hip.h, add it to devenv_dispatch and
// devenv_state_dim below and to the shape checks of fsrl_devenv_create (host_devcollect.inc), rebuild (INTEGRATION.md "Device
// environments").
#pragma once
#include "kernels_sample.hpp"
#include "devcollect_plan.hpp"

#define DEVENV_STATE 64                 // floats of one env's state row
#define DEVENV_STREAM_RESET 0u
#define DEVENV_STREAM_ACT 1u            // the policy's action noise
#define DEVENV_STREAM_STEP 2u

struct DevEnvParams {
    int kind, env_num, Do, Da, max_steps;
    float p[8];
    const float* A;     // LINEAR: [Do][Do]
    const float* B;     // LINEAR: [Da][Do]
};
struct DevEnvArrays {
    float* state;       // [env_num][DEVENV_STATE]
    float* obs;         // [env_num][Do]   the observation the next action is for
    float* nxt;         // [env_num][Do]   the last step's obs_next
    int32_t* t;         // [env_num]       steps taken in the running episode
    int64_t* ordinal;   // [env_num]       resets so far
};
struct DevRng { uint32_t k0, k1, env, ord; };

__device__ __forceinline__ void devenv_block(const DevRng& g, const uint32_t t, const uint32_t stream, const uint32_t blk, uint32_t (&r)[4]) {
    r[0] = g.env; r[1] = g.ord; r[2] = t; r[3] = (stream << 28) | blk;
    philox4x32_10(r, g.k0, g.k1);
}
// N(0, 1), dimension d of `stream` at step t
__device__ __forceinline__ float devenv_normal(const DevRng& g, const uint32_t t, const uint32_t stream, const int d) {
    uint32_t r[4];
    devenv_block(g, t, stream, (uint32_t)d >> 2, r);
    float n0, n1;
    const bool hi = (d & 2) != 0;
    box_muller(hi ? r[2] : r[0], hi ? r[3] : r[1], n0, n1);
    return (d & 1) ? n1 : n0;
}
// U[0, 1) on the 2^-24 grid
__device__ __forceinline__ float devenv_uniform(const DevRng& g, const uint32_t t, const uint32_t stream, const int d) {
    uint32_t r[4];
    devenv_block(g, t, stream, (uint32_t)d >> 2, r);
    const uint32_t w = (d & 2) ? ((d & 1) ? r[3] : r[2]) : ((d & 1) ? r[1] : r[0]);
    return (float)(w >> 8) * (1.0f / 16777216.0f);
}

// BasePolicy.map_action (base_policy.py:226-256) of one action component, as map_env_action does it on the host
__device__ __forceinline__ float devenv_map_action(float a, const int bound_method, const bool scaled, const float lo, const float hi) {
#pragma clang fp contract(off)
    if (bound_method == 1) a = fminf(fmaxf(a, -1.0f), 1.0f);
    else if (bound_method == 2) a = tanhf(a);
    if (scaled) a = lo + (hi - lo) * (a + 1.0f) / 2.0f;
    return a;
}

// ---------------------------------------------------------------- FSRL_DEVENV_POINT_CIRCLE: fsrl_amd/env/toy.py in float32
// state = (pos x, pos y, vel x, vel y); p = (radius, x_lim, dt); obs 6, act 2
struct DevEnvPointCircle {
    static constexpr int STATE = 4;
    __device__ static __forceinline__ void observe(const DevEnvParams& P, const float* s, float* obs) {
#pragma clang fp contract(off)
        const float px = s[0], py = s[1];
        const float rn = sqrtf(px * px + py * py);
        obs[0] = px; obs[1] = py; obs[2] = s[2]; obs[3] = s[3];
        obs[4] = rn - P.p[0];
        obs[5] = P.p[1] - fabsf(px);
    }
    __device__ static __forceinline__ void reset(const DevEnvParams& P, float* s, const DevRng& g, float* obs) {
#pragma clang fp contract(off)
        s[0] = devenv_uniform(g, 0u, DEVENV_STREAM_RESET, 0) - 0.5f;
        s[1] = devenv_uniform(g, 0u, DEVENV_STREAM_RESET, 1) - 0.5f;
        s[2] = 0.0f; s[3] = 0.0f;
        observe(P, s, obs);
    }
    __device__ static __forceinline__ void step(const DevEnvParams& P, float* s, const float* act, const DevRng& g, const uint32_t t,
                                                float* obs_next, double& rew, double& cost, bool& terminated) {
#pragma clang fp contract(off)
        const float radius = P.p[0], x_lim = P.p[1], dt = P.p[2];
        const float a0 = fminf(fmaxf(act[0], -1.0f), 1.0f), a1 = fminf(fmaxf(act[1], -1.0f), 1.0f);
        const float vx = 0.9f * s[2] + dt * a0, vy = 0.9f * s[3] + dt * a1;
        const float px = s[0] + dt * vx, py = s[1] + dt * vy;
        s[0] = px; s[1] = py; s[2] = vx; s[3] = vy;
        const float r = sqrtf(px * px + py * py) + 1e-8f;
        const float d = r - radius;
        rew = (double)((-py * vx + px * vy) / r / (1.0f + fabsf(d)));
        cost = fabsf(px) > x_lim ? 1.0 : 0.0;
        terminated = r > 4.0f * radius;
        observe(P, s, obs_next);
    }
};

// ---------------------------------------------------------------- FSRL_DEVENV_LINEAR: SyntheticSafetyVectorEnv's dynamics
// state = obs; s' = s @ A + act @ B + 0.05 N(0, 1), both sums in ascending index; p = (cost_threshold)
struct DevEnvLinear {
    static constexpr int STATE = DEVENV_STATE;
    __device__ static __forceinline__ void observe(const DevEnvParams& P, const float* s, float* obs) {
#pragma unroll 1
        for (int j = 0; j < P.Do; ++j) obs[j] = s[j];
    }
    __device__ static __forceinline__ void reset(const DevEnvParams& P, float* s, const DevRng& g, float* obs) {
#pragma unroll 1
        for (int j = 0; j < P.Do; ++j) s[j] = devenv_normal(g, 0u, DEVENV_STREAM_RESET, j);
        observe(P, s, obs);
    }
    __device__ static __forceinline__ void step(const DevEnvParams& P, float* s, const float* act, const DevRng& g, const uint32_t t,
                                                float* obs_next, double& rew, double& cost, bool& terminated) {
#pragma clang fp contract(off)
        const int Do = P.Do, Da = P.Da;
#pragma unroll 1
        for (int j = 0; j < Do; ++j) {
            float sa = 0.0f, sb = 0.0f;
#pragma unroll 1
            for (int i = 0; i < Do; ++i) sa = sa + s[i] * P.A[i * Do + j];
#pragma unroll 1
            for (int k = 0; k < Da; ++k) sb = sb + act[k] * P.B[k * Do + j];
            obs_next[j] = (sa + sb) + 0.05f * devenv_normal(g, t, DEVENV_STREAM_STEP, j);
        }
        float a2 = 0.0f;
#pragma unroll 1
        for (int k = 0; k < Da; ++k) a2 = a2 + act[k] * act[k];
#pragma unroll 1
        for (int j = 0; j < Do; ++j) s[j] = obs_next[j];
        rew = (double)(s[0] * act[0] - 0.1f * a2) + 0.5;
        cost = fabsf(s[1]) > P.p[0] ? 1.0 : 0.0;
        terminated = false;
    }
};

// f(Env()) for the env type of `kind`; false: no such kind
template <class F>
static inline bool devenv_dispatch(const int kind, F&& f) {
    switch (kind) {
        case FSRL_DEVENV_POINT_CIRCLE: f(DevEnvPointCircle()); return true;
        case FSRL_DEVENV_LINEAR: f(DevEnvLinear()); return true;
    }
    return false;
}
static inline int devenv_state_dim(const int kind, const int Do) { return kind == FSRL_DEVENV_POINT_CIRCLE ? DevEnvPointCircle::STATE : Do; }

// ---------------------------------------------------------------- the env as a vector env: reset / step / observe of listed envs
// One workgroup of DC_MAX_ENVS threads, a thread per listed env.  ids / act and the outputs are pinned host memory.
struct DevEnvIo {
    const int32_t* ids;     // [n] or NULL = envs 0 .. n - 1
    const float* act;       // [n][Da]
    float* obs;             // [n][Do]
    double* rew; double* cost;
    uint32_t* flags;        // bit 0 terminated, bit 1 truncated
    int n;
};
template <class Env>
__global__ __launch_bounds__(DC_MAX_ENVS) void devenv_reset_kernel(const DevEnvParams P, const DevEnvArrays ea, const DevEnvIo io,
                                                                    const uint32_t k0, const uint32_t k1) {
    const int p = threadIdx.x;
    if (p >= io.n) return;
    const int e = io.ids ? io.ids[p] : p;
    const DevRng g{k0, k1, (uint32_t)e, (uint32_t)ea.ordinal[e]};
    Env::reset(P, ea.state + (size_t)e * DEVENV_STATE, g, ea.obs + (size_t)e * P.Do);
    ea.t[e] = 0;
    ea.ordinal[e] += 1;
    if (io.obs)
        for (int j = 0; j < P.Do; ++j) io.obs[(size_t)p * P.Do + j] = ea.obs[(size_t)e * P.Do + j];
}
template <class Env>
__global__ __launch_bounds__(DC_MAX_ENVS) void devenv_step_kernel(const DevEnvParams P, const DevEnvArrays ea, const DevEnvIo io,
                                                                   const uint32_t k0, const uint32_t k1) {
    const int p = threadIdx.x;
    if (p >= io.n) return;
    const int e = io.ids ? io.ids[p] : p;
    const DevRng g{k0, k1, (uint32_t)e, (uint32_t)(ea.ordinal[e] - 1)};
    const int32_t t = ea.t[e];
    float act[FSRL_MAX_ACT];
    for (int k = 0; k < P.Da; ++k) act[k] = io.act[(size_t)p * P.Da + k];
    double rew, cost;
    bool term;
    float* nxt = ea.nxt + (size_t)e * P.Do;
    Env::step(P, ea.state + (size_t)e * DEVENV_STATE, act, g, (uint32_t)t, nxt, rew, cost, term);
    ea.t[e] = t + 1;
    for (int j = 0; j < P.Do; ++j) { const float v = nxt[j]; ea.obs[(size_t)e * P.Do + j] = v; io.obs[(size_t)p * P.Do + j] = v; }
    io.rew[p] = rew; io.cost[p] = cost;
    io.flags[p] = dc_flags(term, dc_truncated(t + 1, P.max_steps));
}
// fsrl_devenv_set_state: the observations of injected states
template <class Env>
__global__ __launch_bounds__(DC_MAX_ENVS) void devenv_observe_kernel(const DevEnvParams P, const DevEnvArrays ea) {
    const int e = threadIdx.x;
    if (e < P.env_num) Env::observe(P, ea.state + (size_t)e * DEVENV_STATE, ea.obs + (size_t)e * P.Do);
}
