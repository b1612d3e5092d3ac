// kernels_per.hpp -- prioritised experience replay next to the replay store: a float64 sum tree in HBM (tianshou 0.5
// PrioritizedReplayBuffer / SegmentTree restated; the reference reaches them through critics_loss's batch.weight, sac_lag.py:189-201,
// 263, ddpg_lag.py:170-179, 218, and post_process_fn's buffer.update_weight, base_policy.py:326-330).
//   tree[2 * bound], bound = the next power of two at or above the slot count; leaf of global slot s = tree[bound + s] = prio ** alpha,
//   every internal node exactly left + right (one IEEE add), so the tree is a pure function of its leaves; tree[0] is unused.
//   sc[0] = max_prio, sc[1] = min_prio (both raw priorities, 1.0 after a reset), sc[2] = the root as of the last repair.
// Every kernel that repairs ancestors is ONE workgroup: level by level with __syncthreads() between levels.  A parent is
// recomputed from its two children, which is idempotent, so threads that share an ancestor need no atomics; nothing here waits
// across workgroups.
#pragma once
#include "kernels_sample.hpp"
#include "kernels_traj.hpp"

#define PER_THREADS 1024
#define PER_F32_EPS 1.1920928955078125e-07        // np.finfo(np.float32).eps: PrioritizedReplayBuffer.__eps

struct PerDev {
    double* tree;        // [2 * bound]
    double* sc;          // [3] max_prio, min_prio, total
    int* stamp;          // [slots] the batch position that writes a slot (duplicates: the highest wins)
    int bound, slots;
    double alpha;
};

// recompute the ancestors of the leaves slot_of(i), i in [0, n), by all threads of the workgroup (slot_of < 0: none); sc[2] = root
template <class SlotOf>
__device__ __forceinline__ void per_repair(const PerDev& p, const int n, SlotOf slot_of) {
    for (int shift = 1; (p.bound >> shift) >= 1; ++shift) {
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const int s = slot_of(i);
            if (s < 0) continue;
            const int node = (p.bound + s) >> shift;
            p.tree[node] = p.tree[2 * node] + p.tree[2 * node + 1];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) p.sc[2] = p.tree[1];
}

// an empty tree: PrioritizedReplayBuffer.__init__ (fsrl_store_reset, fsrl_store_configure)
__global__ __launch_bounds__(256) void per_reset_kernel(const PerDev p) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < 2 * p.bound; i += gridDim.x * blockDim.x) p.tree[i] = 0.0;
    if (blockIdx.x == 0 && threadIdx.x == 0) { p.sc[0] = 1.0; p.sc[1] = 1.0; p.sc[2] = 0.0; }
}

// every internal node from the leaves (fsrl_per_enable, fsrl_store_fill, a training state coming in)
__global__ __launch_bounds__(PER_THREADS) void per_rebuild_kernel(const PerDev p) {
    for (int lvl = p.bound >> 1; lvl >= 1; lvl >>= 1) {
        for (int node = lvl + threadIdx.x; node < 2 * lvl; node += blockDim.x) p.tree[node] = p.tree[2 * node] + p.tree[2 * node + 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) p.sc[2] = p.tree[1];
}

// PrioritizedReplayBuffer.add behind store_scatter_kernel: the k staged records' slots (byte 16 of a record) get max_prio ** alpha
__global__ __launch_bounds__(PER_THREADS) void per_ingest_kernel(const PerDev p, const uint8_t* __restrict__ recs, const int rec, const int k) {
    const double v = pow(p.sc[0], p.alpha);
    auto slot_of = [&](int i) {
        const int s = *reinterpret_cast<const int*>(recs + (size_t)i * rec + 16);
        return (s >= 0 && s < p.slots) ? s : -1;
    };
    for (int i = threadIdx.x; i < k; i += blockDim.x) {
        const int s = slot_of(i);
        if (s >= 0) p.tree[p.bound + s] = v;
    }
    __syncthreads();
    per_repair(p, k, slot_of);
}

// ... behind collect_device_group_kernel (replay heads): the launch wrote *n_rows rows (DcState::log_rows, at most cap) into the store
// itself and left their slots in `slots`; the same leaves and the same repair as per_ingest_kernel's
__global__ __launch_bounds__(PER_THREADS) void per_slots_kernel(const PerDev p, const int32_t* __restrict__ slots,
                                                                const int32_t* __restrict__ n_rows, const int cap) {
    const double v = pow(p.sc[0], p.alpha);
    const int k = min(max(*n_rows, 0), cap);
    auto slot_of = [&](int i) {
        const int s = slots[i];
        return (s >= 0 && s < p.slots) ? s : -1;
    };
    for (int i = threadIdx.x; i < k; i += blockDim.x) {
        const int s = slot_of(i);
        if (s >= 0) p.tree[p.bound + s] = v;
    }
    __syncthreads();
    per_repair(p, k, slot_of);
}

// ... behind store_fill_kernel: the leaves of every job's destination run (per_rebuild_kernel follows)
__global__ __launch_bounds__(256) void per_fill_kernel(const PerDev p, const TrajJob* __restrict__ jobs, const int n_jobs) {
    const double v = pow(p.sc[0], p.alpha);
    for (int j = blockIdx.x; j < n_jobs; j += gridDim.x) {
        const TrajJob jb = jobs[j];
        for (int i = threadIdx.x; i < jb.rows; i += blockDim.x) {
            const long long s = jb.dst + i;
            if (s >= 0 && s < p.slots) p.tree[p.bound + s] = v;
        }
    }
}

// maximum / minimum over the workgroup's threads, the same value in every thread (exact whatever the order)
template <bool MAX>
__device__ __forceinline__ double per_block_extreme(double v, double* red) {
    __syncthreads();                    // red may still be read from the last call
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = blockDim.x >> 1; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const double o = red[threadIdx.x + s];
            red[threadIdx.x] = MAX ? fmax(red[threadIdx.x], o) : fmin(red[threadIdx.x], o);
        }
        __syncthreads();
    }
    return red[0];
}

// ---- the prioritised sample of one update, ONE workgroup over all B rows (any B).  draw != 0 (library RNG): row b's Philox block
//      (b, 0, update lo, update hi) as sac_sample_index, u = c[0] * 2^-32 in float64, SegmentTree.get_prefix_sum_idx's descent with
//      scalar = u * root, then the n-step chain, end bits and rsample noise exactly as the uniform sampler forms them from an
//      index.  Either mode: the importance weights of the rows in a.idx, (leaf / min_prio) ** (-beta), with weight_norm divided by
//      the batch maximum, as float32.
struct PerBatch {
    float* w;            // [B] importance weights of the loss
    double* wd;          // [B] the same before the normalisation
    int B, weight_norm;
    double beta;
};
#define PER_BOOK_LDS 512
// the body of per_sample_kernel and of per_sample_group_kernel (kernels_per_group.hpp); book_s[PER_BOOK_LDS], red[PER_THREADS]: LDS
__device__ __forceinline__ void per_sample_body(const SacSampleArgs& a, const PerDev& p, const PerBatch& pb, const int draw,
                                                SacBook* book_s, double* red) {
    constexpr int BOOK_LDS = PER_BOOK_LDS;
    const int tid = threadIdx.x, nt = blockDim.x;
    if (draw) {
        const bool in_lds = a.env_num <= BOOK_LDS;
        if (in_lds) {
            for (int e = tid; e < a.env_num; e += nt) book_s[e] = a.book[e];
            __syncthreads();
        }
        const SacBook* __restrict__ book = in_lds ? book_s : a.book;
        const uint32_t k0 = (uint32_t)a.key, k1 = (uint32_t)(a.key >> 32);
        const double root = p.tree[1];
        for (int b = tid; b < a.B; b += nt) {
            uint32_t c[4] = {(uint32_t)b, 0u, (uint32_t)a.counter, (uint32_t)(a.counter >> 32)};
            philox4x32_10(c, k0, k1);
            double scalar = ((double)c[0] * (1.0 / 4294967296.0)) * root;
            int i = 1;
            while (i < p.bound) {
                i *= 2;
                const double l = p.tree[i];
                if (l < scalar) { scalar -= l; i += 1; }
            }
            // a zero leaf (an empty slot, reached only through rounding) is taken as it is, but never past the store
            const int slot = min(i - p.bound, p.slots - 1);
            int idx, term;
            unsigned char f;
            bool head;
            sac_sample_chain(a, book, b, slot, idx, term, f, head);
            sac_sample_end_last(a, b, f, head);
            for (int d0 = 0; d0 < a.Da; d0 += 2) sac_sample_noise(a, b, d0, k0, k1);
        }
    }
    const double min_prio = p.sc[1];
    double mx = 0.0;
    for (int b = tid; b < pb.B; b += nt) {          // row b's index was written by this thread (draw) or by the host's copy
        const int s = min(max(a.idx[b], 0), p.slots - 1);
        const double wv = pow(p.tree[p.bound + s] / min_prio, -pb.beta);
        pb.wd[b] = wv;
        mx = fmax(mx, wv);
    }
    if (pb.weight_norm) mx = per_block_extreme<true>(mx, red);
    for (int b = tid; b < pb.B; b += nt) pb.w[b] = (float)(pb.weight_norm ? pb.wd[b] / mx : pb.wd[b]);
}
__global__ __launch_bounds__(PER_THREADS) void per_sample_kernel(const SacSampleArgs a, const PerDev p, const PerBatch pb, const int draw) {
    __shared__ SacBook book_s[PER_BOOK_LDS];
    __shared__ double red[PER_THREADS];
    per_sample_body(a, p, pb, draw, book_s, red);
}

// ---- PrioritizedReplayBuffer.update_weight, ONE workgroup.  ext == NULL: behind the critics' Q_TRAIN launch, td_avg of row b =
//      the float32 mean over the n_q networks of Q_j - y (critics_loss's td_average: summed in network order, then divided), kept in
//      td_out; ext != NULL: the caller's new weights.  p = |.| + eps in float64, leaf = p ** alpha; of duplicate indices the highest
//      batch position writes (numpy's fancy assignment); max_prio / min_prio take p's extremes over ALL rows.
struct PerUpd {
    const int* idx;      // [B]
    const float* q;      // [n_q][B]
    const float* y;      // [2][B]
    const double* ext;   // [B] or NULL
    float* td_out;       // [B] (ext == NULL)
    int B, n_q, pair_shift;
};
// the body of per_update_kernel and of per_update_group_kernel (kernels_per_group.hpp); red[PER_THREADS]: LDS
__device__ __forceinline__ void per_update_body(const PerDev& p, const PerUpd& u, double* red) {
    const int tid = threadIdx.x, nt = blockDim.x;
    auto slot_of = [&](int b) {
        const int s = u.idx[b];
        return (s >= 0 && s < p.slots) ? s : -1;
    };
    for (int b = tid; b < u.B; b += nt) {
        const int s = slot_of(b);
        if (s >= 0) p.stamp[s] = -1;
    }
    __syncthreads();
    for (int b = tid; b < u.B; b += nt) {
        const int s = slot_of(b);
        if (s >= 0) atomicMax(&p.stamp[s], b);
    }
    __syncthreads();
    double mx = 0.0, mn = INFINITY;
    for (int b = tid; b < u.B; b += nt) {
        double v;
        if (u.ext) v = u.ext[b];
        else {
            float t = 0.0f;
            for (int j = 0; j < u.n_q; ++j) t += u.q[(size_t)j * u.B + b] - u.y[(size_t)(j >> u.pair_shift) * u.B + b];
            t /= (float)u.n_q;
            u.td_out[b] = t;
            v = (double)t;
        }
        const double pr = fabs(v) + PER_F32_EPS;
        mx = fmax(mx, pr); mn = fmin(mn, pr);
        const int s = slot_of(b);
        if (s >= 0 && p.stamp[s] == b) p.tree[p.bound + s] = pow(pr, p.alpha);
    }
    mx = per_block_extreme<true>(mx, red);
    mn = per_block_extreme<false>(mn, red);
    if (tid == 0 && u.B > 0) { p.sc[0] = fmax(p.sc[0], mx); p.sc[1] = fmin(p.sc[1], mn); }
    __syncthreads();
    per_repair(p, u.B, slot_of);
}
__global__ __launch_bounds__(PER_THREADS) void per_update_kernel(const PerDev p, const PerUpd u) {
    __shared__ double red[PER_THREADS];
    per_update_body(p, u, red);
}
