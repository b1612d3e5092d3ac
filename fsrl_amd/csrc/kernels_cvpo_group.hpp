// kernels_cvpo_group.hpp -- grouped CVPO updates (part of fsrl_hip.hip, host side: host_cvpo_group.inc).
// k CVPO contexts of one network shape step in lock step, the member being one more grid coordinate, as in kernels_sac_group.hpp.
// A grouped update is the single-context chain, 9 + 4 * mstep_iter_num launches whatever k is:
//   sample + gather + particle noise -> actor TARGET + PARTICLES -> target Q -> critics' Q_TRAIN (n-step targets in-kernel)
//   -> critics' weight gradients -> critics' Adam + Polyak -> Q over the K * B particles -> E-step
//   -> per M iteration: actor MFWD -> M dual step -> actor MBWD -> actor weight gradients -> actor Adam (the last with the logged row).
// What CVPO shares with SAC-Lag runs through the SAC group's kernels on a SacGroupMember table: the three Q tile launches
// (sac_q_group_kernel: qf = target Q, qt = Q_TRAIN, qd = the particle forward into QK), both weight-gradient forms and the critics'
// Adam.  This file holds the launches that are CVPO's own; they read a second table, CvpoGroupMember.  The per-(update, member)
// values are the SAC group's SacGroupStep (sample arguments with the Philox counter, ring row, active flag, the critics' Adam
// constants); the actor's Adam constants change with every M iteration and sit in CvpoGroupIter [update][iteration][member].
struct CvpoGroupMember {
    float *PA, *MA, *VA;
    const float* GA;               // the actor's (split-K partial) gradient: the member's own buffer
    SacGatherArgs ga;
    CvpoActorArgs at, am, ab;      // TARGET + PARTICLES (two batches), MFWD, MBWD
    CvpoEstepArgs es;
    CvpoMdualArgs md;              // log_it per launch
    CvpoFinalArgs fin;             // fin.stats per step
    float* stats;                  // the member's statistics ring
    int nstats;
    float one_minus_b1, beta2, one_minus_b2, adam_eps;
};
struct CvpoGroupIter { float a_step, a_bc2; };     // Adam lr / bias_correction1 and sqrt(bias_correction2) at the iteration's t_actor

// sample + gather + the particles' noise.  grid = (blocks of the single launch, k)
__global__ __launch_bounds__(256) void cvpo_sample_gather_group_kernel(const CvpoGroupMember* __restrict__ tab,
                                                                      const SacGroupStep* __restrict__ steps) {
    const SacGroupStep& st = steps[blockIdx.y];
    if (!st.active) return;
    cvpo_sample_gather_body(st.sa, tab[blockIdx.y].ga, (int)blockIdx.x);
}

// the actor tile launch: WHICH 0 = TARGET + PARTICLES, 1 = MFWD, 2 = MBWD.  grid = (tiles of the launch, k)
template <int H, int R, int WHICH>
__global__ __launch_bounds__(4 * H) void cvpo_actor_group_kernel(const ModelDesc md, const CvpoGroupMember* __restrict__ tab,
                                                                const SacGroupStep* __restrict__ steps) {
    __shared__ TileSmem<H> sm;
    if (!steps[blockIdx.y].active) return;
    const CvpoGroupMember& g = tab[blockIdx.y];
    cvpo_actor_tile_body<H, R>(sm, g.PA, md, WHICH == 0 ? g.at : (WHICH == 1 ? g.am : g.ab), (int)blockIdx.x);
}

// the E-step: one workgroup per member.  grid = (k)
__global__ __launch_bounds__(1024) void cvpo_estep_group_kernel(const CvpoGroupMember* __restrict__ tab,
                                                               const SacGroupStep* __restrict__ steps) {
    __shared__ double red[3][1024];
    __shared__ float duals[2];
    if (!steps[blockIdx.x].active) return;
    cvpo_estep_body(tab[blockIdx.x].es, red, duals);
}

// the M dual step: one wave per member.  grid = (k)
__global__ __launch_bounds__(64) void cvpo_mdual_group_kernel(const CvpoGroupMember* __restrict__ tab,
                                                             const SacGroupStep* __restrict__ steps, const int log_it) {
    if (!steps[blockIdx.x].active) return;
    CvpoMdualArgs ma = tab[blockIdx.x].md;
    ma.log_it = log_it;
    cvpo_mdual_body(ma);
}

// the actor's Adam of one M iteration; FINAL: the last block of every member writes its logged row (adam_final_kernel +
// cvpo_finalize_row).  grid = (n / 256 + FINAL, k)
template <int FINAL>
__global__ __launch_bounds__(256) void cvpo_adam_group_kernel(const ModelDesc md, const CvpoGroupMember* __restrict__ tab,
                                                             const SacGroupStep* __restrict__ steps,
                                                             const CvpoGroupIter* __restrict__ iters, const int n,
                                                             const int nparts, const int stride) {
    const SacGroupStep& st = steps[blockIdx.y];
    if (!st.active) return;
    const CvpoGroupMember& g = tab[blockIdx.y];
    if (FINAL && blockIdx.x == gridDim.x - 1) {
        if (threadIdx.x < 64) {
            CvpoFinalArgs fa = g.fin;
            fa.stats = g.stats + (size_t)st.row * g.nstats;
            cvpo_finalize_row(fa, threadIdx.x);
        }
        return;
    }
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const CvpoGroupIter it = iters[blockIdx.y];
    const float p = g.PA[i];
    float gs = g.GA[i];                                    // split-K partials, z order
    for (int z = 1; z < nparts; ++z) gs += g.GA[(size_t)z * stride + i];
    adam_element(g.PA, g.MA, g.VA, i, p, gs, 1.0f, 0.0f, g.one_minus_b1, g.beta2, g.one_minus_b2, it.a_step, it.a_bc2, g.adam_eps,
                 md, nullptr, 0.0f, 1.0f);
}
