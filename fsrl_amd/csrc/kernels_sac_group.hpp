// kernels_sac_group.hpp -- grouped SAC-Lagrangian and DDPG-Lagrangian updates (part of fsrl_hip.hip, host side: host_sac_group.inc).
// k SAC-Lag contexts (or k DDPG-Lag contexts) of one network shape step in lock step: every launch of the update carries all active members, the
// member being one more grid coordinate.  Each kernel reads its member's arguments from a device table (SacGroupMember,
// rewritten once per grouped call) and the per-(update, member) values from a step table (SacGroupStep: the sample's arguments,
// Adam step sizes from t_critic / t_actor, stats-ring row, active flag), and then runs the single-context body inlined:
// a member's arithmetic is fsrl_sac_update's.  Nine launches per grouped update, whatever k is:
//   actors' forward (sample + gather folded in)  -> target Q -> critics' Q_TRAIN (n-step targets in-kernel)
//   -> critics' weight gradients -> critics' Adam + Polyak -> Q_DIN -> actor backward -> actor weight gradients
//   -> actor Adam + alpha step + logged row.
// A DDPG-Lag member differs where fsrl_sac_update does: two critics (the y extent of the Q grids), the deterministic actor
// (SacActorArgs::deterministic), the target actor PAT in the first half of the forward launch, and PAT's Polyak update in the
// actor's Adam pass instead of an alpha step.
struct SacGroupMember {
    float *PA, *MA, *VA, *PQ, *PQT, *MQ, *VQ;
    float* PAT;                    // DDPG-Lag: the target actor (actor_old); null for SAC-Lag members
    const float *GA, *GQ;          // split-K partial gradients of the actor / the critics (the member's own buffers)
    FbArgs qf, qt, qd;             // target-Q forward (P = PQT), critics' training launch, Q input gradients (P = PQ)
    SacActorArgs af, ab;           // both actors' forward (its sample: SacGroupStep::sa), actor backward
    WgradPtrs wq, wa;              // weight gradients of batches of up to 512 rows (ppo_wgrad_body)
    FbWgradArgs fq, fa;            // ... of larger batches (fb_wgrad_body, XCD-aware block order)
    SacFinalArgs fin;              // fin.stats per step
    float* stats;                  // the member's statistics ring
    int nstats;
    float one_minus_b1, beta2, one_minus_b2, adam_eps, tau, one_minus_tau;
};
struct SacGroupStep {              // per (update index, member)
    SacSampleArgs sa;              // the update's sample: the member's sample arguments with its Philox counter (its n_updates)
    int row, active;               // stats-ring row; 0 = the member sits this update out
    float c_step, c_bc2, a_step, a_bc2;    // Adam lr / bias_correction1 and sqrt(bias_correction2) at t_critic / t_actor
};

// FWD: both actors' forward, the member's sample drawn and gathered in the same launch (first half: a' at s_{t+n}, from the
// target actor for a DDPG-Lag member; second half: af.P2 = PA at s_t); BWD: the actor's backward.
// grid = (tiles of the launch, k)
template <int H, int R, int MODE>
__global__ __launch_bounds__(4 * H) void sac_actor_group_kernel(const ModelDesc md, const SacGroupMember* __restrict__ tab,
                                                               const SacGroupStep* __restrict__ steps) {
    __shared__ TileSmem<H> sm;
    const SacGroupStep& st = steps[blockIdx.y];
    if (!st.active) return;
    const SacGroupMember& g = tab[blockIdx.y];
    const float* P = (MODE == SAC_A_FWD && g.PAT) ? g.PAT : g.PA;
    sac_actor_tile_body<H, R>(sm, P, md, MODE == SAC_A_FWD ? g.af : g.ab, (int)blockIdx.x, st.sa);
}

// the Q-network tile launches: WHICH 0 = target Q forward, 1 = critics' Q_TRAIN, 2 = Q_DIN.  grid = (tiles, n_q, k)
template <int H, int R, int WHICH>
__global__ __launch_bounds__(4 * H) void sac_q_group_kernel(const ModelDesc md, const SacGroupMember* __restrict__ tab,
                                                           const SacGroupStep* __restrict__ steps) {
    __shared__ TileSmem<H, tile_rows(R)> sm;
    if (!steps[blockIdx.z].active) return;
    const SacGroupMember& g = tab[blockIdx.z];
    const float* P = WHICH == 0 ? g.PQT : g.PQ;
    const FbArgs& a = WHICH == 0 ? g.qf : (WHICH == 1 ? g.qt : g.qd);
    fb_tile_body<H, R>(sm, P, md, a, (int)blockIdx.x * R, (int)blockIdx.x, (int)blockIdx.y, (int)gridDim.y);
}

// weight gradients, batches of up to 512 rows: ppo_wgrad_kernel's body, the final gradient in the member's partial buffer.
// grid = (wg_grid(H, networks), k)
template <int H, int ACTOR>
__global__ __launch_bounds__(1024) void sac_wgrad_group_kernel(const ModelDesc md, const SacGroupMember* __restrict__ tab,
                                                              const SacGroupStep* __restrict__ steps, const int rows) {
    if (!steps[blockIdx.y].active) return;
    const SacGroupMember& g = tab[blockIdx.y];
    const PpoStepArgs none{};
    ppo_wgrad_body<H, false, false>(md, ACTOR ? g.wa : g.wq, rows, none, 0);
}

// weight gradients of larger batches: fb_wgrad_kernel's split-K body in XCD-aware block order (the member's splits and
// summation order are fsrl_sac_update's; only the placement of the blocks differs).  grid = (round_up(remap_total, 8), k)
template <int H, int ACTOR>
__global__ __launch_bounds__(1024) void sac_wgrad_split_group_kernel(const ModelDesc md, const SacGroupMember* __restrict__ tab,
                                                                    const SacGroupStep* __restrict__ steps) {
    if (!steps[blockIdx.y].active) return;
    const SacGroupMember& g = tab[blockIdx.y];
    const FbWgradArgs& wa = ACTOR ? g.fa : g.fq;
    constexpr int NT2 = (H / 64) * (H / 64), NA = H / FB_AUX_COLS;
    const int L = blockIdx.x, per = gridDim.x >> 3;
    const int Lp = (L & 7) * per + (L >> 3);
    if (Lp >= wa.remap_total) return;
    const int NB = NT2 + NA * wa.aux_passes + 1;
    const int gi = Lp / NB;
    fb_wgrad_body<H, false>(md, wa, Lp % NB, gi % wa.remap_ny, gi / wa.remap_ny);
}

// the critics' Adam with the Polyak update of the targets riding along (adam_range_kernel's element path).  grid = (n / 256, k)
__global__ __launch_bounds__(256) void sac_adam_group_kernel(const ModelDesc md, const SacGroupMember* __restrict__ tab,
                                                            const SacGroupStep* __restrict__ steps, const int n,
                                                            const int nparts, const int stride) {
    const SacGroupStep& st = steps[blockIdx.y];
    if (!st.active) return;
    const SacGroupMember& g = tab[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float p = g.PQ[i];
    float gs = g.GQ[i];                                    // split-K partials, z order
    for (int z = 1; z < nparts; ++z) gs += g.GQ[(size_t)z * stride + i];
    adam_element(g.PQ, g.MQ, g.VQ, i, p, gs, 1.0f, 0.0f, g.one_minus_b1, g.beta2, g.one_minus_b2, st.c_step, st.c_bc2, g.adam_eps,
                 md, g.PQT, g.tau, g.one_minus_tau);
}

// the actor's Adam; the last block of every member writes its logged row and steps alpha (adam_final_kernel + sac_finalize_row).
// DDPG-Lag: actor_old <- tau * actor + (1 - tau) * actor_old rides in the same pass, as in fsrl_sac_update.
// grid = (n / 256 + 1, k)
__global__ __launch_bounds__(256) void sac_adam_final_group_kernel(const ModelDesc md, const SacGroupMember* __restrict__ tab,
                                                                  const SacGroupStep* __restrict__ steps, const int n,
                                                                  const int nparts, const int stride) {
    const SacGroupStep& st = steps[blockIdx.y];
    if (!st.active) return;
    const SacGroupMember& g = tab[blockIdx.y];
    if (blockIdx.x == gridDim.x - 1) {
        if (threadIdx.x < 64) {
            SacFinalArgs fa = g.fin;
            fa.stats = g.stats + (size_t)st.row * g.nstats;
            sac_finalize_row(fa, threadIdx.x);
        }
        return;
    }
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float p = g.PA[i];
    float gs = g.GA[i];
    for (int z = 1; z < nparts; ++z) gs += g.GA[(size_t)z * stride + i];
    adam_element(g.PA, g.MA, g.VA, i, p, gs, 1.0f, 0.0f, g.one_minus_b1, g.beta2, g.one_minus_b2, st.a_step, st.a_bc2, g.adam_eps,
                 md, g.PAT, g.tau, g.one_minus_tau);
}
