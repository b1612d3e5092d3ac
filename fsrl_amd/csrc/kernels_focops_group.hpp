// kernels_focops_group.hpp -- grouped FOCOPS updates (part of fsrl_hip.hip, host side: host_focops_group.inc).
// k FOCOPS contexts of one network shape step in lock step on the PPO group's entry points (fsrl_group_ppo_update): every
// launch of a minibatch step carries all active members, the member being one more grid coordinate.  Each kernel reads
// the member's per-pass arguments from a device table (FocGroupMember, rewritten once per pass) and the per-(minibatch step,
// member) arguments from a step table (FocGroupStep: the launch arguments focops_pass builds for that step -- minibatch
// offset and size, Adam step sizes of both optimisers, statistics row, pass bookkeeping, psq / sig_stash parity), and runs
// the single-context body inlined: a member's arithmetic is focops_pass's.  Per minibatch step:
//   three-launch members (minibatches <= 512 rows):  tile -> ppo_wgrad_body                     -> step
//   four-launch members (larger, or set_plan(1)):    tile -> split-K fb_wgrad_body -> prep      -> step
// plus one pass-start prep (nparts = 0) for the three-launch members.  A launch one kind of member does not need returns
// at once for the others, and the host skips launches no active member needs.
// A group of LAYERED members (host_layered_group.inc) runs the layered step instead, 2 L + 5 launches for all members:
//   lin_group_kernel<LIN_F> x (L + 1) -> lay_fb_head_group_kernel -> lin_group_kernel<LIN_X> x L -> <LIN_W> -> prep -> step
// with the finished gradient in G as the prep launch's one "partial", as focops_pass does for a layered context.
struct FocGroupMember {
    const float* P;                // the member's parameters (the tile launch's weights)
    FocopsStepArgs pass_prep;      // three-launch pass start: psq / sig_stash of the pass's first parity (nparts = 0)
    int fast;                      // 1: three-launch step (ppo_wgrad_body), 0: four-launch step (split-K + prep)
};
struct FocGroupStep {              // per (minibatch step, member)
    FbArgs fb;                     // tile launch: the minibatch's rows, cr = 1 / tem_lambda, cc = nu, eta, statp
    WgradPtrs wp;                  // three-launch step: ppo_wgrad_body's pointers (the minibatch's observation rows)
    FbWgradArgs wa;                // four-launch step: the split-K plan of the minibatch
    FocopsStepArgs sa;             // prep / step: Adam step sizes, logged row, pass bookkeeping, pp parity
    int active;                    // 0: the member has no minibatch at this index (ragged, empty or stopped)
    int n_tiles;                   // tile workgroups of the member's minibatch in this launch (4 * tiles with 4-row tiles)
    int rows_pad;                  // 16 * tiles: the side buffers' stride per network
};

// the activation side of all three networks (actor: FOCOPS loss head, critics: regression head).  grid = (tiles, 3, k)
template <int H, int R>
__global__ __launch_bounds__(4 * H) void focops_tile_group_kernel(const ModelDesc md, const FocGroupMember* __restrict__ tab,
                                                                 const FocGroupStep* __restrict__ steps) {
    __shared__ TileSmem<H, tile_rows(R)> sm;
    const FocGroupStep& st = steps[blockIdx.z];
    if (!st.active || (int)blockIdx.x >= st.n_tiles) return;
    fb_tile_body<H, R>(sm, tab[blockIdx.z].P, md, st.fb, (int)blockIdx.x * R, (int)blockIdx.x, (int)blockIdx.y, (int)gridDim.y);
}

// weight gradients of a three-launch step: ppo_wgrad_kernel<H, false, false>'s body.  grid = (wg_grid(H, 3), k)
template <int H>
__global__ __launch_bounds__(1024) void focops_wgrad_group_kernel(const ModelDesc md, const FocGroupMember* __restrict__ tab,
                                                                 const FocGroupStep* __restrict__ steps) {
    const FocGroupStep& st = steps[blockIdx.y];
    if (!st.active || !tab[blockIdx.y].fast) return;
    const PpoStepArgs none{};
    ppo_wgrad_body<H, false, false>(md, st.wp, st.rows_pad, none, 0);
}

// weight gradients of a four-launch step: fb_wgrad_kernel's split-K body in XCD-aware block order (the member's splits and
// summation order are focops_pass's; only the placement of the blocks differs).  grid = (round_up(max remap_total, 8), k)
template <int H>
__global__ __launch_bounds__(1024) void focops_wgrad_split_group_kernel(const ModelDesc md, const FocGroupMember* __restrict__ tab,
                                                                       const FocGroupStep* __restrict__ steps) {
    const FocGroupStep& st = steps[blockIdx.y];
    if (!st.active || tab[blockIdx.y].fast) return;
    const FbWgradArgs& wa = st.wa;
    constexpr int NT2 = (H / 64) * (H / 64), NA = H / FB_AUX_COLS;
    const int L = blockIdx.x, per = gridDim.x >> 3;
    const int Lp = (L & 7) * per + (L >> 3);
    if (Lp >= wa.remap_total) return;
    const int NB = NT2 + NA * wa.aux_passes + 1;
    const int gi = Lp / NB;
    fb_wgrad_body<H, false>(md, wa, Lp % NB, gi % wa.remap_ny, gi / wa.remap_ny);
}

// the loss heads of a LAYERED group's step (kernels_layered.hpp: lay_fb_head_kernel's body on head outputs the grouped forward
// launches left in the member's `out`).  grid = (tiles of the step's largest minibatch, 3, k); heads[member]: the member's buffers
// (out / dout / P / sigma / mbp / Da / unbounded), the step row's fb: the minibatch's row data, size, 1 / tem_lambda, the member's
// nu, eta and the statistics slots -- focops_tile_args' values, mode FB_MODE_FOCOPS from network 0 among them.  Copied into a
// local argument block first, for focops_step_group_kernel's reason below.
__global__ __launch_bounds__(256) void lay_fb_head_group_kernel(const LayHeadArgs* __restrict__ heads,
                                                               const FocGroupStep* __restrict__ steps) {
    const int m = blockIdx.z;
    const int active = steps[m].active;
    const FbArgs fb = steps[m].fb;
    if (!active || (int)blockIdx.x * 16 >= fb.N) return;                // the member's own tile count
    const LayHeadArgs hm = heads[m];
    LayFbHeadArgs h;
    h.out = hm.out; h.dout = hm.dout; h.rd = fb.rd; h.statp = fb.statp;
    h.P = hm.P; h.sigma = hm.sigma;
    h.mbp = hm.mbp; h.net0 = fb.net0; h.ny = 3; h.Da = hm.Da; h.unbounded = hm.unbounded; h.N = fb.N; h.mode = fb.mode;
    h.max_action = fb.max_action; h.cr = fb.cr; h.cc = fb.cc; h.eta = fb.eta;
    lay_fb_head_body(h, (int)blockIdx.x, (int)blockIdx.y);
}

// prep of a four-launch step (PASS_START 0: the split-K partials summed into G, the actor's per-block squares, the critics'
// parameter squares) or of a three-launch pass's start (PASS_START 1: the parameter squares only).  grid = (nb_all, k)
template <int PASS_START>
__global__ __launch_bounds__(256) void focops_prep_group_kernel(const ModelDesc md, const FocGroupMember* __restrict__ tab,
                                                               const FocGroupStep* __restrict__ steps) {
    const FocGroupMember& m = tab[blockIdx.y];
    if (PASS_START) {
        if (!m.fast || !steps[blockIdx.y].active) return;
        focops_prep_body(md, m.pass_prep, (int)blockIdx.x);
    } else {
        const FocGroupStep& st = steps[blockIdx.y];
        if (!st.active || m.fast) return;
        focops_prep_body(md, st.sa, (int)blockIdx.x);
    }
}

// clip + Adam of the three networks; the extra block writes the member's logged row and the pass KL bookkeeping.
// grid = (nb_all + 1, k).  The arguments are taken by value (uniform scalar loads, no scratch): read through a reference into
// global memory, every parameter store could alias them, and the compiler then contracts adam_element's
// `gs * coef + 2 * l2 * p` into the other fma than focops_step_kernel does -- the critics' steps would differ in the last bit.
__global__ __launch_bounds__(256) void focops_step_group_kernel(const ModelDesc md, const FocGroupStep* __restrict__ steps) {
    const FocGroupStep& st = steps[blockIdx.y];
    if (!st.active) return;
    const FocopsStepArgs sa = st.sa;
    focops_step_body(md, sa, (int)blockIdx.x);
}
