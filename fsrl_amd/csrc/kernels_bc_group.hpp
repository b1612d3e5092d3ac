// kernels_bc_group.hpp -- k seeds' behaviour-cloning updates in the TWO launches of one (fsrl_bc_update_group, host_bc_group.inc).
//
// A solo update at batch 256 is 16 workgroups of bc_fwd_bwd_kernel on a 256-CU part and a dependent chain of two launches: its cost is
// the chain, not the arithmetic.  k members' updates share nothing -- each has its own parameters, moments, side buffers and index
// block -- so their workgroups ride in the same two launches:
//   bc_fwd_bwd_group_kernel<H, HEAD>   the grid is the step's ACTIVE members' 16-row tiles laid end to end, sum of ceil(B_m / 16), not
//                                      a k x max-tiles rectangle (batch 16 beside batch 1024 would launch 128 workgroups for 65 tiles).
//                                      A workgroup finds (member, tile) from the step's prefix of tile counts -- sixteen words behind
//                                      one scalar load, fifteen scalar comparisons (dc_wgroup_member, the wide collects' search) --
//                                      reads the member's row with scalar loads and runs bc_fwd_bwd_body on the member's pointers.
//                                      The lookup is the kernel's first instructions, in front of the body's prologue: the small
//                                      parameters, the gathered rows, the forward W2 burst and the early backward fragment
//                                      (BcEarly<H>::JE row groups, held in registers across the forward pass) are issued exactly as
//                                      in the solo kernel, one scalar round trip later.  Every field of the row is uniform, so the
//                                      indirection costs scalar registers only: the body's vector registers are the solo kernel's.
//   bc_wgrad_group_kernel<H>           grid.y the member, grid.x the solo job list dW2 | dW1 | dW3 | (dsigma) | loss of the member with
//                                      the longest one; a workgroup past its member's list, or of a member whose updates are done
//                                      (u >= n_updates: also a member that sits the call out), returns at its first test.  The Adam
//                                      scalars of (step, member) come from the step's row; the tile's Adam step, W2 mirror included,
//                                      is bc_wgrad_body's.
// Both bodies are the solo kernels' (kernels_bc.hpp): the same MFMA order, the same reduction order, the same Adam arithmetic on the
// same host scalars -- a member's losses, gradient, parameters and moments are the solo call's bit for bit.  All members share one
// ModelDesc (the host checks that the shapes agree).  Between the workgroups of a launch no word one writes is read by another: no
// atomics, fences or waits, as in the solo launches.
//
// What is constant for the call sits in BcGroupTable (uploaded once per call), what moves with the step in BcGroupStep[steps]
// (uploaded once per call too; a launch gets its step's address): the tile prefix of the members still active and each member's
// Adam step_size / bc2_sqrt, which depend on its own step count.  A member's index block and loss slot of step u follow from u and
// its batch size; betas and eps are per member and stay in its BcWgradArgs.
#pragma once
#include "kernels_bc.hpp"
#include "kernels_devcollect_wide.hpp"      // dc_uniform_ptr, dc_wgroup_member

struct BcGroupMember {
    const float* P;              // the actor's parameters as bc_fwd_bwd_kernel takes them
    int32_t n_updates, pad;      // the member is active in steps 0 .. n_updates - 1
    BcArgs a;                    // idx: the member's whole [n_updates][B] block
    BcWgradArgs w;               // idx, loss_out likewise: step 0's; step_size / bc2_sqrt are the step row's
};
struct BcGroupTable { BcGroupMember m[FSRL_MAX_GROUP]; };
struct BcGroupStep {
    int32_t prefix[DCWG_MAX_MEMBERS];      // tiles in front of member m among this step's active members; from k on: the grid
    float step_size[FSRL_MAX_GROUP], bc2_sqrt[FSRL_MAX_GROUP];
};

// a pointer field of a member's row: uniform and global, so that what is read through it takes the solo kernel's global loads
template <class T>
__device__ __forceinline__ T* bc_member_ptr(T* p) { return const_cast<T*>(dc_uniform_ptr<1>(static_cast<const T*>(p))); }

template <int H, int HEAD>
__global__ __launch_bounds__(4 * H) void bc_fwd_bwd_group_kernel(const ModelDesc md, const BcGroupTable* __restrict__ tab,
                                                                 const BcGroupStep* __restrict__ step, const int u) {
    const BcGroupStep* sp = dc_uniform_ptr<4>(step);
    const int b = __builtin_amdgcn_readfirstlane((int)blockIdx.x);
    const int m = __builtin_amdgcn_readfirstlane(dc_wgroup_member(sp->prefix, b));
    const int tile = b - sp->prefix[m];
    const BcGroupMember* gm = dc_uniform_ptr<4>(&tab->m[m]);
    BcArgs a;
    a.obs = bc_member_ptr(gm->a.obs); a.act = bc_member_ptr(gm->a.act);
    a.B = gm->a.B; a.loss = gm->a.loss; a.mean_tanh = gm->a.mean_tanh; a.max_action = gm->a.max_action;
    a.idx = bc_member_ptr(gm->a.idx) + (size_t)u * a.B;
    a.A1 = bc_member_ptr(gm->a.A1); a.A2 = bc_member_ptr(gm->a.A2); a.D1 = bc_member_ptr(gm->a.D1); a.D2 = bc_member_ptr(gm->a.D2);
    a.DO = bc_member_ptr(gm->a.DO); a.lossp = bc_member_ptr(gm->a.lossp);
    bc_fwd_bwd_body<H, HEAD>(bc_member_ptr(gm->P), md, a, tile);
}

template <int H>
__global__ __launch_bounds__(256) void bc_wgrad_group_kernel(const ModelDesc md, const BcGroupTable* __restrict__ tab,
                                                             const BcGroupStep* __restrict__ step, const int u) {
    const int m = __builtin_amdgcn_readfirstlane((int)blockIdx.y), b = __builtin_amdgcn_readfirstlane((int)blockIdx.x);
    const BcGroupMember* gm = dc_uniform_ptr<4>(&tab->m[m]);
    if (u >= gm->n_updates) return;
    const int nb = bc_wg_grid(H, md.Do, gm->w.sigma_job);
    if (b >= nb) return;
    const BcGroupStep* sp = dc_uniform_ptr<4>(step);
    BcWgradArgs w;
    w.A1 = bc_member_ptr(gm->w.A1); w.A2 = bc_member_ptr(gm->w.A2); w.D1 = bc_member_ptr(gm->w.D1); w.D2 = bc_member_ptr(gm->w.D2);
    w.DO = bc_member_ptr(gm->w.DO); w.obs = bc_member_ptr(gm->w.obs);
    w.B = gm->w.B; w.rows_pad = gm->w.rows_pad; w.tiles = gm->w.tiles; w.sigma_job = gm->w.sigma_job; w.sigma_zero = gm->w.sigma_zero;
    w.idx = bc_member_ptr(gm->w.idx) + (size_t)u * w.B;
    w.P = bc_member_ptr(gm->w.P); w.M = bc_member_ptr(gm->w.M); w.V = bc_member_ptr(gm->w.V); w.G = bc_member_ptr(gm->w.G);
    w.lossp = bc_member_ptr(gm->w.lossp); w.loss_out = bc_member_ptr(gm->w.loss_out) + u;
    w.one_minus_b1 = gm->w.one_minus_b1; w.beta2 = gm->w.beta2; w.one_minus_b2 = gm->w.one_minus_b2; w.eps = gm->w.eps;
    w.step_size = sp->step_size[m]; w.bc2_sqrt = sp->bc2_sqrt[m];
    bc_wgrad_body<H>(md, w, b, nb);
}
