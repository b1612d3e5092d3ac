// kernels_deveval_wide_group.hpp -- k wide device EVALUATIONS in one launch per vector step (fsrl_evaluate_device_wide_group,
// host_deveval_wide.inc): the grid, the member search and the settle launch of the grouped wide collects
// (kernels_devcollect_wide.hpp "k wide collects in one launch per vector step") around the evaluation's bodies
// (wide_eval_step_body / wide_eval_layered_step_body, kernels_deveval_wide.hpp).
//
// The grid is the members' 16-row tiles laid end to end, the prefix grid of dc_wgroup_prefix over min(env_num, n_episode), fixed for
// the call -- a prefix and not a k x max-tiles rectangle, for the collects' reason: members may differ in env_num by two orders of
// magnitude.  A workgroup finds its member m with scalar loads and fifteen scalar compares (dc_wgroup_member), reads its row of the
// table through constant address space and runs the solo body on member m's WideEvalArgs (env arrays, DcwState, DcwEval, episode
// log), parameters or actor row, under member m's own launch ordinal: launch j of the call runs it on side (par0[m] + j) & 1.
// Everything position-bound is MEMBER-LOCAL: tile = blockIdx.x - prefix[m], so the row of member m's old position p is written by
// member m's tile p / 16 (it exists in every launch of the call: the grid is fixed), the writer of the handed-on scalars is member
// m's tile 0, and dcw_eval_settle runs over member m's flags, live list and park in each of member m's workgroups.  A finished
// member's workgroups exit at the body's first test, behind the rows they own of its last pending step.
// Nothing is shared between members, and inside a member the solo launch's rule holds, so between ALL workgroups of a launch: no
// word one of them writes is read by another, no atomics, fences or waits; park[] and done[] stay doubled by parity.
// The settle launch (settle = 1) is k workgroups, workgroup m the tile 0 of member m with all_rows = true; it also leaves member m's
// settled scalars in settled[m], so that the host reads every member's with one copy of k x 32 bytes per batch.
// md is member 0's: the host checks that the members agree on what it describes (devcollect_group_agree).
// The table is the evaluations' own: WideGroupTable and the collect kernels' argument lists are untouched.
// Registers and LDS: the wrappers hold (m, tile) in scalar registers and nothing else across the body; no instantiation spills or
// uses scratch, and none takes more LDS than its solo counterpart (tests/test_deveval_wide_group_host.py; counts in DESIGN.md 3.4.1).
#pragma once
#include "kernels_deveval_wide.hpp"

struct WideEvalGroupTable {
    int32_t prefix[DCWG_MAX_MEMBERS + 1];       // tiles in front of member m; from k on: the grid, so the search needs no k
    int32_t par0[DCWG_MAX_MEMBERS];             // the PARITY of the member's launch ordinal at the call's first launch
    const WideEvalArgs* wa[DCWG_MAX_MEMBERS];
    const float* P[DCWG_MAX_MEMBERS];           // fused members: the actor's parameters
    const WideLayActor* la[DCWG_MAX_MEMBERS];   // layered members: the actor's row
};
// (member, tile) of this workgroup, both in scalar registers
__device__ __forceinline__ void dcweg_find(const WideEvalGroupTable* tb, const int settle, int& m, int& tile) {
    const int b = __builtin_amdgcn_readfirstlane((int)blockIdx.x);
    m = settle ? b : __builtin_amdgcn_readfirstlane(dc_wgroup_member(tb->prefix, b));
    tile = settle ? 0 : b - tb->prefix[m];
}

template <int H, class Env, int HEAD>
__global__ __launch_bounds__(4 * H) DCW_NO_PK void wide_eval_group_step_kernel(const ModelDesc md, const WideEvalGroupTable* __restrict__ tab,
                                                                               DcwScalars* __restrict__ settled, const int j, const int first,
                                                                               const int settle) {
    const WideEvalGroupTable* tb = dc_uniform_ptr<4>(tab);
    int m, tile;
    dcweg_find(tb, settle, m, tile);
    wide_eval_step_body<H, Env, HEAD>(md, dc_uniform_ptr<1>(tb->P[m]), dc_uniform_ptr<4>(tb->wa[m]), tb->par0[m] + j, first, settle, tile,
                                      settle ? settled + m : nullptr);
}

// layered members: a row names its own WideLayActor -- parameters, LayNet, and in the DEVWS form its own workspace, indexed by the
// tile's number in THAT member's grid.  The members share hidden_sizes (the host checks it): one dynamic LDS size, one form.
template <class Env, int HEAD, bool DEVWS>
__global__ __launch_bounds__(WL_NT) WL_NO_PK void wide_eval_layered_group_step_kernel(const WideEvalGroupTable* __restrict__ tab,
                                                                                      DcwScalars* __restrict__ settled, const int j, const int first,
                                                                                      const int settle) {
    extern __shared__ __align__(16) float wl_lds[];             // !DEVWS: [2][16][ldp]
    __shared__ DevCollectSmem sh;                               // the tile uses its first 16 rows
    __shared__ float raw[16 * FSRL_MAX_ACT];                    // the head's raw rows
    __shared__ int32_t wtot[16];
    const WideEvalGroupTable* tb = dc_uniform_ptr<4>(tab);
    int m, tile;
    dcweg_find(tb, settle, m, tile);
    wide_eval_layered_step_body<Env, HEAD, DEVWS>(tb->wa[m], tb->la[m], tb->par0[m] + j, first, settle, tile, settle ? settled + m : nullptr,
                                                  wl_lds, sh, raw, wtot);
}
