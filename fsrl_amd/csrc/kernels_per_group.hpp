// kernels_per_group.hpp -- prioritised replay for a GROUP of SAC-Lagrangian / DDPG-Lagrangian contexts (part of fsrl_hip.hip, host
// side: host_sac_group.inc, host_sac_group_layered.inc).  The solo prioritised update's two tree launches, and for fused groups the
// plain gather, with the member as the grid coordinate: one workgroup (per_sample, per_update) or one row of workgroups (gather)
// per member runs the solo kernel's body inlined on the member's own arguments, so a member's arithmetic is fsrl_sac_update's.
// The member's tree arguments sit in a table of their own (PerGroupMember, rebuilt per grouped call: fsrl_per_set_beta between
// calls takes effect and a join may move the batch buffers); what changes per update -- whether the member still has updates to run,
// its Philox counter -- is read from the member's SacGroupStep row.  Nothing waits across workgroups: a member's tree is touched
// by its own workgroup alone, and an update's launches follow one another on the group's stream.
#pragma once
#include "kernels_per.hpp"
#include "kernels_layered_sac_group.hpp"   // sac_nstep_group_kernel: the fused prioritised group launches it stand-alone too

struct PerGroupMember {
    PerDev p;
    PerBatch pb;
    PerUpd u;
};

// the prioritised sample of every member's update (library RNG): per_sample_kernel per member.  grid = (members), PER_THREADS
__global__ __launch_bounds__(PER_THREADS) void per_sample_group_kernel(const PerGroupMember* __restrict__ per,
                                                                      const SacGroupStep* __restrict__ steps) {
    __shared__ SacBook book_s[PER_BOOK_LDS];
    __shared__ double red[PER_THREADS];
    const SacGroupStep& st = steps[blockIdx.x];
    if (!st.active) return;
    const SacSampleArgs sa = st.sa;                // by value, as the solo kernel has them: the body's stores alias nothing of them
    const PerDev p = per[blockIdx.x].p;
    const PerBatch pb = per[blockIdx.x].pb;
    per_sample_body(sa, p, pb, 1, book_s, red);
}

// the sampled rows' new priorities behind the critics' Q_TRAIN launch: per_update_kernel per member.  grid = (members), PER_THREADS
__global__ __launch_bounds__(PER_THREADS) void per_update_group_kernel(const PerGroupMember* __restrict__ per,
                                                                      const SacGroupStep* __restrict__ steps) {
    __shared__ double red[PER_THREADS];
    if (!steps[blockIdx.x].active) return;
    const PerDev p = per[blockIdx.x].p;
    const PerUpd u = per[blockIdx.x].u;
    per_update_body(p, u, red);
}

// the plain gather of every member's sampled rows: sac_gather_kernel per member.  Member i's arguments lie `stride` bytes behind
// member i - 1's: a fused group passes the forward launch's (SacGroupMember::af.ga, whose fold is off in a prioritised group), a
// layered group its gather table.  grid = (blocks of the gather, members), 256 threads
__global__ __launch_bounds__(256) void sac_gather_group_kernel(const SacGatherArgs* __restrict__ ga0, const size_t stride,
                                                              const SacGroupStep* __restrict__ steps) {
    if (!steps[blockIdx.y].active) return;
    const SacGatherArgs a = *reinterpret_cast<const SacGatherArgs*>(reinterpret_cast<const char*>(ga0) + blockIdx.y * stride);
    sac_gather_body(a);
}
