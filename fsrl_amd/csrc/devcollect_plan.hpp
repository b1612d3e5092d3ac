// devcollect_plan.hpp -- what a device collect DECIDES (fsrl_collect_device, host_devcollect.inc / kernels_devcollect.hpp): when an
// episode is cut, which finished envs leave the live set (the surplus rule of fsrl/data/fast_collector.py:341-362), and how the host
// replays the kernel's log of rows through the store's bookkeeping.  Plain functions over plain arrays, no HIP and no allocation: the
// collect kernel and the host call the SAME code, and tests/host/devcollect_sim.cpp drives it as a plain program
// (tests/test_devcollect_host.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DC_HD __host__ __device__ inline
#else
#define DC_HD static inline
#endif

#define DC_MAX_ENVS 64          // envs of one device env = rows of one vector step = 4 tiles of 16 rows
#define DC_DEFAULT_STEPS 64     // vector steps per launch when the caller names none: 1.8 - 2.9 ms per launch at 256 x 256 (28 - 45 us per vector step)
#define DC_MAX_STEPS 4096       // upper bound of max_steps_per_launch: the kernel loop's fixed trip count, and the log's size

// one stored transition as the host needs it to replay the bookkeeping: 24 bytes
struct DcLogRow {
    int32_t env;
    uint32_t flags;     // bit 0 terminated, bit 1 truncated
    double rew, cost;
};

// what persists between the launches of one collect (device memory; the host reads it back with the log)
struct DcState {
    int32_t n_live, episodes, n_episode, finished;
    int32_t steps, log_rows, pad0, pad1;        // of the LAST launch
    int32_t live[DC_MAX_ENVS];                  // env ids in position order
    int32_t index[DC_MAX_ENVS];                 // write index of every env's sub-buffer (EnvBook::index)
};

// the time limit belongs to the collect loop, not to the env: t_after = steps taken in this episode, this one included
DC_HD bool dc_truncated(int32_t t_after, int32_t max_episode_steps) { return t_after >= max_episode_steps; }
DC_HD uint32_t dc_flags(bool terminated, bool truncated) { return (terminated ? 1u : 0u) | (truncated ? 2u : 0u); }
// a collect starts from the first min(env_num, n_episode) envs
DC_HD int32_t dc_first_live(int32_t env_num, int32_t n_episode) { return env_num < n_episode ? env_num : n_episode; }

// The end of one vector step (fast_collector.py:341-362).  done[p] != 0: the env at position p finished an episode in this step.
// episodes grows by the number of finished envs; then surplus = live - (n_episode - episodes), and the first `surplus` FINISHED
// positions leave the live set (the others keep their order).  Returns the new number of live envs; *episodes is updated.
// The caller resets every finished env, dropped or not, before it calls this: the rule only decides who goes on.
DC_HD int32_t dc_episode_end(int32_t* live, int32_t n_live, const uint8_t* done, int32_t n_episode, int32_t* episodes) {
    int32_t n_done = 0;
    for (int32_t p = 0; p < n_live; ++p) n_done += done[p] ? 1 : 0;
    if (n_done == 0) return n_live;
    *episodes += n_done;
    int32_t surplus = n_live - (n_episode - *episodes);
    if (surplus <= 0) return n_live;
    int32_t w = 0;
    for (int32_t p = 0; p < n_live; ++p) {
        if (done[p] && surplus > 0) { --surplus; continue; }
        live[w++] = live[p];
    }
    return w;
}
DC_HD bool dc_complete(int32_t episodes, int32_t n_episode) { return episodes >= n_episode; }

// ---- the wide collect (fsrl_collect_device_wide, kernels_devcollect_wide.hpp): one launch per vector step, one workgroup per
// 16-row tile.  dc_episode_end as a rule per POSITION, for threads that each know only their own position: with
// rank = the number of finished positions in front of p, position p leaves iff it finished and rank < surplus, and a survivor moves
// up by the number of leavers in front of it, min(rank, surplus).  tests/host/devcollect_wide_sim.cpp holds it to dc_episode_end.
#ifndef DCW_MAX_ENVS
#define DCW_MAX_ENVS 4096       // envs of one wide device env: one round of 256 tiles (include/fsrl_hip.h has it too)
#endif
#define DCW_MAX_LOG_ROWS (1 << 20)     // log rows of one batch of launches
DC_HD int32_t dc_wide_surplus(int32_t n_live, int32_t n_done, int32_t n_episode, int32_t episodes_after) {
    const int32_t s = n_live - (n_episode - episodes_after);
    return n_done == 0 || s <= 0 ? 0 : s;
}
DC_HD bool dc_wide_leaves(bool done, int32_t rank, int32_t surplus) { return done && rank < surplus; }
DC_HD int32_t dc_wide_new_pos(int32_t p, int32_t rank, int32_t surplus) { return p - (rank < surplus ? rank : surplus); }
DC_HD int32_t dc_wide_n_live(int32_t n_live, int32_t n_done, int32_t surplus) { return n_live - (n_done < surplus ? n_done : surplus); }
// vector steps of one batch when the caller names none: clamp(2^20 / env_num, 1, 64); a named count is cut to the log's cap
DC_HD int32_t dc_wide_batch_steps(int32_t env_num, int32_t asked) {
    const int32_t cap = DCW_MAX_LOG_ROWS / env_num;
    const int32_t s = asked > 0 ? asked : DC_DEFAULT_STEPS;
    return s < cap ? s : (cap < 1 ? 1 : cap);
}
// ---- k wide collects in one launch per vector step (fsrl_collect_device_wide_group).  The grid is the members' tiles laid end to end:
// prefix[m] = tiles in front of member m, and every entry from k on holds the grid, so that a search over all DCWG_MAX_MEMBERS
// entries needs no k.  A workgroup's member is the number of entries 1 .. DCWG_MAX_MEMBERS - 1 at or below its block number: fifteen
// comparisons, the same for every block.  Every member has at least one tile (env_num, n_episode >= 1).
#define DCWG_MAX_MEMBERS 16     // FSRL_MAX_GROUP
DC_HD int32_t dc_wide_tiles(int32_t env_num, int32_t n_episode) { return (dc_first_live(env_num, n_episode) + 15) / 16; }
DC_HD int32_t dc_wgroup_prefix(const int32_t* env_num, const int32_t* n_episode, int32_t k, int32_t* prefix) {      // prefix[DCWG_MAX_MEMBERS + 1] -> the grid
    int32_t at = 0;
    for (int32_t i = 0; i <= DCWG_MAX_MEMBERS; ++i) {
        prefix[i] = at;
        if (i < k) at += dc_wide_tiles(env_num[i], n_episode[i]);
    }
    return at;
}
DC_HD int32_t dc_wgroup_member(const int32_t* prefix, int32_t b) {
    int32_t m = 0;
    for (int32_t i = 1; i < DCWG_MAX_MEMBERS; ++i) m += b >= prefix[i] ? 1 : 0;
    return m;
}
// a batch's step launches: dc_wide_batch_steps of the LARGEST member, so that every member's log holds the batch
DC_HD int32_t dc_wgroup_batch_steps(const int32_t* env_num, int32_t k, int32_t asked) {
    int32_t widest = 1;
    for (int32_t i = 0; i < k; ++i) widest = env_num[i] > widest ? env_num[i] : widest;
    return dc_wide_batch_steps(widest, asked);
}
// ---- wide collects for layered contexts (fsrl_collect_device_wide_layered, kernels_devcollect_wide_layered.hpp): a tile's
// activations are two halves of 16 rows of ld = round_up(max(widest hidden layer, obs_dim), 4) floats.  Up to DCWL_LDS_WIDTH they
// live in dynamic LDS at the row stride dc_wl_stride(ld) -- the first multiple of 4 at or above ld whose quarter is odd, so that the
// sixteen rows of a 16-byte read fall into sixteen different four-bank groups; 128 x 1028 bytes at the limit, next to 10 KB of static
// arrays in a CU's 160 KB -- and beyond it in a per-tile slice of a device-memory workspace, at stride ld.
#define DCWL_LDS_WIDTH 1024
DC_HD bool dc_wl_in_lds(int32_t ld) { return ld <= DCWL_LDS_WIDTH; }
DC_HD int32_t dc_wl_stride(int32_t ld) { return !dc_wl_in_lds(ld) || ((ld >> 2) & 1) ? ld : ld + 4; }
DC_HD int64_t dc_wl_lds_bytes(int32_t ld) { return dc_wl_in_lds(ld) ? (int64_t)2 * 16 * dc_wl_stride(ld) * 4 : 0; }
// What persists between the launches of a wide collect.  Everything a launch writes that another workgroup of the SAME launch reads is
// held twice, by the parity of the launch ordinal t: launch t reads side t & 1 and writes side (t + 1) & 1.  s[] describes the
// collect as the step before left it: `pending` says that this step's flags in done[] have not been through the surplus rule yet (the
// next launch does that first, in every workgroup); lpar names the half of live[] that holds the live list.
struct DcwScalars { int32_t n_live, episodes, finished, log_rows, steps, lpar, pending, pad; };
struct DcwState {
    DcwScalars s[2];
    int32_t n_episode, pad[15];
    int32_t live[2][DCW_MAX_ENVS];              // env ids in position order
    uint32_t done[2][DCW_MAX_ENVS / 4];         // a byte per position: the step's episode ends
    int32_t index[DCW_MAX_ENVS];                // write index of every env's sub-buffer, by env id (its own thread's alone)
};

// ---- wide evaluations (fsrl_evaluate_device_wide, kernels_deveval_wide.hpp): the EPISODE is the unit that leaves the GPU.  An env's
// running return, cost and length are held by env id (its own thread's alone); an ending episode is parked at its POSITION on the
// side of the next launch, and the next launch's settle -- which has every finished position's rank anyway -- moves it to row
// episodes_before + rank of the episode log: step-major, position order inside a step, the order devcollect_replay meets the ending
// rows in.  The row of old position p is written by the workgroup that ran p's tile in the step before, tile p / 16 of the fixed grid
// (it exists in every launch of the collect, whatever the live count has shrunk to); the one-workgroup settle launch writes all.
// tests/host/deveval_wide_sim.cpp holds the rule to a sequential walk of dc_episode_end.
struct DcEpisodeRow {       // 24 bytes: a parked record and a row of the episode log
    double rew, cost;
    int32_t len;
    uint32_t flags;         // of the episode's last step: bit 0 terminated, bit 1 truncated
};
DC_HD int32_t dc_wide_episode_row(bool done, int32_t episodes_before, int32_t rank, int32_t n_episode) {     // -1: no row
    const int32_t r = episodes_before + rank;
    return done && r < n_episode ? r : -1;
}
DC_HD bool dc_wide_row_owner(int32_t p, int32_t tile, bool all_rows) { return all_rows || (p >> 4) == tile; }
struct DcwEval {
    double rew[DCW_MAX_ENVS], cost[DCW_MAX_ENVS];       // the running episode of every env, by env id
    int32_t len[DCW_MAX_ENVS];
    DcEpisodeRow park[2][DCW_MAX_ENVS];                 // by the parity of the launch that settles them, by position
};

// slot of env e's next row and the index behind it (tianshou ReplayBuffer.add: ptr = index, index = (index + 1) % maxsize)
DC_HD int64_t dc_slot(int32_t e, int64_t sub_size, int32_t index) { return (int64_t)e * sub_size + index; }
DC_HD int32_t dc_next_index(int32_t index, int64_t sub_size) { return (int64_t)index + 1 >= sub_size ? 0 : index + 1; }     // index < sub_size: (index + 1) % sub_size without the division

// ---- how many launches a collect may take.  Every launch that is not the last takes max_steps vector steps, each of which stores at
// least one row: at most ceil(n_episode x max_episode_steps / max_steps) + 1 launches finish any collect.
DC_HD int64_t dc_launch_cap(int32_t n_episode, int32_t max_episode_steps, int32_t max_steps) {
    return ((int64_t)n_episode * max_episode_steps + max_steps - 1) / max_steps + 1;
}

// ---- k collects in one launch (fsrl_collect_device_group).  The members' episode arrays are concatenated in member order:
// off[i] = n_episode[0] + .. + n_episode[i - 1], off[k] = the total.
DC_HD void dc_group_offsets(const int32_t* n_episode, int32_t k, int64_t* off) {
    off[0] = 0;
    for (int32_t i = 0; i < k; ++i) off[i + 1] = off[i] + n_episode[i];
}
// the launch goes on until EVERY member is finished, so its cap is the largest of the members' caps
DC_HD int64_t dc_group_launch_cap(const int32_t* n_episode, const int32_t* max_episode_steps, int32_t k, int32_t max_steps) {
    int64_t cap = 0;
    for (int32_t i = 0; i < k; ++i) {
        const int64_t c = dc_launch_cap(n_episode[i], max_episode_steps[i], max_steps);
        cap = c > cap ? c : cap;
    }
    return cap;
}
// "a launch made no step" holds against the members that were UNFINISHED going in only: a finished member's workgroup breaks at the
// loop's first test and reports 0 steps every time.  Returns the first member that was unfinished and made no step, or -1.
DC_HD int32_t dc_group_stalled(const uint8_t* was_finished, const int32_t* steps, int32_t k) {
    for (int32_t i = 0; i < k; ++i)
        if (!was_finished[i] && steps[i] == 0) return i;
    return -1;
}
DC_HD bool dc_group_complete(const uint8_t* finished, int32_t k) {
    for (int32_t i = 0; i < k; ++i)
        if (!finished[i]) return false;
    return true;
}

// ---- host replay.  BOOK has the fields of the store's per-env bookkeeping (index, size, last_index, ep_rew, ep_len, ep_idx); one log
// row moves them exactly as fsrl_store_push moves them for one pushed row.  Returns true when the row ends an episode; then
// *ep_rew / *ep_len hold the episode's return and length (what the push reports in ep_rew_out / ep_len_out).
template <class BOOK>
static inline bool dc_replay_row(BOOK& eb, int64_t sub_size, uint8_t* h_flags, const DcLogRow& r, double* ep_rew, int32_t* ep_len) {
    const int64_t ptr = eb.index;
    h_flags[(size_t)(ptr + (int64_t)r.env * sub_size)] = (uint8_t)r.flags;
    eb.last_index = ptr;
    eb.size = eb.size + 1 < sub_size ? eb.size + 1 : sub_size;
    eb.index = (eb.index + 1) % sub_size;
    eb.ep_rew += r.rew;
    eb.ep_len += 1;
    if (r.flags == 0) return false;
    *ep_rew = eb.ep_rew; *ep_len = eb.ep_len;
    eb.ep_rew = 0.0; eb.ep_len = 0; eb.ep_idx = eb.index;
    return true;
}

// ---- the replay of an evaluation (fsrl_evaluate_device): nothing was stored, so no book moves.  The episode's return and length run
// in accumulators that belong to the evaluated env, one per env, zeroed when an evaluation starts; one log row moves them as
// dc_replay_row moves a book's ep_rew / ep_len, in the same order of additions, and reports an ended episode the same way.
struct DcEvalAcc {
    double ep_rew;
    int32_t ep_len;
};
static inline bool dc_eval_row(DcEvalAcc& acc, const DcLogRow& r, double* ep_rew, int32_t* ep_len) {
    acc.ep_rew += r.rew;
    acc.ep_len += 1;
    if (r.flags == 0) return false;
    *ep_rew = acc.ep_rew; *ep_len = acc.ep_len;
    acc.ep_rew = 0.0; acc.ep_len = 0;
    return true;
}
