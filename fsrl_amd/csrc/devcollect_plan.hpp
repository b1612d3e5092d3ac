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
