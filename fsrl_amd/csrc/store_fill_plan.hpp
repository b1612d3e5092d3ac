// store_fill_plan.hpp -- the host side of fsrl_store_fill (include/fsrl_hip.h): pour archived episodes into a context's store.
// Standard library only (no HIP), so tests/host/store_fill_plan_sim.cpp drives it as a plain program
// (tests/test_store_fill_plan_host.py); host_traj.inc launches store_fill_kernel (kernels_traj.hpp) off the job table.
//
// The model the plan is held to: episode j of the list goes to sub-buffer e_j = (first_env + j) % buffer_num, row by row through
// fsrl_store_push.  Every archived episode is complete -- its last row carries the end flags, no other row has any -- so after an
// episode the sub-buffer's running episode is empty again (ep_rew 0, ep_len 0, ep_idx = index), and the books after the whole fill
// follow from the row counts alone.  A sub-buffer that receives W rows writes the slots (index + w) % sub_size, w = 0 .. W - 1; when
// W > sub_size the first W - sub_size of them are overwritten inside the same fill and are left out: the surviving writes of a
// sub-buffer are consecutive mod sub_size and no more than sub_size, so the launch writes every slot at most once.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

#include "traj_plan.hpp"

namespace fillp {

// the bookkeeping of one sub-buffer (EnvBook of fsrl_hip.hip without its staging count)
struct SubBook {
    int64_t index = 0, size = 0, last_index = 0;
    double ep_rew = 0.0;
    int32_t ep_len = 0;
    int64_t ep_idx = 0;
};

struct FlagEntry { int64_t slot; uint8_t flags; };      // the last row of an episode that survives: the only non-zero flags

enum { FILL_OK = 0, REFUSE_ARG = 1, REFUSE_STATE = 2 };

struct Plan {
    std::vector<trajp::Job> jobs;       // src: row of the archive's current half; dst: slot of the store (global); rows <= JOB_ROWS
    std::vector<SubBook> books;         // the books after the fill (all buffer_num of them)
    std::vector<FlagEntry> ends;        // host flag mirror: every slot of a job becomes 0, then these
    int64_t rows = 0;                   // rows the push loop would have pushed
    int64_t written = 0;                // rows the launch writes (= rows - dropped)
    int64_t dropped = 0;                // rows a later row of the same fill overwrites
    bool wrapped = false;               // a run was cut at the end of a sub-buffer
    int code = FILL_OK;
    std::string err;                    // names the offending field
};

static inline bool refuse(Plan& p, int code, const std::string& msg) { p.code = code; p.err = msg; return false; }

// ids == nullptr: every alive episode in table order (n is ignored).  false: refused, p.code / p.err say why, nothing else is valid.
static inline bool plan(const std::vector<trajp::Episode>& table, const int32_t* ids, int64_t n, int32_t first_env, int64_t sub_size,
                        int32_t buffer_num, const std::vector<SubBook>& books, Plan& p) {
    p = Plan{};
    if (buffer_num < 1 || sub_size < 1 || (int64_t)books.size() < (int64_t)buffer_num)
        return refuse(p, REFUSE_ARG, "store geometry: sub_size " + std::to_string(sub_size) + ", buffer_num " + std::to_string(buffer_num));
    if (first_env < 0 || first_env >= buffer_num)
        return refuse(p, REFUSE_ARG, "first_env " + std::to_string(first_env) + " is outside [0, buffer_num = " + std::to_string(buffer_num) + ")");
    std::vector<const trajp::Episode*> eps;
    if (!ids) {
        for (const trajp::Episode& e : table) eps.push_back(&e);
    } else {
        if (n < 0) return refuse(p, REFUSE_ARG, "episode_ids: negative count");
        std::unordered_map<int32_t, int> at;
        for (size_t i = 0; i < table.size(); ++i) at[table[i].id] = (int)i;
        for (int64_t i = 0; i < n; ++i) {
            auto it = at.find(ids[i]);
            if (it == at.end())
                return refuse(p, REFUSE_ARG, "episode_ids[" + std::to_string(i) + "] = " + std::to_string(ids[i]) + " is not alive in the trajectory archive");
            if (it->second < 0)
                return refuse(p, REFUSE_ARG, "episode_ids[" + std::to_string(i) + "] = " + std::to_string(ids[i]) + " is listed twice");
            eps.push_back(&table[(size_t)it->second]);
            it->second = -1;
        }
    }
    const int64_t E = (int64_t)eps.size();
    // what every sub-buffer receives
    std::vector<int64_t> total((size_t)buffer_num, 0);
    for (int64_t j = 0; j < E; ++j) {
        const int e = (int)((first_env + j) % buffer_num);
        if (books[(size_t)e].ep_len != 0)
            return refuse(p, REFUSE_STATE, "sub-buffer " + std::to_string(e) + " has an episode in progress (ep_len " +
                                         std::to_string(books[(size_t)e].ep_len) + "): fills go between collects");
        total[(size_t)e] += eps[(size_t)j]->rows;
    }
    p.books = books;
    std::vector<int64_t> seen((size_t)buffer_num, 0);       // rows of this fill that went to the sub-buffer so far
    for (int64_t j = 0; j < E; ++j) {
        const trajp::Episode& ep = *eps[(size_t)j];
        const int e = (int)((first_env + j) % buffer_num);
        const SubBook& b0 = books[(size_t)e];
        const int64_t skip = std::max<int64_t>(0, total[(size_t)e] - sub_size);    // the first `skip` writes do not survive
        const int64_t w0 = seen[(size_t)e], rows = ep.rows;
        seen[(size_t)e] += rows;
        p.rows += rows;
        int64_t r = std::max<int64_t>(0, skip - w0);        // first surviving row of the episode
        p.dropped += std::min(r, rows);
        while (r < rows) {
            const int64_t local = (b0.index + w0 + r) % sub_size;
            const int64_t run = std::min(rows - r, sub_size - local);
            if (run < rows - r) p.wrapped = true;
            trajp::add_run(p.jobs, ep.first + r, (int64_t)e * sub_size + local, run);
            r += run;
            p.written += run;
            if (r == rows) p.ends.push_back(FlagEntry{(int64_t)e * sub_size + local + run - 1, ep.end});
        }
        if (rows > 0) {     // the books as `rows` pushes, the last of them done, leave them
            SubBook& b = p.books[(size_t)e];
            b.last_index = (b.index + rows - 1) % sub_size;
            b.size = std::min(b.size + rows, sub_size);
            b.index = (b.index + rows) % sub_size;
            b.ep_rew = 0.0; b.ep_len = 0; b.ep_idx = b.index;
        }
    }
    return true;
}

// the host mirror of the store's flags byte after the fill
static inline void apply_flags(const Plan& p, uint8_t* mirror) {
    for (const trajp::Job& j : p.jobs) std::fill(mirror + j.dst, mirror + j.dst + j.rows, (uint8_t)0);
    for (const FlagEntry& f : p.ends) mirror[f.slot] = f.flags;
}

}  // namespace fillp
