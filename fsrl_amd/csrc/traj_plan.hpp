// traj_plan.hpp -- the host bookkeeping of the trajectory archive (fsrl_traj_*, include/fsrl_hip.h): the episode table, where a
// finished episode goes, and the job tables of the row-moving launches (host_traj.inc launches kernels_traj.hpp off them).
// Standard library only (no HIP), so tests/host/traj_plan_sim.cpp drives it as a plain program (tests/test_traj_plan_host.py).
//
// The archive is two sets of columns of max_rows rows ("halves").  One half is current.  Finished episodes are appended at its
// tail; a compaction copies the alive episodes, in table order, to the front of the OTHER half and makes that one current.  Source
// and destination of a compaction are therefore different memory: no job of a launch can overlap another job or its own source,
// whatever the table order is (fsrl_traj_keep / _replace permute it).
#pragma once
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <string>
#include <unordered_map>
#include <vector>

namespace trajp {

// one launch moves `n` jobs; a job is a run of rows, contiguous at both ends.  Long runs are cut into pieces of at most
// JOB_ROWS rows, so that a workgroup per job is also the right amount of parallelism for three episodes of a thousand rows.
constexpr int JOB_ROWS = 128;
struct Job { int64_t src, dst; int32_t rows, pad; };

struct Episode {
    int64_t first = 0;          // first row in the current half
    int32_t rows = 0, id = 0, source = 0;
    double rew = 0.0, cost = 0.0;
    uint8_t end = 1;            // flags of its last row: terminal | timeout << 1 (every other row of an episode has none)
};

struct Counters {
    int64_t committed = 0, rejected_window = 0, dropped_long = 0, compactions = 0, rows = 0, refused_full = 0, abandoned = 0;
    int64_t import_open = 0;    // fsrl_traj_import: trailing runs without an end flag (open episodes are never archived)
};

static inline void add_run(std::vector<Job>& jobs, int64_t src, int64_t dst, int64_t rows) {
    for (int64_t o = 0; o < rows; o += JOB_ROWS)
        jobs.push_back(Job{src + o, dst + o, (int32_t)std::min<int64_t>(JOB_ROWS, rows - o), 0});
}

struct Book {
    int64_t max_rows = 0;
    int32_t max_episodes = 0, max_len = 0;
    double rmin, rmax, cmin, cmax;
    std::vector<Episode> table;     // alive episodes, table order
    int64_t tail = 0;               // first free row of the current half
    int64_t alive_rows = 0;
    int cur = 0;                    // current half
    bool packed = true;             // the alive episodes lie back to back from row 0, in table order
    int32_t next_id = 0;
    Counters n;
    std::string err;

    Book() { set_window(-__builtin_inf(), __builtin_inf(), -__builtin_inf(), __builtin_inf()); }
    void set_window(double r0, double r1, double c0, double c1) { rmin = r0; rmax = r1; cmin = c0; cmax = c1; }
    // traj_buf.py:71-73
    bool in_window(double rew, double cost) const { return !(rew > rmax || rew < rmin || cost > cmax || cost < cmin); }

    // Room for an episode of `rows` rows at the tail?  0 yes; 1 only after a compaction; -1 never (err names the limit).
    int room(int32_t rows) {
        if ((int64_t)table.size() >= (int64_t)max_episodes) {
            err = "the trajectory archive holds max_episodes = " + std::to_string(max_episodes) + " episodes: keep fewer, or create it larger";
            return -1;
        }
        if (tail + rows <= max_rows) return 0;
        if (alive_rows + rows <= max_rows && (!packed || tail != alive_rows)) return 1;
        err = "the trajectory archive is full: an episode of " + std::to_string(rows) + " rows does not fit max_rows = " +
              std::to_string(max_rows) + " (" + std::to_string(alive_rows) + " rows alive, after compaction)";
        return -1;
    }
    // Append an episode at the tail (room() said 0).  Returns its first row.
    int64_t commit(int32_t rows, int32_t source, double rew, double cost, uint8_t end = 1) {
        Episode e;
        e.first = tail; e.rows = rows; e.id = next_id++; e.source = source; e.rew = rew; e.cost = cost; e.end = end;
        table.push_back(e);
        // appended behind a packed archive, at the end of the table: still packed
        packed = packed && tail == alive_rows;
        tail += rows; alive_rows += rows;
        n.committed += 1; n.rows = alive_rows;
        return e.first;
    }
    // Jobs that copy every alive episode, in table order, to the front of the other half; the book then describes that half.
    void compact(std::vector<Job>& jobs) {
        jobs.clear();
        int64_t at = 0;
        for (Episode& e : table) {
            add_run(jobs, e.first, at, e.rows);
            e.first = at;
            at += e.rows;
        }
        tail = at; cur ^= 1; packed = true;
        n.compactions += 1;
    }
    int find(int32_t id) const {
        for (size_t i = 0; i < table.size(); ++i)
            if (table[i].id == id) return (int)i;
        return -1;
    }
    // Only `ids` stay alive, in the order given (the new table order).  false: an id that is not alive, or twice (nothing changed).
    bool keep(const int32_t* ids, int64_t k) {
        std::unordered_map<int32_t, int> at;
        for (size_t i = 0; i < table.size(); ++i) at[table[i].id] = (int)i;
        std::vector<Episode> nt;
        nt.reserve((size_t)k);
        for (int64_t i = 0; i < k; ++i) {
            auto it = at.find(ids[i]);
            if (it == at.end() || it->second < 0) {
                err = "episode id " + std::to_string(ids[i]) + " is not alive in the trajectory archive (or is named twice)";
                return false;
            }
            nt.push_back(table[(size_t)it->second]);
            it->second = -1;
        }
        table.swap(nt);
        alive_rows = 0;
        for (const Episode& e : table) alive_rows += e.rows;
        n.rows = alive_rows;
        packed = false;
        return true;
    }
    // The newest committed episode (the last of the table) takes the place of `victim` in table order (traj_buf.py:89-93).
    bool replace(int32_t victim) {
        const int v = find(victim);
        if (v < 0 || table.empty()) {
            err = "episode id " + std::to_string(victim) + " is not alive in the trajectory archive";
            return false;
        }
        if (v == (int)table.size() - 1) { err = "the newest episode cannot replace itself"; return false; }
        alive_rows -= table[(size_t)v].rows;
        table[(size_t)v] = table.back();
        table.pop_back();
        n.rows = alive_rows;
        packed = false;
        return true;
    }
    void clear() {
        table.clear(); tail = 0; alive_rows = 0; packed = true; n.rows = 0;
    }
};

// A staging window's finished episodes go to the archive in one launch.  If the batch does not fit behind the tail and a compaction
// can make room, the compaction runs BEFORE the first commit of the batch: the batch's own rows reach the archive only with its
// launch, so a compaction in the middle of it would copy rows that are not there yet.
struct Pending;
static inline bool batch_wants_compaction(const Book& b, const std::vector<Pending>& batch);
// Commit the batch: jobs from the open-episode area (the episode in slot s starts at row s * L) to the tail.  Returns how many episodes
// found no room (b.err names the limit; they are dropped and counted).  ids_out (may be null): per batch entry its id, -1 = refused.
static inline int commit_batch(Book& b, const std::vector<Pending>& batch, int L, int32_t source, std::vector<Job>& jobs,
                               std::vector<int32_t>* ids_out = nullptr);

// One env of one tapped context: the episode it is in.  `rows` counts every pushed row, also those past max_len (which are not
// recorded: the episode is dropped when it ends).  An env has TWO slots of the open-episode area, used in turn (slot 2 e + parity):
// the stage launch writes a window's rows in parallel and the commit launch reads them after it, so a slot may hold rows of one
// episode per window only.  With two slots an episode may end and the next one start inside one window; `ends` counts the episodes
// of this env that ended (or were abandoned) inside the current window, and the row after the second one waits for the flush.
struct OpenEpisode {
    double rew = 0.0, cost = 0.0;
    int32_t rows = 0;
    int32_t ends = 0, parity = 0;
    void next() { rew = cost = 0.0; rows = 0; ends += 1; parity ^= 1; }
};
// an episode that ended inside the current staging window and goes to the archive when the window is flushed
struct Pending { int32_t slot, rows; double rew, cost; uint8_t end = 1; };

static inline bool batch_wants_compaction(const Book& b, const std::vector<Pending>& batch) {
    int64_t need = 0;
    for (const Pending& p : batch) need += p.rows;
    return b.tail + need > b.max_rows && !b.packed;
}
static inline int commit_batch(Book& b, const std::vector<Pending>& batch, int L, int32_t source, std::vector<Job>& jobs,
                               std::vector<int32_t>* ids_out) {
    int refused = 0;
    for (const Pending& p : batch) {
        const bool fits = b.room(p.rows) == 0;
        if (ids_out) ids_out->push_back(fits ? b.next_id : -1);
        if (!fits) { b.n.refused_full += 1; refused += 1; continue; }
        add_run(jobs, (int64_t)p.slot * L, b.commit(p.rows, source, p.rew, p.cost, p.end), p.rows);
    }
    return refused;
}

// ---- fsrl_traj_import: host columns in the export layout -> episodes, committed as tapped ones are.
// An episode ends at every row whose terminal or timeout flag is set; its float64 returns are the sums of its rows in row order.
// A trailing run without an end flag is an open episode: dropped and counted.
struct ImportEpisode { int64_t first; int32_t rows; double rew, cost; uint8_t end; };
static inline void import_scan(Book& b, int64_t rows, const double* rew, const double* cost, const uint8_t* terminals,
                               const uint8_t* timeouts, std::vector<ImportEpisode>& out) {
    out.clear();
    int64_t first = 0;
    double r = 0.0, c = 0.0;
    for (int64_t i = 0; i < rows; ++i) {
        r += rew[i]; c += cost ? cost[i] : 0.0;
        const uint8_t fl = (uint8_t)((terminals && terminals[i] ? 1 : 0) | (timeouts && timeouts[i] ? 2 : 0));
        if (!fl) continue;
        // an episode of 2^31 rows or more is longer than any max_len
        out.push_back(ImportEpisode{first, (int32_t)std::min<int64_t>(i + 1 - first, INT32_MAX), r, c, fl});
        first = i + 1; r = c = 0.0;
    }
    if (first < rows) b.n.import_open += 1;
}
// host rows [src, src + rows) -> rows [dst, dst + rows) of the current half: one copy per column
struct ImportRun { int64_t src, dst, rows; };
// One scanned episode against the limits, the window and the room.  0: committed (its rows are appended to `runs`, merged with the
// run before it where both ends are adjacent); 1: a compaction can make room -- send `runs`, compact, call again; -1: no room (b.err
// names the limit; dropped and counted); -2: too long or outside the window (dropped and counted).
static inline int import_commit(Book& b, const ImportEpisode& e, int32_t source, std::vector<ImportRun>& runs) {
    if (e.rows > b.max_len) { b.n.dropped_long += 1; return -2; }
    if (!b.in_window(e.rew, e.cost)) { b.n.rejected_window += 1; return -2; }
    const int room = b.room(e.rows);
    if (room > 0) return 1;
    if (room < 0) { b.n.refused_full += 1; return -1; }
    const int64_t dst = b.commit(e.rows, source, e.rew, e.cost, e.end);
    if (!runs.empty() && runs.back().src + runs.back().rows == e.first && runs.back().dst + runs.back().rows == dst)
        runs.back().rows += e.rows;
    else
        runs.push_back(ImportRun{e.first, dst, e.rows});
    return 0;
}

}  // namespace trajp
