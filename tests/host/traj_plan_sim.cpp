// traj_plan_sim.cpp -- fsrl_amd/csrc/traj_plan.hpp (the trajectory archive's bookkeeping and job planning) as a stand-alone program:
// its own process, nothing preloaded, built with the address / undefined-behaviour sanitizers (tests/test_traj_plan_host.py).
//
// The device is modelled by arrays of row tags: two archive halves and one open-episode area per source.  A "launch" executes a
// job table the way traj_move_kernel may -- jobs in any order -- after checking what the kernel relies on: every job inside its
// source and destination, source and destination different memory, no two jobs of the launch writing the same row.  The program
// drives the book with random episode lengths, windows of several finished episodes, keeps, replacements and clears, in archives
// that are almost full, and checks after every step that the alive episodes are where the table says, row for row, once.
#include <cassert>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>

#include "traj_plan.hpp"

using namespace trajp;

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

struct Device {
    std::vector<int64_t> half[2];
    std::vector<std::vector<int64_t>> open;      // per source: slots x L
    int64_t launches = 0, jobs = 0;
};
static int64_t tag(int32_t id, int32_t row) { return (int64_t)id * 100000 + row + 1; }

static void launch(Device& d, const std::vector<int64_t>& src, std::vector<int64_t>& dst, const std::vector<Job>& jobs, std::mt19937& g) {
    REQUIRE(src.data() != dst.data());
    std::set<int64_t> written;
    std::vector<size_t> order(jobs.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    std::shuffle(order.begin(), order.end(), g);
    for (size_t i : order) {
        const Job& j = jobs[i];
        REQUIRE(j.rows >= 1 && j.rows <= JOB_ROWS);
        REQUIRE(j.src >= 0 && j.src + j.rows <= (int64_t)src.size());
        REQUIRE(j.dst >= 0 && j.dst + j.rows <= (int64_t)dst.size());
        for (int r = 0; r < j.rows; ++r) {
            REQUIRE(written.insert(j.dst + r).second);
            dst[(size_t)(j.dst + r)] = src[(size_t)(j.src + r)];
        }
    }
    d.launches += 1; d.jobs += (int64_t)jobs.size();
}

// every alive episode is where the table says; alive rows are disjoint; the counters agree
static void check(const Book& b, const Device& d, const std::map<int32_t, int32_t>& rows_of) {
    std::set<int64_t> seen;
    int64_t total = 0;
    for (const Episode& e : b.table) {
        REQUIRE(rows_of.count(e.id) && rows_of.at(e.id) == e.rows);
        REQUIRE(e.first >= 0 && e.first + e.rows <= b.tail && b.tail <= b.max_rows);
        for (int r = 0; r < e.rows; ++r) {
            REQUIRE(d.half[b.cur][(size_t)(e.first + r)] == tag(e.id, r));
            REQUIRE(seen.insert(e.first + r).second);
        }
        total += e.rows;
    }
    REQUIRE(total == b.alive_rows && b.n.rows == total);
    REQUIRE((int64_t)b.table.size() <= b.max_episodes);
    if (b.packed) {
        int64_t at = 0;
        for (const Episode& e : b.table) { REQUIRE(e.first == at); at += e.rows; }
        REQUIRE(at == b.tail);
    }
}

static void compact(Book& b, Device& d, std::mt19937& g) {
    std::vector<Job> jobs;
    const int from = b.cur;
    b.compact(jobs);
    launch(d, d.half[from], d.half[from ^ 1], jobs, g);
    REQUIRE(b.packed && b.tail == b.alive_rows);
}

static void run(unsigned seed, int64_t max_rows, int32_t max_episodes, int L, int n_src, int env_num, int steps) {
    std::mt19937 g(seed);
    Book b;
    b.max_rows = max_rows; b.max_episodes = max_episodes; b.max_len = L;
    Device d;
    d.half[0].assign((size_t)max_rows, 0); d.half[1].assign((size_t)max_rows, 0);
    d.open.assign((size_t)n_src, std::vector<int64_t>((size_t)env_num * L, 0));
    std::map<int32_t, int32_t> rows_of;
    int64_t refused = 0, kept_calls = 0, replaced = 0;
    for (int s = 0; s < steps; ++s) {
        const int what = (int)(g() % 10);
        if (what < 6) {                                  // a window of one source: up to env_num finished episodes, one per slot
            const int src = (int)(g() % n_src);
            std::vector<Pending> batch;
            for (int e = 0; e < env_num; ++e)
                if (g() % 2) batch.push_back(Pending{e, (int32_t)(1 + g() % L), 0.0, 0.0});
            if (batch_wants_compaction(b, batch)) compact(b, d, g);
            std::vector<Job> jobs;
            std::vector<int32_t> ids;
            const size_t before = b.table.size();
            const int nref = commit_batch(b, batch, L, src, jobs, &ids);
            refused += nref;
            REQUIRE(ids.size() == batch.size() && b.table.size() - before + (size_t)nref == batch.size());
            REQUIRE(nref == 0 || b.err.find("max_rows") != std::string::npos || b.err.find("max_episodes") != std::string::npos);
            // what the stage launch put into the open area (tagged with the id the episode got; refused ones with a tag no check
            // accepts), then the commit launch
            size_t at = before;
            for (size_t i = 0; i < batch.size(); ++i) {
                const Pending& p = batch[i];
                for (int r = 0; r < p.rows; ++r) d.open[(size_t)src][(size_t)p.slot * L + r] = ids[i] < 0 ? -7 : tag(ids[i], r);
                if (ids[i] < 0) continue;
                REQUIRE(b.table[at].id == ids[i] && b.table[at].rows == p.rows && b.table[at].source == src);
                rows_of[ids[i]] = p.rows;
                at += 1;
            }
            REQUIRE(at == b.table.size());
            launch(d, d.open[(size_t)src], d.half[b.cur], jobs, g);
        } else if (what < 8 && !b.table.empty()) {       // keep a random subset in a random order
            std::vector<int32_t> ids;
            for (const Episode& e : b.table) if (g() % 3) ids.push_back(e.id);
            std::shuffle(ids.begin(), ids.end(), g);
            REQUIRE(b.keep(ids.data(), (int64_t)ids.size()));
            std::map<int32_t, int32_t> nr;
            for (int32_t id : ids) nr[id] = rows_of[id];
            rows_of.swap(nr);
            compact(b, d, g);
            for (size_t i = 0; i < ids.size(); ++i) REQUIRE(b.table[i].id == ids[i]);
            kept_calls += 1;
            // an id that is gone, and an id twice, are refused and change nothing
            const int32_t gone = b.next_id + 5;
            REQUIRE(!b.keep(&gone, 1));
            if (!ids.empty()) { const int32_t twice[2] = {ids[0], ids[0]}; REQUIRE(!b.keep(twice, 2)); }
            REQUIRE(b.table.size() == ids.size());
        } else if (what == 8 && b.table.size() >= 2) {   // the newest takes a random victim's place
            const size_t v = g() % (b.table.size() - 1);
            const int32_t victim = b.table[v].id, newest = b.table.back().id;
            REQUIRE(b.replace(victim));
            REQUIRE(b.table[v].id == newest && b.find(victim) < 0);
            rows_of.erase(victim);
            REQUIRE(!b.replace(victim));
            replaced += 1;
        } else if (what == 9 && g() % 8 == 0) {
            b.clear(); rows_of.clear();
        }
        check(b, d, rows_of);
    }
    // export: compact if needed, then [0, tail) is the alive episodes in table order
    if (!b.packed) compact(b, d, g);
    check(b, d, rows_of);
    int64_t at = 0;
    for (const Episode& e : b.table)
        for (int r = 0; r < e.rows; ++r) REQUIRE(d.half[b.cur][(size_t)at++] == tag(e.id, r));
    REQUIRE(at == b.tail);
    std::printf("ok run seed=%u committed=%lld refused=%lld compactions=%lld keeps=%lld replaced=%lld launches=%lld jobs=%lld\n", seed,
                (long long)b.n.committed, (long long)refused, (long long)b.n.compactions, (long long)kept_calls, (long long)replaced,
                (long long)d.launches, (long long)d.jobs);
    REQUIRE(b.n.committed > 0 && b.n.compactions > 0);
}

static void window_and_limits() {
    Book b;
    b.max_rows = 10; b.max_episodes = 3; b.max_len = 4;
    REQUIRE(b.in_window(1e300, -1e300));
    b.set_window(-1.0, 2.0, 0.0, 3.0);
    REQUIRE(b.in_window(-1.0, 0.0) && b.in_window(2.0, 3.0) && !b.in_window(2.0000001, 1.0) && !b.in_window(0.0, -1e-9));
    REQUIRE(b.in_window(__builtin_nan(""), 0.0));               // traj_buf.py:71-73: a NaN return fails no comparison, so it is stored
    // exactly full is fine, one more row is not, and the message names the limit
    REQUIRE(b.room(4) == 0); b.commit(4, 0, 0, 0);
    REQUIRE(b.room(4) == 0); b.commit(4, 0, 0, 0);
    REQUIRE(b.room(2) == 0 && b.room(3) == -1 && b.err.find("max_rows = 10") != std::string::npos);
    // a dead episode makes room, after a compaction
    const int32_t only = 1;
    REQUIRE(b.keep(&only, 1));
    REQUIRE(b.room(4) == 1);
    std::vector<Job> jobs;
    b.compact(jobs);
    REQUIRE(jobs.size() == 1 && jobs[0].src == 4 && jobs[0].dst == 0 && jobs[0].rows == 4 && b.room(4) == 0);
    b.commit(4, 0, 0, 0); b.commit(2, 0, 0, 0);
    REQUIRE(b.room(1) == -1 && b.err.find("max_episodes = 3") != std::string::npos);
    // long runs are cut into pieces of at most JOB_ROWS rows that tile the run
    jobs.clear();
    add_run(jobs, 7, 1000, 3 * JOB_ROWS + 5);
    REQUIRE(jobs.size() == 4 && jobs[3].rows == 5 && jobs[3].src == 7 + 3 * JOB_ROWS && jobs[3].dst == 1000 + 3 * JOB_ROWS);
    std::printf("ok window_and_limits\n");
}

int main() {
    window_and_limits();
    run(1, 400, 64, 40, 3, 3, 3000);           // tight rows: compactions because of room
    run(2, 100000, 24, 300, 2, 20, 2000);      // tight table: max_episodes refusals, long episodes cut into several jobs
    run(3, 64, 1000, 9, 1, 5, 4000);           // tiny archive: refusals that name max_rows
    std::printf("ok all\n");
    return 0;
}
