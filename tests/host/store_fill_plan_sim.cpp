// store_fill_plan_sim.cpp -- fsrl_amd/csrc/store_fill_plan.hpp (the plan of fsrl_store_fill) as a stand-alone program: its own
// process, nothing preloaded, built with the address / undefined-behaviour sanitizers (tests/test_store_fill_plan_host.py).
//
// The model is the loop the header defines the call by: episode j of the list goes, row by row, through the bookkeeping of
// fsrl_store_push into sub-buffer (first_env + j) % buffer_num.  The device is modelled by arrays of row tags: the archive half and
// the store.  A "launch" executes the job table the way store_fill_kernel may -- jobs in any order -- after checking what the kernel
// relies on: every job inside the archive and inside the store, at most JOB_ROWS rows, no slot written twice.  After the launch the
// store's tags, every book and the flag mirror must equal what the scalar loop left.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>

#include "store_fill_plan.hpp"

using namespace fillp;
using trajp::Episode;
using trajp::Job;

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

struct Store {
    int64_t S = 0; int B = 0;
    std::vector<int64_t> tag;       // per slot: the archive row it holds (-1: none)
    std::vector<uint8_t> flags;
    std::vector<SubBook> books;
};

// fsrl_store_push for one row (fsrl_hip.hip), bookkeeping only
static void model_push(Store& s, int e, int64_t src_tag, double rew, uint8_t fl) {
    SubBook& b = s.books[(size_t)e];
    const int64_t ptr = b.index, g = ptr + (int64_t)e * s.S;
    s.tag[(size_t)g] = src_tag;
    s.flags[(size_t)g] = fl;
    b.last_index = ptr;
    b.size = std::min(b.size + 1, s.S);
    b.index = (b.index + 1) % s.S;
    b.ep_rew += rew;
    b.ep_len += 1;
    if (fl) { b.ep_rew = 0.0; b.ep_len = 0; b.ep_idx = b.index; }
}

static bool same(const SubBook& a, const SubBook& b) {
    return a.index == b.index && a.size == b.size && a.last_index == b.last_index && a.ep_rew == b.ep_rew && a.ep_len == b.ep_len &&
           a.ep_idx == b.ep_idx;
}

struct Tally { int64_t cases = 0, wrapped = 0, dropped = 0, jobs = 0, subsets = 0, first_env = 0, prewrapped = 0; };

static void one_case(std::mt19937& g, Tally& t, int B, int64_t S, const std::vector<int32_t>& lens, bool subset, int first_env,
                     int prefill) {
    // the archive: episodes at scattered places of one half, ids in commit order, table order shuffled
    std::vector<Episode> table;
    int64_t at = 0;
    for (size_t i = 0; i < lens.size(); ++i) {
        at += (int64_t)(g() % 5);       // dead rows between alive episodes
        Episode e;
        e.first = at; e.rows = lens[i]; e.id = (int32_t)(100 + i); e.end = (uint8_t)(1 + g() % 3);
        table.push_back(e);
        at += lens[i];
    }
    const int64_t archive_rows = at + 3;
    std::shuffle(table.begin(), table.end(), g);
    // the store: part-filled or already wrapped books, all between episodes
    Store s;
    s.S = S; s.B = B;
    s.tag.assign((size_t)(S * B), -1); s.flags.assign((size_t)(S * B), 0); s.books.resize((size_t)B);
    for (int e = 0; e < B; ++e) {
        int64_t n = prefill == 0 ? 0 : (prefill == 1 ? (int64_t)(g() % (uint64_t)S) : S + (int64_t)(g() % (uint64_t)(2 * S)));
        for (int64_t i = 0; i < n; ++i) model_push(s, e, -2 - i, 0.25, (uint8_t)((i == n - 1 || g() % 7 == 0) ? 1 : 0));
        if (n > S) t.prewrapped += 1;
    }
    std::vector<int32_t> ids;
    if (subset) {
        for (const Episode& e : table) if (g() % 3) ids.push_back(e.id);
        std::shuffle(ids.begin(), ids.end(), g);
        t.subsets += 1;
    }
    if (first_env) t.first_env += 1;
    Plan p;
    const int32_t none = 0;     // an empty list is a list (a null pointer means every episode)
    REQUIRE(plan(table, subset ? (ids.empty() ? &none : ids.data()) : nullptr, (int64_t)ids.size(), first_env, S, B, s.books, p));
    // the model
    Store m = s;
    std::vector<const Episode*> eps;
    if (!subset) for (const Episode& e : table) eps.push_back(&e);
    else for (int32_t id : ids) for (const Episode& e : table) if (e.id == id) eps.push_back(&e);
    int64_t pushed = 0;
    for (size_t j = 0; j < eps.size(); ++j) {
        const int e = (int)((first_env + (int64_t)j) % B);
        for (int32_t r = 0; r < eps[j]->rows; ++r, ++pushed)
            model_push(m, e, eps[j]->first + r, 0.5 + (double)(g() % 100), r == eps[j]->rows - 1 ? eps[j]->end : (uint8_t)0);
    }
    REQUIRE(p.rows == pushed);
    // the launch: jobs in a random order
    std::set<int64_t> written;
    std::vector<size_t> order(p.jobs.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    std::shuffle(order.begin(), order.end(), g);
    int64_t wrote = 0;
    for (size_t i : order) {
        const Job& j = p.jobs[i];
        REQUIRE(j.rows >= 1 && j.rows <= trajp::JOB_ROWS);
        REQUIRE(j.src >= 0 && j.src + j.rows <= archive_rows);
        REQUIRE(j.dst >= 0 && j.dst + j.rows <= S * B);
        REQUIRE(j.dst / S == (j.dst + j.rows - 1) / S);       // a run stays inside one sub-buffer
        for (int r = 0; r < j.rows; ++r) {
            REQUIRE(written.insert(j.dst + r).second);
            s.tag[(size_t)(j.dst + r)] = j.src + r;
        }
        wrote += j.rows;
    }
    REQUIRE(wrote == p.written && p.written + p.dropped == p.rows);
    apply_flags(p, s.flags.data());
    REQUIRE(s.tag == m.tag);
    REQUIRE(s.flags == m.flags);
    REQUIRE((int)p.books.size() == B);
    for (int e = 0; e < B; ++e) REQUIRE(same(p.books[(size_t)e], m.books[(size_t)e]));
    t.cases += 1; t.jobs += (int64_t)p.jobs.size();
    if (p.wrapped) t.wrapped += 1;
    if (p.dropped) t.dropped += 1;
}

static void refusals() {
    std::vector<Episode> table(3);
    for (int i = 0; i < 3; ++i) { table[(size_t)i].first = 10 * i; table[(size_t)i].rows = 4; table[(size_t)i].id = i; }
    std::vector<SubBook> books(2);
    Plan p;
    const int32_t unknown[2] = {0, 7}, twice[3] = {1, 2, 1}, good[2] = {2, 0};
    REQUIRE(!plan(table, unknown, 2, 0, 8, 2, books, p) && p.code == REFUSE_ARG && p.err.find("episode_ids[1] = 7") != std::string::npos);
    REQUIRE(!plan(table, twice, 3, 0, 8, 2, books, p) && p.code == REFUSE_ARG && p.err.find("twice") != std::string::npos);
    REQUIRE(!plan(table, good, 2, 2, 8, 2, books, p) && p.code == REFUSE_ARG && p.err.find("first_env") != std::string::npos);
    REQUIRE(!plan(table, good, 2, -1, 8, 2, books, p) && p.code == REFUSE_ARG && p.err.find("first_env") != std::string::npos);
    books[1].ep_len = 3;
    REQUIRE(!plan(table, good, 2, 0, 8, 2, books, p) && p.code == REFUSE_STATE && p.err.find("ep_len") != std::string::npos &&
            p.err.find("between collects") != std::string::npos);
    // one episode into sub-buffer 0 only: the busy sub-buffer 1 is no target
    REQUIRE(plan(table, good, 1, 0, 8, 2, books, p) && p.jobs.size() == 1 && p.rows == 4);
    REQUIRE(plan(table, nullptr, 0, 0, 8, 1, books, p) && p.rows == 12 && p.dropped == 4);
    std::vector<Episode> none;
    REQUIRE(plan(none, nullptr, 0, 0, 8, 2, books, p) && p.jobs.empty() && p.rows == 0);
    std::printf("ok refusals\n");
}

int main() {
    refusals();
    std::mt19937 g(20240607u);
    Tally t;
    // the lengths the cuts depend on: 1, exactly JOB_ROWS, JOB_ROWS + 1, longer than a sub-buffer
    {
        const int64_t S = 200;
        for (int B = 1; B <= 5; ++B)
            for (int prefill = 0; prefill < 3; ++prefill) {
                one_case(g, t, B, S, {1}, false, 0, prefill);
                one_case(g, t, B, S, {128}, false, B - 1, prefill);
                one_case(g, t, B, S, {129}, false, 0, prefill);
                one_case(g, t, B, S, {1, 128, 129, 1, 517, 1}, false, B / 2, prefill);
                one_case(g, t, B, S, {517}, false, 0, prefill);
                one_case(g, t, B, S, {200, 200, 201, 199, 400}, true, B - 1, prefill);
            }
    }
    for (int it = 0; it < 3000; ++it) {
        const int B = 1 + (int)(g() % 5);
        const int64_t S = 1 + (int64_t)(g() % (it % 3 == 0 ? 40 : 300));
        const int n = (int)(g() % 12);
        std::vector<int32_t> lens;
        for (int i = 0; i < n; ++i) {
            const unsigned k = g() % 8;
            lens.push_back(k == 0 ? 1 : k == 1 ? 128 : k == 2 ? 129 : k == 3 ? (int32_t)(S + 1 + (int64_t)(g() % (uint64_t)(2 * S)))
                                                                            : (int32_t)(1 + g() % 300));
        }
        one_case(g, t, B, S, lens, g() % 2 == 0, (int)(g() % (unsigned)B), (int)(g() % 3));
    }
    std::printf("ok cases n=%lld wrapped=%lld dropped=%lld jobs=%lld subsets=%lld first_env=%lld prewrapped=%lld\n", (long long)t.cases,
                (long long)t.wrapped, (long long)t.dropped, (long long)t.jobs, (long long)t.subsets, (long long)t.first_env,
                (long long)t.prewrapped);
    std::printf("ok all\n");
    return 0;
}
