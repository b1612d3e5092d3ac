// devcollect_sim.cpp -- the decisions and the host replay of a device collect (fsrl_amd/csrc/devcollect_plan.hpp) as a plain program
// (tests/test_devcollect_host.py builds it with the address / undefined-behaviour sanitizers).
//   surplus   dc_episode_end against a brute-force restatement of fsrl/data/fast_collector.py:341-362 with index vectors and masks,
//             for every env_num <= 6, n_episode <= 8 and every pattern of episode ends over 4 vector steps
//   replay    a log of rows through dc_replay_row against direct bookkeeping (a list of rows per sub-buffer), sub-buffers that wrap
//             several times included: index, size, last_index, running and finished episode statistics, the flag mirror
//   limits    dc_truncated, dc_first_live, dc_slot / dc_next_index at the edges
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "devcollect_plan.hpp"

#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

// fast_collector.py:341-362, literally: ready / local / mask
struct Brute {
    std::vector<int> ready;
    int episodes = 0;
    void step(const std::vector<uint8_t>& done, int n_episode) {
        std::vector<int> local;
        for (size_t p = 0; p < ready.size(); ++p) if (done[p]) local.push_back((int)p);
        if (local.empty()) return;
        episodes += (int)local.size();
        const int surplus = (int)ready.size() - (n_episode - episodes);
        if (surplus > 0) {
            std::vector<uint8_t> mask(ready.size(), 1);
            for (int i = 0; i < surplus && i < (int)local.size(); ++i) mask[(size_t)local[(size_t)i]] = 0;      // mask[local[:surplus]] = False
            std::vector<int> keep;
            for (size_t p = 0; p < ready.size(); ++p) if (mask[p]) keep.push_back(ready[p]);
            ready.swap(keep);
        }
    }
};

// every pattern of ends over the steps that are left: at each step every subset of the LIVE positions (a pattern's bits beyond the
// live count mean nothing), depth first; a collect that is complete takes no further step
static long g_cases = 0, g_dropped = 0, g_finished = 0;
static void walk(const Brute& b0, const int32_t* live0, int32_t n_live0, int32_t episodes0, int n_episode, int steps_left) {
    if (steps_left == 0 || dc_complete(episodes0, n_episode)) { ++g_cases; return; }
    for (int bits = 0; bits < (1 << n_live0); ++bits) {
        Brute b = b0;
        int32_t live[DC_MAX_ENVS];
        std::memcpy(live, live0, sizeof(int32_t) * (size_t)n_live0);
        int32_t episodes = episodes0;
        uint8_t done[DC_MAX_ENVS];
        for (int p = 0; p < n_live0; ++p) done[p] = (uint8_t)((bits >> p) & 1);
        b.step(std::vector<uint8_t>(done, done + n_live0), n_episode);
        const int32_t n_live = dc_episode_end(live, n_live0, done, n_episode, &episodes);
        g_dropped += n_live0 - n_live;
        REQUIRE(episodes == b.episodes);
        REQUIRE(n_live == (int32_t)b.ready.size());
        for (int p = 0; p < n_live; ++p) REQUIRE(live[p] == b.ready[(size_t)p]);
        REQUIRE(episodes <= n_episode);                                     // never more episodes than asked for
        REQUIRE(n_live <= n_episode - episodes);                            // ... and never more live envs than episodes still wanted
        if (dc_complete(episodes, n_episode)) { REQUIRE(episodes == n_episode && n_live == 0); ++g_finished; }
        walk(b, live, n_live, episodes, n_episode, steps_left - 1);
    }
}

static long test_surplus() {
    for (int env_num = 1; env_num <= 6; ++env_num)
        for (int n_episode = 1; n_episode <= 8; ++n_episode) {
            const int n0 = dc_first_live(env_num, n_episode);
            REQUIRE(n0 == (env_num < n_episode ? env_num : n_episode));
            Brute b;
            int32_t live[DC_MAX_ENVS];
            for (int e = 0; e < n0; ++e) { b.ready.push_back(e); live[e] = e; }
            walk(b, live, n0, 0, n_episode, 4);
        }
    const long cases = g_cases, dropped = g_dropped, finished = g_finished;
    REQUIRE(dropped > 0 && finished > 0);
    std::printf("ok surplus cases=%ld dropped=%ld finished=%ld\n", cases, dropped, finished);
    return cases;
}

struct Book { int64_t index = 0, size = 0, last_index = 0; double ep_rew = 0.0; int32_t ep_len = 0; int64_t ep_idx = 0; };

static void test_replay() {
    const int env_num = 5;
    const int64_t sub = 7;                        // short sub-buffers: every one wraps several times
    std::vector<Book> book((size_t)env_num);
    std::vector<uint8_t> h_flags((size_t)(env_num * sub), 0);
    // direct bookkeeping: every row of every env, in order
    struct Row { double rew; uint32_t fl; };
    std::vector<std::vector<Row>> all((size_t)env_num);
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    long rows = 0, episodes = 0, wraps = 0;
    for (int step = 0; step < 200; ++step) {
        for (int e = 0; e < env_num; ++e) {
            if (rnd() % 4 == 0) continue;                         // not every env is live in every step
            DcLogRow r;
            r.env = e; r.rew = (double)(rnd() % 1000) / 7.0 - 50.0; r.cost = (double)(rnd() % 2);
            const unsigned k = (unsigned)(rnd() % 9);
            r.flags = k == 0 ? 1u : k == 1 ? 2u : k == 2 ? 3u : 0u;
            Book& b = book[(size_t)e];
            const int64_t slot = dc_slot(e, sub, (int32_t)b.index);
            REQUIRE(slot == e * sub + b.index);
            REQUIRE(dc_next_index((int32_t)b.index, sub) == (b.index + 1) % sub);
            if (b.index + 1 == sub) ++wraps;
            double er = -1.0; int32_t el = -1;
            const bool done = dc_replay_row(b, sub, h_flags.data(), r, &er, &el);
            all[(size_t)e].push_back(Row{r.rew, r.flags});
            ++rows;
            // ---- against the direct form
            const std::vector<Row>& mine = all[(size_t)e];
            const int64_t n = (int64_t)mine.size();
            REQUIRE(b.index == n % sub);
            REQUIRE(b.size == (n < sub ? n : sub));
            REQUIRE(b.last_index == (n - 1) % sub);
            REQUIRE(h_flags[(size_t)(e * sub + (n - 1) % sub)] == (uint8_t)r.flags);
            // the running and the last finished episode: walk the env's rows from the start, summing in order
            double acc = 0.0; int32_t len = 0; int64_t ep_first = 0; double last_er = 0.0; int32_t last_el = 0;
            for (int64_t i = 0; i < n; ++i) {
                acc += mine[(size_t)i].rew; ++len;
                if (mine[(size_t)i].fl != 0) { last_er = acc; last_el = len; acc = 0.0; len = 0; ep_first = i + 1; }
            }
            REQUIRE(done == (r.flags != 0));
            if (done) { REQUIRE(er == last_er && el == last_el); ++episodes; }
            else { REQUIRE(er == -1.0 && el == -1); }
            REQUIRE(b.ep_rew == acc && b.ep_len == len);
            if (done) REQUIRE(b.ep_idx == ep_first % sub);
        }
    }
    REQUIRE(wraps > 20 && episodes > 50);
    std::printf("ok replay rows=%ld episodes=%ld wraps=%ld\n", rows, episodes, wraps);
}

static void test_limits() {
    REQUIRE(!dc_truncated(6, 7) && dc_truncated(7, 7) && dc_truncated(8, 7) && dc_truncated(1, 1));
    REQUIRE(dc_flags(false, false) == 0u && dc_flags(true, false) == 1u && dc_flags(false, true) == 2u && dc_flags(true, true) == 3u);
    REQUIRE(dc_first_live(64, 1) == 1 && dc_first_live(1, 64) == 1 && dc_first_live(64, 64) == 64);
    REQUIRE(dc_slot(63, 1000000, 999999) == 63999999ll && dc_next_index(999999, 1000000) == 0 && dc_next_index(0, 1) == 0);
    // all 64 envs end at once with one episode wanted: one episode is counted per finished env, every env leaves
    int32_t live[DC_MAX_ENVS]; uint8_t done[DC_MAX_ENVS];
    for (int e = 0; e < DC_MAX_ENVS; ++e) { live[e] = e; done[e] = 1; }
    int32_t episodes = 0;
    const int32_t n = dc_episode_end(live, 1, done, 1, &episodes);
    REQUIRE(n == 0 && episodes == 1 && dc_complete(episodes, 1));
    REQUIRE(sizeof(DcLogRow) == 24);
    std::printf("ok limits\n");
}

int main() {
    test_limits();
    test_surplus();
    test_replay();
    std::printf("ok all\n");
    return 0;
}
