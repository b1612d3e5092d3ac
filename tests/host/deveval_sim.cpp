// deveval_sim.cpp -- the host replay of a device evaluation (fsrl_amd/csrc/devcollect_plan.hpp dc_eval_row) as a plain program
// (tests/test_deveval_host.py builds it with the address / undefined-behaviour sanitizers).
//   replay    random logs (1 .. 64 envs, rows of the envs interleaved as the kernel writes them: every live env once per vector step,
//             in position order; episode ends by termination, truncation or both; envs that leave the live set) through dc_eval_row
//             and through dc_replay_row over books and a flag mirror: the same episodes -- return bit for bit, length -- in the same
//             order; the evaluation's accumulators are all it writes (a guard band round them stays as it was), and the books of
//             the collect side are never given to it
//   restart   accumulators zeroed between evaluations: an evaluation cut in the middle of an episode leaves nothing behind
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "devcollect_plan.hpp"

#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

struct Book { int64_t index = 0, size = 0, last_index = 0; double ep_rew = 0.0; int32_t ep_len = 0; int64_t ep_idx = 0; };

static uint64_t g_s = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { g_s ^= g_s << 13; g_s ^= g_s >> 7; g_s ^= g_s << 17; return g_s; }
static double rnd_unit() { return (double)(rnd() >> 11) * (1.0 / 9007199254740992.0); }

// one log as the kernel writes it: vector steps over a live set that shrinks by the surplus rule
static std::vector<DcLogRow> make_log(int n, int n_episode, int max_len, long* ends) {
    std::vector<DcLogRow> log;
    int32_t live[DC_MAX_ENVS];
    int32_t t[DC_MAX_ENVS] = {};
    int32_t n_live = dc_first_live(n, n_episode), episodes = 0;
    for (int e = 0; e < n_live; ++e) live[e] = e;
    while (!dc_complete(episodes, n_episode)) {
        uint8_t done[DC_MAX_ENVS];
        for (int p = 0; p < n_live; ++p) {
            const int e = live[p];
            const bool term = rnd() % 9 == 0, trunc = dc_truncated(++t[e], max_len);
            DcLogRow r;
            r.env = e; r.flags = dc_flags(term, trunc);
            r.rew = 3.0 * rnd_unit() - 1.0; r.cost = rnd() % 4 == 0 ? 1.0 : 0.0;       // sums that round: the ORDER of additions shows
            log.push_back(r);
            done[p] = r.flags != 0u;
            if (done[p]) { t[e] = 0; ++*ends; }
        }
        n_live = dc_episode_end(live, n_live, done, n_episode, &episodes);
    }
    return log;
}

static void test_replay() {
    long logs = 0, rows = 0, episodes = 0, ends = 0, many_env_logs = 0;
    for (int round = 0; round < 400; ++round) {
        const int n = 1 + (int)(rnd() % DC_MAX_ENVS), n_episode = 1 + (int)(rnd() % 90), max_len = 1 + (int)(rnd() % 12);
        const std::vector<DcLogRow> log = make_log(n, n_episode, max_len, &ends);
        // the collect side: books over small sub-buffers that wrap, and the flag mirror
        const int64_t sub = 1 + (int64_t)(rnd() % 7);
        std::vector<Book> books((size_t)n);
        std::vector<uint8_t> h_flags((size_t)(n * sub), 0);
        // the evaluation side: the accumulators between two guard bands
        struct Guarded { uint8_t before[64]; DcEvalAcc acc[DC_MAX_ENVS]; uint8_t after[64]; };
        Guarded* g = new Guarded;
        std::memset(g->before, 0xA5, sizeof(g->before)); std::memset(g->after, 0x5A, sizeof(g->after));
        for (int e = 0; e < DC_MAX_ENVS; ++e) g->acc[e] = DcEvalAcc{0.0, 0};
        std::vector<double> cr, er_;
        std::vector<int32_t> cl, el_;
        for (const DcLogRow& r : log) {
            REQUIRE(r.env >= 0 && r.env < n);
            double a = 0.0, b = 0.0; int32_t la = 0, lb = 0;
            const bool dc = dc_replay_row(books[(size_t)r.env], sub, h_flags.data(), r, &a, &la);
            const bool de = dc_eval_row(g->acc[r.env], r, &b, &lb);
            REQUIRE(dc == de);
            if (dc) { cr.push_back(a); cl.push_back(la); }
            if (de) { er_.push_back(b); el_.push_back(lb); }
            // a running episode is the book's running episode, bit for bit
            REQUIRE(std::memcmp(&g->acc[r.env].ep_rew, &books[(size_t)r.env].ep_rew, sizeof(double)) == 0);
            REQUIRE(g->acc[r.env].ep_len == books[(size_t)r.env].ep_len);
        }
        REQUIRE(cr.size() == er_.size() && (int)cr.size() >= n_episode);
        REQUIRE(cr.empty() || std::memcmp(cr.data(), er_.data(), cr.size() * sizeof(double)) == 0);      // same order, same bits
        REQUIRE(cl == el_);
        for (size_t i = 0; i < sizeof(g->before); ++i) REQUIRE(g->before[i] == 0xA5 && g->after[i] == 0x5A);
        for (int e = n; e < DC_MAX_ENVS; ++e) REQUIRE(g->acc[e].ep_rew == 0.0 && g->acc[e].ep_len == 0);       // envs the log never named
        // the surplus rule leaves no episode open at the end of a collect: every accumulator is back at zero
        for (int e = 0; e < n; ++e) REQUIRE(g->acc[e].ep_rew == 0.0 && g->acc[e].ep_len == 0);
        delete g;
        ++logs; rows += (long)log.size(); episodes += (long)cr.size();
        many_env_logs += n > 16 ? 1 : 0;
    }
    REQUIRE(episodes == ends && many_env_logs > 0);
    std::printf("ok replay logs=%ld rows=%ld episodes=%ld many_env_logs=%ld\n", logs, rows, episodes, many_env_logs);
}

static void test_restart() {
    // an evaluation whose log is cut (a failed call) leaves running sums; the next one starts from zeroed accumulators and reports what
    // a fresh book reports
    long cut_open = 0;
    for (int round = 0; round < 100; ++round) {
        const int n = 1 + (int)(rnd() % 8);
        long ends = 0;
        const std::vector<DcLogRow> first = make_log(n, 5, 9, &ends), second = make_log(n, 7, 9, &ends);
        DcEvalAcc acc[DC_MAX_ENVS];
        for (int e = 0; e < DC_MAX_ENVS; ++e) acc[e] = DcEvalAcc{0.0, 0};
        double er = 0.0; int32_t el = 0;
        for (size_t i = 0; i < first.size() / 2; ++i) (void)dc_eval_row(acc[first[i].env], first[i], &er, &el);
        for (int e = 0; e < n; ++e) cut_open += acc[e].ep_len != 0 ? 1 : 0;
        for (int e = 0; e < DC_MAX_ENVS; ++e) acc[e] = DcEvalAcc{0.0, 0};          // what devcollect_begin does for an evaluation
        std::vector<Book> books((size_t)n);
        std::vector<uint8_t> h_flags((size_t)n * 64, 0);
        for (const DcLogRow& r : second) {
            double a = 0.0, b = 0.0; int32_t la = 0, lb = 0;
            const bool dc = dc_replay_row(books[(size_t)r.env], 64, h_flags.data(), r, &a, &la);
            const bool de = dc_eval_row(acc[r.env], r, &b, &lb);
            REQUIRE(dc == de && (!dc || (std::memcmp(&a, &b, sizeof(double)) == 0 && la == lb)));
        }
    }
    REQUIRE(cut_open > 0);
    std::printf("ok restart cut_open=%ld\n", cut_open);
}

int main() {
    test_replay();
    test_restart();
    std::printf("ok all\n");
    return 0;
}
