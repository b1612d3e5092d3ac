// devcollect_group_sim.cpp -- the plain host logic of a grouped device collect (fsrl_amd/csrc/devcollect_plan.hpp: dc_group_offsets,
// dc_launch_cap / dc_group_launch_cap, dc_group_stalled / dc_group_complete) as a plain program
// (tests/test_devcollect_group_host.py builds it with the address / undefined-behaviour sanitizers).
//   offsets   the members' episode arrays are concatenated in member order: against sums taken from scratch for every member, and
//             against writing every member's episodes through its offset into one array (no gap, no overlap)
//   cap       a member's launch cap against counting the launches of its longest possible collect (one env live, every episode
//             max_episode_steps long), one by one; the group's cap against the sorted list of the members' caps
//   stalled   the launch loop of fsrl_collect_device_group over members of random lengths: an honest loop never trips the rule and
//             ends inside the cap, finished members report 0 steps without tripping it, an injected stall names the lowest
//             unfinished member -- against a restatement with index lists
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "devcollect_plan.hpp"

#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)
#define MAX_GROUP 16

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {       // xorshift64*: [0, n)
    g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
    return (uint32_t)((g_rng * 0x2545F4914F6CDD1Dull) >> 33) % n;
}

static void test_offsets() {
    long cases = 0;
    for (int k = 1; k <= MAX_GROUP; ++k)
        for (int rep = 0; rep < 200; ++rep) {
            int32_t n_ep[MAX_GROUP];
            for (int i = 0; i < k; ++i) n_ep[i] = 1 + (int32_t)rnd(rep % 2 ? 5 : 300);
            int64_t off[MAX_GROUP + 1];
            dc_group_offsets(n_ep, k, off);
            for (int i = 0; i <= k; ++i) {
                int64_t want = 0;
                for (int j = 0; j < i; ++j) want += n_ep[j];
                REQUIRE(off[i] == want);
            }
            std::vector<int> owner((size_t)off[k], -1);
            for (int i = 0; i < k; ++i)
                for (int e = 0; e < n_ep[i]; ++e) {
                    REQUIRE(owner[(size_t)(off[i] + e)] == -1);
                    owner[(size_t)(off[i] + e)] = i;
                }
            for (size_t x = 0; x < owner.size(); ++x) REQUIRE(owner[x] >= 0 && (x == 0 || owner[x] >= owner[x - 1]));
            ++cases;
        }
    std::printf("ok offsets cases=%ld\n", cases);
}

static int64_t brute_cap(int n_episode, int max_episode_steps, int max_steps) {
    int64_t left = (int64_t)n_episode * max_episode_steps, launches = 0;      // the longest collect: one env live, every episode full length
    while (left > 0) { left -= std::min<int64_t>(left, max_steps); ++launches; }
    return launches + 1;
}

static void test_cap() {
    long cases = 0;
    for (int n_ep = 1; n_ep <= 40; n_ep += 3)
        for (int mes = 1; mes <= 300; mes = mes * 2 + 1)
            for (int ms : {1, 2, 3, 7, 8, 64, 65, 4096}) {
                REQUIRE(dc_launch_cap(n_ep, mes, ms) == brute_cap(n_ep, mes, ms));
                ++cases;
            }
    for (int k = 1; k <= MAX_GROUP; ++k)
        for (int rep = 0; rep < 100; ++rep) {
            int32_t n_ep[MAX_GROUP], mes[MAX_GROUP];
            const int ms = 1 + (int)rnd(70);
            std::vector<int64_t> caps;
            for (int i = 0; i < k; ++i) {
                n_ep[i] = 1 + (int32_t)rnd(80); mes[i] = 1 + (int32_t)rnd(300);
                caps.push_back(brute_cap(n_ep[i], mes[i], ms));
            }
            std::sort(caps.begin(), caps.end());
            REQUIRE(dc_group_launch_cap(n_ep, mes, k, ms) == caps.back());
            ++cases;
        }
    std::printf("ok cap cases=%ld\n", cases);
}

// the rule with index lists: the unfinished members going in, those of them that made no step, the lowest
static int brute_stalled(const std::vector<uint8_t>& was_finished, const std::vector<int32_t>& steps) {
    std::vector<int> unfinished, idle;
    for (size_t i = 0; i < steps.size(); ++i) if (!was_finished[i]) unfinished.push_back((int)i);
    for (int i : unfinished) if (steps[(size_t)i] == 0) idle.push_back(i);
    return idle.empty() ? -1 : *std::min_element(idle.begin(), idle.end());
}

static void test_stalled() {
    long loops = 0, idle_relaunches = 0, injected = 0;
    for (int k = 1; k <= MAX_GROUP; ++k)
        for (int rep = 0; rep < 150; ++rep) {
            const int ms = 1 + (int)rnd(16);
            int32_t n_ep[MAX_GROUP], mes[MAX_GROUP];
            std::vector<int64_t> left((size_t)k);
            for (int i = 0; i < k; ++i) {
                n_ep[i] = 1 + (int32_t)rnd(6); mes[i] = 1 + (int32_t)rnd(9);
                left[(size_t)i] = 1 + rnd((uint32_t)(n_ep[i] * mes[i]));        // vector steps this member's collect takes: <= n_episode x max_episode_steps
            }
            const int64_t cap = dc_group_launch_cap(n_ep, mes, k, ms);
            const int stall_at = rep % 3 == 0 ? (int)rnd(3) : -1;               // the launch at which one unfinished member stops stepping
            std::vector<uint8_t> finished((size_t)k, 0), was((size_t)k, 0);
            std::vector<int32_t> steps((size_t)k, 0);
            int64_t launches = 0;
            bool stalled_seen = false;
            for (;;) {
                REQUIRE(launches < cap);
                int victim = -1;
                if (launches == stall_at)
                    for (int i = 0; i < k && victim < 0; ++i) if (!finished[(size_t)i]) victim = i;
                for (int i = 0; i < k; ++i) {
                    was[(size_t)i] = finished[(size_t)i];
                    if (finished[(size_t)i]) { steps[(size_t)i] = 0; ++idle_relaunches; continue; }      // breaks at the loop's first test
                    steps[(size_t)i] = i == victim ? 0 : (int32_t)std::min<int64_t>(left[(size_t)i], ms);
                    left[(size_t)i] -= steps[(size_t)i];
                    finished[(size_t)i] = left[(size_t)i] == 0;
                }
                ++launches;
                const int got = dc_group_stalled(was.data(), steps.data(), k);
                REQUIRE(got == brute_stalled(was, steps));
                REQUIRE(got == victim);
                bool all = true;
                for (int i = 0; i < k; ++i) all = all && finished[(size_t)i];
                REQUIRE(dc_group_complete(finished.data(), k) == all);
                if (got >= 0) { stalled_seen = true; ++injected; break; }
                if (all) break;
            }
            REQUIRE(stalled_seen == (stall_at >= 0 && stall_at < launches));
            ++loops;
        }
    REQUIRE(idle_relaunches > 0 && injected > 0);
    std::printf("ok stalled loops=%ld idle_relaunches=%ld injected=%ld\n", loops, idle_relaunches, injected);
}

int main() {
    test_offsets();
    test_cap();
    test_stalled();
    std::printf("ok all\n");
    return 0;
}
