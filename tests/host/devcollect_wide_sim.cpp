// devcollect_wide_sim.cpp -- the per-position form of the surplus rule that wide_collect_step_kernel applies (fsrl_amd/csrc/
// devcollect_plan.hpp: dc_wide_surplus, dc_wide_leaves, dc_wide_new_pos, dc_wide_n_live) against dc_episode_end, as a plain program
// (tests/test_devcollect_wide_host.py builds it with the address / undefined-behaviour sanitizers).
// Random live lists of 1 .. DCW_MAX_ENVS positions, random flags (none, few, half, most, all) and n_episode on both sides of the
// surplus: every position decides for itself from (its flag, the finished positions in front of it) -- the ranks taken as the kernel
// takes them, wave totals of 256 positions plus the count inside the wave -- and the list, its length and the episode count are
// dc_episode_end's.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "devcollect_plan.hpp"

#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {       // xorshift64*: [0, n)
    g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
    return (uint32_t)((g_rng * 0x2545F4914F6CDD1Dull) >> 33) % n;
}

static void test_rule() {
    long cases = 0, none = 0, no_surplus = 0, drops = 0, multi_tile = 0;
    const int sizes[] = {1, 2, 15, 16, 17, 63, 64, 65, 100, 255, 256, 257, 1023, 1024, 1025, 4095, DCW_MAX_ENVS};
    for (int rep = 0; rep < 6000; ++rep) {
        const int n_live = rep % 3 == 0 ? sizes[rnd(sizeof(sizes) / sizeof(sizes[0]))] : 1 + (int)rnd(DCW_MAX_ENVS);
        std::vector<int32_t> live((size_t)n_live), want, got((size_t)n_live, -1);
        std::vector<uint8_t> done((size_t)n_live + 4, 1);          // the bytes behind the list are set: the kernel masks them
        for (int p = 0; p < n_live; ++p) live[(size_t)p] = (int32_t)rnd(DCW_MAX_ENVS);
        const int mode = rep % 5;       // no flag | a few | half | most | all
        for (int p = 0; p < n_live; ++p)
            done[(size_t)p] = mode == 0 ? 0 : mode == 1 ? rnd(64) == 0 : mode == 2 ? rnd(2) : mode == 3 ? rnd(8) != 0 : 1;
        int32_t n_done = 0;
        for (int p = 0; p < n_live; ++p) n_done += done[(size_t)p] ? 1 : 0;
        // n_episode - episodes_before around n_live + n_done: surplus below, at and above zero
        const int32_t episodes0 = (int32_t)rnd(50);
        const int32_t n_episode = episodes0 + 1 + (int32_t)rnd((uint32_t)(2 * n_live + 2));
        want = live;
        int32_t ep_want = episodes0;
        const int32_t n_want = dc_episode_end(want.data(), n_live, done.data(), n_episode, &ep_want);
        // ---- the per-position rule, ranks as the kernel forms them: wave totals (64 dwords = 256 positions), then inside the dword
        const int32_t ep_got = episodes0 + n_done;
        const int32_t surplus = dc_wide_surplus(n_live, n_done, n_episode, ep_got);
        std::vector<int32_t> wtot((size_t)(n_live / 256 + 1), 0);
        for (int p = 0; p < n_live; ++p) wtot[(size_t)(p >> 8)] += done[(size_t)p] ? 1 : 0;
        int32_t n_got = n_live, leavers = 0;
        if (surplus > 0) {
            int32_t in_wave = 0;
            for (int p = 0; p < n_live; ++p) {
                if ((p & 255) == 0) in_wave = 0;
                int32_t rank = in_wave;
                for (int w = 0; w < (p >> 8); ++w) rank += wtot[(size_t)w];
                in_wave += done[(size_t)p] ? 1 : 0;
                if (dc_wide_leaves(done[(size_t)p] != 0, rank, surplus)) { ++leavers; continue; }
                const int32_t q = dc_wide_new_pos(p, rank, surplus);
                REQUIRE(q >= 0 && q < n_live && got[(size_t)q] == -1);
                got[(size_t)q] = live[(size_t)p];
            }
            n_got = dc_wide_n_live(n_live, n_done, surplus);
            REQUIRE(leavers == n_live - n_got);
            if (leavers > 1 && n_live > 32) ++multi_tile;
        } else {
            got = live;
        }
        REQUIRE(n_got == n_want && ep_got == (n_done ? ep_want : episodes0));
        for (int p = 0; p < n_want; ++p) REQUIRE(got[(size_t)p] == want[(size_t)p]);
        REQUIRE(dc_complete(ep_got, n_episode) == (ep_got >= n_episode));
        none += n_done == 0; no_surplus += n_done > 0 && surplus == 0; drops += surplus > 0;
        ++cases;
    }
    REQUIRE(none > 0 && no_surplus > 0 && drops > 0 && multi_tile > 0);
    std::printf("ok rule cases=%ld none=%ld no_surplus=%ld drops=%ld multi_tile=%ld\n", cases, none, no_surplus, drops, multi_tile);
}

int main() {
    test_rule();
    std::printf("ok all\n");
    return 0;
}
