// deveval_wide_sim.cpp -- the per-position episode-row rule of wide evaluations (devcollect_plan.hpp: dc_wide_episode_row,
// dc_wide_row_owner) against a sequential walk of dc_episode_end, as a plain program built with the address / undefined-behaviour
// sanitizers (tests/test_deveval_wide_host.py).  Whole evaluations of 1 .. DCW_MAX_ENVS envs, launch by launch as
// wide_eval_step_kernel runs them; every tile of a launch parks first and copies its rows afterwards -- the worst order the hardware
// may pick -- so a park held once, or by env id, fails.  Ends: random, all envs in every step, and ends that never reach a surplus.
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
struct Rec { int32_t env, step; };       // what identifies an episode: who ended it, in which step
// mode 0: random ends; 1: every live env ends in every step; 2: n_episode so large that no end meets a surplus before the call is cut
static long evaluation(int n, int n_episode, int mode, long* no_surplus, long* drops) {
    const int first = dc_first_live(n, n_episode), grid = (first + 15) / 16;
    std::vector<int32_t> live[2] = {std::vector<int32_t>((size_t)n), std::vector<int32_t>((size_t)n)}, seq((size_t)n);
    std::vector<uint8_t> done[2] = {std::vector<uint8_t>((size_t)n + 4, 1), std::vector<uint8_t>((size_t)n + 4, 1)};
    std::vector<Rec> park[2] = {std::vector<Rec>((size_t)n), std::vector<Rec>((size_t)n)}, log((size_t)n_episode, Rec{-1, -1}), want;
    for (int e = 0; e < n; ++e) live[0][(size_t)e] = seq[(size_t)e] = e;
    int n_live = first, lpar = 0, episodes = 0, pending = 0, seq_live = first, seq_eps = 0;
    for (int t = 0; t < 40 && !dc_complete(episodes, n_episode); ++t) {
        const int side = t & 1, nside = side ^ 1;
        // ---- the settle of step t - 1, as every workgroup computes it (ranks from wave totals and ballots: devcollect_wide_sim.cpp)
        int n_done = 0, surplus = 0;
        const int old_live = n_live, old_lpar = lpar, ep0 = episodes;
        std::vector<int32_t> rank((size_t)old_live, 0);
        if (pending) {
            for (int p = 0; p < old_live; ++p) { rank[(size_t)p] = n_done; n_done += done[side][(size_t)p] ? 1 : 0; }
            episodes += n_done;
            surplus = dc_wide_surplus(old_live, n_done, n_episode, episodes);
            if (surplus > 0) {
                for (int p = 0; p < old_live; ++p) {
                    if (dc_wide_leaves(done[side][(size_t)p] != 0, rank[(size_t)p], surplus)) continue;
                    live[lpar ^ 1][(size_t)dc_wide_new_pos(p, rank[(size_t)p], surplus)] = live[lpar][(size_t)p];
                }
                n_live = dc_wide_n_live(old_live, n_done, surplus); lpar ^= 1; ++*drops;
            } else if (n_done > 0) ++*no_surplus;
        }
        const bool go = !dc_complete(episodes, n_episode);
        // ---- this launch's own step first: flags and parked records of side t + 1, by position
        for (int p = 0; go && p < n_live; ++p) {
            const bool d = mode == 1 || (mode == 0 ? rnd(3) == 0 : rnd(16) == 0);
            done[nside][(size_t)p] = d;
            if (d) park[nside][(size_t)p] = Rec{live[lpar][(size_t)p], t};
        }
        // ---- ... then the rows of step t - 1, tile by tile of the FIXED grid, from the old list's positions
        for (int tile = 0; pending && tile < grid; ++tile)
            for (int p = 16 * tile; p < 16 * tile + 16 && p < old_live; ++p) {
                REQUIRE(dc_wide_row_owner(p, tile, false) && !dc_wide_row_owner(p, tile + 1, false) && dc_wide_row_owner(p, 0, true));
                const int row = dc_wide_episode_row(done[side][(size_t)p] != 0, ep0, rank[(size_t)p], n_episode);
                if (row < 0) continue;
                REQUIRE(row < n_episode && log[(size_t)row].env == -1);         // one writer per row
                log[(size_t)row] = park[side][(size_t)p];
                REQUIRE(log[(size_t)row].env == live[old_lpar][(size_t)p]);
            }
        REQUIRE(old_live <= 16 * grid);         // every old position has a workgroup
        if (pending) {                          // the sequential walk of the same step: episodes in position order, then dc_episode_end
            for (int p = 0; p < seq_live; ++p) if (done[side][(size_t)p]) want.push_back(Rec{seq[(size_t)p], t - 1});
            seq_live = dc_episode_end(seq.data(), seq_live, done[side].data(), n_episode, &seq_eps);
            REQUIRE(seq_live == n_live && seq_eps == episodes);
            for (int p = 0; p < n_live; ++p) REQUIRE(seq[(size_t)p] == live[lpar][(size_t)p]);
        }
        pending = go ? 1 : 0;
    }
    REQUIRE((int)want.size() == episodes && episodes <= n_episode);
    for (int i = 0; i < episodes; ++i) REQUIRE(log[(size_t)i].env == want[(size_t)i].env && log[(size_t)i].step == want[(size_t)i].step);
    for (int i = episodes; i < n_episode; ++i) REQUIRE(log[(size_t)i].env == -1);
    return episodes;
}

int main() {
    long cases = 0, eps = 0, no_surplus = 0, drops = 0, one_step = 0;
    const int sizes[] = {1, 2, 15, 16, 17, 64, 65, 100, 255, 256, 257, 1023, 1024, 1025, 1030, 4095, DCW_MAX_ENVS};
    for (int rep = 0; rep < 600; ++rep) {
        const int n = rep % 3 == 0 ? sizes[rnd(sizeof(sizes) / sizeof(sizes[0]))] : 1 + (int)rnd(DCW_MAX_ENVS), mode = rep % 4 == 3 ? 0 : rep % 4;
        const int n_episode = mode == 2 ? 100 * n : 1 + (int)rnd((uint32_t)(3 * n));
        eps += evaluation(n, n_episode, mode, &no_surplus, &drops);
        one_step += mode == 1; ++cases;
    }
    REQUIRE(eps > 0 && no_surplus > 0 && drops > 0 && one_step > 0);
    std::printf("ok rows cases=%ld episodes=%ld no_surplus=%ld drops=%ld one_step=%ld\nok all\n", cases, eps, no_surplus, drops, one_step);
    return 0;
}
