// devcollect_wide_group_sim.cpp -- the block -> (member, tile) mapping and the batch sizing of the grouped wide collect
// (fsrl_amd/csrc/devcollect_plan.hpp) over ragged member lists, as a plain program (tests/test_devcollect_wide_group_host.py).
#include <cstdio>
#include <cstdlib>

#include "devcollect_plan.hpp"

#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

static void check(const int k, const int32_t* env_num, const int32_t* n_episode) {
    int32_t prefix[DCWG_MAX_MEMBERS + 1], b = 0, widest = 0;
    const int32_t grid = dc_wgroup_prefix(env_num, n_episode, k, prefix);
    for (int i = k; i <= DCWG_MAX_MEMBERS; ++i) REQUIRE(prefix[i] == grid);
    for (int m = 0; m < k; ++m) {           // walking the members' tiles in order gives every block once
        const int32_t live = dc_first_live(env_num[m], n_episode[m]);
        REQUIRE(prefix[m] == b && dc_wide_tiles(env_num[m], n_episode[m]) == (live + 15) / 16);
        for (int32_t t = 0; 16 * t < live; ++t, ++b) REQUIRE(dc_wgroup_member(prefix, b) == m && b - prefix[m] == t);
        widest = env_num[m] > widest ? env_num[m] : widest;
    }
    REQUIRE(b == grid);
    const int32_t asks[] = {0, 4, DC_MAX_STEPS};
    for (const int32_t asked : asks) {      // a batch fits the log of every member
        const int32_t S = dc_wgroup_batch_steps(env_num, k, asked);
        REQUIRE(S >= 1 && S == dc_wide_batch_steps(widest, asked) && (int64_t)S * widest <= DCW_MAX_LOG_ROWS);
    }
}

int main() {
    const int32_t one[] = {1}, ragged[] = {17, 4096, 1, 65, 16}, eps[] = {5, 9000, 1, 65, 3};
    int32_t full[DCWG_MAX_MEMBERS], full_ep[DCWG_MAX_MEMBERS];
    for (int i = 0; i < DCWG_MAX_MEMBERS; ++i) { full[i] = i % 2 ? DCW_MAX_ENVS : 1 + 16 * i; full_ep[i] = i % 3 ? DCW_MAX_ENVS : 7; }
    check(1, one, one);
    check(5, ragged, eps);
    check(DCWG_MAX_MEMBERS, full, full_ep);
    std::printf("ok all\n");
    return 0;
}
