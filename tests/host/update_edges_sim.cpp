// update_edges_sim.cpp -- the host-side decisions of fsrl_ppo_begin's edges (fsrl_amd/csrc/host_decisions.hpp) as a plain program:
// the packed upload's layout, the split of process_fn's workgroups between full and next jobs, the host count of coinciding rows.
// Prints one "ok <name> ..." line per check and exits non-zero at the first failure (tests/test_update_edges_host.py).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "host_decisions.hpp"

#define REQUIRE(c, ...) do { if (!(c)) { printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); return 1; } } while (0)

static int check_layout() {
    long cases = 0;
    const size_t ns[] = {1, 2, 15, 16, 17, 63, 64, 65, 129, 1000, 20000, 100020};
    for (size_t n : ns)
        for (size_t nseg : {(size_t)1, (size_t)3, (size_t)20, n})
            for (size_t nmb : {(size_t)1, (size_t)2, (size_t)78, n}) {
                if (nseg > n || nmb > n) continue;
                const UploadLayout u = upload_layout(n, nseg, nmb);
                // the head is fixed: control block, counter, then the indices -- whatever n is
                REQUIRE(u.ctrl == 0 && u.miss_count == 64 && u.indices == UPLOAD_HEAD, "head n=%zu", n);
                const size_t off[] = {u.ctrl, u.miss_count, u.indices, u.end, u.seg, u.mb_start, u.mb_size, u.total};
                const size_t len[] = {24, 4, n * 4, n, (nseg + 1) * 4, nmb * 4, nmb * 4};
                for (int i = 0; i < 7; ++i) {
                    REQUIRE(off[i] % 64 == 0, "array %d of n=%zu starts at %zu", i, n, off[i]);
                    REQUIRE(off[i] + len[i] <= off[i + 1], "array %d of n=%zu overlaps the next", i, n);
                    REQUIRE(off[i + 1] - off[i] < len[i] + 64 || i < 2, "array %d of n=%zu: more than alignment between arrays", i, n);
                }
                // a store of `rows` rows holds every update of at most that many rows
                for (size_t rows : {n, n + 20, 2 * n}) REQUIRE(u.total <= upload_capacity(rows), "capacity rows=%zu n=%zu", rows, n);
                ++cases;
            }
    printf("ok upload_layout cases=%ld\n", cases);
    return 0;
}

static int check_split() {
    long cases = 0, equal = 0;
    for (int n_cus : {64, 104, 256, 304})
        for (int C : {1, 2, 3, 4})
            for (int actor : {0, 1})
                for (int n_tiles : {1, 2, 7, 9, 51, 52, 1250, 6252}) {
                    const int jobs_y = 2 * C + actor, F = jobs_y - C, gx = infer_grid_x(n_tiles, n_cus, jobs_y);
                    REQUIRE(gx >= 1 && gx <= n_tiles && (long)gx * jobs_y <= std::max(n_cus, jobs_y), "grid n_cus=%d", n_cus);
                    int last_bn = 0;
                    std::vector<int> ms;          // list sizes in tiles, ascending: all of them for a small batch, a spread for a large one
                    if (n_tiles < 64) for (int m = 0; m <= n_tiles; ++m) ms.push_back(m);
                    else ms = {0, 1, 2, 3, 4, 8, 50, n_tiles / 10, n_tiles / 2, n_tiles - 3, n_tiles - 1, n_tiles};
                    for (int m : ms) {
                        const InferSplit s = infer_split(gx, jobs_y, C, n_tiles, m);
                        REQUIRE(C * s.bn + F * s.bf <= gx * jobs_y, "more workgroups than the launch has: m=%d", m);
                        REQUIRE(s.bf >= gx && s.bf <= n_tiles && s.bf >= 1, "full jobs never get fewer than the equal split: bf=%d gx=%d", s.bf, gx);
                        REQUIRE(s.bn <= gx && s.bn <= m && (m == 0) == (s.bn == 0), "bn=%d m=%d gx=%d", s.bn, m, gx);
                        REQUIRE(s.bn >= last_bn, "bn falls as the list grows: m=%d", m);
                        REQUIRE(s.equal == (s.bn == gx && s.bf == gx), "equal flag m=%d", m);
                        if (m == n_tiles) { REQUIRE(s.equal, "no coinciding rows must give the equal split: n_tiles=%d gx=%d bn=%d", n_tiles, gx, s.bn); ++equal; }
                        last_bn = s.bn;
                        ++cases;
                        if (m == n_tiles) break;
                    }
                }
    // the headline shape: 20 000 rows, two critics and the actor on 256 CUs, 20 rows listed
    const InferSplit h = infer_split(infer_grid_x(1250, 256, 5), 5, 2, 1250, 2);
    REQUIRE(h.bn == 1 && h.bf == 84 && !h.equal, "headline split bn=%d bf=%d", h.bn, h.bf);
    // the GPU test's shape: 129 rows (9 tiles), one tile listed
    const InferSplit t = infer_split(infer_grid_x(9, 256, 5), 5, 2, 9, 1);
    REQUIRE(t.bn == 1 && t.bf == 9 && !t.equal, "test split bn=%d bf=%d", t.bn, t.bf);
    printf("ok infer_split cases=%ld equal_at_full_list=%ld headline=%d/%d\n", cases, equal, h.bn, h.bf);
    return 0;
}

static int check_count() {
    const int n = 6, Do = 3;
    float obs[n * Do], nxt[n * Do];
    for (int i = 0; i < n * Do; ++i) obs[i] = (float)(i + 1);
    for (int r = 0; r + 1 < n; ++r) memcpy(nxt + r * Do, obs + (r + 1) * Do, Do * sizeof(float));
    for (int k = 0; k < Do; ++k) nxt[(n - 1) * Do + k] = -1.0f;
    uint32_t o[n * Do], x[n * Do];
    memcpy(o, obs, sizeof(o)); memcpy(x, nxt, sizeof(x));
    REQUIRE(next_same_count(o, x, n, Do) == n - 1, "contiguous");
    obs[2 * Do + 1] = 0.0f; nxt[1 * Do + 1] = -0.0f;                    // equal as floats, not as words
    memcpy(o, obs, sizeof(o)); memcpy(x, nxt, sizeof(x));
    REQUIRE(next_same_count(o, x, n, Do) == n - 2, "sign of zero");
    REQUIRE(next_same_count(o, x, 1, Do) == 0 && next_same_count(o, x, 0, Do) == 0, "short batches");
    printf("ok next_same_count\n");
    return 0;
}

int main() {
    if (check_layout() || check_split() || check_count()) return 1;
    return 0;
}
