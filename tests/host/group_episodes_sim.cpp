// group_episodes_sim.cpp -- fsrl_amd/csrc/group_episodes.hpp (the bookkeeping of fsrl_group_collect_episodes /
// fsrl_collect_episodes_group) as a plain program: fake envs, a fake step call that records what every member is asked to store and
// to act on, and for comparison a single-member collect loop written out here on its own (the rule of FastCollector's fused loop,
// fast_collector.py:283-368: reset the finished envs, drop the first `surplus` of them, stop at n_episode) that does not go through
// the header.  A member's record under the group must equal its record alone ("k1" is fsrl_collect_episodes' own loop: ge_collect
// with one member).  The split loop (ge_collect_split, fsrl_collect_episodes_split) runs against a two-lane loop written out here
// the way FastCollector._collect_split has it: every request, post and wait, in order.  Exits 0 and prints "ok ..." per case.
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>

#include "group_episodes.hpp"

static const int Do = 5, Da = 2;

static uint32_t mix(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    uint32_t h = 2166136261u;
    for (uint32_t x : {a, b, c, d}) { h ^= x + 0x9e3779b9u + (h << 6) + (h >> 2); h *= 16777619u; }
    return h;
}
static float unit(uint32_t h) { return (float)(h % 2001u) / 1000.0f - 1.0f; }

// a fake vector env: everything a function of (member, env, tick), tick = commands this env has seen; the reward also depends on
// the action found in the env's slot, so an action written to the wrong slot shows
struct FakeEnv {
    int member, env_num, ep_len, stagger;
    std::vector<float> obs, act;
    std::vector<double> rew, cost;
    std::vector<uint8_t> term, trunc;
    std::vector<int> tick, t;
    FakeEnv(int member_, int env_num_, int ep_len_, int stagger_)
        : member(member_), env_num(env_num_), ep_len(ep_len_), stagger(stagger_), obs((size_t)env_num_ * Do), act((size_t)env_num_ * Da, -7.f),
          rew((size_t)env_num_), cost((size_t)env_num_), term((size_t)env_num_), trunc((size_t)env_num_), tick((size_t)env_num_, 0),
          t((size_t)env_num_, 0) {
        for (int e = 0; e < env_num; ++e) fill_obs(e);
    }
    int len_of(int e) const { return ep_len + (stagger ? e % 3 : 0); }
    void fill_obs(int e) {
        for (int d = 0; d < Do; ++d) obs[(size_t)e * Do + d] = unit(mix((uint32_t)member, (uint32_t)e, (uint32_t)tick[(size_t)e], (uint32_t)d));
    }
    void step(int e) {
        tick[(size_t)e] += 1; t[(size_t)e] += 1;
        fill_obs(e);
        const uint32_t h = mix((uint32_t)member, (uint32_t)e, (uint32_t)tick[(size_t)e], 99u);
        rew[(size_t)e] = (double)unit(h) + (double)act[(size_t)e * Da] + 2.0 * (double)act[(size_t)e * Da + 1];
        cost[(size_t)e] = (double)(h % 3u == 0u);
        const bool done = t[(size_t)e] >= len_of(e);
        term[(size_t)e] = done && (h % 2u == 0u); trunc[(size_t)e] = done && !term[(size_t)e];
    }
    void reset(int e) { tick[(size_t)e] += 1; t[(size_t)e] = 0; fill_obs(e); }
    GeEnvView view() { return GeEnvView{obs.data(), act.data(), rew.data(), cost.data(), term.data(), trunc.data(), env_num}; }
};

// the fake "store + actor" of one member: records every request, keeps the store's episode accumulators, answers with actions that
// depend on the member, on how many requests it has seen (its "noise stream") and on the observation row
struct FakeAgent {
    int member, calls = 0;
    std::vector<double> acc_rew;
    std::vector<int> acc_len;
    std::vector<double> log;                    // every number of every request, in order
    FakeAgent(int member_, int env_num) : member(member_), acc_rew((size_t)env_num, 0.0), acc_len((size_t)env_num, 0) {}
    void request(int k, const int32_t* ids, const float* obs, const float* act, const double* rew, const double* cost, const uint8_t* term,
                 const uint8_t* trunc, const float* obs_next, double* ep_rew, int32_t* ep_len, int k_act, const float* obs_act,
                 float* act_out, float* env_act_out) {
        if (k == 0 && k_act == 0) return;
        log.push_back(-1000.0 - calls); log.push_back(k); log.push_back(k_act);
        for (int i = 0; i < k; ++i) {
            const size_t e = (size_t)ids[i];
            log.push_back(ids[i]);
            for (int d = 0; d < Do; ++d) log.push_back(obs[(size_t)i * Do + d]);
            for (int d = 0; d < Da; ++d) log.push_back(act[(size_t)i * Da + d]);
            log.push_back(rew[i]); log.push_back(cost[i]); log.push_back(term[i]); log.push_back(trunc[i]);
            for (int d = 0; d < Do; ++d) log.push_back(obs_next[(size_t)i * Do + d]);
            acc_rew[e] += rew[i]; acc_len[e] += 1;
            ep_rew[i] = 0.0; ep_len[i] = 0;
            if (term[i] || trunc[i]) { ep_rew[i] = acc_rew[e]; ep_len[i] = acc_len[e]; acc_rew[e] = 0.0; acc_len[e] = 0; }
        }
        for (int i = 0; i < k_act; ++i) {
            for (int d = 0; d < Do; ++d) log.push_back(obs_act[(size_t)i * Do + d]);
            for (int d = 0; d < Da; ++d) {
                const float a = 0.25f * obs_act[(size_t)i * Do + d] + 0.01f * (float)((calls * 7 + i * 3 + d + member) % 13);
                act_out[(size_t)i * Da + d] = a;
                env_act_out[(size_t)i * Da + d] = 0.5f * a + 0.125f;
            }
        }
        calls += 1;
    }
};

struct Result {
    long long steps = 0; double total_cost = 0.0; int term = 0, trunc = 0, episodes = 0;
    std::vector<double> ep_rew; std::vector<int> ep_len;
    std::vector<double> log;
};

// ---- one member alone, not through the header: arrays and masks the way the interpreted loop has them
static Result collect_alone(int member, int env_num, int ep_len, int stagger, int n_start, int n_episode) {
    FakeEnv env(member, env_num, ep_len, stagger);
    FakeAgent agent(member, env_num);
    Result r;
    std::vector<int32_t> ready;
    for (int i = 0; i < n_start; ++i) ready.push_back(i);
    std::vector<float> obs((size_t)n_start * Do);
    for (int i = 0; i < n_start; ++i) std::copy(env.obs.begin() + (size_t)i * Do, env.obs.begin() + (size_t)(i + 1) * Do, obs.begin() + (size_t)i * Do);
    std::vector<float> act((size_t)n_start * Da), env_act((size_t)n_start * Da);
    agent.request(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, n_start, obs.data(),
                  act.data(), env_act.data());
    while (true) {
        const int k = (int)ready.size();
        for (int i = 0; i < k; ++i)
            for (int d = 0; d < Da; ++d) env.act[(size_t)ready[(size_t)i] * Da + d] = env_act[(size_t)i * Da + d];
        for (int i = 0; i < k; ++i) env.step(ready[(size_t)i]);
        std::vector<double> rew((size_t)k), cost((size_t)k), ep_rew((size_t)k);
        std::vector<uint8_t> term((size_t)k), trunc((size_t)k);
        std::vector<int32_t> ep_len_((size_t)k);
        std::vector<float> obs_next((size_t)k * Do);
        std::vector<int> local;
        for (int i = 0; i < k; ++i) {
            const size_t e = (size_t)ready[(size_t)i];
            rew[(size_t)i] = env.rew[e]; cost[(size_t)i] = env.cost[e]; term[(size_t)i] = env.term[e]; trunc[(size_t)i] = env.trunc[e];
            for (int d = 0; d < Do; ++d) obs_next[(size_t)i * Do + d] = env.obs[e * Do + d];
            r.total_cost += cost[(size_t)i];
            if (term[(size_t)i] || trunc[(size_t)i]) local.push_back(i);
            r.term += term[(size_t)i]; r.trunc += trunc[(size_t)i];
        }
        r.steps += k;
        std::vector<float> nxt = obs_next;
        std::vector<int32_t> nready = ready;
        bool last = false;
        if (!local.empty()) {
            const int n_done = (int)local.size();
            for (int i : local) {
                env.reset(ready[(size_t)i]);
                for (int d = 0; d < Do; ++d) nxt[(size_t)i * Do + d] = env.obs[(size_t)ready[(size_t)i] * Do + d];
            }
            const int surplus = k - (n_episode - r.episodes - n_done);
            if (surplus > 0) {
                std::vector<bool> mask((size_t)k, true);
                for (int j = 0; j < std::min(surplus, n_done); ++j) mask[(size_t)local[(size_t)j]] = false;
                std::vector<float> nx2;
                std::vector<int32_t> nr2;
                for (int i = 0; i < k; ++i)
                    if (mask[(size_t)i]) {
                        nr2.push_back(ready[(size_t)i]);
                        nx2.insert(nx2.end(), nxt.begin() + (size_t)i * Do, nxt.begin() + (size_t)(i + 1) * Do);
                    }
                nxt = nx2; nready = nr2;
            }
            last = r.episodes + n_done >= n_episode;
        }
        const int k_act = last ? 0 : (int)nready.size();
        std::vector<float> act_new((size_t)k_act * Da), env_act_new((size_t)k_act * Da);
        agent.request(k, ready.data(), obs.data(), act.data(), rew.data(), cost.data(), term.data(), trunc.data(), obs_next.data(),
                      ep_rew.data(), ep_len_.data(), k_act, nxt.data(), act_new.data(), env_act_new.data());
        for (int i : local) { r.ep_rew.push_back(ep_rew[(size_t)i]); r.ep_len.push_back(ep_len_[(size_t)i]); r.episodes += 1; }
        if (last) break;
        ready = nready; obs = nxt; act = act_new; env_act = env_act_new;
    }
    r.log = agent.log;
    return r;
}

struct Spec { int env_num, ep_len, stagger, n_episode; };

#define REQUIRE(cond, ...) do { if (!(cond)) { printf("FAILED %s: ", name); printf(__VA_ARGS__); printf("\n"); return 1; } } while (0)

// ---- the group through the header.  fail_member >= 0: the env callback fails for that member at its fail_step-th step command
static int run_case(const char* name, const std::vector<Spec>& specs, int fail_member = -1, int fail_step = 0) {
    const int members = (int)specs.size();
    std::vector<FakeEnv> envs;
    std::vector<FakeAgent> agents;
    std::vector<GeEnvView> views;
    std::vector<int32_t> n, ready, n_episode;
    std::vector<float> obs;
    size_t ep_total = 0;
    for (int m = 0; m < members; ++m) {
        envs.emplace_back(m, specs[(size_t)m].env_num, specs[(size_t)m].ep_len, specs[(size_t)m].stagger);
        agents.emplace_back(m, specs[(size_t)m].env_num);
    }
    for (int m = 0; m < members; ++m) {
        views.push_back(envs[(size_t)m].view());
        const int start = std::min(specs[(size_t)m].env_num, specs[(size_t)m].n_episode);     // fewer episodes than envs: fewer envs start
        n.push_back(start); n_episode.push_back(specs[(size_t)m].n_episode);
        for (int i = 0; i < start; ++i) ready.push_back(i);
        obs.insert(obs.end(), envs[(size_t)m].obs.begin(), envs[(size_t)m].obs.begin() + (size_t)start * Do);
        ep_total += (size_t)specs[(size_t)m].n_episode;
    }
    std::vector<int64_t> steps((size_t)members);
    std::vector<double> total_cost((size_t)members), ep_rew(ep_total, -1.0);
    std::vector<int32_t> term((size_t)members), trunc((size_t)members), episodes((size_t)members), ep_len(ep_total, -1);
    const GeOut out{steps.data(), total_cost.data(), term.data(), trunc.data(), ep_rew.data(), ep_len.data(), episodes.data()};
    int step_cmds = 0, step_calls = 0, env_cmds = 0, step_calls_at_failure = -1, failed = -2;
    std::vector<uint8_t> finished((size_t)members, 0);
    bool rows_after_finish = false;
    const int rc = ge_collect(
        members, views.data(), Do, Da, n.data(), ready.data(), obs.data(), n_episode.data(), out,
        [&](uint32_t cmd, const std::vector<std::vector<int32_t>>& ids, int* bad) {
            env_cmds += 1;
            if (cmd == GE_CMD_STEP) step_cmds += 1;
            for (int m = 0; m < members; ++m) {
                if (cmd == GE_CMD_STEP && m == fail_member && step_cmds == fail_step && !ids[(size_t)m].empty()) {
                    *bad = m;
                    step_calls_at_failure = step_calls;
                    return -1;
                }
                for (int32_t e : ids[(size_t)m]) { if (cmd == GE_CMD_STEP) envs[(size_t)m].step(e); else envs[(size_t)m].reset(e); }
            }
            return 0;
        },
        [&](const GeStep& s) {
            step_calls += 1;
            size_t o = 0, oa = 0;
            for (int m = 0; m < members; ++m) {
                const size_t k = (size_t)s.k[m], ka = (size_t)s.k_act[m];
                if (finished[(size_t)m] && (k || ka)) rows_after_finish = true;
                agents[(size_t)m].request((int)k, s.env_ids + o, s.obs + o * Do, s.act + o * Da, s.rew + o, s.cost + o, s.terminated + o,
                                          s.truncated + o, s.obs_next + o * Do, s.ep_rew_out + o, s.ep_len_out + o, (int)ka,
                                          s.obs_act + oa * Do, s.act_out + oa * Da, s.env_act_out + oa * Da);
                if (k && !ka) finished[(size_t)m] = 1;
                o += k; oa += ka;
            }
            return 0;
        },
        &failed);
    if (fail_member >= 0) {
        REQUIRE(rc == -1 && failed == fail_member, "rc %d, failed member %d (expected -1, %d)", rc, failed, fail_member);
        REQUIRE(step_calls == step_calls_at_failure, "a step call after the env error: %d calls, %d at the failure", step_calls, step_calls_at_failure);
        REQUIRE(step_calls == fail_step, "%d step calls before the failure, expected %d (the first actions + %d steps)", step_calls, fail_step, fail_step - 1);
        printf("ok  %s: stopped at step command %d without a further step call, member %d named\n", name, fail_step, failed);
        return 0;
    }
    REQUIRE(rc == 0 && failed == -1, "rc %d, failed member %d", rc, failed);
    REQUIRE(!rows_after_finish, "a member that had its episodes was given rows again");
    size_t off = 0;
    long long total_steps = 0;
    for (int m = 0; m < members; ++m) {
        const Spec& sp = specs[(size_t)m];
        const Result ref = collect_alone(m, sp.env_num, sp.ep_len, sp.stagger, n[(size_t)m], sp.n_episode);
        REQUIRE(ref.episodes == sp.n_episode, "member %d alone: %d episodes, wanted %d", m, ref.episodes, sp.n_episode);
        REQUIRE(agents[(size_t)m].log == ref.log, "member %d: its requests differ from its own collect's (%zu vs %zu numbers)", m,
                agents[(size_t)m].log.size(), ref.log.size());
        REQUIRE(steps[(size_t)m] == ref.steps && total_cost[(size_t)m] == ref.total_cost && term[(size_t)m] == ref.term &&
                trunc[(size_t)m] == ref.trunc && episodes[(size_t)m] == ref.episodes,
                "member %d: counts differ (steps %lld / %lld, episodes %d / %d)", m, (long long)steps[(size_t)m], ref.steps,
                episodes[(size_t)m], ref.episodes);
        for (int j = 0; j < ref.episodes; ++j)
            REQUIRE(ep_rew[off + (size_t)j] == ref.ep_rew[(size_t)j] && ep_len[off + (size_t)j] == ref.ep_len[(size_t)j],
                    "member %d: episode %d differs", m, j);
        off += (size_t)sp.n_episode;
        total_steps += ref.steps;
    }
    printf("ok  %s: %d members, %lld env steps, %d step calls, %d env commands, every member's requests equal its own collect's\n", name,
           members, total_steps, step_calls, env_cmds);
    return 0;
}

static int run_refusals() {
    const char* name = "refusals";
    FakeEnv a(0, 4, 3, 0), b(1, 3, 3, 0);
    const GeEnvView views[2] = {a.view(), b.view()};
    std::vector<float> obs((size_t)7 * Do, 0.f);
    int64_t steps[2]; double cost[2], ep_rew[8]; int32_t term[2], trunc[2], eps[2], ep_len[8];
    const GeOut out{steps, cost, term, trunc, ep_rew, ep_len, eps};
    int calls = 0;
    auto env_cb = [&](uint32_t, const std::vector<std::vector<int32_t>>&, int*) { calls += 1; return 0; };
    auto step_cb = [&](const GeStep&) { calls += 1; return 0; };
    struct { int32_t n[2]; int32_t ready[7]; int32_t ne[2]; int want, member; } cases[] = {
        {{4, 4}, {0, 1, 2, 3, 0, 1, 2}, {4, 4}, GE_BAD_ROWS, 1},
        {{0, 3}, {0, 1, 2, 3, 0, 1, 2}, {4, 4}, GE_BAD_ROWS, 0},
        {{4, 3}, {0, 1, 2, 3, 0, 1, 2}, {4, 0}, GE_BAD_EPISODES, 1},
        {{4, 3}, {0, 1, 2, 3, 0, 3, 2}, {4, 4}, GE_BAD_ID, 1},
        {{4, 3}, {0, 1, 1, 3, 0, 1, 2}, {4, 4}, GE_DUP_ID, 0},
    };
    for (auto& c : cases) {
        int failed = -2;
        const int rc = ge_collect(2, views, Do, Da, c.n, c.ready, obs.data(), c.ne, out, env_cb, step_cb, &failed);
        REQUIRE(rc == c.want && failed == c.member, "rc %d member %d, expected %d member %d", rc, failed, c.want, c.member);
    }
    REQUIRE(calls == 0, "a refused call reached a callback");
    printf("ok  refusals: row counts, episode counts, env ids out of range and listed twice, with the member\n");
    return 0;
}

// ---- the split loop (ge_collect_split).  One env whose envs sit on two lanes; a posted command takes effect only when its lane is
// waited for, so results read before the wait, or actions put into the slots of a lane that is stepping, show.  Posts and waits go
// into the agent's log between its requests: ONE record of everything the loop does, in order.
struct LaneEnv {
    FakeEnv env;
    FakeAgent agent;
    std::vector<int32_t> lane;                  // of every env
    struct Pending { bool on = false; uint32_t cmd = 0; std::vector<int32_t> ids; } pend[2];
    int posts = 0, waits = 0, step_waits[2] = {0, 0};
    bool misuse = false;                        // a post onto a busy lane or for another lane's env, a wait on an idle lane
    LaneEnv(const std::vector<int32_t>& lane_, int ep_len, int stagger)
        : env(0, (int)lane_.size(), ep_len, stagger), agent(0, (int)lane_.size()), lane(lane_) {}
    void post(int l, const int32_t* ids, int n, uint32_t cmd) {
        posts += 1;
        agent.log.push_back(-2000.0 - l); agent.log.push_back(cmd); agent.log.push_back(n);
        if (pend[l].on) misuse = true;
        for (int i = 0; i < n; ++i) { agent.log.push_back(ids[i]); if (lane[(size_t)ids[i]] != l) misuse = true; }
        pend[l].on = true; pend[l].cmd = cmd; pend[l].ids.assign(ids, ids + n);
    }
    void wait(int l) {
        waits += 1;
        agent.log.push_back(-3000.0 - l);
        if (!pend[l].on) { misuse = true; return; }
        if (pend[l].cmd == GE_CMD_STEP) step_waits[l] += 1;
        for (int32_t e : pend[l].ids) { if (pend[l].cmd == GE_CMD_STEP) env.step(e); else env.reset(e); }
        pend[l].on = false;
    }
    void reset_all() { for (int e = 0; e < env.env_num; ++e) env.reset(e); }        // FastCollector.reset_env between two collects
};

// the two-lane loop written out the way FastCollector._collect_split has it (groups with ready / obs / act / busy, masks, a global
// episode count), not through the header
static Result split_alone(LaneEnv& w, int n_start, int n_episode) {
    struct Group { std::vector<int32_t> ready; std::vector<float> obs, act; bool busy = false; } groups[2];
    Result r;
    int episode_count = 0;
    auto step_async = [&](int l, const std::vector<float>& env_act, const std::vector<int32_t>& ids) {
        for (size_t i = 0; i < ids.size(); ++i)
            for (int d = 0; d < Da; ++d) w.env.act[(size_t)ids[i] * Da + d] = env_act[i * Da + d];
        w.post(l, ids.data(), (int)ids.size(), GE_CMD_STEP);
    };
    for (int l = 0; l < 2; ++l) {
        Group& g = groups[l];
        for (int e = 0; e < n_start; ++e)
            if (w.lane[(size_t)e] == l) {
                g.ready.push_back(e);
                g.obs.insert(g.obs.end(), w.env.obs.begin() + (size_t)e * Do, w.env.obs.begin() + (size_t)(e + 1) * Do);
            }
        if (g.ready.empty()) continue;
        const int k = (int)g.ready.size();
        std::vector<float> env_act((size_t)k * Da);
        g.act.resize((size_t)k * Da);
        w.agent.request(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, k, g.obs.data(),
                        g.act.data(), env_act.data());
        step_async(l, env_act, g.ready);
        g.busy = true;
    }
    while (episode_count < n_episode) {
        if (!groups[0].busy && !groups[1].busy) { printf("split_alone: no env left but episodes are missing\n"); exit(2); }
        for (int l = 0; l < 2; ++l) {
            Group& g = groups[l];
            if (!g.busy) continue;
            const std::vector<int32_t> rdy = g.ready;
            const int k = (int)rdy.size();
            w.wait(l);
            g.busy = false;
            std::vector<double> rew((size_t)k), cost((size_t)k), ep_rew((size_t)k);
            std::vector<uint8_t> term((size_t)k), trunc((size_t)k);
            std::vector<int32_t> ep_len((size_t)k);
            std::vector<float> obs_next((size_t)k * Do);
            std::vector<int> local;
            for (int i = 0; i < k; ++i) {
                const size_t e = (size_t)rdy[(size_t)i];
                rew[(size_t)i] = w.env.rew[e]; cost[(size_t)i] = w.env.cost[e]; term[(size_t)i] = w.env.term[e]; trunc[(size_t)i] = w.env.trunc[e];
                for (int d = 0; d < Do; ++d) obs_next[(size_t)i * Do + d] = w.env.obs[e * Do + d];
                r.total_cost += cost[(size_t)i];
                if (term[(size_t)i] || trunc[(size_t)i]) local.push_back(i);
            }
            r.steps += k;
            std::vector<float> nxt = obs_next;
            std::vector<int32_t> nready = rdy;
            if (!local.empty()) {
                const int n_done = (int)local.size();
                for (int i : local) { r.term += term[(size_t)i]; r.trunc += trunc[(size_t)i]; }
                std::vector<int32_t> reset_ids;
                for (int i : local) reset_ids.push_back(rdy[(size_t)i]);
                w.post(l, reset_ids.data(), n_done, GE_CMD_RESET);                    // env.reset(rdy[local]): this lane is idle
                w.wait(l);
                for (int i : local)
                    for (int d = 0; d < Do; ++d) nxt[(size_t)i * Do + d] = w.env.obs[(size_t)rdy[(size_t)i] * Do + d];
                const int active = (int)(groups[0].ready.size() + groups[1].ready.size());
                const int surplus = active - (n_episode - episode_count - n_done);
                if (surplus > 0) {
                    std::vector<bool> mask((size_t)k, true);
                    for (int j = 0; j < std::min(surplus, n_done); ++j) mask[(size_t)local[(size_t)j]] = false;
                    std::vector<float> nx2;
                    std::vector<int32_t> nr2;
                    for (int i = 0; i < k; ++i)
                        if (mask[(size_t)i]) {
                            nr2.push_back(rdy[(size_t)i]);
                            nx2.insert(nx2.end(), nxt.begin() + (size_t)i * Do, nxt.begin() + (size_t)(i + 1) * Do);
                        }
                    nxt = nx2; nready = nr2;
                }
            }
            const int k_act = (int)nready.size();
            std::vector<float> act_new((size_t)k_act * Da), env_act_new((size_t)k_act * Da);
            w.agent.request(k, rdy.data(), g.obs.data(), g.act.data(), rew.data(), cost.data(), term.data(), trunc.data(), obs_next.data(),
                            ep_rew.data(), ep_len.data(), k_act, k_act ? nxt.data() : nullptr, act_new.data(), env_act_new.data());
            for (int i : local) { r.ep_rew.push_back(ep_rew[(size_t)i]); r.ep_len.push_back(ep_len[(size_t)i]); }
            episode_count += (int)local.size();
            g.ready = nready; g.obs = nxt; g.act = act_new;
            if (k_act) { step_async(l, env_act_new, nready); g.busy = true; }
        }
    }
    for (int l = 0; l < 2; ++l)
        if (groups[l].busy) { w.wait(l); groups[l].busy = false; }
    r.episodes = episode_count;
    return r;
}

struct Collect { int n_start, n_episode; };     // n_start < 0: min(env_num, n_episode), as FastCollector starts

// the collects back to back on one env and agent, through the header and through split_alone.  fail_lane >= 0: the wait of that
// lane's fail_step-th step fails (first collect).  want_trailing >= 0: waits after the last step call of the first collect
static int run_split(const char* name, const std::vector<int32_t>& lane, int ep_len, int stagger, const std::vector<Collect>& collects,
                     int fail_lane = -1, int fail_step = 0, int want_trailing = -1) {
    LaneEnv w(lane, ep_len, stagger), ref(lane, ep_len, stagger);
    long long total_steps = 0;
    for (const Collect& c : collects) {
        const int n = c.n_start < 0 ? std::min((int)lane.size(), c.n_episode) : c.n_start;
        std::vector<int32_t> ready;
        for (int i = 0; i < n; ++i) ready.push_back(i);
        const std::vector<float> obs(w.env.obs.begin(), w.env.obs.begin() + (size_t)n * Do);
        int64_t steps = -1; double total_cost = -1.0; int32_t term = -1, trunc = -1, episodes = -1;
        std::vector<double> ep_rew((size_t)c.n_episode, -1.0);
        std::vector<int32_t> ep_len_((size_t)c.n_episode, -1);
        const GeOut out{&steps, &total_cost, &term, &trunc, ep_rew.data(), ep_len_.data(), &episodes};
        bool busy[2] = {true, true}, null_obs_act_with_rows = false, obs_act_without_rows = false;
        int step_calls = 0, calls_at_failure = -1, waits_at_last_step = 0;
        const int rc = ge_collect_split(
            w.env.view(), lane.data(), Do, Da, n, ready.data(), obs.data(), c.n_episode, out,
            [&](int l, const int32_t* ids, int k, uint32_t cmd) { w.post(l, ids, k, cmd); return 0; },
            [&](int l) {
                if (l == fail_lane && w.pend[l].on && w.pend[l].cmd == GE_CMD_STEP && w.step_waits[l] + 1 == fail_step) {
                    calls_at_failure = step_calls + w.posts;
                    return -1;
                }
                w.wait(l);
                return 0;
            },
            [&](const GeStep& s) {
                step_calls += 1; waits_at_last_step = w.waits;
                if (s.k_act[0] && !s.obs_act) { null_obs_act_with_rows = true; return -2; }
                if (!s.k_act[0] && s.obs_act) obs_act_without_rows = true;
                w.agent.request(s.k[0], s.env_ids, s.obs, s.act, s.rew, s.cost, s.terminated, s.truncated, s.obs_next, s.ep_rew_out,
                                s.ep_len_out, s.k_act[0], s.obs_act, s.act_out, s.env_act_out);
                return 0;
            },
            busy);
        REQUIRE(!w.misuse, "a post onto a busy lane or for another lane's env, or a wait on an idle lane");
        REQUIRE(!null_obs_act_with_rows && !obs_act_without_rows, "obs_act must be null exactly when no row is left to act on");
        if (fail_lane >= 0) {
            REQUIRE(rc == -1, "rc %d, expected the wait's -1", rc);
            REQUIRE(busy[1 - fail_lane] && !busy[fail_lane], "busy %d %d: the other lane is posted, the failed one is not", busy[0], busy[1]);
            REQUIRE(w.pend[1 - fail_lane].on, "the other lane was not posted when the wait failed");
            REQUIRE(step_calls + w.posts == calls_at_failure, "a post or step call after the failed wait");
            printf("ok  %s: lane %d's wait failed at its step %d, lane %d reported busy, no further post or step call\n", name, fail_lane,
                   fail_step, 1 - fail_lane);
            return 0;
        }
        REQUIRE(rc == 0 && !busy[0] && !busy[1], "rc %d, busy %d %d", rc, busy[0], busy[1]);
        REQUIRE(!w.pend[0].on && !w.pend[1].on, "a command is still in flight after the loop");
        if (want_trailing >= 0)
            REQUIRE(w.waits - waits_at_last_step == want_trailing, "%d waits after the last step call, expected %d", w.waits - waits_at_last_step,
                    want_trailing);
        const Result r = split_alone(ref, n, c.n_episode);
        REQUIRE(r.episodes >= c.n_episode, "the written-out loop: %d episodes, wanted %d", r.episodes, c.n_episode);
        REQUIRE(w.agent.log == ref.agent.log, "n_episode %d: requests, posts and waits differ from the written-out loop's (%zu vs %zu numbers)",
                c.n_episode, w.agent.log.size(), ref.agent.log.size());
        REQUIRE(steps == r.steps && total_cost == r.total_cost && term == r.term && trunc == r.trunc && episodes == c.n_episode,
                "n_episode %d: counts differ (steps %lld / %lld, episodes %d)", c.n_episode, (long long)steps, r.steps, episodes);
        for (int j = 0; j < c.n_episode; ++j)
            REQUIRE(ep_rew[(size_t)j] == r.ep_rew[(size_t)j] && ep_len_[(size_t)j] == r.ep_len[(size_t)j], "n_episode %d: episode %d differs",
                    c.n_episode, j);
        total_steps += r.steps;
        w.reset_all(); ref.reset_all();
    }
    printf("ok  %s: %zu collects, %lld env steps, %d posts, %d waits, every request, post and wait equals the written-out loop's\n", name,
           collects.size(), total_steps, w.posts, w.waits);
    return 0;
}

static int run_split_refusals() {
    const char* name = "split refusals";
    FakeEnv a(0, 4, 3, 0);
    std::vector<float> obs((size_t)5 * Do, 0.f);
    int64_t steps; double cost, ep_rew[4]; int32_t term, trunc, eps, ep_len[4];
    const GeOut out{&steps, &cost, &term, &trunc, ep_rew, ep_len, &eps};
    int calls = 0;
    auto post_cb = [&](int, const int32_t*, int, uint32_t) { calls += 1; return 0; };
    auto wait_cb = [&](int) { calls += 1; return 0; };
    auto step_cb = [&](const GeStep&) { calls += 1; return 0; };
    struct { int32_t n; int32_t ready[5]; int32_t lane[4]; int32_t ne; int want; } cases[] = {
        {5, {0, 1, 2, 3, 0}, {0, 0, 1, 1}, 4, GE_BAD_ROWS},
        {0, {0, 1, 2, 3, 0}, {0, 0, 1, 1}, 4, GE_BAD_ROWS},
        {4, {0, 1, 2, 3, 0}, {0, 0, 1, 1}, 0, GE_BAD_EPISODES},
        {4, {0, 1, 4, 3, 0}, {0, 0, 1, 1}, 4, GE_BAD_ID},
        {4, {0, 1, -1, 3, 0}, {0, 0, 1, 1}, 4, GE_BAD_ID},
        {4, {0, 1, 1, 3, 0}, {0, 0, 1, 1}, 4, GE_DUP_ID},
        {4, {0, 1, 2, 3, 0}, {0, 0, 2, 1}, 4, GE_BAD_LANE},
    };
    for (auto& c : cases) {
        bool busy[2] = {true, true};
        const int rc = ge_collect_split(a.view(), c.lane, Do, Da, c.n, c.ready, obs.data(), c.ne, out, post_cb, wait_cb, step_cb, busy);
        REQUIRE(rc == c.want && !busy[0] && !busy[1], "rc %d (busy %d %d), expected %d", rc, busy[0], busy[1], c.want);
    }
    REQUIRE(calls == 0, "a refused call reached a callback");
    printf("ok  split refusals: row counts, episode counts, env ids out of range and listed twice, a lane that is neither 0 nor 1\n");
    return 0;
}

int main() {
    int bad = 0;
    bad += run_case("k3", {{17, 5, 0, 20}, {3, 7, 0, 6}, {4, 4, 0, 2}});
    bad += run_case("k3 staggered", {{17, 5, 1, 20}, {3, 7, 1, 6}, {4, 4, 1, 2}});
    bad += run_case("k1", {{17, 5, 1, 20}});
    bad += run_case("one member's episodes all end in the same step", {{6, 4, 0, 6}, {5, 3, 1, 11}});
    bad += run_case("env failure", {{17, 5, 0, 20}, {3, 7, 0, 6}, {4, 4, 0, 2}}, 1, 3);
    bad += run_refusals();
    const std::vector<int32_t> even{0, 0, 0, 1, 1, 1}, uneven{0, 0, 0, 0, 0, 1}, mixed{0, 1, 1, 0, 1, 1};
    bad += run_split("split basic", even, 19, 0, {{-1, 6}, {-1, 10}, {-1, 3}, {-1, 1}, {-1, 7}, {-1, 12}});
    bad += run_split("split uneven lanes", uneven, 19, 0, {{-1, 6}, {-1, 10}, {-1, 7}});
    bad += run_split("split one lane empty", even, 19, 0, {{3, 5}, {3, 3}});
    bad += run_split("split staggered", even, 19, 1, {{-1, 6}, {-1, 10}, {-1, 7}, {-1, 12}});
    // both lanes finish 3 episodes in the same round with 4 wanted: lane 1 finds 1 left for its 3 and drops them all
    bad += run_split("split both lanes in one round", even, 19, 0, {{6, 4}, {6, 5}});
    // lane 0 = the envs of length 19, which give the 2 episodes; lane 1 (20, 21) has just been posted again: one trailing wait
    bad += run_split("split fewer episodes than envs", mixed, 19, 1, {{6, 2}}, -1, 0, 1);
    bad += run_split("split failing wait", even, 19, 0, {{-1, 6}}, 1, 3);
    bad += run_split_refusals();
    if (bad) { printf("%d case(s) FAILED\n", bad); return 1; }
    printf("ok  all\n");
    return 0;
}
