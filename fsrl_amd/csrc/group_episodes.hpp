// group_episodes.hpp -- the bookkeeping of a lock-step collect of k members over worker-process envs: FastCollector.collect(n_episode)
// of every member (fast_collector.py:283-368; one member: fsrl_collect_episodes, host_collect.inc) with the members' envs stepped
// TOGETHER and ONE step call per vector step for all of them -- GroupCollector's interpreted loop (fsrl_amd/data/group_collector.py),
// keyed by member.  Standard library only (no HIP, no fsrl_ctx): the owner supplies a view of every member's env block and two
// callbacks, so tests/host/group_episodes_sim.cpp drives it as a plain program (tests/test_group_episodes_host.py).
//   run_env(cmd, ids, &failed) -- post command `cmd` (GE_CMD_STEP: the actions are in the blocks already; GE_CMD_RESET) for the envs
//            ids[m] of every member m with a non-empty list, ALL members before the first wait, and return once all of them have
//            answered: 0, or an error with the member whose env failed in `failed`;
//   step(s) -- fsrl_group_collect_step / fsrl_collect_group_step: store every member's s.k[m] finished rows, evaluate its actor on
//            its s.k_act[m] rows of s.obs_act; row arrays concatenated over members: 0 or an error.
// Per member and vector step the calls are the ones its own collect makes, in its order: same rows in the same slots, same noise
// stream.  A member that has its episodes contributes k = 0, k_act = 0 from then on while the others go on.
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>

#define GE_CMD_STEP 1u
#define GE_CMD_RESET 2u
// argument errors (ge_collect's return; the member in *failed_member).  Callbacks return their own NEGATIVE codes, passed through.
enum { GE_OK = 0, GE_BAD_ROWS = 1,              // n[m] outside 1 .. env_num
       GE_BAD_EPISODES = 2,                     // n_episode[m] < 1
       GE_BAD_ID = 3,                           // an env id outside 0 .. env_num - 1
       GE_DUP_ID = 4 };                         // an env id listed twice

// a member's env block: what the workers write (obs, rew, cost, term, trunc: [env_num] rows) and what the collector writes (act)
struct GeEnvView {
    const float* obs; float* act; const double* rew; const double* cost; const uint8_t* term; const uint8_t* trunc;
    int env_num;
};
// one lock-step step, fsrl_group_collect_step's row arguments
struct GeStep {
    const int32_t* k; const int32_t* env_ids; const float* obs; const float* act; const double* rew; const double* cost;
    const uint8_t* terminated; const uint8_t* truncated; const float* obs_next; int64_t* ptr_out; double* ep_rew_out;
    int32_t* ep_len_out; int64_t* ep_idx_out; const int32_t* k_act; const float* obs_act; float* act_out; float* env_act_out;
};
// per member [k]; ep_rew / ep_len: n_episode[m] entries per member at prefix-sum offsets, in the order the loop met the episodes
struct GeOut {
    int64_t* steps; double* total_cost; int32_t* term; int32_t* trunc; double* ep_rew; int32_t* ep_len; int32_t* episodes;
};

// ready / obs: the members' rows back to back, n[m] rows each.  *failed_member: the member of an argument error or of a failed env
// command, -1 otherwise (a failed step call has no member).  After an env error NO further step call is made.
template <class RunEnv, class Step>
static int ge_collect(int members, const GeEnvView* envs, int Do_, int Da_, const int32_t* n, const int32_t* ready_in,
                      const float* obs_in, const int32_t* n_episode, const GeOut& out, RunEnv&& run_env, Step&& step,
                      int* failed_member) {
    const size_t Do = (size_t)Do_, Da = (size_t)Da_;
    struct Member {
        std::vector<int32_t> ready, nready, local;
        std::vector<float> obs, act, env_act, nxt;
        size_t ep_off = 0;                      // its slice of out.ep_rew / out.ep_len
        int n_episode = 0, episodes = 0, k_next = 0;
        bool live = true, last = false;
    };
    *failed_member = -1;
    std::vector<Member> mem((size_t)members);
    size_t cap = 0, ep_off = 0;
    for (int m = 0; m < members; ++m) {
        *failed_member = m;
        if (n[m] < 1 || n[m] > envs[m].env_num) return GE_BAD_ROWS;
        if (n_episode[m] < 1) return GE_BAD_EPISODES;
        std::vector<uint8_t> seen((size_t)envs[m].env_num, 0);
        for (int i = 0; i < n[m]; ++i) {
            const int32_t e = ready_in[cap + (size_t)i];
            if (e < 0 || e >= envs[m].env_num) return GE_BAD_ID;
            if (seen[(size_t)e]) return GE_DUP_ID;
            seen[(size_t)e] = 1;
        }
        Member& q = mem[(size_t)m];
        q.ready.assign(ready_in + cap, ready_in + cap + (size_t)n[m]);
        q.obs.assign(obs_in + cap * Do, obs_in + (cap + (size_t)n[m]) * Do);
        q.act.resize((size_t)n[m] * Da); q.env_act.resize((size_t)n[m] * Da);
        q.n_episode = n_episode[m]; q.ep_off = ep_off;
        out.steps[m] = 0; out.total_cost[m] = 0.0; out.term[m] = 0; out.trunc[m] = 0; out.episodes[m] = 0;
        cap += (size_t)n[m]; ep_off += (size_t)n_episode[m];
    }
    *failed_member = -1;
    // the step call's rows, concatenated over members (a member never has more rows than it started with)
    std::vector<int32_t> k((size_t)members), k_act((size_t)members), ids(cap), elen(cap);
    std::vector<float> obs(cap * Do), act(cap * Da), obs_next(cap * Do), obs_act(cap * Do), act_out(cap * Da), env_act_out(cap * Da);
    std::vector<double> rew(cap), cost(cap), erew(cap);
    std::vector<uint8_t> term(cap), trunc(cap);
    std::vector<int64_t> ptr(cap), eidx(cap);
    std::vector<std::vector<int32_t>> cmd_ids((size_t)members);
    const GeStep s{k.data(), ids.data(), obs.data(), act.data(), rew.data(), cost.data(), term.data(), trunc.data(), obs_next.data(),
                   ptr.data(), erew.data(), elen.data(), eidx.data(), k_act.data(), obs_act.data(), act_out.data(), env_act_out.data()};
    // a member's new actions: its k_act rows of the step's outputs
    auto take_actions = [&]() {
        size_t oa = 0;
        for (int m = 0; m < members; ++m) {
            Member& q = mem[(size_t)m];
            const size_t ka = (size_t)k_act[(size_t)m];
            q.act.assign(act_out.begin() + oa * Da, act_out.begin() + (oa + ka) * Da);
            q.env_act.assign(env_act_out.begin() + oa * Da, env_act_out.begin() + (oa + ka) * Da);
            oa += ka;
        }
    };
    // the first actions: nothing to store yet
    for (int m = 0; m < members; ++m) { k[(size_t)m] = 0; k_act[(size_t)m] = n[m]; }
    memcpy(obs_act.data(), obs_in, cap * Do * 4);
    int rc = step(s);
    if (rc) return rc;
    take_actions();
    for (;;) {
        bool any_live = false;
        for (int m = 0; m < members; ++m) {
            Member& q = mem[(size_t)m];
            cmd_ids[(size_t)m].clear();
            if (!q.live) continue;
            any_live = true;
            for (size_t i = 0; i < q.ready.size(); ++i)
                memcpy(envs[m].act + (size_t)q.ready[i] * Da, q.env_act.data() + i * Da, Da * 4);
            cmd_ids[(size_t)m] = q.ready;
        }
        if (!any_live) break;
        // ---- env.step(env_act, ready) of every live member at once
        rc = run_env(GE_CMD_STEP, cmd_ids, failed_member);
        if (rc) return rc;
        // ---- results of the step; the envs whose episode ended
        size_t o = 0;
        bool any_done = false;
        for (int m = 0; m < members; ++m) {
            Member& q = mem[(size_t)m];
            cmd_ids[(size_t)m].clear();
            k[(size_t)m] = 0;
            if (!q.live) continue;
            const GeEnvView& v = envs[m];
            const size_t kk = q.ready.size();
            k[(size_t)m] = (int32_t)kk;
            q.local.clear();
            memcpy(obs.data() + o * Do, q.obs.data(), kk * Do * 4);
            memcpy(act.data() + o * Da, q.act.data(), kk * Da * 4);
            for (size_t i = 0; i < kk; ++i) {
                const size_t e = (size_t)q.ready[i], r = o + i;
                ids[r] = q.ready[i];
                rew[r] = v.rew[e]; cost[r] = v.cost[e]; term[r] = v.term[e]; trunc[r] = v.trunc[e];
                memcpy(obs_next.data() + r * Do, v.obs + e * Do, Do * 4);
                out.total_cost[m] += cost[r];
                if (term[r] || trunc[r]) { q.local.push_back((int32_t)i); cmd_ids[(size_t)m].push_back(q.ready[i]); }
                out.term[m] += term[r] ? 1 : 0; out.trunc[m] += trunc[r] ? 1 : 0;
            }
            out.steps[m] += (int64_t)kk;
            any_done = any_done || !q.local.empty();
            o += kk;
        }
        // ---- env.reset(finished envs) of every member that has some, at once
        if (any_done) {
            rc = run_env(GE_CMD_RESET, cmd_ids, failed_member);
            if (rc) return rc;
        }
        // ---- per member: the observations to act on -- reset ones in place, surplus envs dropped (fast_collector.py:341-362: the
        //      first `surplus` finished envs of the step leave); none once the member has its episodes
        o = 0;
        size_t oa = 0;
        for (int m = 0; m < members; ++m) {
            Member& q = mem[(size_t)m];
            k_act[(size_t)m] = 0;
            if (!q.live) continue;
            const GeEnvView& v = envs[m];
            const size_t kk = q.ready.size();
            q.nxt.assign(obs_next.begin() + o * Do, obs_next.begin() + (o + kk) * Do);
            q.nready = q.ready;
            q.last = false;
            if (!q.local.empty()) {
                const int n_done = (int)q.local.size();
                for (int32_t i : q.local) memcpy(q.nxt.data() + (size_t)i * Do, v.obs + (size_t)q.ready[(size_t)i] * Do, Do * 4);
                const int surplus = (int)kk - (q.n_episode - q.episodes - n_done);
                if (surplus > 0) {
                    std::vector<uint8_t> drop(kk, 0);
                    for (int j = 0; j < surplus && j < n_done; ++j) drop[(size_t)q.local[(size_t)j]] = 1;
                    size_t w = 0;
                    for (size_t i = 0; i < kk; ++i) {
                        if (drop[i]) continue;
                        q.nready[w] = q.ready[i];
                        if (w != i) memmove(q.nxt.data() + w * Do, q.nxt.data() + i * Do, Do * 4);
                        ++w;
                    }
                    q.nready.resize(w); q.nxt.resize(w * Do);
                }
                q.last = q.episodes + n_done >= q.n_episode;
            }
            q.k_next = q.last ? 0 : (int)q.nready.size();
            k_act[(size_t)m] = q.k_next;
            memcpy(obs_act.data() + oa * Do, q.nxt.data(), (size_t)q.k_next * Do * 4);
            o += kk; oa += (size_t)q.k_next;
        }
        // ---- buffer.add(rows) + policy(obs) + noise + map_action of every member: ONE call
        rc = step(s);
        if (rc) return rc;
        take_actions();
        o = 0;
        for (int m = 0; m < members; ++m) {
            Member& q = mem[(size_t)m];
            if (!q.live) continue;
            const size_t kk = q.ready.size();
            for (int32_t i : q.local) {
                if (q.episodes < q.n_episode) {
                    out.ep_rew[q.ep_off + (size_t)q.episodes] = erew[o + (size_t)i];
                    out.ep_len[q.ep_off + (size_t)q.episodes] = elen[o + (size_t)i];
                }
                q.episodes += 1;
            }
            out.episodes[m] = q.episodes < q.n_episode ? q.episodes : q.n_episode;
            o += kk;
            if (q.last) { q.live = false; continue; }
            q.ready.swap(q.nready);
            q.obs.swap(q.nxt);
        }
    }
    return GE_OK;
}
