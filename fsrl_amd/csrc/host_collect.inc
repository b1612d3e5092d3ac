// host_collect.inc -- the collector's hot loop over the worker-process env, native (part of fsrl_hip.hip).
//
// Reference: FastCollector.collect (fsrl/data/fast_collector.py:252-368) runs, per vector step, the policy forward, the
// exploration noise, map_action, env.step over the worker pipes, buffer.add and the reset / surplus bookkeeping in Python.
// fsrl_collect_step already folds forward + noise + map_action + buffer.add into one library call; what was left per
// step was the interpreter: the env's handshake wrappers, the gather / scatter of the rows, the loop itself (~35 us of
// the ~60 us a vector step of the zero-cost env took).  fsrl_collect_run keeps going in C for as long as NOTHING the
// interpreter must decide happens: it writes the actions into the env's shared block, posts the step to the workers'
// lanes (the futex handshake of fsrl_amd/env/csrc/fsrl_env.c, compiled into this library as static functions), sleeps
// until they are done, stores the transitions and evaluates the actor on the new observations -- and returns at the
// first vector step in which an episode ends (or after max_steps), with that step's results NOT yet stored: the reset
// of the finished envs and the dropping of surplus envs (fast_collector.py:341-362) stay where they were.
#define FSRL_ENV_API static
#include "../env/csrc/fsrl_env.c"
static double mono_seconds() {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

// ---- liveness: a worker that raised writes its error word before it leaves (fsrl_amd/env/shmem.py), one that was killed is
// found with waitid(WNOWAIT) on its pid (the collector is its parent).  Returns the first dead / failed worker of `ws`, or -1.
#include <sys/wait.h>
#include <signal.h>
// error words only (no syscall): what the success path of a wait looks at
static int shm_err_worker(const fsrl_shm_env* env, const std::vector<int32_t>& ws) {
    if (!env->err) return -1;
    for (int32_t w : ws)
        if (__atomic_load_n(env->err + (size_t)w * 16, __ATOMIC_ACQUIRE) != 0u) return w;
    return -1;
}
static int shm_failed_worker(const fsrl_shm_env* env, const std::vector<int32_t>& ws) {
    const int e = shm_err_worker(env, ws);
    if (e >= 0) return e;
    for (int32_t w : ws) {
        if (env->pids && env->pids[w] > 0) {
            siginfo_t si; si.si_pid = 0;
            const int wr = waitid(P_PID, (id_t)env->pids[w], &si, WEXITED | WNOHANG | WNOWAIT);
            if (wr == 0 && si.si_pid == env->pids[w]) return w;          // exited, not yet reaped
            // ECHILD: not OUR child (forkserver start method, SIGCHLD ignored) or already reaped -- ask the kernel whether
            // the pid still exists instead of assuming death (a live worker of a fork server must not fail a slow step)
            if (wr != 0 && errno == ECHILD && kill((pid_t)env->pids[w], 0) != 0 && errno == ESRCH) return w;
        }
    }
    return -1;
}
// wait for a lane's command: sleeps on the completion word in slices of 500 ms and looks at the workers between them, so a dead
// worker fails the call within half a second instead of after the 60 s the handshake allows a slow env.  The success path
// reads the error words only; the waitid / kill probes run between the 500 ms slices.
static int shm_wait_lane(fsrl_shm_env* env, int l, const std::vector<int32_t>& ws) {
    for (int slice = 0; slice < 120; ++slice) {
        if (fsrl_env_wait_done(env->hs + (l * 3 + 1) * 16, slice == 0 ? env->spin : 0u, 500) == 0) {
            const int w = shm_err_worker(env, ws);
            if (w >= 0) return fail(FSRL_ESTATE, "env worker %d raised inside its env (see its traceback on stderr)", w);
            return 0;
        }
        const int w = shm_failed_worker(env, ws);
        if (w >= 0) return fail(FSRL_ESTATE, "env worker %d died; the vector env cannot be used any more", w);
    }
    return fail(FSRL_ESTATE, "env workers of lane %d did not answer within 60 s", l);
}
// which workers a set of envs touches, per lane
static void shm_touched(const fsrl_shm_env* env, const int32_t* ids, int n, std::vector<int32_t> (&touched)[2]) {
    std::vector<uint8_t> seen((size_t)env->workers, 0);
    touched[0].clear(); touched[1].clear();
    for (int i = 0; i < n; ++i) {
        const int w = env->owner[ids[i]];
        if (!seen[(size_t)w]) { seen[(size_t)w] = 1; touched[env->lane_of_worker[w]].push_back(w); }
    }
}
// post a command for the envs `ids` (all of lane l) to lane l only: the OTHER lane's participation flags are not touched -- its
// workers may be reading them right now (split-phase collect)
static void shm_post_lane(fsrl_shm_env* env, int l, const int32_t* ids, int n, const std::vector<int32_t>& ws, uint32_t cmd) {
    for (int e = 0; e < env->env_num; ++e)
        if (env->lane_of_worker[env->owner[e]] == l) env->active[e] = 0;
    for (int i = 0; i < n; ++i) env->active[ids[i]] = 1;
    uint32_t g = (env->gen[l] + 1u) & 0x7FFFFFFFu;
    if (g == 0u) g = 1u;
    env->gen[l] = g;
    for (int32_t w : ws) env->want[(size_t)w * 16] = g;
    env->hs[(l * 3 + 2) * 16] = cmd;
    fsrl_env_post(env->hs + (l * 3 + 0) * 16, env->hs + (l * 3 + 1) * 16, (uint32_t)ws.size(), g);
}

// ---- one command (step / reset) for a set of envs: actions are already in the block; stamps, post to the lanes, wait
static int shm_run_cmd(fsrl_shm_env* env, const int32_t* ids, int n, uint32_t cmd) {
    std::vector<int32_t> touched[2];
    shm_touched(env, ids, n, touched);
    std::vector<int32_t> lane_ids[2];
    for (int i = 0; i < n; ++i) lane_ids[env->lane_of_worker[env->owner[ids[i]]]].push_back(ids[i]);
    for (int l = 0; l < env->n_lanes; ++l)
        if (!touched[l].empty()) shm_post_lane(env, l, lane_ids[l].data(), (int)lane_ids[l].size(), touched[l], cmd);
    for (int l = 0; l < env->n_lanes; ++l) {
        if (touched[l].empty()) continue;
        int rc = shm_wait_lane(env, l, touched[l]);
        if (rc) return rc;
    }
    return 0;
}

extern "C" int fsrl_collect_run(fsrl_ctx* c, fsrl_shm_env* env, const int32_t* ready, int32_t n, float* obs, float* act,
                                float* env_act, int32_t deterministic, int32_t bound_method, const float* act_low,
                                const float* act_high, int32_t max_steps, int32_t* steps_out, double* cost_sum_out,
                                double* rew_out, double* cost_out, uint8_t* term_out, uint8_t* trunc_out,
                                float* obs_next_out) {
    CHECK_ARG(c && env && ready && obs && act && env_act && steps_out && cost_sum_out, "null argument");
    CHECK_ARG(rew_out && cost_out && term_out && trunc_out && obs_next_out, "null output");
    CHECK_ARG(n >= 1 && n <= env->env_num && max_steps >= 1, "bad row / step count");
    CHECK_ARG(env->obs_dim == c->cfg.obs_dim && env->act_dim == c->cfg.act_dim, "env shape != context shape");
    CHECK_ARG(env->n_lanes >= 1 && env->n_lanes <= 2, "n_lanes must be 1 or 2");
    const int Do = env->obs_dim, Da = env->act_dim;
    for (int i = 0; i < n; ++i) CHECK_ARG(ready[i] >= 0 && ready[i] < env->env_num, "env id out of range");
    std::vector<int64_t> ptr((size_t)n), eidx((size_t)n);
    std::vector<double> erew((size_t)n);
    std::vector<int32_t> elen((size_t)n);
    int steps = 0;
    double cost_sum = 0.0;
    *steps_out = 0; *cost_sum_out = 0.0;
    for (;;) {
        // ---- env.step(env_act, ready): actions in place, the lanes' participation stamps, one post per lane
        for (int i = 0; i < n; ++i) memcpy(env->act + (size_t)ready[i] * Da, env_act + (size_t)i * Da, (size_t)Da * 4);
        {
            int rc = shm_run_cmd(env, ready, n, 1u);                       // _CMD_STEP
            if (rc) return rc;
        }
        // ---- results of the step
        bool any_done = false;
        for (int i = 0; i < n; ++i) {
            const int e = ready[i];
            rew_out[i] = env->rew[e]; cost_out[i] = env->cost[e];
            term_out[i] = env->term[e]; trunc_out[i] = env->trunc[e];
            memcpy(obs_next_out + (size_t)i * Do, env->obs + (size_t)e * Do, (size_t)Do * 4);
            any_done = any_done || term_out[i] || trunc_out[i];
            cost_sum += cost_out[i];
        }
        ++steps;
        *steps_out = steps; *cost_sum_out = cost_sum;
        if (any_done || steps >= max_steps) return 0;       // this step's rows are the caller's to store (after its resets)
        // ---- buffer.add(rows) + policy(obs_next) + noise + map_action, as one collect step
        int rc = fsrl_collect_step(c, ready, n, obs, act, rew_out, cost_out, term_out, trunc_out, obs_next_out, ptr.data(),
                                   erew.data(), elen.data(), eidx.data(), obs_next_out, n, deterministic, bound_method,
                                   act_low, act_high, act, env_act);
        if (rc) return rc;
        memcpy(obs, obs_next_out, (size_t)n * Do * 4);
    }
}

// FastCollector.collect(n_episode=...) over the worker-process env as ONE call (fsrl/data/fast_collector.py:283-368): the
// vector steps, the store, the actor, AND what fsrl_collect_run left to the interpreter -- the reset of the envs whose episode
// ended (a reset command to their workers), the episode accounting, and the dropping of surplus envs once the envs still
// running cover the episodes still wanted (fast_collector.py:341-362: the first `surplus` finished envs of the step leave).
// Same calls in the same order as the interpreted loop around fsrl_collect_step: the same rows in the same slots and the same
// noise stream.  ep_rew_out / ep_len_out: one entry per finished episode in the order the loop met them ([n_episode] each).
extern "C" int fsrl_collect_episodes(fsrl_ctx* c, fsrl_shm_env* env, const int32_t* ready_in, int32_t n, const float* obs_in,
                                     int32_t n_episode, int32_t deterministic, int32_t bound_method, const float* act_low,
                                     const float* act_high, int64_t* steps_out, double* total_cost_out, int32_t* term_count_out,
                                     int32_t* trunc_count_out, double* ep_rew_out, int32_t* ep_len_out, int32_t* episodes_out) {
    CHECK_ARG(c && env && ready_in && obs_in && steps_out && total_cost_out && term_count_out && trunc_count_out, "null argument");
    CHECK_ARG(ep_rew_out && ep_len_out && episodes_out, "null output");
    CHECK_ARG(n >= 1 && n <= env->env_num && n_episode >= 1, "bad row / episode count");
    CHECK_ARG(env->obs_dim == c->cfg.obs_dim && env->act_dim == c->cfg.act_dim, "env shape != context shape");
    CHECK_ARG(env->n_lanes >= 1 && env->n_lanes <= 2, "n_lanes must be 1 or 2");
    const size_t Do = (size_t)env->obs_dim, Da = (size_t)env->act_dim;
    for (int i = 0; i < n; ++i) CHECK_ARG(ready_in[i] >= 0 && ready_in[i] < env->env_num, "env id out of range");
    std::vector<int32_t> ready(ready_in, ready_in + n), nready;
    std::vector<float> obs(obs_in, obs_in + (size_t)n * Do), act((size_t)n * Da), env_act((size_t)n * Da), nxt, obs_next((size_t)n * Do);
    std::vector<float> act_new((size_t)n * Da), env_act_new((size_t)n * Da);
    std::vector<double> rew((size_t)n), cost((size_t)n), erew((size_t)n);
    std::vector<uint8_t> term((size_t)n), trunc((size_t)n);
    std::vector<int64_t> ptr((size_t)n), eidx((size_t)n);
    std::vector<int32_t> elen((size_t)n), local, reset_ids;
    int64_t steps = 0;
    double total_cost = 0.0;
    int episodes = 0, term_count = 0, trunc_count = 0;
    c->t_collect_env = c->t_collect_act = 0.0;
    // env commands are synchronous here (post + wait inside shm_run_cmd), so a failure never leaves one half-handled; what CAN
    // be left behind is a device actor evaluation still writing the pinned head outputs: drained before the error goes up
    auto bail = [&](int code) { pactor_release(c); (void)hipStreamSynchronize(c->compute); (void)hipStreamSynchronize(c->side); return code; };
    // the first actions: nothing to store yet
    int rc = fsrl_collect_step(c, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                               nullptr, obs.data(), n, deterministic, bound_method, act_low, act_high, act.data(), env_act.data());
    if (rc) return bail(rc);
    for (;;) {
        const int k = (int)ready.size();
        for (int i = 0; i < k; ++i) memcpy(env->act + (size_t)ready[(size_t)i] * Da, env_act.data() + (size_t)i * Da, Da * 4);
        const double t_e0 = mono_seconds();
        rc = shm_run_cmd(env, ready.data(), k, 1u);                    // _CMD_STEP
        if (rc) return bail(rc);
        const double t_e1 = mono_seconds();
        c->t_collect_env += t_e1 - t_e0;
        local.clear();
        for (int i = 0; i < k; ++i) {
            const int e = ready[(size_t)i];
            rew[(size_t)i] = env->rew[e]; cost[(size_t)i] = env->cost[e];
            term[(size_t)i] = env->term[e]; trunc[(size_t)i] = env->trunc[e];
            memcpy(obs_next.data() + (size_t)i * Do, env->obs + (size_t)e * Do, Do * 4);
            total_cost += cost[(size_t)i];
            if (term[(size_t)i] || trunc[(size_t)i]) local.push_back(i);
            term_count += term[(size_t)i] ? 1 : 0; trunc_count += trunc[(size_t)i] ? 1 : 0;
        }
        steps += k;
        if (local.empty()) {
            rc = fsrl_collect_step(c, ready.data(), k, obs.data(), act.data(), rew.data(), cost.data(), term.data(), trunc.data(),
                                   obs_next.data(), ptr.data(), erew.data(), elen.data(), eidx.data(), obs_next.data(), k, deterministic,
                                   bound_method, act_low, act_high, act.data(), env_act.data());
            if (rc) return bail(rc);
            c->t_collect_act += mono_seconds() - t_e1;
            obs.swap(obs_next);
            obs_next.resize((size_t)k * Do);
            continue;
        }
        // ---- an episode ended in this step: reset those envs, drop surplus ones, store the step, act on what is left
        const int n_done = (int)local.size();
        nxt.assign(obs_next.begin(), obs_next.begin() + (size_t)k * Do);
        reset_ids.clear();
        for (int i : local) reset_ids.push_back(ready[(size_t)i]);
        rc = shm_run_cmd(env, reset_ids.data(), n_done, 2u);           // _CMD_RESET
        if (rc) return bail(rc);
        for (int i : local) memcpy(nxt.data() + (size_t)i * Do, env->obs + (size_t)ready[(size_t)i] * Do, Do * 4);
        const int surplus = k - (n_episode - episodes - n_done);
        nready.clear();
        std::vector<float> nxt_kept;
        nxt_kept.reserve((size_t)k * Do);
        {
            std::vector<uint8_t> drop((size_t)k, 0);
            for (int j = 0; j < surplus && j < n_done; ++j) drop[(size_t)local[(size_t)j]] = 1;
            for (int i = 0; i < k; ++i) {
                if (drop[(size_t)i]) continue;
                nready.push_back(ready[(size_t)i]);
                nxt_kept.insert(nxt_kept.end(), nxt.begin() + (size_t)i * Do, nxt.begin() + (size_t)(i + 1) * Do);
            }
        }
        const bool last = episodes + n_done >= n_episode;
        const int k_next = last ? 0 : (int)nready.size();
        rc = fsrl_collect_step(c, ready.data(), k, obs.data(), act.data(), rew.data(), cost.data(), term.data(), trunc.data(),
                               obs_next.data(), ptr.data(), erew.data(), elen.data(), eidx.data(), last ? nullptr : nxt_kept.data(), k_next,
                               deterministic, bound_method, act_low, act_high, act_new.data(), env_act_new.data());
        if (rc) return bail(rc);
        for (int i : local) {
            if (episodes < n_episode) { ep_rew_out[episodes] = erew[(size_t)i]; ep_len_out[episodes] = elen[(size_t)i]; }
            episodes += 1;
        }
        if (last) break;
        ready.swap(nready);
        obs.assign(nxt_kept.begin(), nxt_kept.end());
        act.assign(act_new.begin(), act_new.begin() + (size_t)k_next * Da);
        env_act.assign(env_act_new.begin(), env_act_new.begin() + (size_t)k_next * Da);
        obs_next.resize((size_t)k_next * Do);
    }
    *steps_out = steps; *total_cost_out = total_cost; *term_count_out = term_count; *trunc_count_out = trunc_count;
    *episodes_out = episodes;
    pactor_release(c);                        // the collect is over: the resident actor ends here, not at its idle timeout
    return 0;
}

// The same collect over the env's TWO LANES, split-phase (the native form of FastCollector._collect_split): while lane A's
// workers step, the collector stores lane B's finished transitions, evaluates the actor on lane B's next observations and posts
// lane B's next step -- an env whose step costs more than the actor call hides that call behind the other lane's step.  Episode
// accounting is global (envs of either lane leave once the envs still running cover the episodes still wanted), so exactly
// n_episode episodes are collected (fast_collector.py:341-362).  The library calls are the interpreted split loop's, in its
// order: the same rows in the same slots and the same noise stream as that loop (NOT as the single-phase loop: the noise
// stream is consumed lane by lane).  Rows of one env stay chronological, so sample(0) and the GAE scan see what they expect.
extern "C" int fsrl_collect_episodes_split(fsrl_ctx* c, fsrl_shm_env* env, const int32_t* ready_in, int32_t n, const float* obs_in,
                                           int32_t n_episode, int32_t deterministic, int32_t bound_method, const float* act_low,
                                           const float* act_high, int64_t* steps_out, double* total_cost_out,
                                           int32_t* term_count_out, int32_t* trunc_count_out, double* ep_rew_out,
                                           int32_t* ep_len_out, int32_t* episodes_out) {
    CHECK_ARG(c && env && ready_in && obs_in && steps_out && total_cost_out && term_count_out && trunc_count_out, "null argument");
    CHECK_ARG(ep_rew_out && ep_len_out && episodes_out, "null output");
    CHECK_ARG(n >= 1 && n <= env->env_num && n_episode >= 1, "bad row / episode count");
    CHECK_ARG(env->obs_dim == c->cfg.obs_dim && env->act_dim == c->cfg.act_dim, "env shape != context shape");
    CHECK_ARG(env->n_lanes == 2, "the split-phase collect needs an env with two lanes");
    const size_t Do = (size_t)env->obs_dim, Da = (size_t)env->act_dim;
    for (int i = 0; i < n; ++i) CHECK_ARG(ready_in[i] >= 0 && ready_in[i] < env->env_num, "env id out of range");
    struct Grp {
        std::vector<int32_t> ready, touched;
        std::vector<float> obs, act, env_act;
        bool busy = false;
    } g[2];
    for (int i = 0; i < n; ++i) {
        Grp& q = g[env->lane_of_worker[env->owner[ready_in[i]]]];
        q.ready.push_back(ready_in[i]);
        q.obs.insert(q.obs.end(), obs_in + (size_t)i * Do, obs_in + (size_t)(i + 1) * Do);
    }
    auto post_step = [&](int l) {
        Grp& q = g[l];
        const int k = (int)q.ready.size();
        for (int i = 0; i < k; ++i) memcpy(env->act + (size_t)q.ready[(size_t)i] * Da, q.env_act.data() + (size_t)i * Da, Da * 4);
        std::vector<int32_t> tl[2];
        shm_touched(env, q.ready.data(), k, tl);
        q.touched = tl[l];
        shm_post_lane(env, l, q.ready.data(), k, q.touched, 1u);
        q.busy = true;
    };
    int rc = 0;
    // an error leaves with NO command in flight: the other lane's step (if any) is waited for first -- bounded, 2 s, the
    // error text of the first failure is kept -- so a caller that catches the error cannot post onto a lane whose completion
    // counter the workers are still decrementing (the Python side marks the env broken as well)
    auto bail = [&](int code) {
        const std::string keep = g_err;
        pactor_release(c);                                        // the resident actor ends here, not at its idle timeout
        for (int l = 0; l < 2; ++l)
            if (g[l].busy) { fsrl_env_wait_done(env->hs + (l * 3 + 1) * 16, 0u, 2000); g[l].busy = false; }
        (void)hipStreamSynchronize(c->compute); (void)hipStreamSynchronize(c->side);       // as fsrl_collect_episodes' bail
        g_err = keep;
        return code;
    };
    c->t_collect_env = c->t_collect_act = 0.0;
    for (int l = 0; l < 2; ++l) {
        Grp& q = g[l];
        const int k = (int)q.ready.size();
        if (!k) continue;
        q.act.resize((size_t)k * Da); q.env_act.resize((size_t)k * Da);
        rc = fsrl_collect_step(c, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                               nullptr, q.obs.data(), k, deterministic, bound_method, act_low, act_high, q.act.data(), q.env_act.data());
        if (rc) return bail(rc);
        post_step(l);
    }
    int64_t steps = 0;
    double total_cost = 0.0;
    int episodes = 0, term_count = 0, trunc_count = 0;
    std::vector<double> rew, cost, erew;
    std::vector<uint8_t> term, trunc;
    std::vector<int64_t> ptr, eidx;
    std::vector<int32_t> elen, local, nready, reset_ids;
    std::vector<float> obs_next, nxt, nxt_kept, act_new, env_act_new;
    while (episodes < n_episode) {
        if (!g[0].busy && !g[1].busy) return bail(fail(FSRL_ESTATE, "split-phase collect: no env left but episodes are missing"));
        for (int l = 0; l < 2; ++l) {
            Grp& q = g[l];
            if (!q.busy) continue;
            const int k = (int)q.ready.size();
            const double t_e0 = mono_seconds();
            q.busy = false;                                       // waited for (or failed) either way
            rc = shm_wait_lane(env, l, q.touched);
            if (rc) return bail(rc);
            const double t_e1 = mono_seconds();
            c->t_collect_env += t_e1 - t_e0;
            q.busy = false;
            rew.resize((size_t)k); cost.resize((size_t)k); erew.resize((size_t)k); term.resize((size_t)k); trunc.resize((size_t)k);
            ptr.resize((size_t)k); eidx.resize((size_t)k); elen.resize((size_t)k); obs_next.resize((size_t)k * Do);
            act_new.resize((size_t)k * Da); env_act_new.resize((size_t)k * Da);
            local.clear();
            for (int i = 0; i < k; ++i) {
                const int e = q.ready[(size_t)i];
                rew[(size_t)i] = env->rew[e]; cost[(size_t)i] = env->cost[e];
                term[(size_t)i] = env->term[e]; trunc[(size_t)i] = env->trunc[e];
                memcpy(obs_next.data() + (size_t)i * Do, env->obs + (size_t)e * Do, Do * 4);
                total_cost += cost[(size_t)i];
                if (term[(size_t)i] || trunc[(size_t)i]) local.push_back(i);
                term_count += term[(size_t)i] ? 1 : 0; trunc_count += trunc[(size_t)i] ? 1 : 0;
            }
            steps += k;
            if (local.empty()) {
                rc = fsrl_collect_step(c, q.ready.data(), k, q.obs.data(), q.act.data(), rew.data(), cost.data(), term.data(),
                                       trunc.data(), obs_next.data(), ptr.data(), erew.data(), elen.data(), eidx.data(), obs_next.data(), k,
                                       deterministic, bound_method, act_low, act_high, q.act.data(), q.env_act.data());
                if (rc) return bail(rc);
                q.obs.assign(obs_next.begin(), obs_next.end());
                post_step(l);
                c->t_collect_act += mono_seconds() - t_e1;
                continue;
            }
            // ---- an episode ended in this lane's step: reset those envs (this lane is idle now), drop surplus ones
            const int n_done = (int)local.size();
            nxt.assign(obs_next.begin(), obs_next.end());
            reset_ids.clear();
            for (int i : local) reset_ids.push_back(q.ready[(size_t)i]);
            {
                std::vector<int32_t> tl[2];
                shm_touched(env, reset_ids.data(), n_done, tl);
                shm_post_lane(env, l, reset_ids.data(), n_done, tl[l], 2u);                 // _CMD_RESET
                rc = shm_wait_lane(env, l, tl[l]);
                if (rc) return bail(rc);
            }
            for (int i : local) memcpy(nxt.data() + (size_t)i * Do, env->obs + (size_t)q.ready[(size_t)i] * Do, Do * 4);
            const int active = (int)(g[0].ready.size() + g[1].ready.size());
            const int surplus = active - (n_episode - episodes - n_done);
            nready.clear(); nxt_kept.clear();
            {
                std::vector<uint8_t> drop((size_t)k, 0);
                for (int j = 0; j < surplus && j < n_done; ++j) drop[(size_t)local[(size_t)j]] = 1;
                for (int i = 0; i < k; ++i) {
                    if (drop[(size_t)i]) continue;
                    nready.push_back(q.ready[(size_t)i]);
                    nxt_kept.insert(nxt_kept.end(), nxt.begin() + (size_t)i * Do, nxt.begin() + (size_t)(i + 1) * Do);
                }
            }
            const int k_next = (int)nready.size();
            rc = fsrl_collect_step(c, q.ready.data(), k, q.obs.data(), q.act.data(), rew.data(), cost.data(), term.data(), trunc.data(),
                                   obs_next.data(), ptr.data(), erew.data(), elen.data(), eidx.data(), k_next ? nxt_kept.data() : nullptr,
                                   k_next, deterministic, bound_method, act_low, act_high, act_new.data(), env_act_new.data());
            if (rc) return bail(rc);
            for (int i : local) {
                if (episodes < n_episode) { ep_rew_out[episodes] = erew[(size_t)i]; ep_len_out[episodes] = elen[(size_t)i]; }
                episodes += 1;
            }
            q.ready = nready;
            q.obs.assign(nxt_kept.begin(), nxt_kept.end());
            q.act.assign(act_new.begin(), act_new.begin() + (size_t)k_next * Da);
            q.env_act.assign(env_act_new.begin(), env_act_new.begin() + (size_t)k_next * Da);
            if (k_next) post_step(l);
            c->t_collect_act += mono_seconds() - t_e1;
        }
    }
    // the interpreted loop leaves its while at the same point: a lane may still be stepping envs nobody needs any more
    for (int l = 0; l < 2; ++l)
        if (g[l].busy) { g[l].busy = false; rc = shm_wait_lane(env, l, g[l].touched); if (rc) return bail(rc); }
    *steps_out = steps; *total_cost_out = total_cost; *term_count_out = term_count; *trunc_count_out = trunc_count;
    *episodes_out = std::min(episodes, n_episode);
    pactor_release(c);
    return 0;
}

// seconds the last fsrl_collect_episodes / _split spent waiting for the env workers (out[0]) and in its store + actor calls
// (out[1]): FastCollector(split_phase="auto") picks the split loop when the env outweighs the actor call it could hide
extern "C" int fsrl_collect_timing(fsrl_ctx* c, double* out2) {
    CHECK_ARG(c && out2, "null argument");
    out2[0] = c->t_collect_env; out2[1] = c->t_collect_act;
    return 0;
}

// r6: the collector's actor as a resident workgroup (actor_resident_kernel).  on = 0: one launch per actor call, as up to round 5;
// idle_timeout_us: how long the kernel waits for a doorbell before it ends by itself (<= 0 keeps the current value; 2000 by default).
// Takes effect with the next actor call.  Identical actions either way.
extern "C" int fsrl_actor_set_resident(fsrl_ctx* c, int32_t on, double idle_timeout_us) {
    CHECK_ARG(c, "null ctx");
    ENTER_DEV(c);                             // has ended the kernel (pactor_release): rr_set_resident's own release finds nothing live
    return rr_code(rr_set_resident(c->pa, on, idle_timeout_us), "");
}

// out3 = {kernel launches, requests served through the doorbell, 1 if a resident kernel is live now}
extern "C" int fsrl_actor_resident_stats(fsrl_ctx* c, int64_t* out3) {
    CHECK_ARG(c && out3, "null argument");
    rr_stats(c->pa, out3);
    return 0;
}

extern "C" int fsrl_actor_release(fsrl_ctx* c) {
    CHECK_ARG(c, "null ctx");
    pactor_release(c);
    return 0;
}
