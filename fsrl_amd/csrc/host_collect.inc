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
// The whole collect, episode boundaries included, is fsrl_collect_episodes[_split] below: the episode loop itself is written once,
// in group_episodes.hpp (shared with the grouped calls of host_group_episodes.inc); this file holds the env handshake and the glue.
#define FSRL_ENV_API static
#include "../env/csrc/fsrl_env.c"
#include "group_episodes.hpp"
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
// post a command for those of the envs `ids` that sit on lane l (ws: their workers) to lane l only: the OTHER lane's participation
// flags are not touched -- its workers may be reading them right now (split-phase collect)
static void shm_post_lane(fsrl_shm_env* env, int l, const int32_t* ids, int n, const std::vector<int32_t>& ws, uint32_t cmd) {
    for (int e = 0; e < env->env_num; ++e)
        if (env->lane_of_worker[env->owner[e]] == l) env->active[e] = 0;
    for (int i = 0; i < n; ++i)
        if (env->lane_of_worker[env->owner[ids[i]]] == l) env->active[ids[i]] = 1;
    uint32_t g = (env->gen[l] + 1u) & 0x7FFFFFFFu;
    if (g == 0u) g = 1u;
    env->gen[l] = g;
    for (int32_t w : ws) env->want[(size_t)w * 16] = g;
    env->hs[(l * 3 + 2) * 16] = cmd;
    fsrl_env_post(env->hs + (l * 3 + 0) * 16, env->hs + (l * 3 + 1) * 16, (uint32_t)ws.size(), g);
}

// ---- one command (step / reset) for the envs ids[m] of every member m (a single env: envs = &env): the actions are in the blocks
// already; stamps and posts on all lanes of all members first, then waits for all of them, so the workers of all members step at
// once.  The first failure is reported (code, text, member in *failed); the other commands are still waited for.
static int shm_run_cmd(fsrl_shm_env* const* envs, const std::vector<std::vector<int32_t>>& ids, uint32_t cmd, int* failed) {
    struct Posted { std::vector<int32_t> touched[2]; };
    const size_t members = ids.size();
    std::vector<Posted> posted(members);
    for (size_t m = 0; m < members; ++m) {
        if (ids[m].empty()) continue;
        shm_touched(envs[m], ids[m].data(), (int)ids[m].size(), posted[m].touched);
        for (int l = 0; l < envs[m]->n_lanes; ++l)
            if (!posted[m].touched[l].empty()) shm_post_lane(envs[m], l, ids[m].data(), (int)ids[m].size(), posted[m].touched[l], cmd);
    }
    int rc = 0;
    std::string first;
    for (size_t m = 0; m < members; ++m) {
        if (ids[m].empty()) continue;
        for (int l = 0; l < envs[m]->n_lanes; ++l) {
            if (posted[m].touched[l].empty()) continue;
            const int r = shm_wait_lane(envs[m], l, posted[m].touched[l]);
            if (r && !rc) { rc = r; *failed = (int)m; first = g_err; }
        }
    }
    if (rc) g_err = first;
    return rc;
}

// ---- what every native collect checks of an env against its context.  who: "" or "member i: "
static int shm_check_env(const fsrl_ctx* c, const fsrl_shm_env* env, int min_lanes, const char* who) {
    CHECK_ARG(c && env, "%snull context / env", who);
    CHECK_ARG(env->obs_dim == c->cfg.obs_dim && env->act_dim == c->cfg.act_dim,
              "%senv shape (obs %d, act %d) != context shape (obs %d, act %d)", who, env->obs_dim, env->act_dim, c->cfg.obs_dim,
              c->cfg.act_dim);
    CHECK_ARG(env->n_lanes >= min_lanes && env->n_lanes <= 2, "%s%s", who,
              min_lanes == 2 ? "the split-phase collect needs an env with two lanes" : "n_lanes must be 1 or 2");
    return 0;
}
// group_episodes.hpp's argument errors, as text
static const char* const ge_what[] = {"", "the row count must be 1 .. env_num", "n_episode must be >= 1", "env id out of range",
                                      "an env id is listed twice", "an env's lane is neither 0 nor 1"};
// f() with its seconds added to t: fsrl_collect_timing's two figures
template <class F>
static int timed(double& t, F&& f) {
    const double t0 = mono_seconds();
    const int r = f();
    t += mono_seconds() - t0;
    return r;
}

extern "C" int fsrl_collect_run(fsrl_ctx* c, fsrl_shm_env* env, const int32_t* ready, int32_t n, float* obs, float* act,
                                float* env_act, int32_t deterministic, int32_t bound_method, const float* act_low,
                                const float* act_high, int32_t max_steps, int32_t* steps_out, double* cost_sum_out,
                                double* rew_out, double* cost_out, uint8_t* term_out, uint8_t* trunc_out,
                                float* obs_next_out) {
    int rc = shm_check_env(c, env, 1, "");
    if (rc) return rc;
    CHECK_ARG(ready && obs && act && env_act && steps_out && cost_sum_out, "null argument");
    CHECK_ARG(rew_out && cost_out && term_out && trunc_out && obs_next_out, "null output");
    CHECK_ARG(n >= 1 && n <= env->env_num && max_steps >= 1, "bad row / step count");
    const int Do = env->obs_dim, Da = env->act_dim;
    for (int i = 0; i < n; ++i) CHECK_ARG(ready[i] >= 0 && ready[i] < env->env_num, "env id out of range");
    std::vector<int64_t> ptr((size_t)n), eidx((size_t)n);
    std::vector<double> erew((size_t)n);
    std::vector<int32_t> elen((size_t)n);
    const std::vector<std::vector<int32_t>> ids{std::vector<int32_t>(ready, ready + n)};
    int steps = 0, failed = -1;
    double cost_sum = 0.0;
    *steps_out = 0; *cost_sum_out = 0.0;
    for (;;) {
        // ---- env.step(env_act, ready): actions in place, the lanes' participation stamps, one post per lane
        for (int i = 0; i < n; ++i) memcpy(env->act + (size_t)ready[i] * Da, env_act + (size_t)i * Da, (size_t)Da * 4);
        rc = shm_run_cmd(&env, ids, GE_CMD_STEP, &failed);
        if (rc) return rc;
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
        rc = fsrl_collect_step(c, ready, n, obs, act, rew_out, cost_out, term_out, trunc_out, obs_next_out, ptr.data(),
                               erew.data(), elen.data(), eidx.data(), obs_next_out, n, deterministic, bound_method,
                               act_low, act_high, act, env_act);
        if (rc) return rc;
        memcpy(obs, obs_next_out, (size_t)n * Do * 4);
    }
}

// FastCollector.collect(n_episode=...) over the worker-process env as ONE call (fsrl/data/fast_collector.py:283-368): the vector
// steps, the store, the actor, AND what fsrl_collect_run leaves to the interpreter -- the reset of the envs whose episode ended (a
// reset command to their workers), the episode accounting, and the dropping of surplus envs.  The loop itself is
// group_episodes.hpp's; here are its callbacks, the checks and the way out:
//   fsrl_collect_episodes       = ge_collect with ONE member: the env callback is shm_run_cmd, the step callback fsrl_collect_step.
//       The same calls in the same order as the interpreted loop around fsrl_collect_step: same rows in the same slots, same noise
//       stream.  ep_rew_out / ep_len_out: one entry per finished episode in the order the loop met them ([n_episode] each).
//   fsrl_collect_episodes_split = ge_collect_split over the env's TWO LANES (the native form of FastCollector._collect_split): while
//       lane A's workers step, the collector stores lane B's finished transitions, evaluates the actor on lane B's next observations
//       and posts lane B's next step -- an env whose step costs more than the actor call hides that call behind the other lane's
//       step.  post = shm_touched + shm_post_lane, wait = shm_wait_lane.  The calls are the interpreted split loop's, in its order
//       (NOT the single-phase loop's: the noise stream is consumed lane by lane).  Rows of one env stay chronological, so sample(0)
//       and the GAE scan see what they expect.
// The way out of both.  Success: the resident actor ends here, not at its idle timeout.  Failure: the first error text is kept; every
// lane still reported busy gets a bounded 2 s wait, so a caller that catches the error cannot post onto a lane whose completion
// counter the workers are still decrementing (the Python side marks the env broken as well); the actor ends and the streams are
// drained: no actor evaluation may still be writing the pinned head outputs when the error goes up.
static int collect_leave(fsrl_ctx* c, fsrl_shm_env* env, int rc, const bool (&busy)[2]) {
    const std::string keep = g_err;
    for (int l = 0; rc && l < 2; ++l)
        if (busy[l]) fsrl_env_wait_done(env->hs + (l * 3 + 1) * 16, 0u, 2000);
    pactor_release(c);
    if (rc) { (void)hipStreamSynchronize(c->compute); (void)hipStreamSynchronize(c->side); g_err = keep; }
    return rc;
}

static int collect_episodes(fsrl_ctx* c, fsrl_shm_env* env, bool split, const int32_t* ready_in, int32_t n, const float* obs_in,
                            int32_t n_episode, int32_t deterministic, int32_t bound_method, const float* act_low, const float* act_high,
                            int64_t* steps_out, double* total_cost_out, int32_t* term_count_out, int32_t* trunc_count_out,
                            double* ep_rew_out, int32_t* ep_len_out, int32_t* episodes_out) {
    int rc = shm_check_env(c, env, split ? 2 : 1, "");
    if (rc) return rc;
    CHECK_ARG(ready_in && obs_in && steps_out && total_cost_out && term_count_out && trunc_count_out, "null argument");
    CHECK_ARG(ep_rew_out && ep_len_out && episodes_out, "null output");
    const GeEnvView view{env->obs, env->act, env->rew, env->cost, env->term, env->trunc, env->env_num};
    const GeOut out{steps_out, total_cost_out, term_count_out, trunc_count_out, ep_rew_out, ep_len_out, episodes_out};
    c->t_collect_env = c->t_collect_act = 0.0;
    auto step = [&](const GeStep& s) {
        return timed(c->t_collect_act, [&] {
            return fsrl_collect_step(c, s.env_ids, s.k[0], s.obs, s.act, s.rew, s.cost, s.terminated, s.truncated, s.obs_next, s.ptr_out,
                                     s.ep_rew_out, s.ep_len_out, s.ep_idx_out, s.obs_act, s.k_act[0], deterministic, bound_method, act_low,
                                     act_high, s.act_out, s.env_act_out);
        });
    };
    bool busy[2] = {false, false};              // the lock-step loop's env commands are synchronous: none is ever left in flight
    if (!split) {
        int failed = -1;
        rc = ge_collect(1, &view, env->obs_dim, env->act_dim, &n, ready_in, obs_in, &n_episode, out,
                        [&](uint32_t cmd, const std::vector<std::vector<int32_t>>& ids, int* bad) {
                            return timed(c->t_collect_env, [&] { return shm_run_cmd(&env, ids, cmd, bad); });
                        },
                        step, &failed);
    } else {
        std::vector<int32_t> lane((size_t)env->env_num), touched[2];
        for (int e = 0; e < env->env_num; ++e) lane[(size_t)e] = env->lane_of_worker[env->owner[e]];
        rc = ge_collect_split(view, lane.data(), env->obs_dim, env->act_dim, n, ready_in, obs_in, n_episode, out,
                              [&](int l, const int32_t* ids, int k, uint32_t cmd) {
                                  return timed(c->t_collect_env, [&] {
                                      std::vector<int32_t> tl[2];       // the other lane's list is in use: it is stepping
                                      shm_touched(env, ids, k, tl);
                                      touched[l].swap(tl[l]);
                                      shm_post_lane(env, l, ids, k, touched[l], cmd);
                                      return 0;
                                  });
                              },
                              [&](int l) { return timed(c->t_collect_env, [&] { return shm_wait_lane(env, l, touched[l]); }); }, step, busy);
    }
    if (rc == GE_STALLED) rc = fail(FSRL_ESTATE, "split-phase collect: no env left but episodes are missing");
    else if (rc > 0) return fail(FSRL_EINVAL, "%s", ge_what[rc]);           // an argument error: nothing was posted, nothing launched
    return collect_leave(c, env, rc, busy);
}

extern "C" int fsrl_collect_episodes(fsrl_ctx* c, fsrl_shm_env* env, const int32_t* ready_in, int32_t n, const float* obs_in,
                                     int32_t n_episode, int32_t deterministic, int32_t bound_method, const float* act_low,
                                     const float* act_high, int64_t* steps_out, double* total_cost_out, int32_t* term_count_out,
                                     int32_t* trunc_count_out, double* ep_rew_out, int32_t* ep_len_out, int32_t* episodes_out) {
    return collect_episodes(c, env, false, ready_in, n, obs_in, n_episode, deterministic, bound_method, act_low, act_high, steps_out,
                            total_cost_out, term_count_out, trunc_count_out, ep_rew_out, ep_len_out, episodes_out);
}

extern "C" int fsrl_collect_episodes_split(fsrl_ctx* c, fsrl_shm_env* env, const int32_t* ready_in, int32_t n, const float* obs_in,
                                           int32_t n_episode, int32_t deterministic, int32_t bound_method, const float* act_low,
                                           const float* act_high, int64_t* steps_out, double* total_cost_out,
                                           int32_t* term_count_out, int32_t* trunc_count_out, double* ep_rew_out,
                                           int32_t* ep_len_out, int32_t* episodes_out) {
    return collect_episodes(c, env, true, ready_in, n, obs_in, n_episode, deterministic, bound_method, act_low, act_high, steps_out,
                            total_cost_out, term_count_out, trunc_count_out, ep_rew_out, ep_len_out, episodes_out);
}

// seconds the last fsrl_collect_episodes / _split spent inside env commands -- step AND reset, post and wait (out[0]) -- and inside
// its step calls, the first one and those of steps that end an episode included (out[1]): what the grouped calls report in
// t_env_act_out2.  FastCollector(split_phase="auto") picks the split loop when the env outweighs the actor call it could hide
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
