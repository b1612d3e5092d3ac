// host_group_episodes.inc -- GroupCollector.collect(n_episode) over worker-process envs as ONE library call (part of fsrl_hip.hip,
// after host_collect_group.inc): every member's FastCollector.collect (fsrl_collect_episodes, host_collect.inc) with the members'
// envs stepped TOGETHER and one actor request per vector step for all of them.  The loop and all its bookkeeping are
// group_episodes.hpp's ge_collect -- fsrl_collect_episodes' own loop, keyed by member (no HIP there: tests/host/group_episodes_sim.cpp
// drives it); here are its two callbacks and the checks:
//   * the env callback is host_collect.inc's shm_run_cmd: the command of every member posted on both lanes, and only then the waits,
//     so the workers of all members step at once -- the interpreted loop steps member 0's env, waits, steps member 1's ...;
//   * the step callback is fsrl_group_collect_step / fsrl_collect_group_step as it is: the group's resident actor kernel for fused
//     members, the L + 2 launches for layered ones.  Nothing on the device is new.
// A failure (a dead worker, an env that raised, a failed step) waits for every command already posted, ends the group's resident
// actor and drains the group's and the members' streams; only the failing member's env may be left with a half-handled command.
#include "group_episodes.hpp"

// the checks and the loop; step(GeStep) is the owner's lock-step step, leave(failed) ends its resident actor (and, after a failure,
// drains its streams)
template <class Step, class Leave>
static int group_collect_episodes(fsrl_ctx* const* mem, int members, fsrl_shm_env* const* envs, const int32_t* n, const int32_t* ready,
                                  const float* obs, const int32_t* n_episode, int64_t* steps_out, double* total_cost_out,
                                  int32_t* term_out, int32_t* trunc_out, double* ep_rew_out, int32_t* ep_len_out,
                                  int32_t* episodes_out, double* t_env_act_out2, int32_t* failed_member_out, Step&& step, Leave&& leave) {
    CHECK_ARG(envs && n && ready && obs && n_episode && steps_out && total_cost_out && term_out && trunc_out, "null argument");
    CHECK_ARG(ep_rew_out && ep_len_out && episodes_out && failed_member_out, "null output");
    const int Do = mem[0]->cfg.obs_dim, Da = mem[0]->cfg.act_dim;
    std::vector<GeEnvView> views((size_t)members);
    for (int i = 0; i < members; ++i) {
        const fsrl_shm_env* env = envs[i];
        *failed_member_out = i;
        const int bad = shm_check_env(mem[i], env, 1, ("member " + std::to_string(i) + ": ").c_str());
        if (bad) return bad;
        for (int j = 0; j < i; ++j)
            CHECK_ARG(envs[j] != env && envs[j]->hs != env->hs, "member %d: its env is member %d's (an env listed twice)", i, j);
        views[(size_t)i] = GeEnvView{env->obs, env->act, env->rew, env->cost, env->term, env->trunc, env->env_num};
    }
    *failed_member_out = -1;
    double t_env = 0.0, t_act = 0.0;
    const GeOut out{steps_out, total_cost_out, term_out, trunc_out, ep_rew_out, ep_len_out, episodes_out};
    int failed = -1;
    const int rc = ge_collect(
        members, views.data(), Do, Da, n, ready, obs, n_episode, out,
        [&](uint32_t cmd, const std::vector<std::vector<int32_t>>& ids, int* bad) {
            const int r = timed(t_env, [&] { return shm_run_cmd(envs, ids, cmd, bad); });
            if (r) g_err = "member " + std::to_string(*bad) + ": " + g_err;
            return r;
        },
        [&](const GeStep& s) { return timed(t_act, [&] { return step(s); }); }, &failed);
    *failed_member_out = failed;
    if (t_env_act_out2) { t_env_act_out2[0] = t_env; t_env_act_out2[1] = t_act; }
    if (rc > 0) return fail(FSRL_EINVAL, "member %d: %s", failed, ge_what[rc]);       // an argument error: nothing posted, nothing launched
    // the collect is over, or failed: the group's resident actor ends here, not at its idle timeout; after a failure no actor
    // evaluation may still be writing the pinned outputs and no store flush may be in flight when the error goes up
    const std::string keep = g_err;
    leave(rc != 0);
    if (rc) g_err = keep;
    return rc;
}

static void group_episodes_drain(fsrl_ctx* const* mem, int members, hipStream_t stream) {
    (void)hipSetDevice(mem[0]->device);
    (void)hipStreamSynchronize(stream);
    for (int i = 0; i < members; ++i) {
        rr_release(mem[i]->pa);                 // off the resident path a member's own actor served its rows
        (void)hipStreamSynchronize(mem[i]->compute); (void)hipStreamSynchronize(mem[i]->side);
    }
}

extern "C" int fsrl_group_collect_episodes(fsrl_group* g, fsrl_shm_env* const* envs, const int32_t* n, const int32_t* ready,
                                           const float* obs, const int32_t* n_episode, int32_t deterministic, int32_t bound_method,
                                           const float* act_low, const float* act_high, int64_t* steps_out, double* total_cost_out,
                                           int32_t* term_out, int32_t* trunc_out, double* ep_rew_out, int32_t* ep_len_out,
                                           int32_t* episodes_out, double* t_env_act_out2, int32_t* failed_member_out) {
    CHECK_ARG(g, "null group");
    if (g->broken) return fail(FSRL_ESTATE, "a member of this group has been destroyed");
    return group_collect_episodes(
        g->m.data(), (int)g->m.size(), envs, n, ready, obs, n_episode, steps_out, total_cost_out, term_out, trunc_out, ep_rew_out,
        ep_len_out, episodes_out, t_env_act_out2, failed_member_out,
        [&](const GeStep& s) {
            return fsrl_group_collect_step(g, s.k, s.env_ids, s.obs, s.act, s.rew, s.cost, s.terminated, s.truncated, s.obs_next, s.ptr_out,
                                           s.ep_rew_out, s.ep_len_out, s.ep_idx_out, s.k_act, s.obs_act, deterministic, bound_method,
                                           act_low, act_high, s.act_out, s.env_act_out);
        },
        [&](bool failed) {
            group_actor_release(g);
            if (failed) group_episodes_drain(g->m.data(), (int)g->m.size(), g->stream);
        });
}

extern "C" int fsrl_collect_episodes_group(fsrl_collect_group* g, fsrl_shm_env* const* envs, const int32_t* n, const int32_t* ready,
                                           const float* obs, const int32_t* n_episode, int32_t deterministic, int32_t bound_method,
                                           const float* act_low, const float* act_high, int64_t* steps_out, double* total_cost_out,
                                           int32_t* term_out, int32_t* trunc_out, double* ep_rew_out, int32_t* ep_len_out,
                                           int32_t* episodes_out, double* t_env_act_out2, int32_t* failed_member_out) {
    CHECK_ARG(g, "null group");
    if (g->broken) return fail(FSRL_ESTATE, "a member of this collect group has been destroyed");
    return group_collect_episodes(
        g->m.data(), (int)g->m.size(), envs, n, ready, obs, n_episode, steps_out, total_cost_out, term_out, trunc_out, ep_rew_out,
        ep_len_out, episodes_out, t_env_act_out2, failed_member_out,
        [&](const GeStep& s) {
            return fsrl_collect_group_step(g, s.k, s.env_ids, s.obs, s.act, s.rew, s.cost, s.terminated, s.truncated, s.obs_next, s.ptr_out,
                                           s.ep_rew_out, s.ep_len_out, s.ep_idx_out, s.k_act, s.obs_act, deterministic, bound_method,
                                           act_low, act_high, s.act_out, s.env_act_out);
        },
        [&](bool failed) {
            collect_group_end_kernel(g);
            if (failed) group_episodes_drain(g->m.data(), (int)g->m.size(), g->stream);
        });
}
