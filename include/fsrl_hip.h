/*
 * fsrl_hip.h -- C ABI of libfsrl_hip.so, the MI355X (gfx950) policy-update engine that sits
 * behind FSRL's Python seam (fsrl.agent / fsrl.policy / fsrl.trainer).
 *
 * The reference (liuzuxin/FSRL) is pure Python and has no FFI; its seam is the duck-typed
 * contract between trainer/collector and policy+buffer.  Each entry
 * point below names the reference interface it replaces (file:line under the reference
 * tree).  INTEGRATION.md shows the ctypes stub a reference maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success, a negative code on failure (FSRL_E*);
 *     fsrl_last_error() returns a thread-local human-readable message.
 *   - all pointer arguments are HOST pointers owned by the caller for the duration of
 *     the call; the library owns every device allocation (store, parameters, Adam
 *     moments, activations) and copies in/out.
 *   - one context per GPU, not re-entrant; single caller thread (like the reference).
 *   - parameters travel as ONE flat float32 vector in torch `parameters()` order:
 *       actor  : sigma_param[Da] W1[H1,Do] b1[H1] W2[H2,H1] b2[H2] Wmu[Da,H2] bmu[Da]
 *       critic : W1[H1,Do] b1[H1] W2[H2,H1] b2[H2] W3[1,H2] b3[1]     (x n_critics)
 *     (tianshou-0.5 Net+ActorProb / Net+Critic as built at
 *      fsrl/agent/ppo_lag_agent.py:136-153; weights row-major [out,in] like nn.Linear).
 */
#ifndef FSRL_HIP_H
#define FSRL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FSRL_OK 0
#define FSRL_EINVAL (-22)   /* shape / flag violation (reference: assert / TypeError)  */
#define FSRL_ENOMEM (-12)
#define FSRL_EHIP (-5)      /* a HIP runtime call failed; see fsrl_last_error()        */
#define FSRL_ESTATE (-1)    /* call order violation (e.g. pass before begin)           */

#define FSRL_ALGO_PPO_LAG 0
#define FSRL_ALGO_TRPO_LAG 1
#define FSRL_ALGO_CPO 2
#define FSRL_ALGO_SAC_LAG 3
#define FSRL_ALGO_FOCOPS 4

#define FSRL_MAX_CRITICS 4
#define FSRL_MAX_HIDDEN 8      /* hidden layers of a layered context (fsrl_config.n_hidden)                          */
#define FSRL_MAX_WIDTH 4096    /* widest hidden layer of a layered context                                            */
#define FSRL_PPO_NSTATS 11  /* rescaling, lagrangian, actor_safety, actor_rew, actor_total,
                               kl, vf0, vf1, vf_total, total, entropy  (logger keys of
                               fsrl/policy/ppo_lag.py:169-170,204-211,245-247 and
                               fsrl/policy/lagrangian_base.py:158-165)                  */

typedef struct fsrl_ctx fsrl_ctx;

/* Hyper-parameters; field names follow PPOLagAgent.__init__ (fsrl/agent/ppo_lag_agent.py:82-116)
 * and PPOLagrangian.__init__ (fsrl/policy/ppo_lag.py:85-133). */
typedef struct fsrl_config {
    int32_t algo;            /* FSRL_ALGO_*                                              */
    int32_t obs_dim;         /* Do  (1..128)                                             */
    int32_t act_dim;         /* Da  (1..16)                                              */
    int32_t hidden;          /* two hidden layers of this width; with hidden1 / hidden2 set: 0, or the padded width       */
    int32_t n_critics;       /* 1 + number of cost constraints (2 for one cost)          */
    int32_t env_num;         /* number of per-env sub-buffers (VectorReplayBuffer)       */
    int64_t buffer_size;     /* total rows requested; sub-buffers get ceil(total/env_num)*/
    float max_action;        /* env.action_space.high[0]                                 */
    double gamma;            /* 0.99                                                     */
    double gae_lambda;       /* 0.95                                                     */
    float eps_clip;          /* 0.2                                                      */
    float dual_clip;         /* 0 = off, else > 1                                        */
    float vf_coef;           /* 0.25                                                     */
    float max_grad_norm;     /* 0 = off (agent default None), cfg default 0.5            */
    float target_kl;         /* 0.02; early stop when pass-mean KL > 1.5*target_kl       */
    int32_t norm_adv;        /* per-minibatch advantage normalisation                    */
    int32_t use_lagrangian;
    float lr;                /* Adam, one optimiser over actor+critics                   */
    float beta1, beta2, adam_eps;
    int32_t recompute_adv;   /* PPO-Lag, FOCOPS: recompute V, GAE, returns with the CURRENT critics before every pass after
                                the first (ppo_lag.py:218-221, focops.py:223-226 recompute_advantage); logp_old stays */
    int32_t unbounded;       /* on-policy actor: 1 = mean head without max_action * tanh (ActorProb(unbounded=True),
                                tianshou 0.5 utils/net/continuous.py; fsrl/agent/ppo_lag_agent.py:134)                */
    int32_t rew_norm;        /* reward_normalization (base_policy.py:114, 430-444): critics learn returns divided by the
                                running std of the returns; on-policy contexts                                        */
    int32_t value_clip;      /* PPO: clipped value loss (ppo_lag.py:158-164); needs rew_norm like the reference      */
    int32_t hidden1, hidden2; /* hidden_sizes = (hidden1, hidden2) of the agents (fsrl/agent/ppo_lag_agent.py:91,136), any
                                widths in [1, 256]; 0, 0 = (hidden, hidden).  Every flat parameter vector of the API (set /
                                get, gradients, trust-region vectors, the replay agents' actor / critic vectors) has the
                                caller's layout; the kernels run at 64 / 128 / 256 with zero-padded units               */
    int32_t n_hidden;        /* 0, or the length of hidden_sizes[] below: `hidden_sizes` of the agents as ANY tuple
                                (fsrl/agent/ppo_lag_agent.py:91,136-145; tianshou Net(hidden_sizes=...)), 1 .. FSRL_MAX_HIDDEN
                                layers of 1 .. FSRL_MAX_WIDTH units; leave hidden1 / hidden2 0 with it.  Two layers of at most
                                256 units select the fused kernels exactly like hidden1 / hidden2.  Anything else makes a
                                LAYERED context (every algorithm): the same entry points (store, collector actor,
                                fsrl_ppo_* / fsrl_tr_* / fsrl_sac_* / fsrl_cvpo_*, parameters, snapshot, lr), the same float64 scans and logged rows, but the network
                                math runs one MFMA GEMM launch per Linear (2 L + 5 launches per minibatch step instead of 3)
                                on activations kept in HBM.  Grouped PPO-Lag, FOCOPS, SAC-Lag and DDPG-Lag updates and their
                                lock-step collection take layered members (all members of one `hidden_sizes`); grouped CVPO
                                updates and fsrl_launch_floors refuse a layered context with FSRL_EINVAL.
                                Limits, as enforced: the replay agents (fsrl_sac_* / fsrl_cvpo_*) run every depth 1 ..
                                FSRL_MAX_HIDDEN with two or four Q-networks -- a weight-side job table larger than one launch
                                holds (32 jobs; four Q-networks of eight layers are 36) goes out in launches of whole
                                networks, bit-identical to one launch.  An on-policy step needs its table in ONE launch:
                                fsrl_ctx_create refuses (1 + n_critics) * (n_hidden + 1) + 1 > 32 with FSRL_EINVAL; with
                                n_critics <= 2, the present limit, every depth up to FSRL_MAX_HIDDEN fits (28 jobs).  */
    int32_t hidden_sizes[FSRL_MAX_HIDDEN];
    int32_t force_layered;   /* tests: run a two-layer network of at most 256 units through the layered kernels as well   */
} fsrl_config;

const char* fsrl_last_error(void);
void fsrl_config_default(fsrl_config* cfg); /* reference defaults for PPO-Lag            */

/* ---- memory ------------------------------------------------------------------------- */
/* Device and pinned blocks (and their bytes) this process holds through the library right now, over every context, state, env,
 * archive and group.  Read-only, no context, any thread; NULL outputs are skipped.  After everything is destroyed the four
 * figures are back where they were before it was created: the leak test's exact statement. */
int fsrl_mem_live(int64_t* dev_blocks, int64_t* dev_bytes, int64_t* pinned_blocks, int64_t* pinned_bytes);

/* ---- context ------------------------------------------------------------------------ */
/* replaces: PPOLagAgent.__init__ building nets + optimiser + policy on `device`
 * (fsrl/agent/ppo_lag_agent.py:127-200). */
int fsrl_ctx_create(int device_id, const fsrl_config* cfg, fsrl_ctx** out);
int fsrl_ctx_destroy(fsrl_ctx* ctx);
int fsrl_sync(fsrl_ctx* ctx);                       /* drain both internal streams       */

/* ---- parameters  (policy.state_dict()/load_state_dict(), base_agent.py:293-297) ------ */
int64_t fsrl_param_count(const fsrl_ctx* ctx);
int fsrl_params_set(fsrl_ctx* ctx, const float* flat, int64_t n);
int fsrl_params_get(fsrl_ctx* ctx, float* flat, int64_t n);
int fsrl_grads_get(fsrl_ctx* ctx, float* flat, int64_t n);   /* last minibatch gradient  */
int fsrl_optim_reset(fsrl_ctx* ctx);                /* zero Adam moments and step count  */
/* Device-resident checkpoint of the training state of an ON-POLICY context (PPO-Lag, FOCOPS, CPO, TRPO-Lag: parameters with
 * their W2 mirrors, Adam moments, step counts, and with reward_normalization the running return statistics), kept in HBM; the
 * collector's noise stream and the library's shuffle stream are NOT part of it.  Replay contexts (SAC / DDPG / CVPO keep actor,
 * Q, target and alpha state of their own) are refused with FSRL_EINVAL. snapshot / restore are device-to-device copies on the compute stream, no host round
 * trip and no synchronisation.  The reference has no counterpart (copy.deepcopy(policy.state_dict()) is the host-side
 * equivalent); bench.py restores the same start state before every timed update with it.                                */
int fsrl_state_snapshot(fsrl_ctx* ctx);
int fsrl_state_restore(fsrl_ctx* ctx);
/* The FULL training state of a context as bytes, for a run that is to continue in another process exactly as it would have
 * here: parameters (with their device-layout mirrors), every Adam moment and step counter, the optimiser groups' current
 * rates (fsrl_set_lr), the collector's noise stream and the minibatch shuffle stream, the return statistics; FOCOPS: nu and
 * its step counters; CPO / TRPO-Lag: the critics' step counter; replay contexts: actor / critics / targets, the
 * temperature and the CVPO duals with their Adam state, the update counter and the sampler's Philox key.  with_store != 0
 * adds the transition store: its geometry, every sub-buffer's bookkeeping (the episode in progress included) and the live
 * rows of the six columns.  Hyper-parameters are NOT state: they come from the importing context's own configuration.
 *   blob = header (magic, version, flags, the FINGERPRINT of everything the layout depends on: algorithm and mode, fused
 *          or layered, obs_dim, act_dim, hidden widths, n_critics, env_num, allocated store rows, rew_norm, Q-networks)
 *          | tagged sections (tag, length, payload zero-padded to 8 bytes) | 64-bit checksum.
 * A pure function of the state: export(import(b)) == b byte for byte.  DESIGN.md has the inventory.
 * size: the bytes an export would write now (< 0: an error code).  export: flushes the staging window first; writes
 * *written <= cap bytes.  import: checks magic, version, checksum, the fingerprint field by field (the error names the
 * first field that differs, with both values), the section list (unknown / duplicate / missing tag, wrong length, a
 * length past the end) and the store's bookkeeping BEFORE it writes anything: a refused import (FSRL_EINVAL) leaves the
 * context exactly as it was.  A blob without the store leaves the context's store untouched.  copy: the same state
 * device-to-device between two contexts of equal fingerprint on one device.
 * import and copy (into dst) invalidate what is derived from the state: the current batch, the HBM snapshot of
 * fsrl_state_snapshot, cached Hessian operands, a prefetched sample, the device copies of the sub-buffer books; rows of
 * the SAC statistics ring that were not drained yet are dropped.  export, import and copy end a resident actor kernel that holds the
 * context's weights (its own, its group's, its collect group's); none may be called inside an update (FSRL_ESTATE).
 * Members of a group may export and import between grouped calls.  Env state is not part of any of this.             */
int64_t fsrl_train_state_size(fsrl_ctx* ctx, int32_t with_store);
int fsrl_train_state_export(fsrl_ctx* ctx, int32_t with_store, void* out, int64_t cap, int64_t* written);
int fsrl_train_state_import(fsrl_ctx* ctx, const void* blob, int64_t n);
int fsrl_train_state_copy(fsrl_ctx* dst, fsrl_ctx* src, int32_t with_store);
/* lr_scheduler.step() at the end of BasePolicy.update (fsrl/policy/base_policy.py:352-354): the caller's torch
 * scheduler owns the schedule, this call moves the new rate of one optimiser into the engine; it applies from the next
 * optimiser step.  group: on-policy contexts 0 (the one Adam; for CPO / TRPO-Lag the critics' Adam); FOCOPS 0 actor,
 * 1 critics; replay contexts (SAC / DDPG / CVPO) 0 actor, 1 critics, 2 alpha.  fsrl_get_lr returns < 0 for a bad group. */
/* BasePolicy.ret_rms (fsrl/policy/base_policy.py:111, 442-444): per critic the running (mean, var, count) of the normalised
 * returns, rows of 3 doubles, n = 3 * n_critics.  Only in contexts created with rew_norm.  The reference keeps these outside
 * state_dict; a host that wants them to survive a restart carries them itself. */
int fsrl_ret_rms_get(fsrl_ctx* ctx, double* out, int32_t n);
int fsrl_ret_rms_set(fsrl_ctx* ctx, const double* in, int32_t n);
int fsrl_set_lr(fsrl_ctx* ctx, int32_t group, float lr);
float fsrl_get_lr(const fsrl_ctx* ctx, int32_t group);

/* ---- HIP-resident transition store (tianshou VectorReplayBuffer as used at
 *      fsrl/agent/base_agent.py:279, fsrl/data/fast_collector.py:333-335,
 *      fsrl/trainer/onpolicy.py:109) ------------------------------------------------- */
/* add(batch, buffer_ids) -> (ptr, ep_rew, ep_len, ep_idx).  Rows are staged in pinned host
 * memory and copied with hipMemcpyAsync on the side stream; the call does not wait.       */
int fsrl_store_push(fsrl_ctx* ctx, const int32_t* env_ids, int32_t k, const float* obs,
                    const float* act, const double* rew, const double* cost,
                    const uint8_t* terminated, const uint8_t* truncated,
                    const float* obs_next, int64_t* ptr_out, double* ep_rew_out,
                    int32_t* ep_len_out, int64_t* ep_idx_out);
int fsrl_store_reset(fsrl_ctx* ctx, int keep_statistics);   /* buffer.reset()            */
int64_t fsrl_store_len(const fsrl_ctx* ctx);                /* len(buffer)               */
/* buffer[indices] (tianshou ReplayBufferManager.__getitem__ as FSRL's evaluation / dataset tooling uses it): the rows
 * stored at the given slots, copied to the host; any output pointer may be NULL.  Not on the training path.            */
int fsrl_store_read(fsrl_ctx* ctx, const int64_t* indices, int64_t n, float* obs_out, float* act_out, double* rew_out,
                    double* cost_out, uint8_t* terminated_out, uint8_t* truncated_out, float* obs_next_out);
/* VectorReplayBuffer(total_size, buffer_num) built inside learn() (fsrl/agent/base_agent.py:279,
 * fsrl/agent/sac_lag_agent.py learn): re-cut the store into buffer_num sub-buffers of ceil(total_size / buffer_num)
 * rows -- slot numbering, wrap-around and sample indices then are the reference's for that geometry.  It must fit the
 * allocation of fsrl_ctx_create (cfg.buffer_size rows, cfg.env_num sub-buffers), else FSRL_EINVAL; empties the store. */
int fsrl_store_configure(fsrl_ctx* ctx, int64_t total_size, int32_t buffer_num);
int fsrl_store_geometry(const fsrl_ctx* ctx, int64_t* sub_size_out, int32_t* buffer_num_out);
/* The store's version: 1 at creation, bumped by every push (one per call, i.e. per vector step) and every reset; device copies of
 * the bookkeeping and samples drawn ahead are valid for one version.  For tests that hold two ways of filling a store against
 * each other. */
int fsrl_store_version(const fsrl_ctx* ctx, uint64_t* version_out);
/* buffer.sample_indices(0): env-major, chronological inside each sub-buffer.             */
int fsrl_store_sample0(fsrl_ctx* ctx, int64_t* indices_out, int64_t cap, int64_t* n_out);

/* ---- actor inference for the collector (policy.forward under no_grad,
 *      fsrl/policy/base_policy.py:178-190; sampling stays on the host RNG) ------------ */
int fsrl_actor_forward(fsrl_ctx* ctx, const float* obs, int32_t k, float* mu_out,
                       float* sigma_out);
/* Collector-time sampling (fsrl/data/fast_collector.py:283-300 -> policy.forward -> dist.sample()): actor on
 * the device, k x act_dim draws from the library RNG (seed != 0 re-keys it).  On-policy contexts:
 * a = mu + exp(sigma_param) * eps; SAC contexts: a = tanh(mu + sigma(s) * eps).  deterministic != 0: the
 * mean.  act_out[k][act_dim] is the raw policy output (what the buffer stores; map_action stays with the
 * caller).  Not torch's random stream -- the host mirror of the actor remains for stream-exact runs.   */
int fsrl_actor_sample(fsrl_ctx* ctx, const float* obs, int32_t k, int32_t deterministic, uint64_t seed,
                      float* act_out);
/* One vector step of FastCollector.collect (fsrl/data/fast_collector.py:283-368) with the actor on the device, in
 * ONE call: (1) launch the actor on obs_act[k_act] -- the observations the NEXT actions are for (obs_next with the
 * reset observations of finished envs put in, surplus envs dropped); (2) while it runs, store the k transitions that
 * just finished exactly as fsrl_store_push does (k = 0 on the first step of a collect); (3) wait, draw the noise
 * as fsrl_actor_sample does (same stream: the two calls one after the other give the same numbers), and map the
 * action for env.step as BasePolicy.map_action does (base_policy.py:226-256): bound_method 0 none / 1 clip to
 * [-1, 1] / 2 tanh, then low + (high - low) * (a + 1) / 2 when act_low / act_high are given.
 * act_out[k_act][act_dim]: the policy's action (what the buffer stores); env_act_out: what the env takes.        */
int fsrl_collect_step(fsrl_ctx* ctx, const int32_t* env_ids, int32_t k, const float* obs, const float* act,
                      const double* rew, const double* cost, const uint8_t* terminated, const uint8_t* truncated,
                      const float* obs_next, int64_t* ptr_out, double* ep_rew_out, int32_t* ep_len_out,
                      int64_t* ep_idx_out, const float* obs_act, int32_t k_act, int32_t deterministic,
                      int32_t bound_method, const float* act_low, const float* act_high, float* act_out,
                      float* env_act_out);
/* The worker-process vector env as the native collector loop sees it: pointers into the env's shared-memory block
 * (fsrl_amd/env/shmem.py lays it out; tianshou's ShmemVectorEnv is what the reference uses,
 * examples/mlp/train_ppol_agent.py:120-123) and the geometry of its two handshake lanes.                            */
typedef struct fsrl_shm_env {
    float* obs;                 /* [env_num][obs_dim]  written by the workers                          */
    float* act;                 /* [env_num][act_dim]  written by the collector                        */
    double* rew; double* cost;  /* [env_num]                                                           */
    uint8_t* term; uint8_t* trunc; uint8_t* active;     /* [env_num]                                   */
    uint32_t* hs;               /* [2][3][16]: per lane generation | pending workers | command         */
    uint32_t* want;             /* [workers][16]: generation of the last command a worker takes part in */
    const int32_t* owner;       /* [env_num] worker of each env                                        */
    const int32_t* lane_of_worker;  /* [workers]                                                       */
    int32_t env_num, obs_dim, act_dim, workers, n_lanes;
    uint32_t gen[2];            /* in / out: last generation posted per lane                           */
    uint32_t spin;              /* polls before the collector sleeps on a lane's completion word       */
    const uint32_t* err;        /* [workers][16] or NULL: non-zero once a worker raised inside its env */
    const int32_t* pids;        /* [workers] or NULL: the workers' process ids (children of the caller): a killed worker
                                 * fails the native collect within 0.5 s instead of after the 60 s handshake timeout */
} fsrl_shm_env;
/* FastCollector.collect's inner loop (fast_collector.py:252-340) over that env, in C: starting from the envs `ready`
 * with observations obs[n], policy actions act[n] and mapped actions env_act[n] (the outputs of the last
 * fsrl_collect_step), repeat { env.step -> store the transitions, evaluate the actor on the new observations
 * (= fsrl_collect_step) } until a vector step finishes an episode or max_steps steps were taken.  THAT step's results
 * come back unstored in rew_out / cost_out / term_out / trunc_out / obs_next_out[n] (the caller resets the finished envs,
 * drops surplus ones and stores the rows with its next fsrl_collect_step, fast_collector.py:341-362); obs / act /
 * env_act then hold the inputs of that step.  *steps_out: vector steps taken (>= 1), *cost_sum_out: sum of their costs.
 * Same random stream and the same stored rows as the per-step calls.                                               */
int fsrl_collect_run(fsrl_ctx* ctx, fsrl_shm_env* env, const int32_t* ready, int32_t n, float* obs, float* act,
                     float* env_act, int32_t deterministic, int32_t bound_method, const float* act_low,
                     const float* act_high, int32_t max_steps, int32_t* steps_out, double* cost_sum_out, double* rew_out,
                     double* cost_out, uint8_t* term_out, uint8_t* trunc_out, float* obs_next_out);
/* replaces: FastCollector.collect(n_episode=...) as a whole over the worker-process env (fsrl/data/fast_collector.py:283-368): the
 * loop of fsrl_collect_run PLUS the episode boundaries -- reset of the finished envs (a reset command to their workers), episode
 * accounting, dropping of surplus envs (fast_collector.py:341-362).  ready / obs: the envs to start from and their current
 * observations.  Outputs: env steps taken, the summed cost, terminated / truncated counts, and per finished episode its
 * reward and length ([n_episode] each, in the order the loop met them); *episodes_out == n_episode on success.  The same
 * fsrl_collect_step calls in the same order as the interpreted loop: same rows in the same slots, same noise stream. */
int fsrl_collect_episodes(fsrl_ctx* ctx, fsrl_shm_env* env, const int32_t* ready, int32_t n, const float* obs, int32_t n_episode,
                          int32_t deterministic, int32_t bound_method, const float* act_low, const float* act_high,
                          int64_t* steps_out, double* total_cost_out, int32_t* term_count_out, int32_t* trunc_count_out,
                          double* ep_rew_out, int32_t* ep_len_out, int32_t* episodes_out);

/* The same collect, split-phase over the env's two lanes (needs n_lanes == 2): one lane's workers step while the collector stores
 * the other lane's transitions and evaluates the actor on its next observations; exactly n_episode episodes, global surplus rule
 * (fast_collector.py:341-362).  Rows and noise stream equal the interpreted split loop's (FastCollector._collect_split).   */
int fsrl_collect_episodes_split(fsrl_ctx* ctx, fsrl_shm_env* env, const int32_t* ready, int32_t n, const float* obs, int32_t n_episode,
                                int32_t deterministic, int32_t bound_method, const float* act_low, const float* act_high,
                                int64_t* steps_out, double* total_cost_out, int32_t* term_count_out, int32_t* trunc_count_out,
                                double* ep_rew_out, int32_t* ep_len_out, int32_t* episodes_out);
/* Of the last fsrl_collect_episodes[_split]: out2[0] = seconds inside env commands (step AND the once-per-episode reset; post and
 * wait), out2[1] = seconds inside its fsrl_collect_step calls (the first one and those of steps that end an episode included; the
 * gather of the rows belongs to neither).  The same two figures as t_env_act_out2 of the grouped calls.                          */
int fsrl_collect_timing(fsrl_ctx* ctx, double* out2);
/* The collector's actor as a RESIDENT workgroup (contexts with the fused two-layer networks, up to 64 rows per call):
 * instead of one kernel launch per vector step (fast_collector.py:283-300: `self.policy(self.data, last_state)` per step) one
 * workgroup stays on its CU for the length of a collect; the host rings a doorbell in pinned memory with the observations next to
 * it and spins on a completion word.  The kernel ends on the next library call that enqueues other work on the context's stream
 * (which is thereby ordered behind it), at the end of fsrl_collect_episodes[_split], and by itself after idle_timeout_us without a
 * doorbell (default 2000; <= 0 keeps the value).  on = 0: one launch per call.  Same actions bit for bit either way.           */
int fsrl_actor_set_resident(fsrl_ctx* ctx, int32_t on, double idle_timeout_us);
/* out3 = {resident kernels launched, actor calls served through the doorbell, 1 if a resident kernel is live}                  */
int fsrl_actor_resident_stats(fsrl_ctx* ctx, int64_t* out3);
/* end the resident kernel now (the caller's collect is over); a no-op when none is live.  Never needed for correctness.           */
int fsrl_actor_release(fsrl_ctx* ctx);

/* Fill level of the first n sub-buffers (len(buffer.buffers[e]); ReplayBufferManager.sample_indices weighs by it). */
int fsrl_store_sizes(const fsrl_ctx* ctx, int64_t* sizes_out, int32_t n);

/* ---- PPO-Lagrangian update = BasePolicy.update (base_policy.py:332-355) -------------- */
/* begin: buffer.sample(0) + PPOLagrangian.process_fn (ppo_lag.py:134-150): gathers the
 * batch in sample(0) order, V_i(obs), V_i(obs_next), float64 GAE per critic, logp_old.
 * lagrangians[n_critics-1] and rescaling come from LagrangianPolicy (lagrangian_base.py:
 * 145-166) and are host float64 like in the reference.  *n_out = rows in the batch.      */
int fsrl_ppo_begin(fsrl_ctx* ctx, const double* lagrangians, double rescaling,
                   int32_t batch_size, int64_t* n_out);
/* one pass of PPOLagrangian.learn's outer loop (ppo_lag.py:217-255): minibatches of
 * batch_size in the order `perm` (= np.random.permutation(n), merge_last=True); fwd, loss,
 * bwd, grad clip, Adam for each; *stopped_out = 1 if the pass-mean approx-KL exceeded
 * 1.5*target_kl (the caller must then stop calling, like the reference's break).
 * perm == NULL: the library draws its own permutation (xoshiro256**, seeded by `seed`).  */
int fsrl_ppo_pass(fsrl_ctx* ctx, const int64_t* perm, uint64_t seed, int32_t* stopped_out);
/* stopped_out == NULL above only enqueues the pass: the caller may draw the next permutation while the device works
 * (rolling its RNG back if the pass turns out to be the last) and collects the verdict here before the next call.       */
int fsrl_ppo_pass_result(fsrl_ctx* ctx, int32_t* stopped_out);
/* end: drains per-minibatch stats ([n_steps][FSRL_PPO_NSTATS] float32, row-major).       */
int fsrl_ppo_end(fsrl_ctx* ctx, float* stats_out, int64_t cap_steps, int64_t* n_steps_out);
/* abandon an update after fsrl_ppo_begin when fsrl_ppo_end cannot be reached (an exception between the calls on the
 * caller's side, base_policy.py:345-351 has no such state): drains the stream and clears the begin/end state.       */
int fsrl_ppo_abort(fsrl_ctx* ctx);
/* convenience: begin + `repeat` passes (perms = [repeat][n] or NULL) + end.              */
int fsrl_ppo_update(fsrl_ctx* ctx, const double* lagrangians, double rescaling,
                    int32_t batch_size, int32_t repeat, const int64_t* perms, uint64_t seed,
                    float* stats_out, int64_t cap_steps, int64_t* n_steps_out,
                    int32_t* stopped_pass_out);

/* Launch plan of the minibatch step's forward / backward launch (A/B and tests; every plan gives the same bits): how many leading tiles of a
 * network are 32 rows tall.  -1 automatic (default: all of them once the 16-row tiles exceed the CU count, i.e. minibatches above
 * ~1 360 rows with three networks), 0 none, n > 0 min(n, tiles / 2).  Needs hidden >= 128 and obs_dim <= 64.                        */
int fsrl_ppo_set_plan(fsrl_ctx* ctx, int32_t tall_tiles);

/* The clipped PPO-Lagrangian step (max_grad_norm > 0) in TWO launches: the weight-gradient launch exchanges its workgroups' squared-norm
 * partials inside the launch and applies clip + Adam itself (same bits as the three-launch step).  Taken by a solo fused context whose
 * weight-gradient grid fits the chip, for minibatches of at most 512 rows, without recompute_adv and reward normalisation.  The
 * workgroups wait for each other at most `limit_ticks` ticks of 10 ns (< 0: the default, 5 000 = 50 us; 0: every workgroup gives up at
 * once).  An update in which a wait ran out (a shared GPU) is restored from its snapshot and replayed with three launches per step
 * inside the call that notices it; the context then keeps the three-launch step.  mode: -1 automatic (default), 0 off, 1 on.
 * Environment: FSRL_NO_CLIP_FUSE (read at fsrl_ctx_create) keeps the three-launch step.
 * fsrl_ppo_clip_fuse_stats: out[4] = {two-launch step still available (0 / 1), updates replayed, two-launch steps enqueued,
 * last update took it (0 / 1)}; grad_norm_out (may be NULL; between updates only): the gradient norm the last clipped step saw.   */
int fsrl_ppo_set_clip_fuse(fsrl_ctx* ctx, int32_t mode, int32_t limit_ticks);
int fsrl_ppo_clip_fuse_stats(fsrl_ctx* ctx, int64_t* out, float* grad_norm_out);

/* process_fn of a fused PPO-Lagrangian context takes V(obs_next[r]) from the V(obs) pass wherever obs_next[r] and obs[r + 1] of the batch
 * are equal word for word (every row of an on-policy store but the ends of episodes and the ring's seam) and evaluates only the other
 * rows -- the same bits as evaluating every row.  Environment: FSRL_NO_VNEXT_REUSE (read at fsrl_ctx_create) evaluates every row.
 * fsrl_ppo_process_stats (after fsrl_ppo_begin; waits for the device): out[4] = {rows taken from the V(obs) pass, rows evaluated
 * (per critic; they add up to the batch), the launch ran the equal split of its workgroups (0 / 1), the reuse was on (0 / 1)}.   */
int fsrl_ppo_process_stats(fsrl_ctx* ctx, int64_t* out);

/* ---- grouped updates: k independent PPO-Lagrangian agents, or k FOCOPS agents, of ONE network shape on one GPU, stepped in lock step
 *      (multi-seed runs; SURVEY 8e "within-GPU batching of k seeds").  The reference runs seeds as separate jobs; one
 *      agent's update is a chain of small dependent launches that leaves most of an MI355X idle, so k agents share every
 *      launch of the minibatch step (grid.y = member).  Per member the result is fsrl_ppo_update's on that member
 *      alone within the golden tests' tolerances, and bit-identical only when the launch shapes agree (a group of one,
 *      minibatches of at most 512 rows): the group picks its tile height from the number of active members and keeps the
 *      in-kernel weight-gradient reduction above 512 rows.  Members keep their own store, parameters,
 *      Adam state and random streams; batch lengths N_i may differ.  A PPO-Lagrangian group may be a SWEEP: members must agree
 *      on the network shape, n_critics, max_action, unbounded and on whether max_grad_norm is on (> 0: the step has 3 launches,
 *      2 without the clip) -- the refusal names the member and the field -- and may differ in eps_clip, dual_clip, vf_coef, the
 *      value of max_grad_norm, target_kl (the pass-level KL stop is watched when any member has a target; a member without
 *      one never stops), norm_adv, use_lagrangian, rew_norm, value_clip, recompute_adv, lr, beta1, beta2 and adam_eps; minibatch
 *      size and passes per member: fsrl_group_ppo_update_each.  A FOCOPS group is not a sweep: its members share all of these.
 *      While grouped, a member's own update calls still work (they run on the group's stream).
 *      A group has one algorithm.  FOCOPS members must have run fsrl_focops_init and share l2_reg, delta,
 *      eta, tem_lambda, max_grad_norm and fsrl_focops_set_plan (learning rates may differ); checked again at every update.
 *      Per fused FOCOPS member the result is bit-identical to its own update wherever the group keeps the member's tile height.
 *      LAYERED PPO-Lagrangian or FOCOPS members (fsrl_config.n_hidden: any other hidden_sizes) form a group when ALL members are
 *      layered and n_hidden, hidden_sizes[] and force_layered agree (a mix of fused and layered members, or of widths: "one
 *      network shape"; a FOCOPS group's message for the mix also says "layered").  The group then runs the layered minibatch step
 *      with every member in each of its 2 L + 5 launches (L hidden layers), whatever k; per member the update is bit-identical
 *      to its own fsrl_ppo_update (FOCOPS: its own pass-by-pass FOCOPS update), for every k, batch length and minibatch size.  */
typedef struct fsrl_group fsrl_group;
int fsrl_group_create(fsrl_ctx** ctxs, int32_t k, fsrl_group** out);       /* 1 <= k <= 16; members are not owned   */
int fsrl_group_destroy(fsrl_group* group);
/* Launch plan of the group's forward / backward launch (A/B and tests; every plan gives the same bits): how many leading tiles of a
 * (member, network) are 32 rows tall.  -1 automatic (default: all of them once the 16-row tiles of the group exceed the CU count, e.g.
 * 8 members x 3 networks x 256 rows: 192 workgroups of 32 rows instead of 384 of 16), 0 none, n > 0 min(n, tiles / 2).
 * Needs hidden >= 128 and obs_dim <= 64 (else 16-row tiles whatever the plan).  A group of layered contexts accepts the call and
 * ignores it (the layered step has no tile plan).                                                                                    */
int fsrl_group_set_plan(fsrl_group* group, int32_t tall_tiles);
/* k x BasePolicy.update (base_policy.py:332-355).  lagrangians [k][n_critics - 1], rescaling [k]; perms: NULL (library
 * shuffle, member i seeded by seed + 1000003 i + pass) or k pointers to [repeat][N_i]; stats_out: NULL or k pointers to
 * [cap_steps][FSRL_PPO_NSTATS]; n_steps_out [k]; stopped_pass_out [k] (-1 = ran every pass).
 * A FOCOPS group: k x FOCOPS learn with each member's fsrl_focops_set_nu values; lagrangians and rescaling are ignored (may
 * be NULL); the delta KL stop is always watched, and a member that stops sits out the later passes.                    */
int fsrl_group_ppo_update(fsrl_group* group, const double* lagrangians, const double* rescaling, int32_t batch_size,
                          int32_t repeat, const int64_t* const* perms, uint64_t seed, float* const* stats_out,
                          int64_t cap_steps, int64_t* n_steps_out, int32_t* stopped_pass_out);
/* The same update with member i's own minibatch size batch_sizes[i] and number of passes repeats[i] (a sweep over batch_size /
 * repeat_per_collect); fsrl_group_ppo_update is this call with its scalars repeated.  Member i is active for passes
 * 0 .. repeats[i] - 1 and then leaves the update as a KL-stopped member does, but with stopped_pass_out[i] = -1; repeats[i] == 0:
 * it sits the update out (its batch is sampled and processed as by its own update with repeat 0; no rows, parameters and Adam
 * counters untouched).  perms: NULL or k pointers to [repeats[i]][N_i]; cap_steps [k]: rows that stats_out[i] holds.  The update
 * runs max(repeats) passes.  A FOCOPS group takes per-member batch sizes and pass counts the same way.                         */
int fsrl_group_ppo_update_each(fsrl_group* group, const double* lagrangians, const double* rescaling, const int32_t* batch_sizes,
                               const int32_t* repeats, const int64_t* const* perms, uint64_t seed, float* const* stats_out,
                               const int64_t* cap_steps, int64_t* n_steps_out, int32_t* stopped_pass_out);
/* Lock-step collection: fsrl_collect_step on every member, member order, in ONE call with ONE actor request for all of them --
 * same stored rows and slots, same actions, same library-RNG consumption per member, bit for bit.  Row arrays are concatenated
 * over members: k[m] transitions to store (env_ids / obs / act / rew / cost / terminated / truncated / obs_next and the
 * ptr / ep_* outputs) and k_act[m] observations to act on (obs_act, act_out, env_act_out) for member m; 0 is allowed.
 * act_low / act_high: NULL or [k_members][act_dim], member m's action bounds.  The request goes to ONE resident actor kernel for
 * the group (a workgroup per member and 16-row tile, on the group's stream); it ends before the group's stream gets other work
 * (fsrl_group_ppo_update, a member's own library calls, fsrl_group_destroy), on fsrl_group_actor_release and after its idle
 * timeout.  Off the resident path (fsrl_group_actor_set_resident(0), a member asking for more rows than its 16 * min(4,
 * ceil(env_num / 16)) tiles): one actor launch per member inside the same call, the same bits.
 * A group of LAYERED contexts has no resident kernel: the members' rows are staged side by side in pinned memory and ONE sequence of
 * L + 2 launches on the group's stream (one job per member that has rows) serves the request, for any row count per member; the
 * host waits on completion words with a bounded poll.  fsrl_group_actor_set_resident(g, 0, ..) selects the member-by-member calls
 * (k (L + 2) launches), fsrl_group_actor_resident_stats reports {shared launch sequences, requests served by them, 0}, and
 * fsrl_group_actor_release has nothing to end.  The same bits either way.                                                */
int fsrl_group_collect_step(fsrl_group* group, const int32_t* k, const int32_t* env_ids, const float* obs, const float* act,
                            const double* rew, const double* cost, const uint8_t* terminated, const uint8_t* truncated,
                            const float* obs_next, int64_t* ptr_out, double* ep_rew_out, int32_t* ep_len_out,
                            int64_t* ep_idx_out, const int32_t* k_act, const float* obs_act, int32_t deterministic,
                            int32_t bound_method, const float* act_low, const float* act_high, float* act_out,
                            float* env_act_out);
/* the group's resident collect kernel: on (default) / off, idle timeout (default 2000 us; <= 0 keeps the value) */
int fsrl_group_actor_set_resident(fsrl_group* group, int32_t on, double idle_timeout_us);
/* out3 = {group kernels launched, grouped actor requests served through the doorbell, 1 if the group kernel is live}      */
int fsrl_group_actor_resident_stats(fsrl_group* group, int64_t* out3);
/* end the group's resident kernel now (a grouped collect is over); a no-op when none is live                               */
int fsrl_group_actor_release(fsrl_group* group);

/* read back process_fn products of the current batch: which = "values" | "rets" | "advs"
 * ([n][n_critics] float32, like torch.stack(.., -1)) | "logp_old" ([n]).                 */
int fsrl_batch_get(fsrl_ctx* ctx, const char* which, float* out, int64_t cap);

/* ---- stand-alone float64 GAE scan on the device (gae_return, base_policy.py:524-540);
 *      v_next already masked.  Bit-exact with the sequential reference.                  */
int fsrl_gae_return(fsrl_ctx* ctx, const float* v, const float* v_next, const double* rew,
                    const uint8_t* end_flag, int64_t n, double gamma, double gae_lambda,
                    double* adv_out);

/* ---- stand-alone float64 n-step return on the device (nstep_return, base_policy.py:543-567; called from
 *      compute_nstep_returns :453-512 with metric = rew / info.cost of the WHOLE buffer :481, end_flag = done | unfinished,
 *      target_q already value-masked, indices = the buffer.next chain [n_step][bsz]).  out[bsz][q] float64.
 *      Bit-exact with the sequential reference.  n_step < 1 -> FSRL_EINVAL (the reference asserts, :472).   */
int fsrl_nstep_return(fsrl_ctx* ctx, const double* metric, const uint8_t* end_flag, int64_t len,
                      const float* target_q, const int64_t* indices, int64_t bsz, int64_t q, double gamma,
                      int32_t n_step, double* out);

/* ---- trust-region policy updates: CPO (fsrl/policy/cpo.py) and TRPO-Lagrangian
 *      (fsrl/policy/trpo_lag.py).  Same context / store / parameter layout as PPO-Lag;
 *      full batch (the reference runs them with batch_size = 99999).                       */
typedef struct fsrl_tr_config {
    float target_kl;            /* delta: 0.01 (CPO), 0.001 (TRPO-Lag)                       */
    float backtrack_coeff;      /* 0.8                                                       */
    float damping;              /* 0.1  (cpo.py:182 damping_coeff, trpo_lag.py:115)          */
    float l2_reg;               /* CPO critics: + l2_reg * sum(theta^2)   (cpo.py:155-156)   */
    float critic_lr;            /* Adam over the critic parameters                           */
    int32_t max_backtracks;     /* 10 (agent default) / 100 (cpo_cfg.py:17)                  */
    int32_t optim_critic_iters; /* critic Adam steps per repeat                              */
    int32_t cg_iters;           /* 10                                                        */
    int32_t norm_adv;           /* full-batch advantage normalisation                        */
    double cost_limit;          /* CPO                                                       */
} fsrl_tr_config;

#define FSRL_CPO_NSTATS 17  /* kl, entropy, rew_loss, cost_loss, optim_A, optim_B, optim_C, optim_Q,
                               optim_R, optim_S, optim_lam, optim_nu, optim_case, step_size
                               (cpo.py:335-350) then vf0, vf1, vf_total (cpo.py:160-161)     */
#define FSRL_TRPO_NSTATS 11 /* rescaling, lagrangian, actor_safety, actor_rew, actor_total, vf0,
                               vf1, vf_total, kl, step_size, entropy (trpo_lag.py:140-171,241-249) */

/* begin: buffer.sample(0) + process_fn (cpo.py:123-145 / trpo_lag.py:117-134): GAE, full-batch
 * advantage normalisation, logp_old, mean_old / std_old.                                      */
int fsrl_tr_begin(fsrl_ctx* ctx, const fsrl_tr_config* cfg, int64_t* n_out);
/* CPO.learn (cpo.py:353-370): `repeat` x { optim_critic_iters critic steps ; policy_loss }.
 * ave_cost_return = stats_train["cost"] (cpo.py:112-113).  stats_out: [repeat][FSRL_CPO_NSTATS]. */
int fsrl_cpo_learn(fsrl_ctx* ctx, double ave_cost_return, int32_t repeat, float* stats_out);
/* TRPOLagrangian.learn (trpo_lag.py:173-251).  stats_out: [repeat][FSRL_TRPO_NSTATS].          */
int fsrl_trpo_learn(fsrl_ctx* ctx, const double* lagrangians, double rescaling, int32_t repeat,
                    float* stats_out);
/* The same two with Batch.split(batch_size, shuffle=True, merge_last=True) INSIDE learn (cpo.py:357-358, trpo_lag.py:178):
 * every repeat walks the minibatches of one permutation (a remainder is merged into the last one), critic steps and the
 * policy step per minibatch, one stats row per minibatch.  perms: [repeat][N] (np.random.permutation draws of the caller)
 * or NULL = the library shuffles (seed).  batch_size >= N: one minibatch, the whole batch in store order (perms ignored:
 * the reference's shuffle of a full batch only reorders sums) -- fsrl_cpo_learn / fsrl_trpo_learn are that case.
 * stats_out: [cap_rows][FSRL_*_NSTATS]; *n_rows_out = rows written = repeat x minibatches.                              */
int fsrl_cpo_learn_mb(fsrl_ctx* ctx, double ave_cost_return, int32_t repeat, int32_t batch_size, const int64_t* perms,
                      uint64_t seed, float* stats_out, int64_t cap_rows, int64_t* n_rows_out);
int fsrl_trpo_learn_mb(fsrl_ctx* ctx, const double* lagrangians, double rescaling, int32_t repeat, int32_t batch_size,
                       const int64_t* perms, uint64_t seed, float* stats_out, int64_t cap_rows, int64_t* n_rows_out);
/* policy evaluations the line search of each repeat of the last learn call made (cpo.py:306-333,
 * trpo_lag.py:205-231); returns the number written.  The reference samples an action in every one of them --
 * callers that follow its random streams need the count.                                        */
int32_t fsrl_tr_linesearch_evals(fsrl_ctx* ctx, int32_t* out, int32_t cap);
/* building blocks, exposed for the parity tests (all on the batch of the last fsrl_tr_begin):
 * which = 0: grad of mean(ratio*A_r)   1: grad of -mean(ratio*A_c)   2: grad of mean KL(old||new)
 * out: flat ACTOR parameter vector (sigma_param, W1, b1, W2, b2, W3, b3).                      */
int64_t fsrl_actor_param_count(const fsrl_ctx* ctx);
int fsrl_tr_grad(fsrl_ctx* ctx, int32_t which, float* out, int64_t n);
/* out = H v (no damping), H = Hessian of mean KL(N(mean_old,std_old) || pi_theta) at the current theta */
int fsrl_tr_hvp(fsrl_ctx* ctx, const float* v, float* out, int64_t n);
/* the same product for a caller that promises that theta, the batch and mean_old / std_old are those of its previous
 * fsrl_tr_hvp / fsrl_tr_hvp_cached call: the theta-only activations (h1, h2, dout, dz2) are read back instead of recomputed --
 * the kernel the conjugate-gradient solves inside fsrl_cpo_learn / fsrl_trpo_learn run for their 2nd .. 11th product
 * (cpo.py:184-204).  Bit-identical to fsrl_tr_hvp.                                                                     */
int fsrl_tr_hvp_cached(fsrl_ctx* ctx, const float* v, float* out, int64_t n);
/* the conjugate-gradient solve of the learn calls on its own (cpo.py:184-204 / trpo_lag.py:261-283): x_out = (H + damping)^-1 rhs
 * after at most nsteps (0 .. 64; 0: x = 0) iterations at the current theta, stopping after the first iteration that leaves
 * r.r < tol (the remaining ones are no-ops on the device).  rhs, x_out: flat ACTOR vectors like fsrl_tr_grad's out.
 * *iters_out = iterations that ran, *rs_out = the last r.r the device computed.                                       */
int fsrl_tr_cg(fsrl_ctx* ctx, const float* rhs, int64_t n, float damping, int32_t nsteps, float tol, float* x_out,
               int32_t* iters_out, float* rs_out);
/* stats8: mean(ratio*A_r), mean(ratio*A_c), mean KL, mean(logp_old - logp), mean A_r, mean A_c, 0, 0 */
int fsrl_tr_eval(fsrl_ctx* ctx, double* stats8);
/* Kernel plan of the full-batch path, for A/B timing and the bit-identity tests (no reference counterpart: the reference
 * has one code path).  tile_rows: 0 = automatic (mixed 32- / 16-row tiles; at 256-wide layers, obs_dim <= 64 and act_dim <= 4
 * as TWO co-resident 512-thread workgroups per CU: fb_tile_co_kernel), 16 = 16-row tiles only, 32 = mixed tiles with one
 * 1024-thread workgroup per CU (round 4's kernel); adding 64 runs the critics' regression steps on the compute stream, one
 * launch after the other, instead of on a stream of their own beside the actor's step (r5; same launches, same order inside
 * each chain: identical results).  hvp: 0 = automatic (mixed tiles; the theta-only activations of the KL
 * Hessian product are computed by the first product of a conjugate-gradient solve and read back by the others: cpo.py:184-204
 * calls _MVP 10 + 1 times per right-hand side at one theta; the cached products run as two co-resident workgroups per CU at
 * 256-wide layers: fb_hvp_co_kernel), 1 = the 16-row kernel that recomputes everything, 2 = mixed tiles without the cache,
 * 3 = mixed tiles + cache with one 1024-thread workgroup per CU (round 4's kernel); adding 4 to any of them switches the
 * Gauss-Newton form of the product off (A/B): by default, whenever mean_old / std_old of the batch were computed at the present
 * theta -- every TRPO-Lag product (trpo_lag.py:189-190), CPO's products until its first line-search step -- the KL gradient
 * is identically zero and the heads use mu - mean_old = 0, std_old = sigma exactly (as the reference's autograd does on its
 * detached copy of the same forward), so the dz2 / dout terms vanish and are not computed.  wgrad (the weight-side products):
 * 0 = automatic -- round 6's tile jobs (fb_wgrad3_kernel: every workgroup a 64 x 64 MFMA tile job, 512 threads, two per CU,
 * XCD-aware block order) at 256-wide layers over >= 4096 rows, else round 5's split-K kernel;
 * 1 = the split-K kernel with XCD-aware placement of its blocks, 2 = the split-K kernel; 3 = the one-pass streaming kernel
 * (one workgroup per network, output quarter and row slice; operands by LDS-DMA); 4 = the tile jobs in
 * plain block order; 5 = the same in XCD-aware order with half the row splits; 6 = both.  The tile_rows / hvp plans give
 * bit-identical results under EVERY wgrad plan; wgrad 1 and 2 agree to the bit, 0 and 4 where the tile jobs run; the kernel
 * families add the rows up in different orders (fp32 MFMA chains of different lengths, partials in float64): their results
 * agree to rounding (tests/test_gpu_fullsize.py states the tolerance).  tile_rows + 64: the critics' steps on the compute
 * stream instead of beside the actor's step; tile_rows + 128: the host-side read-backs of an update (line-search statistics,
 * dot products of the dual solve) by hipMemcpyAsync + hipStreamSynchronize instead of completion words the reducing kernels
 * write to pinned memory (r6: CPO configs[2] 28.3 -> 27.65 ms per update); same results.                                   */
int fsrl_tr_set_plan(fsrl_ctx* ctx, int32_t tile_rows, int32_t hvp, int32_t wgrad);
/* A/B only: force how many 32-row tiles (per network) the co-resident launches of the tile kernel / of the cached Hessian
 * product start with, the remaining rows going to 16-row tiles behind them; -1 = automatic.  A PERSISTENT form exists:
 * 2 x (number of CUs) workgroups draw their tiles from a device counter, so every CU keeps a pair of tiles in
 * flight until the batch runs out -- that is the A/B form, selected by -2 in either argument; the default is one workgroup per
 * tile (the hardware dispatcher already hands tiles out dynamically, and 1 250 draws on one counter cost ~50 us per launch).  Neither the split nor the scheduling changes a result (a row's arithmetic does not depend on its tile's
 * height or on the workgroup that computes it).                                                                        */
int fsrl_tr_set_tile_split(fsrl_ctx* ctx, int32_t n32_tile, int32_t n32_hvp);
/* A/B only: how late the SECOND co-resident workgroup of every CU starts its first tile, in periods of 8 128 shader cycles
 * (s_sleep 127), for the tile kernel / the cached Hessian product; -1 = the built-in default.  Two workgroups that start in
 * the same cycle run their phases in lockstep and never overlap; the offset is created once per launch.  No effect on a result. */
int fsrl_tr_set_co_delay(fsrl_ctx* ctx, int32_t tile_periods, int32_t hvp_periods);

/* ---- FOCOPS (fsrl/policy/focops.py:126-251), on the PPO entry points: create the context
 *      with algo = FSRL_ALGO_FOCOPS (same networks and parameter vector as PPO-Lag), call fsrl_focops_init once,
 *      then per update: fsrl_focops_set_nu (the host-side nu step, focops.py:154-159) -> fsrl_ppo_begin
 *      (lagrangians / rescaling ignored) -> fsrl_ppo_pass x repeat (pass-level KL early stop against `delta`)
 *      -> fsrl_ppo_end.  Stats rows keep FSRL_PPO_NSTATS floats; the first FSRL_FOCOPS_NSTATS are
 *      nu_loss, nu_value, actor_loss, kl, entropy, vf0, vf1, vf_total (focops.py:158,208-213,166-176).      */
typedef struct fsrl_focops_config {
    float actor_lr, critic_lr;   /* two Adam optimisers: actor / both critics                              */
    float l2_reg;                /* critics: + l2_reg * sum(theta^2)                                       */
    float delta;                 /* pass-level mean-KL early stop                                          */
    float eta;                   /* rows with KL(new||old) > eta leave the actor loss                      */
    float tem_lambda;            /* temperature lambda                                                     */
    float max_grad_norm;         /* clip_grad_norm_ over the ACTOR parameters; 0 = off                     */
} fsrl_focops_config;
#define FSRL_FOCOPS_NSTATS 8
int fsrl_focops_init(fsrl_ctx* ctx, const fsrl_focops_config* cfg);
/* A/B and tests only: 1 = every FOCOPS minibatch step as the four-launch sequence (split-K weight gradients + their sum); 0 =
 * three launches whenever the minibatch has at most 512 rows (the default).  Same arithmetic per element, different
 * summation order of the weight gradients. */
int fsrl_focops_set_plan(fsrl_ctx* ctx, int32_t four_launch);
int fsrl_focops_set_nu(fsrl_ctx* ctx, double nu, double nu_loss);

/* ---- SAC-Lagrangian (fsrl/policy/sac_lag.py), off-policy on the HIP-resident replay store.
 *      Create the context with algo = FSRL_ALGO_SAC_LAG (obs_dim, act_dim <= 8, hidden, env_num,
 *      buffer_size, gamma are read from fsrl_config), then fsrl_sac_init.
 *      Parameter vectors in torch parameters() order:
 *        actor   : W1[H,Do] b1 W2[H,H] b2 Wmu[Da,H] bmu Wsig[Da,H] bsig   (ActorProb, conditioned sigma;
 *                  sac_lag_agent.py:126-134.  The mean is the head itself by default, ActorProb(unbounded=True),
 *                  or max_action * tanh(head): fsrl_sac_config.actor_mean)
 *        critics : for (reward, cost): pre1(W1[H,Do+Da] b1 W2 b2) pre2(..) last1(W[1,H] b) last2(W b)
 *                  (DoubleCritic, fsrl/utils/net/continuous.py:13-101)                          */
typedef struct fsrl_sac_config {
    float actor_lr, critic_lr, alpha_lr;   /* 5e-4, 1e-3, 3e-4                                   */
    float tau;                             /* Polyak, 0.05                                       */
    float alpha;                           /* fixed temperature when auto_alpha == 0             */
    float target_entropy;                  /* -act_dim                                           */
    int32_t n_step;                        /* 2 (sacl_cfg.py:21)                                 */
    int32_t auto_alpha;
    int32_t use_lagrangian;
    /* DDPG-Lagrangian (fsrl/policy/ddpg_lag.py:125-223) on the same entry points: deterministic actor
     * a = max_action * tanh(MLP(s)) with a target copy, ONE critic per metric (tianshou Critic on
     * concat(s, a)) with target copies, no entropy term.  Parameter vectors then are
     *   actor: W1 b1 W2 b2 W3[Da,H] b3      critics: for (reward, cost): W1[H,Do+Da] b1 W2 b2 W3[1,H] b3
     * fsrl_sac_params_get which = 3 returns the target actor.  exploration_sigma: std of the Gaussian
     * exploration noise fsrl_actor_sample adds (GaussianNoise, ddpg_lag_agent.py:80,160).              */
    int32_t deterministic;
    float exploration_sigma;
    /* How the Gaussian actor's mean head becomes the mean (ActorProb's `unbounded`, fsrl/utils/net/continuous.py):
     *   0 = the kind's default (SAC-Lag: mu = head; CVPO: mu = max_action * tanh(head)),
     *   1 = unbounded, mu = head,   2 = bounded, mu = max_action * tanh(head)   -- for either kind.
     * The action is a = tanh(mu + sigma * eps) either way.  deterministic = 1 (tianshou's Actor has no such option) takes 0 only. */
    int32_t actor_mean;
} fsrl_sac_config;
#define FSRL_ACTOR_MEAN_DEFAULT 0
#define FSRL_ACTOR_MEAN_UNBOUNDED 1
#define FSRL_ACTOR_MEAN_TANH 2
#define FSRL_SAC_NSTATS 10  /* rescaling, lagrangian, actor_safety, alpha_loss, alpha_value, actor_rew,
                               actor_total (sac_lag.py:231-257) then q0, q1, q_total (:203-208) */
int fsrl_sac_init(fsrl_ctx* ctx, const fsrl_sac_config* cfg);
/* A/B and tests only; plan is a 7-bit mask, 0..127 (default 0):
 *   bit 0 (1): split-K weight gradients (fb_wgrad_kernel) at every batch size (default: batches of up to 512 rows use the
 *              PPO step's one-workgroup-per-tile kernel; same products, different summation order);
 *   bit 1 (2): the sampler and the row gather as two launches (default: one launch);
 *   bit 2 (4): the float64 n-step targets (base_policy.py:453-512) as a launch of their own (default: the critics' tile
 *              launch computes its targets itself).  Layered contexts (hidden_sizes outside the fused kernels) ALWAYS run the
 *              stand-alone n-step launch, whatever the caller set;
 *   bit 3 (8): prefetch the next update's sample + gather on the side stream (double-buffered batch);
 *   bit 4 (16): sample + gather as ONE launch of their own (round 4: 10 launches per update).  Default (r5): the forward launch of
 *              both actors draws and gathers its own rows first (9 launches per update; fused two-layer networks only);
 *   bit 5 (32): no rider blocks.  Default (r6) where the actor's weight-gradient launch is fb_wgrad_kernel (batches above 512 rows):
 *              that launch leaves 150 CUs idle, and extra blocks of it draw + gather the NEXT update's batch into a second set of
 *              batch arrays, in stream order; the next update uses them if nothing that determines the sample changed (store
 *              contents, batch size, key, update count) and draws its own otherwise.  The reference's trainer runs its updates
 *              back to back between collects (offpolicy trainer: round(update_per_step * steps) calls of policy.update), so
 *              every update but the first after a collect finds its rows in place.
 *   bit 6 (64): the critics' split-K weight-gradient launch in plain block order.  Default (r6): XCD-aware order -- the blocks of one
 *              (network, split), which stream the same rows, behind one L2: 46 -> 20 MB of memory-side traffic per launch, same time.
 * Bits 1 .. 6 keep the same Philox counters, the same float64 operations and the same sums: bit-identical results. */
int fsrl_sac_set_plan(fsrl_ctx* ctx, int32_t plan);
int64_t fsrl_sac_param_count(const fsrl_ctx* ctx, int32_t which);    /* 0 actor, 1 critics         */
int fsrl_sac_params_set(fsrl_ctx* ctx, const float* actor, int64_t na, const float* critics, int64_t nc,
                        float log_alpha);   /* also copies critics -> critics_old, resets Adam    */
/* which: 0 actor, 1 critics, 2 critics_old (targets)                                            */
int fsrl_sac_params_get(fsrl_ctx* ctx, int32_t which, float* out, int64_t n, float* alpha_out);
/* Checkpoint load (policy.load_state_dict): overwrite ONE parameter set, same `which` as above; targets,
 * Adam moments and step counts are left alone.                                                        */
int fsrl_sac_params_put(fsrl_ctx* ctx, int32_t which, const float* in, int64_t n);
/* One SACLagrangian.update(batch_size, buffer) = sample + n-step targets + critic step + actor
 * step + alpha step + Polyak (sac_lag.py:185-269, base_policy.py:356-395,453-512).
 * Sampling: indices / eps_target / eps_pi are given TOGETHER (the caller's numpy / torch RNG
 * streams -- parity mode) or are all NULL (library RNG on the device: Philox4x32-10 keyed by
 * `seed` (0 = keep the current key), uniform over the stored rows -- nothing is staged from the host).
 * stats_out: FSRL_SAC_NSTATS floats, synchronous; NULL = the call only enqueues work and the row is
 * kept in a device ring for fsrl_sac_stats_drain.                                                  */
int fsrl_sac_update(fsrl_ctx* ctx, int32_t batch_size, const int64_t* indices, const float* eps_target,
                    const float* eps_pi, uint64_t seed, const double* lagrangians, double rescaling,
                    float* stats_out);
/* Statistics rows of the updates issued with stats_out == NULL since the last drain, oldest first
 * (the ring keeps the newest 4096).  Returns the number of rows written (>= 0) or an error code.   */
int64_t fsrl_sac_stats_drain(fsrl_ctx* ctx, float* out, int64_t max_rows);
/* The sample the last fsrl_sac_update used, either mode (tests: library-RNG updates can be replayed
 * through the caller-RNG arguments).                                                              */
int fsrl_sac_last_sample(fsrl_ctx* ctx, int64_t* indices, float* eps_target, float* eps_pi, int32_t batch_size);
/* ... and its n-step chains [n_step][batch_size] with their end bits (done | unfinished tail), as the update used them. */
int fsrl_sac_last_chain(fsrl_ctx* ctx, int64_t* chain_out, uint8_t* end_out, int32_t batch_size);

/* ---- Prioritised experience replay for SAC-Lagrangian / DDPG-Lagrangian contexts (fused or layered), solo or grouped: tianshou 0.5
 *      PrioritizedReplayBuffer / SegmentTree, which the reference reaches through critics_loss's batch.weight (sac_lag.py:189-201,
 *      ddpg_lag.py:170-179), learn's `batch.weight = td` (sac_lag.py:263, ddpg_lag.py:218) and post_process_fn's
 *      buffer.update_weight (base_policy.py:326-330).  One float64 sum tree over the whole store lives in HBM: 2 * bound nodes, bound
 *      = the next power of two at or above buffer_num * sub_size, the leaf of global slot env * sub_size + local = priority ** alpha,
 *      every internal node exactly left + right.  max_prio and min_prio (raw priorities) start at 1.
 *        a row reaching the store (fsrl_store_push, fsrl_store_fill)   leaf = max_prio ** alpha, max_prio as of the last update
 *                                                                      issued before the push
 *        fsrl_store_reset / fsrl_store_configure                       empty tree, both scalars back at 1
 *        fsrl_sac_update, library RNG     row b: u = word 0 of Philox block (b, 0, update count) * 2^-32 in float64, scalar = u * root;
 *                                         i = 1; while i < bound: i *= 2; l = tree[i]; if l < scalar: scalar -= l, i += 1; slot =
 *                                         i - bound.  n-step chain, end bits and noise as the uniform sampler forms them.
 *        fsrl_sac_update, caller RNG      the caller's indices; weights and priorities as below
 *        importance weight of a row       (leaf / min_prio) ** (-beta), with weight_norm divided by the batch's maximum, as float32;
 *                                         the critics' loss per Q-network is mean(td^2 * w), and the logged loss/q* are the weighted ones
 *        behind the critic step           td_avg = float32 mean over the update's Q-networks of Q_j - target (the values the step used);
 *                                         p = |td_avg| + float32 eps in float64; leaf[idx] = p ** alpha (duplicate indices: the highest
 *                                         batch position wins); max_prio = max(max_prio, max p), min_prio = min(min_prio, min p)
 *      A prioritised update draws its sample in a launch of its own, gathers in a second and computes the n-step targets in a third
 *      (the folds into other launches are off, and so is the sample drawn one update ahead: the next sample depends on this
 *      update's priorities).  Refused, with the reason in fsrl_last_error: CVPO contexts and fsrl_cvpo_group_create over a member that
 *      has it on; fsrl_per_enable on a context that is already in a SAC / CVPO group.
 *      Groups: fsrl_sac_group_create takes members that ALL have prioritised replay on (alpha, beta and weight_norm may differ) or all
 *      off, and names the two members that disagree otherwise.  fsrl_sac_group_update over prioritised members runs the same sequence
 *      with every member in each launch (one workgroup per member draws its sample and one writes its priorities; 13 launches per
 *      update for fused members whatever the group size) and leaves each member -- tree, last sample, chain, weights, TD averages --
 *      as its own fsrl_sac_update calls would.
 *      fsrl_per_enable         switches it on (again: from scratch); rows already stored get max_prio ** alpha = 1.
 *      fsrl_per_set_beta       the exponent of the NEXT sample's weights (PrioritizedReplayBuffer.set_beta).
 *      fsrl_per_update_weight  PrioritizedReplayBuffer.update_weight(indices, weights) from the host, n entries; waits.
 *      fsrl_per_state          leaves_out[n] (n = buffer_num * sub_size; NULL: none) and the scalars; total = the root.  Waits for
 *                              everything issued so far on both streams.
 *      fsrl_per_last_weights   the float32 weights of the last fsrl_sac_update's batch; fsrl_per_last_td its td_avg per row.   */
int fsrl_per_enable(fsrl_ctx* ctx, double alpha, double beta, int32_t weight_norm);
int fsrl_per_set_beta(fsrl_ctx* ctx, double beta);
int fsrl_per_update_weight(fsrl_ctx* ctx, const int64_t* indices, const double* weights, int64_t n);
int fsrl_per_state(fsrl_ctx* ctx, double* leaves_out, int64_t n, double* max_prio, double* min_prio, double* total);
int fsrl_per_last_weights(fsrl_ctx* ctx, float* w_out, int32_t batch_size);
int fsrl_per_last_td(fsrl_ctx* ctx, float* td_out, int32_t batch_size);

/* the actor for the collector: mu and sigma = exp(clamp(log sigma)) of the tanh-Gaussian policy   */
int fsrl_sac_actor_forward(fsrl_ctx* ctx, const float* obs, int32_t k, float* mu_out, float* sigma_out);

/* ---- Grouped SAC-Lagrangian and DDPG-Lagrangian updates: k SAC-Lag contexts (fsrl_sac_init, stochastic actor), or k DDPG-Lag
 *      contexts (fsrl_sac_init with deterministic = 1; act_dim up to 16), of one shape on one device, each stepped n_updates[i]
 *      times per call in lock step; every launch of an update (nine, whatever k is) carries all members that still have updates
 *      to run.  The group's kind is member 0's; the two kinds do not mix.  Members keep their own streams, stores, parameters,
 *      targets (DDPG-Lag: the target actor too, moved by the member's own tau in the actor's Adam pass), Adam state, alpha, Philox
 *      key and statistics ring, and stay ordinary contexts between calls (a call ends a member's resident actor; its next collect
 *      relaunches it).  Shapes (obs / act / hidden), n_step, auto_alpha and use_lagrangian must agree; learning rates, tau, seeds
 *      and store contents may differ.  Rejected with FSRL_EINVAL: a mixture of SAC-Lag and DDPG-Lag members (either order), CVPO
 *      contexts, a member listed twice or already in a SAC group.  A member destroyed before its group makes the next update fail; fsrl_sac_group_destroy still works.
 *      LAYERED members (fsrl_config.n_hidden: any other hidden_sizes) form a group when ALL members are layered and n_hidden,
 *      hidden_sizes[] and force_layered agree (a mix of fused and layered members, either order: "layered"; of widths or depths:
 *      "one network shape"; layered CVPO contexts are refused as CVPO contexts: their groups are fsrl_cvpo_group_*).  Each update is then the launch sequence of the
 *      member's own layered fsrl_sac_update (9 L + 19 launches for L hidden layers, whatever k is) with every launch carrying all
 *      members that still have updates to run, and a member's grouped update is bit-identical to its own at every k and batch size. */
typedef struct fsrl_sac_group fsrl_sac_group;
int fsrl_sac_group_create(fsrl_ctx** ctxs, int32_t k, fsrl_sac_group** out);   /* 1 <= k <= 16, members not owned */
int fsrl_sac_group_destroy(fsrl_sac_group* g);
/* n_updates[k] back-to-back fsrl_sac_update calls per member (library RNG), all members in lock step; a member with fewer updates
 * sits out the later ones (0: left untouched).  lagrangians [k][n_critics-1] (NULL when use_lagrangian is off), rescaling [k].
 * Statistics rows go to each member's own ring (fsrl_sac_stats_drain works unchanged).  Enqueues only: each member's stream
 * waits for the call before its next work.                                                                                   */
int fsrl_sac_group_update(fsrl_sac_group* g, int32_t batch_size, const int32_t* n_updates,
                          const double* lagrangians, const double* rescaling);

/* ---- CVPO (fsrl/policy/cvpo.py:71-430), on the replay context of SAC-Lagrangian: create the
 *      context with algo = FSRL_ALGO_SAC_LAG, then fsrl_cvpo_init INSTEAD of fsrl_sac_init.
 *      Networks (cvpo_agent.py:143-186): Gaussian actor, mu = max_action * tanh(head) by default or mu = head
 *      (fsrl_cvpo_config.actor_mean; the reference's MujocoBaseCfg sets unbounded=True), sigma = exp(clamp(head,
 *      -20, 2)), NOT squashed after sampling, with a hard-copied actor_old; per metric one SingleCritic
 *      (double_critic == 0; vector layout as DDPG-Lag's critics) or one DoubleCritic (layout as SAC's) with
 *      Polyak targets.  Parameters move through fsrl_sac_params_set / _get / _put (which = 3 is actor_old);
 *      the collector's actor through fsrl_sac_actor_forward / fsrl_actor_sample; the statistics ring through
 *      fsrl_sac_stats_drain with rows of FSRL_CVPO_NSTATS floats.                                            */
typedef struct fsrl_cvpo_config {
    float actor_lr, critic_lr;             /* 5e-4, 1e-3                           (cvpo_agent.py:101-102) */
    float tau;                             /* Polyak of critics_old, 0.05                                  */
    int32_t n_step;                        /* 2                                                            */
    int32_t double_critic;                 /* 0: SingleCritic (default), 1: DoubleCritic, predict = min    */
    int32_t sample_act_num;                /* K particles per state, 16                                    */
    int32_t estep_iter_num, mstep_iter_num;/* 1, 1                                                         */
    float estep_kl, estep_dual_max, estep_dual_lr;                 /* 0.02, 20, 0.02                       */
    float mstep_kl_mu, mstep_kl_std, mstep_dual_max, mstep_dual_lr;/* 0.005, 0.0005, 0.5, 0.1              */
    double qc_thres;                       /* cost_limit * (1 - gamma^T) / (1 - gamma) / T   (cvpo.py:138-141) */
    int32_t actor_mean;                    /* FSRL_ACTOR_MEAN_*: 0 = CVPO's default (tanh), 1 = unbounded, 2 = tanh */
} fsrl_cvpo_config;
#define FSRL_CVPO_NSTATS 17 /* estep_loss, dual0 (eta), dual1 (lambda)                      (cvpo.py:346-354)
                               kl_mu, kl_std, loss_kl, loss_mle, loss_total, dual_mu, dual_std, entropy (:405-415)
                               loss_q0, val_q0, loss_q1, val_q1, thres_q1, q_total           (:262-275)    */
int fsrl_cvpo_init(fsrl_ctx* ctx, const fsrl_cvpo_config* cfg);
/* CVPO.pre_update_fn (cvpo.py:178-188): zero the two M-step multipliers and their Adam state.             */
int fsrl_cvpo_pre_update(fsrl_ctx* ctx);
/* CVPO.post_update_fn (cvpo.py:190-193): actor_old <- actor.                                              */
int fsrl_cvpo_post_update(fsrl_ctx* ctx);
/* CVPO.update_cost_limit (cvpo.py:165-176): the new E-step threshold on Qc.                               */
int fsrl_cvpo_set_thres(fsrl_ctx* ctx, double qc_thres);
/* One CVPO.update(batch_size, buffer): sample + n-step targets (a' ~ actor, critics_old) + critic step +
 * E-step (K particles of actor_old through the UPDATED critics, Adam on (eta, lambda), softmax weights) +
 * M-step (weighted decoupled-Gaussian likelihood + KL multipliers, actor Adam) + Polyak (cvpo.py:206-430).
 * Sampling as fsrl_sac_update: indices [B], eps_target [B][Da] and eps_particles [K][B][Da] are given
 * together (caller RNG) or all NULL (Philox on the device).  stats_out: FSRL_CVPO_NSTATS floats or NULL.    */
int fsrl_cvpo_update(fsrl_ctx* ctx, int32_t batch_size, const int64_t* indices, const float* eps_target,
                     const float* eps_particles, uint64_t seed, float* stats_out);
/* out[0..3] = eta, lambda (estep_dual, clamped) and mstep_dual_mu, mstep_dual_std (stored unclipped).      */
int fsrl_cvpo_duals_get(fsrl_ctx* ctx, float* out4);
/* The K particles' N(0,1) block of the last update ([K][B][Da]); indices / eps_target: fsrl_sac_last_sample. */
int fsrl_cvpo_last_particles(fsrl_ctx* ctx, float* eps_particles, int64_t n);

/* ---- Grouped CVPO updates: k CVPO contexts (fsrl_cvpo_init) on one device, each stepped n_updates[i] times per call in lock
 *      step; every launch of an update (9 + 4 * mstep_iter_num, whatever k is) carries all members that still have updates to
 *      run.  Members keep their own streams, stores, parameters, targets, actor_old, Adam state, duals, Philox key and
 *      statistics ring, and stay ordinary contexts between calls: fsrl_cvpo_pre_update / _post_update / _set_thres and own
 *      fsrl_cvpo_update calls order against grouped calls on the member's stream (a call ends a member's resident actor; its
 *      next collect relaunches it).  Members must share what decides the launch structure: obs_dim, act_dim, the hidden layer
 *      widths, n_step, double_critic, sample_act_num, estep_iter_num, mstep_iter_num and fsrl_sac_set_plan bit 0; learning
 *      rates, tau, the KL bounds, dual learning rates and caps, qc_thres, seeds and store contents may differ.  Rejected with
 *      FSRL_EINVAL and the reason in fsrl_last_error: SAC-Lag and DDPG-Lag contexts, another device, a mismatch of the
 *      list above, a member listed twice or already in a SAC or CVPO group.  A member destroyed before its group makes the
 *      next update fail (FSRL_ESTATE); fsrl_cvpo_group_destroy still works.
 *      LAYERED members (fsrl_config.n_hidden: any other hidden_sizes) form a group when ALL members are layered and n_hidden,
 *      hidden_sizes[] and force_layered agree (a mix of fused and layered members, either order: "layered"; of widths or depths:
 *      "one network shape"; fsrl_sac_set_plan bit 0 does not apply).  Each update is then the launch sequence of the member's own
 *      layered fsrl_cvpo_update with every launch carrying all members that still have updates to run, without the second actor
 *      forward of an M iteration (it recomputes the first): 6 L + 15 + mstep_iter_num (2 L + 6) launches for L hidden layers,
 *      whatever k is, against 6 L + 15 + mstep_iter_num (3 L + 7) of the member's own update.  A member's grouped update is
 *      bit-identical to its own at every k and batch size.                                                                   */
typedef struct fsrl_cvpo_group fsrl_cvpo_group;
int fsrl_cvpo_group_create(fsrl_ctx** ctxs, int32_t k, fsrl_cvpo_group** out);   /* 1 <= k <= 16, members not owned */
int fsrl_cvpo_group_destroy(fsrl_cvpo_group* g);
/* n_updates[k] back-to-back fsrl_cvpo_update calls per member (library RNG: the member's Philox key, its update count as the
 * counter), all members in lock step; a member with fewer updates sits out the later ones (0: left untouched).  Statistics
 * rows go to each member's own ring (fsrl_sac_stats_drain).  Enqueues only: each member's stream waits for the call before its
 * next work.                                                                                                                */
int fsrl_cvpo_group_update(fsrl_cvpo_group* g, int32_t batch_size, const int32_t* n_updates);

/* ---- Lock-step collection for seeds that keep their own streams: k SAC-Lag, k DDPG-Lag or k CVPO contexts (FSRL_ALGO_SAC_LAG
 *      after fsrl_sac_init / fsrl_cvpo_init), or k on-policy contexts (see ON-POLICY members below), on one device collect with ONE call and ONE request per vector step to one resident actor
 *      kernel (a workgroup per member and 16-row tile, running the member's actor network; raw head rows come back through a
 *      pinned ring).  Per member every result is bit-identical to fsrl_collect_step on that member: its own store and side
 *      stream, its own noise stream, its own bounds.  The object is independent of the update groups: a member may also be in an
 *      fsrl_sac_group or fsrl_cvpo_group, keeps its own streams and its own resident actor, and is not owned.
 *      The kernel runs on a stream of the group's own.  Before it is launched that stream waits for everything the members have
 *      enqueued on their compute streams; it holds the actors' weights in registers, so it is told to end by everything that
 *      can change a member's actor or runs the member's actor itself (every member entry point but fsrl_store_push and the
 *      read-only queries: own updates, fsrl_sac_put_params, fsrl_sac_group_update / fsrl_cvpo_group_update, own
 *      fsrl_collect_step / fsrl_actor_sample), by fsrl_collect_group_actor_release, and by its idle timeout; the next step
 *      launches it again.
 *      LAYERED members of any of the three kinds (all members layered, one n_hidden / hidden_sizes[] / force_layered) have no resident
 *      kernel: a request is one launch sequence on the group's stream for all members -- the observation rows side by side in
 *      pinned memory, L + 1 linear launches with one job per member that has rows, one launch that leaves the raw head rows and
 *      completion words in pinned memory -- L + 2 launches per vector step instead of k (L + 2), any row count per member.  The
 *      releases listed above mark such a group instead of ending a kernel: its next request first waits for everything the
 *      members have enqueued on their compute streams; requests between two releases are ordered by the group's stream alone.
 *      ON-POLICY members.  The fourth kind of member is an on-policy context: CPO, TRPO-Lag, or a PPO-Lag / FOCOPS context that is
 *      not in an fsrl_group (one that is shares that group's stream and collects through fsrl_group_collect_step).  Only the actor
 *      matters to this object and every on-policy actor is the same Gaussian actor, so CPO and TRPO-Lag members may share a group;
 *      on-policy and replay members do not mix.  Fused members are served by the resident kernel of fsrl_group_collect_step (the
 *      on-policy head: means and the member's sigma_param row) with member 0's max_action, layered members by that call's L + 2
 *      launches, both with the ordering described above; nothing on the update side is grouped -- the members run their own
 *      fsrl_tr_begin / fsrl_cpo_learn / fsrl_trpo_learn (fsrl_ppo_update ...), each on its own streams.
 *      THREADS.  Members' entry points may run on several host threads at once (one thread per member's update): the release they
 *      all perform on this group's kernel is serialised inside the library, and it still waits for nothing on the device.  A member's
 *      entry point that runs CONCURRENTLY WITH A STEP of its collect group remains a caller error: the step would answer with
 *      parameters in the middle of a change.  Finish the step first, or the members' calls first.
 *      create rejects with FSRL_EINVAL and the reason, naming the member, in fsrl_last_error: a mix of on-policy and replay
 *      contexts, a mix of fused and layered contexts, another device, another network shape (obs_dim, act_dim, hidden; layered:
 *      hidden_sizes[], force_layered; on-policy: n_critics, which places the actor's parameters), a member listed twice or already
 *      in a collect group, k outside 1..16; replay members: contexts without fsrl_sac_init / fsrl_cvpo_init, mixed kinds, another
 *      actor_mean; on-policy members: a member of an fsrl_group, another max_action, another `unbounded`.
 *      A member destroyed before its group breaks it: later steps fail with FSRL_ESTATE, fsrl_collect_group_destroy still works. */
typedef struct fsrl_collect_group fsrl_collect_group;
int fsrl_collect_group_create(fsrl_ctx** ctxs, int32_t k, fsrl_collect_group** out);
int fsrl_collect_group_destroy(fsrl_collect_group* g);
/* fsrl_collect_step on every member in member order; arguments as fsrl_group_collect_step: row arrays concatenated over members,
 * k[m] / k_act[m] >= 0 rows of member m, act_low / act_high NULL or [members][act_dim].  Off the resident path
 * (fsrl_collect_group_actor_set_resident(0), a member that waits with stream synchronisations, a member asking for more than its
 * 16 * min(4, ceil(env_num / 16)) rows) every member's own actor call runs inside the same call: the same bits.             */
int fsrl_collect_group_step(fsrl_collect_group* g, const int32_t* k, const int32_t* env_ids, const float* obs, const float* act,
                            const double* rew, const double* cost, const uint8_t* terminated, const uint8_t* truncated,
                            const float* obs_next, int64_t* ptr_out, double* ep_rew_out, int32_t* ep_len_out, int64_t* ep_idx_out,
                            const int32_t* k_act, const float* obs_act, int32_t deterministic, int32_t bound_method,
                            const float* act_low, const float* act_high, float* act_out, float* env_act_out);
/* on = 0: no resident kernel; idle_timeout_us > 0 sets the idle timeout (default 2000, at most 1e6).  Ends a live kernel.
 * A group of layered members accepts the call and ignores it.                                                                  */
int fsrl_collect_group_actor_set_resident(fsrl_collect_group* g, int32_t on, double idle_timeout_us);
/* out3 = {kernel launches, requests served through the doorbell, 1 if the kernel is live now}; a group of layered members:
 * {requests, requests, 0}                                                                                                      */
int fsrl_collect_group_actor_resident_stats(fsrl_collect_group* g, int64_t* out3);
/* the collect is over: end the kernel now instead of at its idle timeout (a group of layered members: nothing to end)         */
int fsrl_collect_group_actor_release(fsrl_collect_group* g);

/* ---- a whole lock-step collect of a group over worker-process envs in ONE call: fsrl_collect_episodes of every member (the
 *      reference's FastCollector.collect(n_episode), fsrl/data/fast_collector.py:283-368), the members' envs stepped TOGETHER --
 *      every member's step (or reset) command is posted to its workers before the first one is waited for -- and one
 *      fsrl_group_collect_step / fsrl_collect_group_step per vector step for all members.  Per member the same calls in the same
 *      order as its own collect: same rows in the same slots, same noise stream.  A member that has its episodes contributes no
 *      rows from then on while the others go on.
 *      envs[k]: member m's env (no env twice); n[k]: its rows; ready / obs: the members' env ids / observations back to back, n[m]
 *      rows each; n_episode[k] >= 1; act_low / act_high: NULL or [k][act_dim].  Outputs per member [k]: env steps, summed cost,
 *      terminated / truncated counts, finished episodes; ep_rew_out / ep_len_out: n_episode[m] entries per member at prefix-sum
 *      offsets, in the order the loop met them.  t_env_act_out2 (may be NULL): seconds spent waiting for the env workers /
 *      in the step calls.  *failed_member_out: -1, or the member an argument error names (FSRL_EINVAL; nothing was posted or
 *      launched), or the member whose env failed (a dead worker, a worker that raised): the commands posted to the other
 *      members' envs have been waited for, the group's resident actor has ended and the group's and the members' streams are
 *      drained; only that member's env may be left with a half-handled command.  On success the resident actor ends with the call.
 *      Single-phase only (no counterpart of fsrl_collect_episodes_split).                                                    */
int fsrl_group_collect_episodes(fsrl_group* g, fsrl_shm_env* const* envs, const int32_t* n, const int32_t* ready, const float* obs,
                                const int32_t* n_episode, int32_t deterministic, int32_t bound_method, const float* act_low,
                                const float* act_high, int64_t* steps_out, double* total_cost_out, int32_t* term_out,
                                int32_t* trunc_out, double* ep_rew_out, int32_t* ep_len_out, int32_t* episodes_out,
                                double* t_env_act_out2, int32_t* failed_member_out);
int fsrl_collect_episodes_group(fsrl_collect_group* g, fsrl_shm_env* const* envs, const int32_t* n, const int32_t* ready,
                                const float* obs, const int32_t* n_episode, int32_t deterministic, int32_t bound_method,
                                const float* act_low, const float* act_high, int64_t* steps_out, double* total_cost_out,
                                int32_t* term_out, int32_t* trunc_out, double* ep_rew_out, int32_t* ep_len_out,
                                int32_t* episodes_out, double* t_env_act_out2, int32_t* failed_member_out);

/* ---- timing of the last update, measured with hipEvents on the compute stream --------- */
/* out[0] = process_fn ms, out[1] = learn ms (all passes), out[2] = fused fwd/bwd kernel
 * total ms over the update (sum of per-launch event pairs when profiling is enabled),
 * out[3] = number of fwd/bwd launches, out[4] (if n >= 5) = the raw event-bracket sum (no
 * overhead correction).                                                                   */
int fsrl_set_profiling(fsrl_ctx* ctx, int enable);
int fsrl_last_timing(fsrl_ctx* ctx, double* out, int32_t n);

/* The part of a PPO optimiser step (ppo_lag.py:224-243: forward/backward, clip, Adam = three dependent launches here) that no
 * kernel work can remove, measured on this device: empty kernels with the step's grids, block sizes and LDS footprints for a
 * minibatch of mb_rows rows, `iters` times back to back on the compute stream.  out_us[0..2] = one launch of the forward/backward,
 * weight-gradient and Adam grid behind itself, out_us[3] = the three behind each other (microseconds per launch / per triple). */
int fsrl_launch_floors(fsrl_ctx* ctx, int32_t mb_rows, int32_t iters, double* out_us);

/* ---- the one collective of the multi-GPU layout: independent agents, one process per GPU; once per epoch the
 *      ranks sum a short float64 metric vector [n_st, n_ep, sum rew, sum cost, ...] (fsrl_amd/parallel.py EPOCH_KEYS).  The
 *      reference has no multi-GPU code.  RCCL (ncclAllReduce, sum, float64, on the context's compute stream) is reached through
 *      dlopen -- the copy of librccl the process already uses (torch's, when torch.distributed runs "nccl"), else /opt/rocm's --
 *      so the library links against nothing and loads on boxes without RCCL.  The Python host may equally use torch.distributed
 *      (fsrl_amd.parallel.reduce_epoch does when no communicator was initialised here).
 *      fsrl_comm_unique_id: rank 0, 128 bytes (ncclUniqueId), handed to every rank by the caller (file / TCP / launcher store);
 *      fsrl_comm_init: every rank, collective; fsrl_metrics_allreduce: in place, 1 <= n <= 64, the identity without a communicator. */
int fsrl_comm_unique_id(uint8_t* id_out, int32_t cap);
int fsrl_comm_init(fsrl_ctx* ctx, int32_t rank, int32_t world, const uint8_t* id, int32_t id_bytes);
int fsrl_metrics_allreduce(fsrl_ctx* ctx, double* v, int32_t n);
int fsrl_comm_info(const fsrl_ctx* ctx, int32_t* rank_out, int32_t* world_out);
int fsrl_comm_destroy(fsrl_ctx* ctx);

/* ---- the trajectory archive (fsrl/data/traj_buf.py TrajectoryBuffer, fed as basic_collector.py:238-248 feeds it): every finished
 *      episode of the contexts that feed it, kept in HBM in the DSRL column layout -- observations / next_observations [rows][obs_dim]
 *      and actions [rows][act_dim] float32, rewards / costs float64, terminals / timeouts uint8 -- until fsrl_traj_export
 *      hands them to the host or fsrl_store_fill to a replay store; fsrl_traj_import reads exported columns back.
 *      A context that feeds an archive has a TAP on its store ingest: every row that goes through fsrl_store_push (so every collect
 *      call, solo, grouped or over worker-process envs) also reaches the archive, whatever the store's geometry does meanwhile
 *      (fsrl_store_reset, fsrl_store_configure, a sub-buffer that wraps).  The rows of an env are gathered in an open-episode area;
 *      when the episode ends its float64 reward and cost returns (sums in push order, as `current_rew += rew.item()`) are held
 *      against the window (traj_buf.py:71-73) and the episode is appended to the archive -- or dropped.  An episode that is still
 *      open is never exported.  The `actions` column holds the action the ENV received: BasePolicy.map_action (bound_method 0 none /
 *      1 clip / 2 tanh, then act_low / act_high, NULL = no scaling) of the pushed action, the very function -- and so bit for bit the
 *      values -- fsrl_collect_step hands out as env_act.  The store keeps the raw policy action, as before.
 *      Episodes longer than max_episode_len are dropped (and counted); the episode after one is intact.  The archive never
 *      overwrites: when an episode does not fit max_rows it compacts (dead rows come from fsrl_traj_keep / _replace), and when it
 *      still does not fit the push (or flush) that ends the episode returns FSRL_ENOMEM, the message naming max_rows; the episode
 *      is dropped and counted.  Episode ids are the commit serial numbers, from 0, over all sources.
 *      A context without a tap runs the code it ran before taps existed.  The archive is no part of fsrl_train_state_export.
 *      Not thread safe: the calls of one archive and the pushes of the contexts that feed it come from one thread.
 *
 *      fsrl_traj_create   ctx gives the device and (obs_dim, act_dim); it is NOT attached.  Memory: two sets of columns of max_rows
 *                         rows (a compaction copies from one to the other, so no run overlaps its destination).
 *      fsrl_traj_attach   a context has at most one tap; several contexts of one (obs_dim, act_dim) on the archive's device may feed
 *                         one archive (the seeds of a group).  Another shape or device: FSRL_EINVAL naming the field.  *source_out
 *                         (may be NULL): the number the episodes of this context carry (0, 1, ... in attach order).  Allocates the
 *                         context's open-episode area: 2 x env_num x max_episode_len rows.
 *      fsrl_traj_detach   finished episodes are archived first; open ones are discarded.  A context destroyed while attached detaches
 *                         itself; an archive destroyed first leaves its contexts untapped.
 *      fsrl_traj_abandon  the open episodes of this context are discarded (and counted): its envs were reset in mid-episode, as a
 *                         collector does at the end of a collect with the envs that were not needed for the episode count.
 *      fsrl_traj_flush    the synchronisation point: every row pushed so far is in the archive or in an open episode, and the device
 *                         work is complete.  _episodes and _counters report the state as of the last flush (_keep, _replace, _export
 *                         and _clear flush themselves).
 *      fsrl_traj_episodes the alive episodes in table order (commit order until _keep / _replace change it): id, rows, reward return,
 *                         cost return, source; every output may be NULL, *n_out is always set.
 *      fsrl_traj_keep     only these ids stay alive, in the order given = the new table order; the archive is compacted.
 *      fsrl_traj_replace  the newest episode takes victim_id's place in table order (traj_buf.py:89-93); the victim is dead.
 *      fsrl_traj_export   the alive episodes in table order, rows contiguous and chronological inside an episode: plain device-to-host
 *                         copies of the compacted columns.  Every column may be NULL (all NULL: only *rows_out).
 *      fsrl_traj_clear    drops every archived episode; open episodes go on.
 *      fsrl_traj_counters out[0..n): episodes committed, rejected by the window, dropped as longer than max_episode_len, compactions,
 *                         rows alive, episodes refused for lack of room, episodes alive, tap launches, tap host-to-device bytes, open
 *                         episodes abandoned, open trailing runs dropped by fsrl_traj_import, fsrl_store_fill launches,
 *                         fsrl_store_fill host-to-device copies.
 *
 *      Datasets in: the two calls that make the archive readable as well as writable.
 *      fsrl_traj_import   `rows` rows of host columns in the export layout (what fsrl_traj_export writes; cost, terminals or timeouts
 *                         may be NULL = all zero, not both flag columns).  An episode ends at every row where terminals | timeouts is
 *                         set; a trailing run without an end flag is an open episode, dropped and counted.  An imported episode is
 *                         committed exactly as a tapped one: float64 reward and cost returns summed on the host in row order, held
 *                         against the window and max_episode_len, id = the next commit serial number, `source` the caller's number;
 *                         the archive compacts when it lacks room, and when it still lacks room the call returns FSRL_ENOMEM, the
 *                         message naming max_rows -- that episode is dropped and counted, the ones accepted before (and after) it
 *                         stay.  Only accepted rows cross the bus: neighbouring accepted episodes go in one copy per column, on the
 *                         archive's own stream, and the call waits for them.  *episodes_out / *rows_out (may be NULL): accepted.
 *      fsrl_store_fill    pours alive episodes of the archive into ctx's store, in the order given (episode_ids == NULL: all of them,
 *                         in table order; n is then ignored).  Defined by a model: with e_j = (first_env + j) % buffer_num for the
 *                         j-th episode, the result is what this loop leaves -- for every j in order, for every row of episode j in
 *                         order, fsrl_store_push(ctx, &e_j, 1, obs, inv(act), rew, cost, terminal, timeout, next_obs, ...) -- in the
 *                         six store columns, the host flag mirror, every field of the sub-buffers' bookkeeping (index, size,
 *                         last_index, ep_rew, ep_len, ep_idx) and a bumped store version (device books, a prefetched sample and the
 *                         side -> compute stream join refresh as after a push).  Two intended differences: the rows are not tapped
 *                         (filling from an archive ctx itself feeds adds nothing to it), and the whole fill is ONE host-to-device
 *                         copy of a job table plus ONE launch on ctx's side stream.  A sub-buffer may wrap during a fill: where the
 *                         loop would write a slot more than once only the last write is planned, the launch writes every slot at most
 *                         once.  Rows in ctx's staging window land first; the archive is flushed first (fsrl_traj_flush).
 *                         inv is BasePolicy.map_action_inverse (base_policy.py:258-283) under the parameters of THIS call: with
 *                         act_low / act_high (NULL = no scaling) scale = high - low, + float32 eps where below eps, then
 *                         a = (a - low) * 2 / scale - 1 in float32, every operation rounded on its own, in that order; with
 *                         bound_method 2 (tanh) then a = (log(1 + a) - log(1 - a)) / 2.  One deliberate departure from the reference:
 *                         a is clamped to +-(1 - 2^-24) before the tanh inverse -- at +-1 the reference returns +-inf, which no update
 *                         survives, and a recorded, saturated tanh action is exactly +-1.  (The two logarithms are taken in float64 and
 *                         the result rounded once.)  0 none and 1 clip add nothing after the rescale.
 *                         Refused before the first write, the message naming the field: obs_dim / act_dim / device of ctx and the
 *                         archive differ, first_env outside [0, buffer_num), bound_method outside {0, 1, 2}, an episode id that is
 *                         unknown, dead or listed twice (episode_ids[i]) -- FSRL_EINVAL; ctx inside an update, or a target sub-buffer
 *                         with an episode in progress (ep_len != 0: fills go between collects) -- FSRL_ESTATE.
 *                         *rows_out (may be NULL): the rows the loop would have pushed.  */
typedef struct fsrl_traj fsrl_traj;
int fsrl_traj_create(fsrl_ctx* ctx, int64_t max_rows, int32_t max_episodes, int32_t max_episode_len, int32_t bound_method,
                     const float* act_low, const float* act_high, fsrl_traj** out);
int fsrl_traj_destroy(fsrl_traj* t);
int fsrl_traj_attach(fsrl_traj* t, fsrl_ctx* ctx, int32_t* source_out);
int fsrl_traj_detach(fsrl_traj* t, fsrl_ctx* ctx);
int fsrl_traj_abandon(fsrl_traj* t, fsrl_ctx* ctx);
int fsrl_traj_set_window(fsrl_traj* t, double rmin, double rmax, double cmin, double cmax);
int fsrl_traj_flush(fsrl_traj* t);
int fsrl_traj_episodes(fsrl_traj* t, int64_t cap, int32_t* ids_out, int32_t* rows_out, double* rew_out, double* cost_out,
                       int32_t* source_out, int64_t* n_out);
int fsrl_traj_keep(fsrl_traj* t, const int32_t* episode_ids, int64_t n);
int fsrl_traj_replace(fsrl_traj* t, int32_t victim_id);
int fsrl_traj_export(fsrl_traj* t, float* obs, float* next_obs, float* act, double* rew, double* cost, uint8_t* terminals,
                     uint8_t* timeouts, int64_t rows_cap, int64_t* rows_out);
int fsrl_traj_clear(fsrl_traj* t);
int fsrl_traj_counters(fsrl_traj* t, int64_t* out, int32_t n);
int fsrl_traj_import(fsrl_traj* t, int64_t rows, const float* obs, const float* next_obs, const float* act,
                     const double* rew, const double* cost, const uint8_t* terminals, const uint8_t* timeouts,
                     int32_t source, int64_t* episodes_out, int64_t* rows_out);
int fsrl_store_fill(fsrl_ctx* ctx, fsrl_traj* t, const int32_t* episode_ids, int64_t n, int32_t first_env,
                    int32_t bound_method, const float* act_low, const float* act_high, int64_t* rows_out);

/* ---- Device environments: envs written as device functions, and whole collects on the GPU for on-policy and replay contexts.
 *      (fsrl_amd/csrc/device_env.hpp, kernels_devcollect.hpp, host_devcollect.inc, host_devcollect_group.inc; INTEGRATION.md "Device environments")
 *
 *      A device env holds env_num envs of one kind in device memory: per env a state row, the current observation, the step count of
 *      the running episode and the env's reset ordinal.  Kinds:
 *        FSRL_DEVENV_POINT_CIRCLE  fsrl_amd/env/toy.py in float32: obs 6, act 2, state (pos, vel) = 4 floats; p = (radius, x_lim, dt);
 *                                  a reset draws pos ~ U(-0.5, 0.5)^2, vel = 0
 *        FSRL_DEVENV_LINEAR        SyntheticSafetyVectorEnv: s' = s @ A + act @ B + 0.05 N(0, 1), A[obs_dim][obs_dim] and
 *                                  B[act_dim][obs_dim] copied at creation; p = (cost_threshold); 2 <= obs_dim <= 64; state = obs;
 *                                  a reset draws s ~ N(0, 1)
 *      truncated = steps of the episode >= max_episode_steps, decided by the stepping kernel, not by the env.
 *      Random numbers: Philox4x32-10, key = seed * 0x9E3779B97F4A7C15 + 0x243F6A8885A308D3, counter = (env id, reset ordinal, step in
 *      the episode, stream << 28 | dimension / 4); streams 0 reset draws, 1 action noise, 2 step noise.  The reset ordinal of an env
 *      counts its resets since creation or the last fsrl_devenv_seed (which zeroes it and leaves the env states alone).
 *
 *      fsrl_devenv_create    ctx gives the device, obs_dim / act_dim must be the context's; env_num <= 64.  The envs are NOT reset.
 *      fsrl_devenv_reset / _step   the env as an ordinary vector env for the existing collectors: one small launch on the env's own
 *                            stream (a live resident actor keeps running) and a wait.  ids == NULL: envs 0 .. n - 1.  Outputs are per
 *                            listed env; after a step the env's observation is obs_next (a finished env is reset by the caller).
 *      fsrl_devenv_get_state / _set_state   tests: state [env_num][state floats] (4 / obs_dim), steps [env_num], ordinals [env_num];
 *                            every pointer may be NULL.  set_state recomputes the observations.
 *      fsrl_collect_device   FastCollector.collect(n_episode) as a whole on the device: actor, action noise, map_action, env step,
 *                            store write and episode bookkeeping in one workgroup that loops for up to max_steps_per_launch vector
 *                            steps per launch (<= 0: the default, 64; at most 4096); the host launches again until n_episode episodes
 *                            are complete, replays the launch's log of rows through the store's bookkeeping (as if fsrl_store_push had
 *                            been called once per vector step), and at the end resets ALL envs, as FastCollector.reset_env does.
 *                            A collect starts from envs 0 .. min(env_num, n_episode) - 1 in their current state.  Rows in the staging
 *                            window are flushed first, a live resident actor is ended first.  Outputs as fsrl_collect_episodes;
 *                            *launches_out (may be NULL): launches of the collect kernel.  The call is fsrl_collect_device_group's
 *                            launch with one member -- one kernel family, one host loop -- on an ungrouped context; its messages
 *                            name no member.
 *                            Replay contexts (after fsrl_sac_init / fsrl_cvpo_init): the fused actor's raw head row becomes the action
 *                            on the device, in float32 with every operation rounded on its own, as fsrl_collect_step forms it on the
 *                            host -- SAC-Lag a = tanh(m + sigma eps), CVPO a = m + sigma eps, with m = the head or max_action tanh(head)
 *                            (actor_mean) and sigma = exp(clamp(log sigma head, -20, 2)); DDPG-Lag a = max_action tanh(head) +
 *                            exploration_sigma eps; deterministic: eps = 0.  eps is the env's action stream, not the context's
 *                            xoshiro stream, and the device's tanhf / expf are not the host's: rows agree with fsrl_collect_step to
 *                            float32 rounding, not bit for bit.  With prioritised replay on, every written slot gets the leaf
 *                            fsrl_store_push would give it (max_prio ** alpha, ancestors repaired) by a launch behind the collect's.
 *                            Refused before anything changes, the message naming the reason: layered contexts, grouped contexts
 *                            (update groups, collect groups, replay groups), a context with a trajectory tap, a replay context
 *                            before fsrl_sac_init / fsrl_cvpo_init -- FSRL_EINVAL; a context inside an update -- FSRL_ESTATE; env_num
 *                            above 64 or above the store's sub-buffers, obs_dim / act_dim that differ from the context's, a devenv
 *                            of another context -- FSRL_EINVAL.  */
#define FSRL_DEVENV_POINT_CIRCLE 0
#define FSRL_DEVENV_LINEAR 1
typedef struct fsrl_devenv_config {
    int32_t kind, env_num, obs_dim, act_dim, max_episode_steps;
    uint64_t seed;
    float p[8];
    const float* A;
    const float* B;
} fsrl_devenv_config;
typedef struct fsrl_devenv fsrl_devenv;
int fsrl_devenv_create(fsrl_ctx* ctx, const fsrl_devenv_config* cfg, fsrl_devenv** out);
int fsrl_devenv_destroy(fsrl_devenv* env);
int fsrl_devenv_seed(fsrl_devenv* env, uint64_t seed);
int fsrl_devenv_reset(fsrl_devenv* env, const int32_t* ids, int32_t n, float* obs_out);
int fsrl_devenv_step(fsrl_devenv* env, const int32_t* ids, int32_t n, const float* env_act, float* obs_next_out, double* rew_out,
                     double* cost_out, uint8_t* term_out, uint8_t* trunc_out);
int fsrl_devenv_get_state(fsrl_devenv* env, float* state_out, int32_t* t_out, int64_t* ordinal_out);
int fsrl_devenv_set_state(fsrl_devenv* env, const float* state, const int32_t* t, const int64_t* ordinal);
int fsrl_collect_device(fsrl_ctx* ctx, fsrl_devenv* env, int32_t n_episode, int32_t deterministic, int32_t bound_method,
                        const float* act_low, const float* act_high, int32_t max_steps_per_launch, int64_t* steps_out,
                        double* total_cost_out, int32_t* term_count_out, int32_t* trunc_count_out, double* ep_rew_out,
                        int32_t* ep_len_out, int32_t* episodes_out, int32_t* launches_out);
/*      fsrl_collect_device_group   k seeds' collects in ONE looping launch: workgroup i of every launch runs member i's collect, the
 *                            loop of fsrl_collect_device on member i's store, envs and Philox counters, so that a member's rows, env
 *                            states, statistics and store_version are those of fsrl_collect_device on it, bit for bit.  1 <= k <= 16.
 *                            A free function over contexts: a member may be ungrouped or belong to an fsrl_group, an
 *                            fsrl_collect_group, an fsrl_sac_group or an fsrl_cvpo_group (its group's resident kernel is ended
 *                            first); fsrl_collect_device on such a context stays refused.  n_episode [k]; act_low / act_high
 *                            [k][act_dim] or both NULL; deterministic, bound_method and max_steps_per_launch are the call's.
 *                            Outputs per member: steps / total_cost / term_count / trunc_count / episodes [k]; ep_rew / ep_len
 *                            concatenated in member order, member i at offset n_episode[0] + .. + n_episode[i - 1] (sum of n_episode
 *                            entries); *launches_out (may be NULL): launches of the collect kernel, until EVERY member is finished
 *                            (a finished member's workgroup idles through the later ones).  The launches go on member 0's compute
 *                            stream, behind every member's compute stream; every launch is waited for.  Prioritised members get
 *                            their leaves by their own small launch behind each collect launch.  At the end ALL envs of ALL members
 *                            are reset.
 *                            Refused before anything changes, the message naming the member and the reason: k outside 1..16; a
 *                            context or env listed twice; members on several devices; whatever fsrl_collect_device refuses of a
 *                            member, the grouped clause apart; members that differ in obs_dim, act_dim, hidden or n_critics, in the
 *                            env kind or max_episode_steps, in the head kind (on-policy | SAC-Lag, CVPO | DDPG-Lag), in `unbounded`
 *                            (on-policy) or actor_mean (replay).  env_num, n_episode, env seeds, bounds, max_action, and prioritised
 *                            replay on or off may differ.  */
int fsrl_collect_device_group(fsrl_ctx** ctxs, fsrl_devenv** envs, int32_t k, const int32_t* n_episode, int32_t deterministic,
                              int32_t bound_method, const float* act_low, const float* act_high, int32_t max_steps_per_launch,
                              int64_t* steps_out, double* total_cost_out, int32_t* term_count_out, int32_t* trunc_count_out,
                              double* ep_rew_out, int32_t* ep_len_out, int32_t* episodes_out, int32_t* launches_out);
/*      fsrl_evaluate_device / fsrl_evaluate_device_group   the collect that stores nothing: FastCollector(policy, test_envs) with no
 *                            buffer.  The same loop, actor, action noise (the evaluated env's own Philox stream), env functions and
 *                            episode rule as fsrl_collect_device / _group, the same arguments and the same outputs -- on twin
 *                            contexts and twin envs an evaluation and a collect return the same numbers and leave the same env state,
 *                            bit for bit -- in the store-less form of the kernel: no slot, no write index, no row.  The solo call is
 *                            the grouped call with k = 1 (one table-driven launch family).  It changes the evaluated env (its state
 *                            arrays, as a collect does, the reset of ALL envs at the end included; its DcState, log and arguments)
 *                            and ends a live resident actor; it changes NOTHING else: store rows and flags, the per-env books, the
 *                            staging window, store_version, the prioritised-replay tree and max_prio, a replay context's
 *                            pre-drawn sample, every random stream of the library, the return statistics, other envs.  Episode
 *                            returns and lengths come from the log alone, through accumulators of the env.
 *                            Accepted where a collect is refused: a context with a trajectory tap (nothing reaches the archive), an
 *                            env with more envs than the store has sub-buffers (<= 64) and any store geometry, a context that is a
 *                            member of any kind of group (the solo call too).  Refused as a collect refuses, before anything
 *                            changes: layered contexts, an env of another context, shapes, bound_method, max_steps_per_launch above
 *                            4096, n_episode < 1, null outputs, a call inside an update (FSRL_ESTATE), a replay context before
 *                            fsrl_sac_init / fsrl_cvpo_init; in the grouped call also what members must agree on, the member named.  */
int fsrl_evaluate_device(fsrl_ctx* ctx, fsrl_devenv* env, int32_t n_episode, int32_t deterministic, int32_t bound_method,
                         const float* act_low, const float* act_high, int32_t max_steps_per_launch, int64_t* steps_out,
                         double* total_cost_out, int32_t* term_count_out, int32_t* trunc_count_out, double* ep_rew_out,
                         int32_t* ep_len_out, int32_t* episodes_out, int32_t* launches_out);
int fsrl_evaluate_device_group(fsrl_ctx** ctxs, fsrl_devenv** envs, int32_t k, const int32_t* n_episode, int32_t deterministic,
                               int32_t bound_method, const float* act_low, const float* act_high, int32_t max_steps_per_launch,
                               int64_t* steps_out, double* total_cost_out, int32_t* term_count_out, int32_t* trunc_count_out,
                               double* ep_rew_out, int32_t* ep_len_out, int32_t* episodes_out, int32_t* launches_out);
/*      fsrl_collect_device_layered / fsrl_evaluate_device_layered   the two _group calls for LAYERED contexts (hidden_sizes of any
 *                            depth and width, or force_layered): the same arguments, outputs, checks, launch loop, log replay,
 *                            prioritised-replay launches and reset of all envs at the end, with one looping kernel for every shape
 *                            in the launch -- a workgroup per member that streams the actor's weights from L2 every vector step and
 *                            keeps its activations in a workspace of 2 x 64 x round_up(max(widest layer, obs_dim), 4) floats the env
 *                            owns from its first layered collect on.  Every output element of a layer is accumulated by the MFMA
 *                            sequence of the layered forward launches, so a deterministic on-policy collect stores the actions
 *                            fsrl_collect_step computes on the same context, bit for bit; replay contexts agree to float32
 *                            rounding, as in fsrl_collect_device.  k = 1 is the solo collect (its failures name no member);
 *                            members may sit in any kind of group or in none.
 *                            Refused before anything changes: a fused member (the message names fsrl_collect_device /
 *                            fsrl_evaluate_device, which keep their refusal of layered contexts); members whose hidden_sizes[] or
 *                            force_layered differ; everything fsrl_collect_device_group / fsrl_evaluate_device_group refuse.  */
int fsrl_collect_device_layered(fsrl_ctx** ctxs, fsrl_devenv** envs, int32_t k, const int32_t* n_episode, int32_t deterministic,
                              int32_t bound_method, const float* act_low, const float* act_high, int32_t max_steps_per_launch,
                              int64_t* steps_out, double* total_cost_out, int32_t* term_count_out, int32_t* trunc_count_out,
                              double* ep_rew_out, int32_t* ep_len_out, int32_t* episodes_out, int32_t* launches_out);
int fsrl_evaluate_device_layered(fsrl_ctx** ctxs, fsrl_devenv** envs, int32_t k, const int32_t* n_episode, int32_t deterministic,
                               int32_t bound_method, const float* act_low, const float* act_high, int32_t max_steps_per_launch,
                               int64_t* steps_out, double* total_cost_out, int32_t* term_count_out, int32_t* trunc_count_out,
                               double* ep_rew_out, int32_t* ep_len_out, int32_t* episodes_out, int32_t* launches_out);

#ifdef __cplusplus
}
#endif
#endif /* FSRL_HIP_H */
