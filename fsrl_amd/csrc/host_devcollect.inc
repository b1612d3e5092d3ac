// host_devcollect.inc -- device environments and whole collects on the GPU (part of fsrl_hip.hip; include/fsrl_hip.h "Device environments").
//
// fsrl_devenv_reset / _step make a device env an ordinary vector env: one small launch on the env's OWN stream (so that a resident
// actor on the compute stream keeps running: a launch behind it would wait for its idle timeout) over pinned host memory, and a wait.
// A device collect runs collect_device_group_kernel on the context's compute stream -- behind every update, in front of the next --
// once per max_steps_per_launch vector steps, reads the launch's DcState and log back and replays the log through the bookkeeping of
// fsrl_store_push (devcollect_plan.hpp dc_replay_row: EnvBook, h_flags, store_version), so that the store, the episode statistics
// and everything derived from them are as if the rows had been pushed one vector step at a time.
// Replay contexts (SAC-Lag, DDPG-Lag, CVPO): the same kernel with their fused actor's parameters and its head arithmetic on the device
// (DC_HEAD_GAUSS / DC_HEAD_DDPG); with prioritised replay on, a small launch behind every collect launch gives the rows' slots their
// leaves (host_per.inc per_devcollect).
// This file holds what ONE member of such a call needs: the checks, the entry and the log replay (devcollect_check, devcollect_begin,
// devcollect_replay).  The launch loop and all four entry points -- fsrl_collect_device, fsrl_evaluate_device and their _group forms
// -- are in host_devcollect_group.inc, behind the SAC code: the solo calls are the one-member launch.
// Evaluations go through the same checks and entry with `store = false` -- whatever concerns the store is skipped, nothing of the
// context but its resident actor is touched -- and replay the log through the env's own accumulators.
// Layered contexts come in through fsrl_collect_device_layered / fsrl_evaluate_device_layered: the same checks, entry, loop and replay
// with `layered = true`, lay_collect_kernel (kernels_devcollect_layered.hpp) in the launch and the env's activation workspace.
#include "kernels_devcollect_layered.hpp"
static bool sac_devcollect_head(fsrl_ctx* c, DevCollectArgs* a, int* head, bool layered);      // defined with the SAC / CVPO code
static bool devcollect_lay_actor(fsrl_ctx* c, const float** P, const LayNet** net, int* hmax);    // ... and behind the layered code
static int sac_devcollect_enter(fsrl_ctx* c);

struct fsrl_devenv {
    fsrl_ctx* c = nullptr;
    fsrl_devenv_config cfg{};
    Mem mem;
    uint64_t key = 0;
    hipStream_t es = nullptr;           // reset / step launches
    DevEnvArrays ea{};
    float *dA = nullptr, *dB = nullptr;
    char* h_io = nullptr;               // pinned: ids | act | obs | rew | cost | flags, for env_num rows
    DcState* d_state = nullptr; DcState* h_state = nullptr;     // device / pinned
    DcLogRow* d_log = nullptr; DcLogRow* h_log = nullptr; int log_steps = 0;
    int32_t* d_slot = nullptr;          // [log_steps][env_num]: the log rows' store slots (prioritised replay's leaves)
    DevCollectArgs* d_args = nullptr; DevCollectArgs* h_args = nullptr;     // the collect kernel's arguments: device / pinned
    // the launch loop's (host_devcollect_group.inc): made by the env's first collect or evaluation in that role and kept
    // (devcollect_group_ensure, devcollect_group_run); the table goes with `mem`, the events in devenv_free
    hipEvent_t g_ready = nullptr;       // a later member on a stream of its own: that stream as the call found it
    hipEvent_t g_done = nullptr;        // member 0's env: behind the launch
    DevCollectGroupTable* d_tab = nullptr; DevCollectGroupTable* h_tab = nullptr;      // member 0's env: the member table, device / pinned
    // layered collects: the activation workspace [2][DC_MAX_ENVS][ws_ld], made by the env's first layered collect (an env belongs to
    // one context, so once), and member 0's env: the layered member table, device / pinned
    float* d_ws = nullptr; int ws_ld = 0;
    LayCollectTable* d_ltab = nullptr; LayCollectTable* h_ltab = nullptr;
    DcEvalAcc acc[DC_MAX_ENVS] = {};    // fsrl_evaluate_device: the running episode of every env, from the log alone
};
static uint64_t devenv_key(uint64_t seed) { return seed * 0x9E3779B97F4A7C15ull + 0x243F6A8885A308D3ull; }
static DevEnvParams devenv_params(const fsrl_devenv* v) {
    DevEnvParams P{};
    P.kind = v->cfg.kind; P.env_num = v->cfg.env_num; P.Do = v->cfg.obs_dim; P.Da = v->cfg.act_dim; P.max_steps = v->cfg.max_episode_steps;
    memcpy(P.p, v->cfg.p, sizeof(P.p));
    P.A = v->dA; P.B = v->dB;
    return P;
}
struct DevEnvIoLayout { int32_t* ids; float* act; float* obs; double* rew; double* cost; uint32_t* flags; };
static DevEnvIoLayout devenv_io(const fsrl_devenv* v) {
    const size_t n = (size_t)v->cfg.env_num, Do = (size_t)v->cfg.obs_dim, Da = (size_t)v->cfg.act_dim;
    char* b = v->h_io;
    DevEnvIoLayout l;
    l.rew = (double*)b; l.cost = l.rew + n;
    l.ids = (int32_t*)(l.cost + n); l.flags = (uint32_t*)(l.ids + n);
    l.act = (float*)(l.flags + n); l.obs = l.act + n * Da;
    (void)Do;
    return l;
}
static size_t devenv_io_bytes(int n, int Do, int Da) { return (size_t)n * (8 + 8 + 4 + 4 + 4 * (size_t)(Do + Da)); }

static void devenv_free(fsrl_devenv* v) {
    if (!v) return;
    if (v->es) { (void)hipStreamSynchronize(v->es); (void)hipStreamDestroy(v->es); }
    v->mem.release_all();
    if (v->g_ready) (void)hipEventDestroy(v->g_ready);
    if (v->g_done) (void)hipEventDestroy(v->g_done);
    delete v;
}

extern "C" int fsrl_devenv_create(fsrl_ctx* c, const fsrl_devenv_config* cfg, fsrl_devenv** out) {
    CHECK_ARG(c && cfg && out, "null argument");
    CHECK_ARG(cfg->kind == FSRL_DEVENV_POINT_CIRCLE || cfg->kind == FSRL_DEVENV_LINEAR, "kind %d: no such device env", cfg->kind);
    CHECK_ARG(cfg->env_num >= 1 && cfg->env_num <= DC_MAX_ENVS, "env_num %d: a device env holds 1 .. %d envs", cfg->env_num, DC_MAX_ENVS);
    CHECK_ARG(cfg->obs_dim == c->cfg.obs_dim && cfg->act_dim == c->cfg.act_dim,
              "env shape (obs_dim %d, act_dim %d) != context shape (obs_dim %d, act_dim %d)", cfg->obs_dim, cfg->act_dim, c->cfg.obs_dim,
              c->cfg.act_dim);
    CHECK_ARG(cfg->act_dim >= 1 && cfg->act_dim <= FSRL_MAX_ACT, "act_dim %d above %d", cfg->act_dim, FSRL_MAX_ACT);
    CHECK_ARG(cfg->max_episode_steps >= 1, "max_episode_steps must be >= 1");
    if (cfg->kind == FSRL_DEVENV_POINT_CIRCLE) {
        CHECK_ARG(cfg->obs_dim == 6 && cfg->act_dim == 2, "the point-circle env has obs_dim 6 and act_dim 2");
    } else {
        CHECK_ARG(cfg->obs_dim >= 2 && cfg->obs_dim <= DEVENV_STATE, "the linear env takes 2 <= obs_dim <= %d", DEVENV_STATE);
        CHECK_ARG(cfg->A && cfg->B, "the linear env needs A[obs_dim][obs_dim] and B[act_dim][obs_dim]");
    }
    HIPCHK(hipSetDevice(c->device));
    fsrl_devenv* v = new fsrl_devenv();
    v->c = c; v->cfg = *cfg; v->cfg.A = nullptr; v->cfg.B = nullptr;
    v->key = devenv_key(cfg->seed);
    const size_t n = (size_t)cfg->env_num, Do = (size_t)cfg->obs_dim, Da = (size_t)cfg->act_dim;
    auto bail = [&](hipError_t e, const char* what) {
        devenv_free(v);
        return fail(FSRL_EHIP, "%s failed: %s", what, hipGetErrorString(e));
    };
#define DEVENV_TRY(expr) do { const hipError_t _e = (expr); if (_e != hipSuccess) return bail(_e, #expr); } while (0)
    DEVENV_TRY(hipStreamCreateWithFlags(&v->es, hipStreamNonBlocking));
    DEVENV_TRY(v->mem.dev(&v->ea.state, n * DEVENV_STATE * 4));
    DEVENV_TRY(v->mem.dev(&v->ea.obs, n * Do * 4));
    DEVENV_TRY(v->mem.dev(&v->ea.nxt, n * Do * 4));
    DEVENV_TRY(v->mem.dev(&v->ea.t, n * 4));
    DEVENV_TRY(v->mem.dev(&v->ea.ordinal, n * 8));
    DEVENV_TRY(hipMemset(v->ea.state, 0, n * DEVENV_STATE * 4));
    DEVENV_TRY(hipMemset(v->ea.obs, 0, n * Do * 4));
    DEVENV_TRY(hipMemset(v->ea.nxt, 0, n * Do * 4));
    DEVENV_TRY(hipMemset(v->ea.t, 0, n * 4));
    DEVENV_TRY(hipMemset(v->ea.ordinal, 0, n * 8));
    if (cfg->kind == FSRL_DEVENV_LINEAR) {
        DEVENV_TRY(v->mem.dev(&v->dA, Do * Do * 4));
        DEVENV_TRY(v->mem.dev(&v->dB, Da * Do * 4));
        DEVENV_TRY(hipMemcpy(v->dA, cfg->A, Do * Do * 4, hipMemcpyHostToDevice));
        DEVENV_TRY(hipMemcpy(v->dB, cfg->B, Da * Do * 4, hipMemcpyHostToDevice));
    }
    DEVENV_TRY(v->mem.pinned(&v->h_io, devenv_io_bytes((int)n, (int)Do, (int)Da)));
    DEVENV_TRY(v->mem.dev(&v->d_state, sizeof(DcState)));
    DEVENV_TRY(v->mem.pinned(&v->h_state, sizeof(DcState)));
    DEVENV_TRY(v->mem.dev(&v->d_args, sizeof(DevCollectArgs)));
    DEVENV_TRY(v->mem.pinned(&v->h_args, sizeof(DevCollectArgs)));
#undef DEVENV_TRY
    c->devenvs.push_back(v);
    *out = v;
    return 0;
}

static void devenv_ctx_gone(fsrl_ctx* c) { for (fsrl_devenv* v : c->devenvs) v->c = nullptr; }     // destroy is all such an env still takes
extern "C" int fsrl_devenv_destroy(fsrl_devenv* v) {
    if (!v) return 0;
    if (v->c) {
        (void)hipSetDevice(v->c->device);
        (void)hipStreamSynchronize(v->c->compute);      // a collect kernel reads the env's arrays
        v->c->devenvs.erase(std::remove(v->c->devenvs.begin(), v->c->devenvs.end(), v), v->c->devenvs.end());
    }
    devenv_free(v);
    return 0;
}

extern "C" int fsrl_devenv_seed(fsrl_devenv* v, uint64_t seed) {
    CHECK_ARG(v, "null env");
    HIPCHK(hipSetDevice(v->c->device));
    HIPCHK(hipStreamSynchronize(v->es));
    v->cfg.seed = seed;
    v->key = devenv_key(seed);
    HIPCHK(hipMemset(v->ea.ordinal, 0, (size_t)v->cfg.env_num * 8));
    return 0;
}

// ids (or NULL) of a reset / step call, checked and copied into the pinned block
static int devenv_take_ids(fsrl_devenv* v, const int32_t* ids, int32_t n, const DevEnvIoLayout& l) {
    CHECK_ARG(n >= 0 && n <= v->cfg.env_num, "%d rows but the device env has %d envs", n, v->cfg.env_num);
    if (!ids) return 0;
    uint64_t seen = 0;
    for (int i = 0; i < n; ++i) {
        CHECK_ARG(ids[i] >= 0 && ids[i] < v->cfg.env_num, "env id %d out of range", ids[i]);
        CHECK_ARG(!(seen >> ids[i] & 1ull), "env id %d is listed twice", ids[i]);
        seen |= 1ull << ids[i];
        l.ids[i] = ids[i];
    }
    return 0;
}

static int devenv_reset_launch(fsrl_devenv* v, const DevEnvIo& io, hipStream_t s) {
    const DevEnvParams P = devenv_params(v);
    const uint32_t k0 = (uint32_t)v->key, k1 = (uint32_t)(v->key >> 32);
    devenv_dispatch(v->cfg.kind, [&](auto env) {
        using Env = decltype(env);
        hipLaunchKernelGGL(devenv_reset_kernel<Env>, dim3(1), dim3(DC_MAX_ENVS), 0, s, P, v->ea, io, k0, k1);
    });
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int fsrl_devenv_reset(fsrl_devenv* v, const int32_t* ids, int32_t n, float* obs_out) {
    CHECK_ARG(v, "null env");
    HIPCHK(hipSetDevice(v->c->device));       // keeps a resident actor alive
    const DevEnvIoLayout l = devenv_io(v);
    if (!ids && n <= 0) n = v->cfg.env_num;
    int rc = devenv_take_ids(v, ids, n, l);
    if (rc) return rc;
    if (n == 0) return 0;
    DevEnvIo io{};
    io.ids = ids ? l.ids : nullptr; io.obs = l.obs; io.n = n;
    rc = devenv_reset_launch(v, io, v->es);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(v->es));
    if (obs_out) memcpy(obs_out, l.obs, (size_t)n * v->cfg.obs_dim * 4);
    return 0;
}

extern "C" int fsrl_devenv_step(fsrl_devenv* v, const int32_t* ids, int32_t n, const float* env_act, float* obs_next_out,
                                double* rew_out, double* cost_out, uint8_t* term_out, uint8_t* trunc_out) {
    CHECK_ARG(v && env_act && obs_next_out && rew_out && cost_out && term_out && trunc_out, "null argument");
    HIPCHK(hipSetDevice(v->c->device));       // keeps a resident actor alive
    const DevEnvIoLayout l = devenv_io(v);
    if (!ids && n <= 0) n = v->cfg.env_num;
    int rc = devenv_take_ids(v, ids, n, l);
    if (rc) return rc;
    if (n == 0) return 0;
    const int Do = v->cfg.obs_dim, Da = v->cfg.act_dim;
    memcpy(l.act, env_act, (size_t)n * Da * 4);
    DevEnvIo io{};
    io.ids = ids ? l.ids : nullptr; io.act = l.act; io.obs = l.obs; io.rew = l.rew; io.cost = l.cost; io.flags = l.flags; io.n = n;
    const DevEnvParams P = devenv_params(v);
    const uint32_t k0 = (uint32_t)v->key, k1 = (uint32_t)(v->key >> 32);
    devenv_dispatch(v->cfg.kind, [&](auto env) {
        using Env = decltype(env);
        hipLaunchKernelGGL(devenv_step_kernel<Env>, dim3(1), dim3(DC_MAX_ENVS), 0, v->es, P, v->ea, io, k0, k1);
    });
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(v->es));
    memcpy(obs_next_out, l.obs, (size_t)n * Do * 4);
    for (int i = 0; i < n; ++i) {
        rew_out[i] = l.rew[i]; cost_out[i] = l.cost[i];
        term_out[i] = (uint8_t)(l.flags[i] & 1u); trunc_out[i] = (uint8_t)((l.flags[i] >> 1) & 1u);
    }
    return 0;
}

extern "C" int fsrl_devenv_get_state(fsrl_devenv* v, float* state_out, int32_t* t_out, int64_t* ordinal_out) {
    CHECK_ARG(v, "null env");
    HIPCHK(hipSetDevice(v->c->device));
    HIPCHK(hipStreamSynchronize(v->es));
    HIPCHK(hipStreamSynchronize(v->c->compute));
    const int n = v->cfg.env_num, sd = devenv_state_dim(v->cfg.kind, v->cfg.obs_dim);
    if (state_out)
        HIPCHK(hipMemcpy2D(state_out, (size_t)sd * 4, v->ea.state, (size_t)DEVENV_STATE * 4, (size_t)sd * 4, (size_t)n, hipMemcpyDeviceToHost));
    if (t_out) HIPCHK(hipMemcpy(t_out, v->ea.t, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (ordinal_out) HIPCHK(hipMemcpy(ordinal_out, v->ea.ordinal, (size_t)n * 8, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int fsrl_devenv_set_state(fsrl_devenv* v, const float* state, const int32_t* t, const int64_t* ordinal) {
    CHECK_ARG(v, "null env");
    HIPCHK(hipSetDevice(v->c->device));
    HIPCHK(hipStreamSynchronize(v->es));
    HIPCHK(hipStreamSynchronize(v->c->compute));
    const int n = v->cfg.env_num, sd = devenv_state_dim(v->cfg.kind, v->cfg.obs_dim);
    if (t) for (int e = 0; e < n; ++e) CHECK_ARG(t[e] >= 0, "t[%d] is negative", e);
    if (ordinal) for (int e = 0; e < n; ++e) CHECK_ARG(ordinal[e] >= 0, "ordinal[%d] is negative", e);
    if (state)
        HIPCHK(hipMemcpy2D(v->ea.state, (size_t)DEVENV_STATE * 4, state, (size_t)sd * 4, (size_t)sd * 4, (size_t)n, hipMemcpyHostToDevice));
    if (t) HIPCHK(hipMemcpy(v->ea.t, t, (size_t)n * 4, hipMemcpyHostToDevice));
    if (ordinal) HIPCHK(hipMemcpy(v->ea.ordinal, ordinal, (size_t)n * 8, hipMemcpyHostToDevice));
    if (state) {
        const DevEnvParams P = devenv_params(v);
        devenv_dispatch(v->cfg.kind, [&](auto env) {
            using Env = decltype(env);
            hipLaunchKernelGGL(devenv_observe_kernel<Env>, dim3(1), dim3(DC_MAX_ENVS), 0, v->es, P, v->ea);
        });
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(v->es));
    }
    return 0;
}

// ---- one member of a collect.  Everything that can refuse the call is checked before anything is touched.  named = false: the solo
// calls; fsrl_collect_device refuses grouped contexts, and the _group calls run the same checks on every member without that clause.
// store = false (an evaluation, grouped or not): nothing is stored, so a tap, a group and the store's geometry are no reasons.
static int devcollect_check(const fsrl_ctx* c, const fsrl_devenv* v, int32_t n_episode, int32_t bound_method, const float* act_low,
                            const float* act_high, int32_t max_steps, bool named, bool store, bool layered) {
    const char* const what = store ? "collects" : "evaluations";
    CHECK_ARG(c && v, "null context / env");
    CHECK_ARG(v->c == c, "the device env was created on another context");
    if (!layered) CHECK_ARG(!c->lay, "device %s are not supported on layered contexts yet", what);
    else CHECK_ARG(c->lay, "a fused context (two hidden layers of at most 256 units): its device %s go through %s", what,
                   store ? "fsrl_collect_device" : "fsrl_evaluate_device");
    if (!named && store && !layered)
        CHECK_ARG(!c->group && !c->cgroup && !c->sac_group && !c->cvpo_group, "device collects are not supported on grouped contexts yet");
    if (ctx_is_replay(c)) {
        const float* P; const ModelDesc* md; const LayNet* net; int hmax;
        CHECK_ARG(layered ? devcollect_lay_actor(const_cast<fsrl_ctx*>(c), &P, &net, &hmax) : sac_actor_resident_args(const_cast<fsrl_ctx*>(c), &P, &md),
                  "device %s on replay contexts (SAC-Lag, DDPG-Lag, CVPO) need fsrl_sac_init / fsrl_cvpo_init first", what);
        CHECK_ARG(sac_raw_cols(c) <= FSRL_MAX_ACT, "the actor's %d head outputs do not fit a head row of %d", sac_raw_cols(c), FSRL_MAX_ACT);
    }
    if (store) CHECK_ARG(!c->tap, "device collects are not supported on a context with a trajectory tap attached yet");
    if (c->in_update)
        return fail(FSRL_ESTATE, "%s%s inside an update", store ? "fsrl_collect_device" : "fsrl_evaluate_device",
                    layered ? "_layered" : named ? "_group" : "");
    CHECK_ARG(v->cfg.env_num <= DC_MAX_ENVS, "env_num %d above %d", v->cfg.env_num, DC_MAX_ENVS);
    if (store) CHECK_ARG(v->cfg.env_num <= c->active_envs, "env_num %d but the store has %d sub-buffers", v->cfg.env_num, c->active_envs);
    CHECK_ARG(v->cfg.obs_dim == c->cfg.obs_dim && v->cfg.act_dim == c->cfg.act_dim, "env shape (obs_dim %d, act_dim %d) != context shape",
              v->cfg.obs_dim, v->cfg.act_dim);
    CHECK_ARG(n_episode >= 1, "n_episode must be >= 1");
    CHECK_ARG(bound_method >= 0 && bound_method <= 2, "bound_method: 0 none, 1 clip, 2 tanh");
    CHECK_ARG((act_low == nullptr) == (act_high == nullptr), "act_low and act_high are given together");
    CHECK_ARG(max_steps <= DC_MAX_STEPS, "max_steps_per_launch %d above %d", max_steps, DC_MAX_STEPS);
    if (store) CHECK_ARG(c->sub_size >= 1 && c->maxsize <= INT_MAX, "the store's geometry does not fit a device collect");
    return 0;
}

// What a collect does on entry, for one context: its resident actor ends (and through the release hooks its group's), the env's own
// stream is waited for, the staging window lands, the log holds max_steps vector steps, and the initial DcState and the kernel's
// arguments go up on the context's compute stream.  *P / *md / *head: whose actor the kernel runs.
// store = false: the staging window stays as it is, the write indices, the store's pointers and the slot array are not arguments,
// a sample drawn ahead stays valid (no row is overwritten), and the env's episode accumulators start at zero.
// layered = true: the actor is (P, net) of devcollect_lay_actor, md stays null, and the env's activation workspace exists.
struct DcActor { const float* P; const ModelDesc* md; int head; const LayNet* net; };
static int devcollect_begin(fsrl_ctx* c, fsrl_devenv* v, int32_t n_episode, int32_t deterministic, int32_t bound_method,
                            const float* act_low, const float* act_high, int max_steps, DcActor* actor, bool store, bool layered) {
    const int n = v->cfg.env_num, Da = v->cfg.act_dim;
    ENTER_DEV(c);                                   // a live resident actor ends first
    HIPCHK(hipStreamSynchronize(v->es));            // the env's own launches are complete (they are, every call waits; cheap)
    int rc = store ? join_store(c) : 0;             // rows in the staging window land first; the side stream is in front of the kernel
    if (rc) return rc;
    if (v->log_steps < max_steps) {
        const size_t rows = (size_t)max_steps * n;
        HIPCHK(v->mem.regrow(v->log_steps, max_steps, max_steps, {Mem::D(&v->d_log, rows * sizeof(DcLogRow)),
                             Mem::D(&v->d_slot, rows * sizeof(int32_t)), Mem::H(&v->h_log, rows * sizeof(DcLogRow))}));
    }
    DcState& hs = *v->h_state;
    memset(&hs, 0, sizeof(hs));
    hs.n_live = dc_first_live(n, n_episode); hs.n_episode = n_episode;
    for (int e = 0; e < DC_MAX_ENVS; ++e) hs.live[e] = e < n ? e : 0;
    for (int e = 0; e < n && store; ++e) hs.index[e] = (int32_t)c->env[(size_t)e].index;
    if (!store) for (int e = 0; e < DC_MAX_ENVS; ++e) v->acc[e] = DcEvalAcc{0.0, 0};
    hipStream_t s = c->compute;
    HIPCHK(hipMemcpyAsync(v->d_state, &hs, sizeof(DcState), hipMemcpyHostToDevice, s));
    // the arguments travel through device memory: ~350 bytes of kernel arguments held in scalar registers next to tile_forward's own
    // pushed the 256-wide kernel over its 128-VGPR cap (scalar spills live in vector registers)
    DevCollectArgs& a = *v->h_args;
    a = DevCollectArgs{};
    a.ep = devenv_params(v); a.ea = v->ea; a.k0 = (uint32_t)v->key; a.k1 = (uint32_t)(v->key >> 32);
    if (store) { a.st = c->st; a.sub_size = c->sub_size; }
    a.state = v->d_state; a.log = v->d_log; a.max_steps = max_steps;
    a.deterministic = deterministic ? 1 : 0; a.bound_method = bound_method; a.scaled = act_low ? 1 : 0;
    for (int d = 0; d < Da && act_low; ++d) { a.low[d] = act_low[d]; a.high[d] = act_high[d]; }
    a.max_action = c->cfg.max_action;
    a.magic_per = div_magic(2 * v->cfg.obs_dim + Da); a.magic_da = div_magic(Da);
    // whose actor: the context's own networks, or a replay context's fused actor with its head arithmetic
    actor->head = DC_HEAD_ONPOLICY; actor->P = c->P; actor->md = &c->md; actor->net = nullptr;
    if (layered) {
        int hmax = 0;
        actor->md = nullptr;
        if (!devcollect_lay_actor(c, &actor->P, &actor->net, &hmax)) return fail(FSRL_ESTATE, "no layered actor network");
        const int ld = round_up(std::max(hmax, v->cfg.obs_dim), 4);        // layer 0's input, the observations, is gathered into it too
        HIPCHK(v->mem.regrow(v->ws_ld, ld, ld, {Mem::D(&v->d_ws, (size_t)2 * DC_MAX_ENVS * ld * sizeof(float))}));
    }
    if (ctx_is_replay(c)) {
        if ((!layered && !sac_actor_resident_args(c, &actor->P, &actor->md)) || !sac_devcollect_head(c, &a, &actor->head, layered))
            return fail(FSRL_ESTATE, "no %s actor network", layered ? "layered" : "fused");
        rc = store ? sac_devcollect_enter(c) : 0;
        if (rc) return rc;
        a.slots = store && c->per ? v->d_slot : nullptr;
    }
    HIPCHK(hipMemcpyAsync(v->d_args, v->h_args, sizeof(DevCollectArgs), hipMemcpyHostToDevice, s));
    return 0;
}

// One launch's log (in v->h_log, hs = what the kernel reported), row by row in the kernel's order, and the call's running totals.
// A collect's rows go through the bookkeeping of fsrl_store_push on the context's book, with one store_version bump per pushed
// vector step; an evaluation's through the env's own accumulators: the same totals and episodes, in the same order, and no book.
struct DcTotals { int64_t rows = 0; double total_cost = 0.0; int32_t terms = 0, truncs = 0, episodes = 0; };
static bool devcollect_state_sane(const DcState& hs, int max_steps, int n) {
    return hs.log_rows >= 0 && hs.log_rows <= max_steps * n && hs.steps >= 0 && hs.steps <= max_steps;
}
static int devcollect_replay(fsrl_ctx* c, fsrl_devenv* v, const DcState& hs, int32_t n_episode, DcTotals& t, double* ep_rew_out,
                             int32_t* ep_len_out, bool store) {
    const int n = v->cfg.env_num;
    for (int i = 0; i < hs.log_rows; ++i) {
        const DcLogRow& r = v->h_log[i];
        if (r.env < 0 || r.env >= n) return fail(FSRL_ESTATE, "device %s: log row %d names env %d", store ? "collect" : "evaluation", i, r.env);
        double er = 0.0; int32_t el = 0;
        const bool done = store ? dc_replay_row(c->env[(size_t)r.env], c->sub_size, c->h_flags.data(), r, &er, &el)
                                : dc_eval_row(v->acc[r.env], r, &er, &el);
        t.total_cost += r.cost;
        t.terms += (int32_t)(r.flags & 1u); t.truncs += (int32_t)((r.flags >> 1) & 1u);
        if (done) {
            if (t.episodes < n_episode) { ep_rew_out[t.episodes] = er; ep_len_out[t.episodes] = el; }
            ++t.episodes;
        }
    }
    t.rows += hs.log_rows;
    if (store) c->store_version += (uint64_t)hs.steps;
    return 0;
}
