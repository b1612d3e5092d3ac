// host_comm.inc -- the ONE collective of the multi-GPU layout inside the C ABI: fsrl_metrics_allreduce (SURVEY 8b / 8e; part
// of fsrl_hip.hip).  Independent agents, one process per GPU; once per epoch every rank contributes a short float64 vector
// (<= 64 entries) and gets the element-wise sum back -- ncclAllReduce(sum, float64) on the context's compute stream, RCCL over
// xGMI.  A 512-byte message is latency-bound: no ring / tree tuning, no overlap to arrange.
//
// RCCL is reached through dlopen, not linked: a process that already runs torch.distributed's "nccl" backend has torch's own
// copy of librccl loaded, and two copies in one process are one too many -- the already loaded one is taken when there is one
// (RTLD_NOLOAD), /opt/rocm's otherwise.  The library stays loadable on boxes without RCCL; the calls then fail with FSRL_ESTATE.
#include <dlfcn.h>

#define FSRL_COMM_ID_BYTES 128      // sizeof(ncclUniqueId)
#define FSRL_COMM_MAX 64

struct FsrlUniqueId { char internal[FSRL_COMM_ID_BYTES]; };
typedef int (*nccl_get_unique_id_t)(FsrlUniqueId*);
typedef int (*nccl_comm_init_rank_t)(void** comm, int nranks, FsrlUniqueId id, int rank);
typedef int (*nccl_all_reduce_t)(const void* send, void* recv, size_t count, int dtype, int op, void* comm, hipStream_t s);
typedef int (*nccl_comm_destroy_t)(void* comm);
typedef const char* (*nccl_get_error_string_t)(int);

struct RcclApi {
    void* handle = nullptr;
    nccl_get_unique_id_t get_unique_id = nullptr;
    nccl_comm_init_rank_t comm_init_rank = nullptr;
    nccl_all_reduce_t all_reduce = nullptr;
    nccl_comm_destroy_t comm_destroy = nullptr;
    nccl_get_error_string_t err = nullptr;
};
static RcclApi g_rccl;

static int rccl_load() {
    if (g_rccl.handle) return 0;
    void* h = nullptr;
    for (const char* name : {"librccl.so", "librccl.so.1"}) {
        h = dlopen(name, RTLD_NOW | RTLD_NOLOAD);              // the copy this process already uses (torch's), if any
        if (h) break;
    }
    if (!h)
        for (const char* name : {"librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so"}) {
            h = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (h) break;
        }
    if (!h) return fail(FSRL_ESTATE, "RCCL is not available in this process (dlopen librccl.so: %s)", dlerror());
    RcclApi a;
    a.handle = h;
    a.get_unique_id = (nccl_get_unique_id_t)dlsym(h, "ncclGetUniqueId");
    a.comm_init_rank = (nccl_comm_init_rank_t)dlsym(h, "ncclCommInitRank");
    a.all_reduce = (nccl_all_reduce_t)dlsym(h, "ncclAllReduce");
    a.comm_destroy = (nccl_comm_destroy_t)dlsym(h, "ncclCommDestroy");
    a.err = (nccl_get_error_string_t)dlsym(h, "ncclGetErrorString");
    if (!a.get_unique_id || !a.comm_init_rank || !a.all_reduce || !a.comm_destroy)
        return fail(FSRL_ESTATE, "librccl.so lacks ncclGetUniqueId / ncclCommInitRank / ncclAllReduce / ncclCommDestroy");
    g_rccl = a;
    return 0;
}
#define RCCLCHK(expr)                                                                                          \
    do {                                                                                                       \
        int _r = (expr);                                                                                       \
        if (_r != 0) return fail(FSRL_EHIP, "%s failed: %s", #expr, g_rccl.err ? g_rccl.err(_r) : "rccl error"); \
    } while (0)

struct CommState {
    void* comm = nullptr;
    Mem mem;
    int rank = 0, world = 1;
    double* d_buf = nullptr; double* h_buf = nullptr;      // device / pinned staging of the vector
};

static void comm_free(fsrl_ctx* c) {
    CommState* m = c->comm;
    if (!m) return;
    if (m->comm && g_rccl.comm_destroy) (void)g_rccl.comm_destroy(m->comm);
    m->mem.release_all();
    delete m;
    c->comm = nullptr;
}

// rank 0 calls this and hands the 128 bytes to every rank (file, TCP, the launcher's store: the caller's business)
extern "C" int fsrl_comm_unique_id(uint8_t* id_out, int32_t cap) {
    CHECK_ARG(id_out && cap >= FSRL_COMM_ID_BYTES, "id_out must hold %d bytes", FSRL_COMM_ID_BYTES);
    int rc = rccl_load();
    if (rc) return rc;
    FsrlUniqueId id;
    RCCLCHK(g_rccl.get_unique_id(&id));
    memcpy(id_out, id.internal, FSRL_COMM_ID_BYTES);
    return 0;
}

// every rank, same id: joins the communicator (collective call: returns when all `world` ranks have arrived)
extern "C" int fsrl_comm_init(fsrl_ctx* c, int32_t rank, int32_t world, const uint8_t* id, int32_t id_bytes) {
    CHECK_ARG(c && id, "null argument");
    CHECK_ARG(world >= 1 && rank >= 0 && rank < world, "rank %d of world %d", rank, world);
    CHECK_ARG(id_bytes == FSRL_COMM_ID_BYTES, "the id is %d bytes", FSRL_COMM_ID_BYTES);
    ENTER_DEV(c);
    int rc = rccl_load();
    if (rc) return rc;
    comm_free(c);
    CommState* m = new CommState();
    c->comm = m;
    m->rank = rank; m->world = world;
    FsrlUniqueId uid;
    memcpy(uid.internal, id, FSRL_COMM_ID_BYTES);
    // a context never keeps a half-built communicator: fsrl_metrics_allreduce treats c->comm != null as usable
    const int r = g_rccl.comm_init_rank(&m->comm, world, uid, rank);
    if (r != 0) {
        m->comm = nullptr;
        comm_free(c);
        return fail(FSRL_EHIP, "ncclCommInitRank failed: %s", g_rccl.err ? g_rccl.err(r) : "rccl error");
    }
    if (m->mem.dev(&m->d_buf, FSRL_COMM_MAX * sizeof(double)) != hipSuccess ||
        m->mem.pinned(&m->h_buf, FSRL_COMM_MAX * sizeof(double)) != hipSuccess) {
        comm_free(c);
        return fail(FSRL_EHIP, "staging buffers of the metric exchange: %s", hipGetErrorString(hipGetLastError()));
    }
    return 0;
}

// in place: v[i] <- sum over ranks of v[i].  Without fsrl_comm_init (a single-GPU run) it is the identity.
extern "C" int fsrl_metrics_allreduce(fsrl_ctx* c, double* v, int32_t n) {
    CHECK_ARG(c && v, "null argument");
    CHECK_ARG(n >= 1 && n <= FSRL_COMM_MAX, "1 <= n <= %d metrics", FSRL_COMM_MAX);
    CommState* m = c->comm;
    if (!m) return 0;
    ENTER_DEV(c);
    hipStream_t s = c->compute;
    memcpy(m->h_buf, v, (size_t)n * sizeof(double));
    HIPCHK(hipMemcpyAsync(m->d_buf, m->h_buf, (size_t)n * sizeof(double), hipMemcpyHostToDevice, s));
    RCCLCHK(g_rccl.all_reduce(m->d_buf, m->d_buf, (size_t)n, /*ncclFloat64*/ 8, /*ncclSum*/ 0, m->comm, s));
    HIPCHK(hipMemcpyAsync(m->h_buf, m->d_buf, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    memcpy(v, m->h_buf, (size_t)n * sizeof(double));
    return 0;
}

extern "C" int fsrl_comm_info(const fsrl_ctx* c, int32_t* rank_out, int32_t* world_out) {
    CHECK_ARG(c && rank_out && world_out, "null argument");
    *rank_out = c->comm ? c->comm->rank : 0;
    *world_out = c->comm ? c->comm->world : 1;
    return 0;
}

extern "C" int fsrl_comm_destroy(fsrl_ctx* c) {
    CHECK_ARG(c, "null ctx");
    ENTER_DEV(c);
    (void)hipStreamSynchronize(c->compute);
    comm_free(c);
    return 0;
}
