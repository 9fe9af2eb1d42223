// nb_shard.inc -- the multi-GPU host side inside the library: one rank's share of a scene and the per-step exchange.
// Included at the end of nb_api.hip (it uses that file's planning and launch helpers).  Mirrors nenbody_amd/dist.py,
// which does the same over torch.distributed; this form needs no torch: RCCL is loaded with dlopen, or the host
// supplies the exchange.

namespace {

// ---- RCCL, resolved at run time (the library must load on hosts without it) -------------------------------
struct RcclId {
    char internal[NB_COMM_ID_BYTES];
};
static_assert(sizeof(RcclId) == 128, "ncclUniqueId is 128 bytes");
struct RcclApi {
    void *handle = nullptr;
    int (*GetUniqueId)(RcclId *) = nullptr;
    int (*CommInitRank)(void **comm, int nranks, RcclId id, int rank) = nullptr;
    int (*AllGather)(const void *send, void *recv, size_t sendcount, int datatype, void *comm, hipStream_t stream) = nullptr;
    int (*CommDestroy)(void *comm) = nullptr;
    // the pairs form's second exchange (point to point, grouped); a library without them keeps the ordered fold
    int (*Send)(const void *send, size_t count, int datatype, int peer, void *comm, hipStream_t stream) = nullptr;
    int (*Recv)(void *recv, size_t count, int datatype, int peer, void *comm, hipStream_t stream) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    // consensus among the ranks (nb_shard_verify_exchanges, nb_shard_choose_form): a collective other than the ones being checked
    int (*AllReduce)(const void *send, void *recv, size_t count, int datatype, int op, void *comm, hipStream_t stream) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    std::string why;
};
constexpr int kRcclInt8 = 0;  // ncclInt8 / ncclChar (rccl.h): the exchange moves bytes
constexpr int kRcclUint32 = 3, kRcclMax = 2;  // ncclUint32, ncclMax

RcclApi &rccl_api()
{
    static RcclApi *api = [] {
        RcclApi *a = new RcclApi();
        const char *env = std::getenv("NENBODY_RCCL");
        if (env && *env) a->handle = dlopen(env, RTLD_NOW | RTLD_LOCAL);
        // the copy already in the process first (a host that runs torch has torch's own librccl.so.1 loaded, built
        // against the HIP runtime that is live here), then the loader's search path, then the ROCm install
        if (!a->handle) a->handle = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD);
        if (!a->handle) a->handle = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!a->handle) a->handle = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!a->handle) {
            const char *e = dlerror();
            a->why = std::string("librccl.so.1 could not be loaded (set NENBODY_RCCL): ") + (e ? e : "unknown error");
            return a;
        }
        a->GetUniqueId = (decltype(a->GetUniqueId))dlsym(a->handle, "ncclGetUniqueId");
        a->CommInitRank = (decltype(a->CommInitRank))dlsym(a->handle, "ncclCommInitRank");
        a->AllGather = (decltype(a->AllGather))dlsym(a->handle, "ncclAllGather");
        a->CommDestroy = (decltype(a->CommDestroy))dlsym(a->handle, "ncclCommDestroy");
        a->GetErrorString = (decltype(a->GetErrorString))dlsym(a->handle, "ncclGetErrorString");
        a->Send = (decltype(a->Send))dlsym(a->handle, "ncclSend");
        a->Recv = (decltype(a->Recv))dlsym(a->handle, "ncclRecv");
        a->GroupStart = (decltype(a->GroupStart))dlsym(a->handle, "ncclGroupStart");
        a->GroupEnd = (decltype(a->GroupEnd))dlsym(a->handle, "ncclGroupEnd");
        a->AllReduce = (decltype(a->AllReduce))dlsym(a->handle, "ncclAllReduce");
        if (!a->GetUniqueId || !a->CommInitRank || !a->AllGather || !a->CommDestroy || !a->GetErrorString) {
            a->why = "the RCCL library lacks ncclGetUniqueId / ncclCommInitRank / ncclAllGather / ncclCommDestroy";
            a->handle = nullptr;
        }
        return a;
    }();
    return *api;
}

}  // namespace

struct nb_shard {
    uint32_t n = 0, slot = 0, first = 0, count = 0;
    int rank = 0, world = 1;
    nb_params p{};
    Plan plan{};
    hipStream_t stream = nullptr;
    float4 *pos[2] = {nullptr, nullptr};      // world*slot records each: the replica, ping-pong
    float4 *vel = nullptr;                    // this rank's velocities (slot records)
    float4 *velfull[2] = {nullptr, nullptr};  // boids: replicas of ALL velocities, built on first use
    float4 *pvstage = nullptr;                // boids, world > 1: [world][pos slot | vel slot], what ONE all-gather per step moves
    bool velfull_valid = false;
    void *scratch = nullptr;
    size_t scratch_bytes = 0;  // what `scratch` holds: the largest need of the forms this shard may take (it only ever grows)
    StatusWord status;       // sticky failure word of this shard's block-chain launches
    float *stage = nullptr;  // 3n floats: packing / unpacking
    float4 *inst = nullptr;
    int cur = 0;
    bool uploaded = false;
    uint64_t steps = 0;
    nb_gather_fn gather = nullptr;
    void *gather_user = nullptr;
    // FAST, equal ranks: every unordered pair once, the other ranks' halves leaving in a second exchange (nb_nbody_ring.inc)
    RingPlan ring{};           // partners == 0: the shape keeps the ordered fold
    bool ring_wanted = true;   // nb_shard_set_pairs
    float4 *sums = nullptr, *recv = nullptr;  // (partners + 1) * count and partners * count records
    nb_ring_fn ring_fn = nullptr;
    void *ring_user = nullptr;
    bool boids_split = false;      // nb_shard_set_boids_split: the boids step's j range in slices (a tolerance form)
    float4 *boids_partial = nullptr;
    size_t boids_partial_bytes = 0;
    // FAST with the exchange overlapped (nb_shard_set_overlap): a step folds this rank's own slot of the snapshot while the
    // all-gather of the other slots is still in flight on `xstream`, then waits for it and folds the rest
    bool overlap = false, gather_pending = false;
    PhasePlan phases{};
    hipStream_t xstream = nullptr;
    hipEvent_t ev_step = nullptr, ev_gather = nullptr, ev_ring = nullptr;
    // how the exchanges are issued (nb_shard_verify_exchanges may move either to its fallback) and whether the form was decided
    bool gather_copy = false;        // the all-gather from a COPY of this rank's slot instead of in place
    bool ring_per_distance = false;  // the second exchange as one group of send + receive per distance instead of one group
    bool form_decided = false;       // nb_shard_set_pairs / nb_shard_choose_form was called: the first step does not choose by itself
    bool exchanges_verified = false, in_choose = false;
    bool own_ready = false;          // the phases: the last thing that used `scratch` was the fused finish of the step before -- the own slot's planes are in place
    bool ring_failed = false;        // nb_shard_verify_exchanges: the second exchange loses data in every form -- no pairs form on this shard
    float4 *sendbuf = nullptr;       // gather_copy: the copy
    size_t sendbuf_bytes = 0;
    uint32_t *word = nullptr;        // a device word for the checks and the consensus (pinned host mirror: word_host)
    uint32_t *word_all = nullptr;    // world words: a host-supplied gather as the consensus channel
    // the exchanges as pulls over xGMI (nb_peers.inc; nb_shard_peer_export / _import): buffers 0, 1 = the position replicas, 2 = sums
    nb_peers *peers = nullptr;
    bool peers_on = false;
    int peers_pending = -1;          // overlapped forms: the replica (0 / 1) whose gather is signalled but not pulled yet
    void *comm = nullptr;  // ncclComm_t
    bool rccl_solo = false;  // nb_diag_rccl_solo(1) (tests, tools/step_overhead.py): a communicator of ONE rank whatever `world`
                             // is -- the whole RCCL call path of a step on a one-GPU box; the exchange then moves nothing
    std::string err;
};

namespace {

#define NB_SH(sh, call)                                                                           \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            (sh)->err = std::string(#call " failed: ") + hipGetErrorString(e_);                   \
            return NB_ERR_HIP;                                                                    \
        }                                                                                         \
    } while (0)

// makes `stream` wait for the exchange in flight, if any
int shard_join_exchange(nb_shard *sh)
{
    if (sh->peers_pending >= 0) {  // pulls: the signal went out behind the last finish; the waits and the copy come now, in-stream
        const int buf = sh->peers_pending;
        sh->peers_pending = -1;
        if (nb_peers_gather(sh->peers, 0, buf, (size_t)sh->slot * sizeof(float4), (void *)sh->stream) != NB_OK) {
            sh->err = std::string("nb_peers_gather: ") + nb_peers_last_error(sh->peers);
            return NB_ERR_STATE;
        }
    }
    if (sh->gather_pending) {
        NB_SH(sh, hipStreamWaitEvent(sh->stream, sh->ev_gather, 0));
        sh->gather_pending = false;
    }
    return NB_OK;
}

// `records_per_slot`: 0 = one record per body (a position or velocity replica); 2 * slot for the boids staging buffer
int shard_exchange(nb_shard *sh, float4 *buf, hipStream_t on = nullptr, size_t records_per_slot = 0)
{
    const hipStream_t stream = on ? on : sh->stream;
    if (sh->world == 1 && !sh->rccl_solo) return NB_OK;
    RoctxRange range("nb_shard_exchange");
    const size_t slot_bytes = (records_per_slot ? records_per_slot : (size_t)sh->slot) * sizeof(float4);
    if (sh->peers_on && records_per_slot == 0 && (buf == sh->pos[0] || buf == sh->pos[1])) {  // pulls over xGMI: signal, wait for every peer, one copy kernel
        const int b = buf == sh->pos[0] ? 0 : 1;
        if (nb_peers_signal(sh->peers, 0, (void *)stream) != NB_OK || nb_peers_gather(sh->peers, 0, b, slot_bytes, (void *)stream) != NB_OK) {
            sh->err = std::string("nb_peers (all-gather): ") + nb_peers_last_error(sh->peers);
            return NB_ERR_STATE;
        }
        return NB_OK;
    }
    if (sh->comm) {
        RcclApi &api = rccl_api();
        // in place: the send buffer is this rank's slot of the receive buffer
        char *send = (char *)buf + (size_t)sh->rank * slot_bytes;
        if (sh->gather_copy && !sh->rccl_solo) {  // fallback (nb_shard_verify_exchanges): the send buffer is a copy of the slot
            if (sh->sendbuf_bytes < slot_bytes) {
                if (sh->sendbuf) (void)hipFree(sh->sendbuf);
                sh->sendbuf = nullptr, sh->sendbuf_bytes = 0;
                NB_SH(sh, hipMalloc((void **)&sh->sendbuf, slot_bytes));
                sh->sendbuf_bytes = slot_bytes;
            }
            NB_SH(sh, hipMemcpyAsync(sh->sendbuf, send, slot_bytes, hipMemcpyDeviceToDevice, stream));
            send = (char *)sh->sendbuf;
        }
        int r = api.AllGather(send, sh->rccl_solo ? (void *)send : (void *)buf, slot_bytes, kRcclInt8, sh->comm, stream);
        if (r != 0) {
            sh->err = std::string("ncclAllGather failed: ") + api.GetErrorString(r);
            return NB_ERR_STATE;
        }
        return NB_OK;
    }
    if (sh->gather) {
        if (sh->gather(sh->gather_user, buf, slot_bytes, sh->rank, sh->world, (void *)stream) != 0) {
            sh->err = "the host's exchange function failed";
            return NB_ERR_STATE;
        }
        return NB_OK;
    }
    sh->err = "no exchange chosen: call nb_shard_use_rccl or nb_shard_use_gather before stepping a world > 1";
    return NB_ERR_STATE;
}

// does a step take the pairs form?  The shape must allow it and the second exchange must exist: RCCL's send / receive, or the host's
bool shard_ring_active(const nb_shard *sh)
{
    if (!sh->ring_wanted || sh->ring_failed || sh->ring.partners == 0u || !sh->sums) return false;
    if (sh->peers_on) return true;
    if (sh->comm) return rccl_api().Send && rccl_api().Recv && rccl_api().GroupStart && rccl_api().GroupEnd;
    return sh->ring_fn != nullptr;
}

// the second exchange: chunk d of `sums` to rank + d, chunk d - 1 of `recv` from rank - d, d = 1..partners; `on`: the stream it is
// ordered on (NULL: the shard's)
int shard_ring_exchange(nb_shard *sh, hipStream_t on = nullptr)
{
    RoctxRange range("nb_shard_ring_exchange");
    const hipStream_t stream = on ? on : sh->stream;
    const size_t chunk = (size_t)sh->count * sizeof(float4);
    const int D = (int)sh->ring.partners;
    if (sh->peers_on) {  // pulls: my chunks are final -> signal; wait for the D ranks behind; one kernel copies their chunks for me
        if (nb_peers_signal(sh->peers, 1, (void *)stream) != NB_OK || nb_peers_ring(sh->peers, 1, 2, sh->recv, chunk, D, (void *)stream) != NB_OK) {
            sh->err = std::string("nb_peers (second exchange): ") + nb_peers_last_error(sh->peers);
            return NB_ERR_STATE;
        }
        return NB_OK;
    }
    if (sh->comm) {
        RcclApi &api = rccl_api();
        int r = sh->ring_per_distance ? 0 : api.GroupStart();
        for (int d = 1; d <= D && r == 0; ++d) {
            // (a communicator of one -- nb_diag_rccl_solo -- sends to itself: the whole call path, nothing on the wire)
            const int to = sh->rccl_solo ? 0 : (sh->rank + d) % sh->world, from = sh->rccl_solo ? 0 : (sh->rank - d + sh->world) % sh->world;
            if (sh->ring_per_distance) r = api.GroupStart();  // fallback: every rank sends to rank + d and receives from rank - d, then the next d
            if (r == 0) r = api.Send((const char *)sh->sums + (size_t)d * chunk, chunk, kRcclInt8, to, sh->comm, stream);
            if (r == 0) r = api.Recv((char *)sh->recv + (size_t)(d - 1) * chunk, chunk, kRcclInt8, from, sh->comm, stream);
            if (sh->ring_per_distance) {
                const int r2 = api.GroupEnd();
                if (r == 0) r = r2;
            }
        }
        if (!sh->ring_per_distance) {
            const int r2 = api.GroupEnd();
            if (r == 0) r = r2;
        }
        if (r != 0) {
            sh->err = std::string("ncclSend / ncclRecv failed: ") + api.GetErrorString(r);
            return NB_ERR_STATE;
        }
        return NB_OK;
    }
    if (sh->ring_fn(sh->ring_user, (const char *)sh->sums + chunk, sh->recv, chunk, D, sh->rank, sh->world, (void *)stream) != 0) {
        sh->err = "the host's second exchange function failed";
        return NB_ERR_STATE;
    }
    return NB_OK;
}

int shard_alloc(nb_shard *sh)
{
    const size_t padded = (size_t)sh->slot * sh->world * sizeof(float4);
    NB_SH(sh, hipStreamCreateWithFlags(&sh->stream, hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) {
        NB_SH(sh, hipMalloc((void **)&sh->pos[i], padded));
        NB_SH(sh, hipMemsetAsync(sh->pos[i], 0, padded, sh->stream));  // records past n are never read by a kernel; keep them defined for the exchange
    }
    NB_SH(sh, hipMalloc((void **)&sh->vel, (size_t)sh->slot * sizeof(float4)));
    NB_SH(sh, hipMemsetAsync(sh->vel, 0, (size_t)sh->slot * sizeof(float4), sh->stream));
    NB_SH(sh, hipMalloc((void **)&sh->stage, (size_t)sh->n * 3 * sizeof(float)));
    if (sh->count) {
        size_t sb = plan_scratch_bytes(sh->plan, sh->count);
        if (sh->ring.partners) {
            sb = std::max(sb, ring_scratch_bytes(sh->ring, sh->n, sh->first, sh->count));
            const size_t chunk = (size_t)sh->count * sizeof(float4);
            NB_SH(sh, hipMalloc((void **)&sh->sums, (sh->ring.partners + 1u) * chunk));
            NB_SH(sh, hipMalloc((void **)&sh->recv, sh->ring.partners * chunk));
            NB_SH(sh, hipMemsetAsync(sh->sums, 0, (sh->ring.partners + 1u) * chunk, sh->stream));
            NB_SH(sh, hipMemsetAsync(sh->recv, 0, sh->ring.partners * chunk, sh->stream));
        }
        if (sb) NB_SH(sh, hipMalloc(&sh->scratch, sb));
        sh->scratch_bytes = sb;
    }
    NB_SH(sh, hipStreamSynchronize(sh->stream));
    return check_status(&sh->status, &sh->err);
}

int shard_ready(nb_shard *sh, const char *who)
{
    if (!sh) {
        g_tls_error = std::string(who) + ": shard is null";
        return NB_ERR_INVALID;
    }
    if (!sh->uploaded) {
        sh->err = std::string(who) + ": no state uploaded (call nb_shard_upload first)";
        return NB_ERR_STATE;
    }
    return NB_OK;
}

}  // namespace

NB_EXPORT int nb_comm_id(void *id)
{
    if (!id) {
        g_tls_error = "nb_comm_id: id is null";
        return NB_ERR_INVALID;
    }
    RcclApi &api = rccl_api();
    if (!api.handle) {
        g_tls_error = "nb_comm_id: " + api.why;
        return NB_ERR_UNSUPPORTED;
    }
    int rc = check_device(&g_tls_error);
    if (rc != NB_OK) return rc;
    RcclId tmp;
    int r = api.GetUniqueId(&tmp);
    if (r != 0) {
        g_tls_error = std::string("nb_comm_id: ncclGetUniqueId failed: ") + api.GetErrorString(r);
        return NB_ERR_STATE;
    }
    std::memcpy(id, &tmp, sizeof(tmp));
    return NB_OK;
}

NB_EXPORT int nb_shard_create(uint32_t n, int rank, int world, const nb_params *params, nb_shard **out)
{
    if (!out) {
        g_tls_error = "nb_shard_create: out is null";
        return NB_ERR_INVALID;
    }
    *out = nullptr;
    if (n == 0 || world <= 0 || rank < 0 || rank >= world) {
        g_tls_error = "nb_shard_create: need n > 0 and 0 <= rank < world";
        return NB_ERR_INVALID;
    }
    const nb_params p = params_or_default(params);
    const uint32_t slot = (uint32_t)(((uint64_t)n + (uint32_t)world - 1u) / (uint32_t)world);
    const uint64_t lo = (uint64_t)rank * slot;
    const uint32_t first = lo < n ? (uint32_t)lo : n;
    const uint32_t count = std::min<uint32_t>(slot, n - first);
    Plan plan{};
    int rc = make_plan(p, n, count ? count : 1u, &plan, &g_tls_error);  // an empty rank still validates the constants
    if (rc != NB_OK) return rc;
    rc = check_device(&g_tls_error);
    if (rc != NB_OK) return rc;
    nb_shard *sh = new (std::nothrow) nb_shard();
    if (!sh) {
        g_tls_error = "nb_shard_create: out of host memory";
        return NB_ERR_ALLOC;
    }
    sh->n = n;
    sh->slot = slot;
    sh->first = first;
    sh->count = count;
    sh->rank = rank;
    sh->world = world;
    sh->p = p;
    sh->plan = plan;
    if (world > 1 && count && (uint64_t)slot * (uint32_t)world == n) {  // equal ranks: FAST may take the pairs form (nb_nbody_ring.inc)
        rc = make_ring_plan(p, n, first, count, &sh->ring, &g_tls_error);
        if (rc != NB_OK) {
            delete sh;
            return rc;
        }
    }
    rc = shard_alloc(sh);
    if (rc != NB_OK) {
        g_tls_error = "nb_shard_create: " + sh->err;
        nb_shard_destroy(sh);
        return rc;
    }
    *out = sh;
    return NB_OK;
}

NB_EXPORT void nb_shard_destroy(nb_shard *sh)
{
    if (!sh) return;
    // an overlapped exchange may still be running on xstream: both streams drain before the communicator goes
    if (sh->stream) (void)hipStreamSynchronize(sh->stream);
    if (sh->xstream) (void)hipStreamSynchronize(sh->xstream);
    if (sh->peers) nb_peers_destroy(sh->peers);
    if (sh->comm) (void)rccl_api().CommDestroy(sh->comm);
    void *bufs[] = {sh->pos[0], sh->pos[1], sh->vel, sh->velfull[0], sh->velfull[1], sh->pvstage, sh->scratch, sh->stage, sh->inst, sh->status.w,
                    sh->sums,   sh->recv, sh->boids_partial, sh->sendbuf, sh->word, sh->word_all};
    for (void *b : bufs)
        if (b) (void)hipFree(b);
    if (sh->ev_step) (void)hipEventDestroy(sh->ev_step);
    if (sh->ev_gather) (void)hipEventDestroy(sh->ev_gather);
    if (sh->ev_ring) (void)hipEventDestroy(sh->ev_ring);
    if (sh->xstream) (void)hipStreamDestroy(sh->xstream);
    if (sh->stream) (void)hipStreamDestroy(sh->stream);
    delete sh;
}

NB_EXPORT const char *nb_shard_last_error(const nb_shard *sh) { return sh ? sh->err.c_str() : g_tls_error.c_str(); }

NB_EXPORT int nb_shard_use_rccl(nb_shard *sh, const void *id)
{
    if (!sh || !id) {
        g_tls_error = "nb_shard_use_rccl: null argument";
        return NB_ERR_INVALID;
    }
    RcclApi &api = rccl_api();
    if (!api.handle) {
        sh->err = "nb_shard_use_rccl: " + api.why;
        return NB_ERR_UNSUPPORTED;
    }
    if (sh->comm) {
        (void)api.CommDestroy(sh->comm);
        sh->comm = nullptr;
    }
    RcclId tmp;
    std::memcpy(&tmp, id, sizeof(tmp));
    sh->rccl_solo = g_rccl_solo.load(std::memory_order_relaxed);
    int r = sh->rccl_solo ? api.CommInitRank(&sh->comm, 1, tmp, 0) : api.CommInitRank(&sh->comm, sh->world, tmp, sh->rank);
    if (r != 0) {
        sh->comm = nullptr;
        sh->err = std::string("nb_shard_use_rccl: ncclCommInitRank failed: ") + api.GetErrorString(r);
        return NB_ERR_STATE;
    }
    sh->gather = nullptr;
    sh->ring_failed = sh->exchanges_verified = sh->gather_copy = sh->ring_per_distance = false;
    return NB_OK;
}

NB_EXPORT int nb_shard_set_overlap(nb_shard *sh, int on)
{
    if (!sh) {
        g_tls_error = "nb_shard_set_overlap: shard is null";
        return NB_ERR_INVALID;
    }
    int rc = shard_join_exchange(sh);
    if (rc != NB_OK) return rc;
    if (!on || sh->p.mode != NB_MODE_FAST || sh->world == 1) {  // STRICT keeps the reference's order of additions: never overlapped
        sh->overlap = false;
        return NB_OK;
    }
    if (sh->count) {  // (the phases of the ORDERED fold; a shard that takes the pairs form overlaps through nb_launch_ring_fold_phase instead)
        rc = make_phase_plan(sh->p, sh->n, sh->count, sh->first, sh->first + sh->count, &sh->phases, &sh->err);
        if (rc != NB_OK) return rc;
        const size_t need = phase_scratch_bytes(sh->phases, sh->count);
        sh->own_ready = false;
        if (need > sh->scratch_bytes) {  // (never shrinks: the pairs form on shards may need more than the phases do)
            NB_SH(sh, hipStreamSynchronize(sh->stream));
            if (sh->scratch) (void)hipFree(sh->scratch);
            sh->scratch = nullptr;
            sh->scratch_bytes = 0;
            NB_SH(sh, hipMalloc(&sh->scratch, need));
            sh->scratch_bytes = need;
        }
    }
    if (!sh->xstream) NB_SH(sh, hipStreamCreateWithFlags(&sh->xstream, hipStreamNonBlocking));
    if (!sh->ev_step) NB_SH(sh, hipEventCreateWithFlags(&sh->ev_step, hipEventDisableTiming));
    if (!sh->ev_gather) NB_SH(sh, hipEventCreateWithFlags(&sh->ev_gather, hipEventDisableTiming));
    if (!sh->ev_ring) NB_SH(sh, hipEventCreateWithFlags(&sh->ev_ring, hipEventDisableTiming));
    sh->overlap = true;
    return NB_OK;
}

NB_EXPORT int nb_shard_use_gather(nb_shard *sh, nb_gather_fn fn, void *user)
{
    if (!sh || !fn) {
        g_tls_error = "nb_shard_use_gather: null argument";
        return NB_ERR_INVALID;
    }
    if (sh->comm) {
        (void)rccl_api().CommDestroy(sh->comm);
        sh->comm = nullptr;
    }
    sh->gather = fn;
    sh->gather_user = user;
    sh->ring_failed = sh->exchanges_verified = sh->gather_copy = sh->ring_per_distance = false;
    return NB_OK;
}

// The exchanges as pulls over xGMI (nb_peers.inc): nb_shard_peer_export fills this rank's blob (nb_peers_blob_bytes()), the host
// hands every rank all blobs, rank-major, and nb_shard_peer_import maps the others' buffers; from then on both exchanges of a step
// are a signal, stream waits on the peers' flag words and one copy kernel on the shard's own stream (the boids controller, which
// moves another buffer, keeps the exchange chosen before).  nb_shard_use_peers(sh, 0) goes back to that exchange.
NB_EXPORT int nb_shard_peer_export(nb_shard *sh, void *blob)
{
    if (!sh || !blob) {
        g_tls_error = "nb_shard_peer_export: null argument";
        return NB_ERR_INVALID;
    }
    if (sh->peers) {
        nb_peers_destroy(sh->peers);
        sh->peers = nullptr;
        sh->peers_on = false;
    }
    int rc = nb_peers_create(sh->rank, sh->world, &sh->peers);
    if (rc != NB_OK) {
        sh->err = "nb_shard_peer_export: " + g_tls_error;
        return rc;
    }
    const size_t padded = (size_t)sh->slot * sh->world * sizeof(float4);
    void *bufs[3] = {sh->pos[0], sh->pos[1], sh->sums};
    // (`sums`: every rank of an equal split plans the pairs form or none does, so all ranks register the same number of buffers)
    size_t bytes[3] = {padded, padded, sh->sums ? (sh->ring.partners + 1u) * (size_t)sh->count * sizeof(float4) : 0};
    rc = nb_peers_export(sh->peers, bufs, bytes, sh->sums ? 3 : 2, blob);
    if (rc != NB_OK) sh->err = std::string("nb_shard_peer_export: ") + nb_peers_last_error(sh->peers);
    return rc;
}

NB_EXPORT int nb_shard_peer_import(nb_shard *sh, const void *blobs)
{
    if (!sh || !blobs) {
        g_tls_error = "nb_shard_peer_import: null argument";
        return NB_ERR_INVALID;
    }
    if (!sh->peers) {
        sh->err = "nb_shard_peer_import: nb_shard_peer_export has not run";
        return NB_ERR_STATE;
    }
    int rc = shard_join_exchange(sh);
    if (rc != NB_OK) return rc;
    rc = nb_peers_import(sh->peers, blobs);
    if (rc == NB_OK) rc = nb_peers_probe(sh->peers, 10000);  // first contact with a deadline (a stream of its own)
    if (rc != NB_OK) {
        sh->err = std::string("nb_shard_peer_import: ") + nb_peers_last_error(sh->peers);
        return rc;
    }
    sh->peers_on = true;
    sh->ring_failed = sh->exchanges_verified = sh->gather_copy = sh->ring_per_distance = false;
    return NB_OK;
}

NB_EXPORT int nb_shard_use_peers(nb_shard *sh, int on)
{
    if (!sh) {
        g_tls_error = "nb_shard_use_peers: shard is null";
        return NB_ERR_INVALID;
    }
    if (on && !(sh->peers && sh->peers->imported)) {
        sh->err = "nb_shard_use_peers: nb_shard_peer_export / nb_shard_peer_import have not run";
        return NB_ERR_STATE;
    }
    int rc = shard_join_exchange(sh);
    if (rc != NB_OK) return rc;
    sh->peers_on = on != 0;
    sh->ring_failed = sh->exchanges_verified = false;
    return NB_OK;
}

NB_EXPORT int nb_shard_use_ring(nb_shard *sh, nb_ring_fn fn, void *user)
{
    if (!sh) {
        g_tls_error = "nb_shard_use_ring: shard is null";
        return NB_ERR_INVALID;
    }
    sh->ring_fn = fn;  // NULL: a host-supplied exchange then keeps the ordered fold
    sh->ring_user = user;
    sh->ring_failed = sh->exchanges_verified = false;  // another exchange: whatever was found out about the last one is void
    return NB_OK;
}

NB_EXPORT int nb_shard_set_pairs(nb_shard *sh, int on)
{
    if (!sh) {
        g_tls_error = "nb_shard_set_pairs: shard is null";
        return NB_ERR_INVALID;
    }
    sh->ring_wanted = on != 0;
    sh->form_decided = true;
    return NB_OK;
}

NB_EXPORT int nb_shard_set_boids_split(nb_shard *sh, int on)
{
    if (!sh) {
        g_tls_error = "nb_shard_set_boids_split: shard is null";
        return NB_ERR_INVALID;
    }
    sh->boids_split = on != 0;
    return NB_OK;
}

NB_EXPORT int nb_shard_pairs_partners(const nb_shard *sh)
{
    if (!sh) {
        g_tls_error = "nb_shard_pairs_partners: shard is null";
        return NB_ERR_INVALID;
    }
    return shard_ring_active(sh) ? (int)sh->ring.partners : 0;
}

namespace {
// the largest `v` of any rank (every rank gets it): RCCL's all-reduce -- a collective other than the two being verified --, or the
// host's all-gather of one word per rank
int shard_all_max(nb_shard *sh, uint32_t v, uint32_t *out)
{
    *out = v;
    if (sh->world == 1 || sh->rccl_solo) return NB_OK;
    if (!sh->word) NB_SH(sh, hipMalloc((void **)&sh->word, 64));
    if (sh->comm) {
        RcclApi &api = rccl_api();
        if (!api.AllReduce) {
            sh->err = "the RCCL library lacks ncclAllReduce (the ranks cannot agree on a verdict)";
            return NB_ERR_UNSUPPORTED;
        }
        NB_SH(sh, hipMemcpyAsync(sh->word, &v, sizeof(v), hipMemcpyHostToDevice, sh->stream));
        int r = api.AllReduce(sh->word, sh->word, 1, kRcclUint32, kRcclMax, sh->comm, sh->stream);
        if (r != 0) {
            sh->err = std::string("ncclAllReduce failed: ") + api.GetErrorString(r);
            return NB_ERR_STATE;
        }
        NB_SH(sh, hipMemcpyAsync(out, sh->word, sizeof(v), hipMemcpyDeviceToHost, sh->stream));
        NB_SH(sh, hipStreamSynchronize(sh->stream));
        return NB_OK;
    }
    if (sh->peers_on && !sh->gather) {
        // pulls only: my value into one of two words of my flags block (a rank is at most one round ahead of a peer), a signal on the
        // last channel, and every peer's word read through its mapping once it has signalled this round
        nb_peers *p = sh->peers;
        const int ch = NB_PEERS_CHANNELS - 1;
        const uint32_t round = p->sent[ch] + 1u;
        uint32_t *const my_word = p->flags + 512u + (round & 1u) * 16u;
        NB_SH(sh, hipMemcpyAsync(my_word, &v, sizeof(v), hipMemcpyHostToDevice, sh->stream));
        if (nb_peers_signal(p, ch, (void *)sh->stream) != NB_OK) {
            sh->err = std::string("nb_peers_signal: ") + nb_peers_last_error(p);
            return NB_ERR_STATE;
        }
        ++p->awaited[ch];
        std::vector<uint32_t> vals((size_t)sh->world, 0u);
        for (int q = 0; q < sh->world; ++q) {
            if (q == sh->rank) continue;
            NB_SH(sh, hipStreamWaitValue32(sh->stream, p->their_flags[q] + (size_t)ch * kPeerFlagStride, round, hipStreamWaitValueGte, 0xffffffffu));
            NB_SH(sh, hipMemcpyAsync(&vals[(size_t)q], p->their_flags[q] + 512u + (round & 1u) * 16u, sizeof(uint32_t), hipMemcpyDeviceToHost, sh->stream));
        }
        NB_SH(sh, hipStreamSynchronize(sh->stream));
        for (int q = 0; q < sh->world; ++q) *out = std::max(*out, vals[(size_t)q]);
        return NB_OK;
    }
    if (!sh->gather) {
        sh->err = "no exchange chosen: call nb_shard_use_rccl, nb_shard_use_gather or nb_shard_peer_import first";
        return NB_ERR_STATE;
    }
    const size_t slot = 16;  // bytes per rank
    if (!sh->word_all) NB_SH(sh, hipMalloc((void **)&sh->word_all, slot * (size_t)sh->world));
    uint32_t mine[4] = {v, 0, 0, 0};
    NB_SH(sh, hipMemcpyAsync((char *)sh->word_all + slot * (size_t)sh->rank, mine, slot, hipMemcpyHostToDevice, sh->stream));
    if (sh->gather(sh->gather_user, sh->word_all, slot, sh->rank, sh->world, (void *)sh->stream) != 0) {
        sh->err = "the host's exchange function failed";
        return NB_ERR_STATE;
    }
    std::vector<uint32_t> all(4 * (size_t)sh->world);
    NB_SH(sh, hipMemcpyAsync(all.data(), sh->word_all, slot * (size_t)sh->world, hipMemcpyDeviceToHost, sh->stream));
    NB_SH(sh, hipStreamSynchronize(sh->stream));
    for (int r = 0; r < sh->world; ++r) *out = std::max(*out, all[4 * (size_t)r]);
    return NB_OK;
}

// mismatching records of `src` against the pattern (rank, salt), counted on the device
int shard_count_mismatches(nb_shard *sh, const float4 *src, uint32_t count, float rank, float salt, uint32_t *total)
{
    if (!sh->word) NB_SH(sh, hipMalloc((void **)&sh->word, 64));
    NB_SH(sh, hipMemsetAsync(sh->word, 0, sizeof(uint32_t), sh->stream));
    NB_SH(sh, nbk::launch_exchange_check(src, count, rank, salt, sh->word, sh->stream));
    uint32_t got = 0;
    NB_SH(sh, hipMemcpyAsync(&got, sh->word, sizeof(got), hipMemcpyDeviceToHost, sh->stream));
    NB_SH(sh, hipStreamSynchronize(sh->stream));
    *total += got;
    return NB_OK;
}
}  // namespace

// Both exchanges of a step, once, on a known per-rank pattern, checked on every rank (collective; the ranks agree on every verdict
// through a third collective).  The in-place all-gather and the grouped sends / receives had run on a one-rank communicator and
// through host-supplied exchanges only when this was written (no multi-GPU box in the build): a mismatch moves the exchange to
// its fallback -- the all-gather from a copy of the slot; the second exchange as one group per distance, then not at all (the
// ordered fold) -- without restarting anything.  gather_path: 0 in place, 1 from a copy; ring_path: -1 no pairs form planned,
// 0 one group, 1 one group per distance, 2 dropped.  Uses the scratch side of the position ping-pong and sums / recv.
NB_EXPORT int nb_shard_verify_exchanges(nb_shard *sh, int *gather_path, int *ring_path)
{
    if (!sh) {
        g_tls_error = "nb_shard_verify_exchanges: shard is null";
        return NB_ERR_INVALID;
    }
    if (gather_path) *gather_path = 0;
    if (ring_path) *ring_path = -1;
    if (sh->world == 1 || sh->rccl_solo) return NB_OK;
    int rc = shard_join_exchange(sh);
    if (rc != NB_OK) return rc;
    float4 *buf = sh->pos[sh->cur ^ 1];
    const uint32_t padded = sh->slot * (uint32_t)sh->world;
    bool ok = false;
    const bool pulls = sh->peers_on;   // the pulls over xGMI first; a mismatch sends BOTH exchanges back to whatever was chosen before
    for (int attempt = pulls ? -1 : 0; attempt < (sh->comm ? 2 : 1) && !ok; ++attempt) {
        if (attempt == 0 && pulls) {
            sh->peers_on = false;
            if (!sh->comm && !sh->gather) break;   // nothing to fall back to
        }
        sh->gather_copy = attempt == 1;
        // (the pulls are checked TWICE from the same buffers with different patterns: a reader that kept lines of a peer's memory in a
        // cache would pass the first round and show the first pattern again in the second; the agreement between the rounds is also the
        // barrier behind which a rank may rewrite a buffer its peers have pulled from)
        uint32_t any = 0;
        for (int round = 0; round < (attempt < 0 ? 2 : 1) && any == 0u; ++round) {
            const float salt = 7.f + 2.f * (float)round;
            NB_SH(sh, nbk::launch_exchange_pattern(buf, padded, 0.f, 0.f, true, sh->stream));
            NB_SH(sh, nbk::launch_exchange_pattern(buf + (size_t)sh->rank * sh->slot, sh->slot, (float)sh->rank, salt, false, sh->stream));
            rc = shard_exchange(sh, buf);
            if (rc != NB_OK) return rc;
            uint32_t bad = 0;
            for (int r = 0; r < sh->world; ++r) {
                rc = shard_count_mismatches(sh, buf + (size_t)r * sh->slot, sh->slot, (float)r, salt, &bad);
                if (rc != NB_OK) return rc;
            }
            rc = shard_all_max(sh, bad ? 1u : 0u, &any);
            if (rc != NB_OK) return rc;
        }
        ok = any == 0u;
    }
    NB_SH(sh, hipMemsetAsync(buf, 0, (size_t)padded * sizeof(float4), sh->stream));
    if (!ok) {
        sh->err = "nb_shard_verify_exchanges: the all-gather does not deliver every rank's slot" + std::string(pulls ? " (as pulls over xGMI" : " (") +
                  std::string(sh->comm ? ", in place or from a copy)" : ")");
        return NB_ERR_STATE;
    }
    if (gather_path) *gather_path = sh->peers_on ? 2 : sh->gather_copy ? 1 : 0;
    if (shard_ring_active(sh)) {
        const uint32_t S = sh->count, D = sh->ring.partners;
        int path = 2;
        const bool ring_pulls = sh->peers_on;
        for (int attempt = ring_pulls ? -1 : 0; attempt < (sh->comm ? 2 : 1); ++attempt) {
            if (attempt == 0 && ring_pulls) {   // the pulls lost data: both exchanges go back (the all-gather is re-verified by the host's next call)
                sh->peers_on = false;
                sh->exchanges_verified = false;
                if (!(sh->comm ? (rccl_api().Send && rccl_api().Recv) : sh->ring_fn != nullptr)) break;
            }
            sh->ring_per_distance = attempt == 1;
            uint32_t any = 0;
            for (int round = 0; round < (attempt < 0 ? 2 : 1) && any == 0u; ++round) {   // (pulls: twice from the same buffers, as above)
                const float salt = 16.f * (float)round;
                for (uint32_t d = 1; d <= D; ++d)
                    NB_SH(sh, nbk::launch_exchange_pattern(sh->sums + (size_t)d * S, S, (float)sh->rank, salt + (float)d, false, sh->stream));
                NB_SH(sh, nbk::launch_exchange_pattern(sh->recv, D * S, 0.f, 0.f, true, sh->stream));
                rc = shard_ring_exchange(sh);
                if (rc != NB_OK) return rc;
                uint32_t bad = 0;
                for (uint32_t d = 1; d <= D; ++d) {
                    rc = shard_count_mismatches(sh, sh->recv + (size_t)(d - 1) * S, S, (float)((sh->rank - (int)d % sh->world + sh->world) % sh->world), salt + (float)d,
                                                &bad);
                    if (rc != NB_OK) return rc;
                }
                rc = shard_all_max(sh, bad ? 1u : 0u, &any);
                if (rc != NB_OK) return rc;
            }
            if (any == 0u) {
                path = attempt < 0 ? 3 : attempt;
                break;
            }
        }
        if (path == 2) {  // neither form delivers: the ordered fold and its one exchange, whatever is asked later
            sh->ring_failed = true;
            sh->ring_per_distance = false;
        }
        if (ring_path) *ring_path = path;
    }
    sh->exchanges_verified = true;
    return NB_OK;
}

// Which form should a FAST step take on THIS machine?  Times `steps` steps (after two of warm-up) of every form the shard can take
// -- 1: the pairs form, its exchanges in sequence; 2: the same in phases, the exchanges behind compute (where nb_ring_phased); 0:
// the ordered fold and its one exchange -- on the state in hand, takes the SLOWEST rank's time of each (collective), keeps the
// fastest for the steps to come and puts the state back.  ms3 (may be NULL): milliseconds per step of forms 0, 1, 2 (< 0: not
// offered).  STRICT shards, worlds of one and shapes without the pairs form answer 0 at once.
NB_EXPORT int nb_shard_choose_form(nb_shard *sh, uint32_t steps, int *chosen, double *ms3)
{
    int rc = shard_ready(sh, "nb_shard_choose_form");
    if (rc != NB_OK) return rc;
    if (chosen) *chosen = 0;
    if (ms3) ms3[0] = ms3[1] = ms3[2] = -1.0;
    sh->form_decided = true;
    if (!sh->exchanges_verified && sh->world > 1 && !sh->rccl_solo && (sh->comm || sh->gather || sh->peers_on)) {  // nothing is timed over an exchange that loses data
        rc = nb_shard_verify_exchanges(sh, nullptr, nullptr);
        if (rc != NB_OK) return rc;
    }
    struct Busy {  // (the steps below must not come back here)
        bool &b, was;
        explicit Busy(bool &x) : b(x), was(x) { b = true; }
        ~Busy() { b = was; }
    } busy(sh->in_choose);
    const bool was_wanted = sh->ring_wanted;
    sh->ring_wanted = true;
    const bool can_pairs = shard_ring_active(sh);
    sh->ring_wanted = was_wanted;
    if (!can_pairs || sh->world == 1) return NB_OK;
    if (steps == 0u) steps = 4u;
    rc = shard_join_exchange(sh);
    if (rc != NB_OK) return rc;
    NB_SH(sh, hipStreamSynchronize(sh->stream));
    // the state in hand
    const size_t padded = (size_t)sh->slot * sh->world * sizeof(float4), vbytes = (size_t)sh->slot * sizeof(float4);
    float4 *keep = nullptr;
    NB_SH(sh, hipMalloc((void **)&keep, 2 * padded + vbytes));
    NB_SH(sh, hipMemcpyAsync(keep, sh->pos[0], padded, hipMemcpyDeviceToDevice, sh->stream));
    NB_SH(sh, hipMemcpyAsync((char *)keep + padded, sh->pos[1], padded, hipMemcpyDeviceToDevice, sh->stream));
    NB_SH(sh, hipMemcpyAsync((char *)keep + 2 * padded, sh->vel, vbytes, hipMemcpyDeviceToDevice, sh->stream));
    const int cur = sh->cur;
    const uint64_t steps_done = sh->steps;
    const bool velfull_valid = sh->velfull_valid, overlap0 = sh->overlap;
    auto restore = [&]() -> int {
        int r = shard_join_exchange(sh);
        if (r != NB_OK) return r;
        NB_SH(sh, hipMemcpyAsync(sh->pos[0], keep, padded, hipMemcpyDeviceToDevice, sh->stream));
        NB_SH(sh, hipMemcpyAsync(sh->pos[1], (char *)keep + padded, padded, hipMemcpyDeviceToDevice, sh->stream));
        NB_SH(sh, hipMemcpyAsync(sh->vel, (char *)keep + 2 * padded, vbytes, hipMemcpyDeviceToDevice, sh->stream));
        NB_SH(sh, hipStreamSynchronize(sh->stream));
        sh->cur = cur, sh->steps = steps_done, sh->velfull_valid = velfull_valid;
        sh->own_ready = false;  // (the planes a fused finish left are of a state that is gone)
        return NB_OK;
    };
    double ms[3] = {-1.0, -1.0, -1.0};
    for (int form = 0; form < 3 && rc == NB_OK; ++form) {
        if (form == 2 && !sh->ring.phased) continue;
        sh->ring_wanted = form != 0;
        if (form == 2)
            rc = nb_shard_set_overlap(sh, 1);
        else
            sh->overlap = false;
        if (rc == NB_OK) rc = nb_shard_step(sh, 2);
        if (rc == NB_OK) rc = nb_shard_sync(sh);
        uint32_t dummy = 0;
        if (rc == NB_OK) rc = shard_all_max(sh, 0u, &dummy);  // (a barrier: every rank starts the timed steps together)
        const auto t0 = std::chrono::steady_clock::now();
        if (rc == NB_OK) rc = nb_shard_step(sh, steps);
        if (rc == NB_OK) rc = nb_shard_sync(sh);
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / steps;
        uint32_t slowest = 0;
        if (rc == NB_OK) rc = shard_all_max(sh, (uint32_t)std::min(us * 16.0, 4.0e9), &slowest);  // sixteenths of a microsecond
        ms[form] = slowest / 16.0e3;
        if (rc == NB_OK) rc = restore();
    }
    (void)hipFree(keep);
    sh->ring_wanted = was_wanted;
    sh->overlap = overlap0;
    if (rc != NB_OK) return rc;
    int best = 1;  // (ties keep the plainer pairs form)
    if (ms[0] >= 0.0 && ms[0] < ms[best]) best = 0;
    if (ms[2] >= 0.0 && ms[2] < ms[best] && ms[2] < ms[1]) best = 2;
    sh->ring_wanted = best != 0;
    if (best == 2)
        rc = nb_shard_set_overlap(sh, 1);
    else if (best == 1)
        sh->overlap = false;  // (the ordered fold keeps what the host had asked for)
    if (chosen) *chosen = best;
    if (ms3) ms3[0] = ms[0], ms3[1] = ms[1], ms3[2] = ms[2];
    return rc;
}

NB_EXPORT int nb_shard_pairs_overlapped(const nb_shard *sh)
{
    if (!sh) {
        g_tls_error = "nb_shard_pairs_overlapped: shard is null";
        return NB_ERR_INVALID;
    }
    return (shard_ring_active(sh) && sh->overlap && sh->ring.phased) ? 1 : 0;
}

NB_EXPORT int nb_shard_range(const nb_shard *sh, uint32_t *first, uint32_t *count)
{
    if (!sh) {
        g_tls_error = "nb_shard_range: shard is null";
        return NB_ERR_INVALID;
    }
    if (first) *first = sh->first;
    if (count) *count = sh->count;
    return NB_OK;
}

NB_EXPORT int nb_shard_upload(nb_shard *sh, const float *pos_xyz, const float *vel_xyz)
{
    if (!sh) {
        g_tls_error = "nb_shard_upload: shard is null";
        return NB_ERR_INVALID;
    }
    if (!pos_xyz || !vel_xyz) {
        sh->err = "nb_shard_upload: null array";
        return NB_ERR_INVALID;
    }
    // The last overlapped step's all-gather may still be writing the other ranks' slots of pos[cur] on xstream, and after an
    // even number of steps pos[cur] IS pos[0]: the upload below must come after it, or the old exchange lands on the new state.
    int rc = shard_join_exchange(sh);
    if (rc != NB_OK) return rc;
    sh->cur = 0;
    NB_SH(sh, hipMemcpyAsync(sh->stage, pos_xyz, (size_t)sh->n * 3 * sizeof(float), hipMemcpyHostToDevice, sh->stream));
    NB_SH(sh, nbk::launch_pack(sh->n, sh->stage, sh->pos[0], sh->stream));
    NB_SH(sh, hipStreamSynchronize(sh->stream));  // stage is reused; the host array is not retained
    if (sh->count) {
        NB_SH(sh, hipMemcpyAsync(sh->stage, vel_xyz + (size_t)sh->first * 3, (size_t)sh->count * 3 * sizeof(float),
                                 hipMemcpyHostToDevice, sh->stream));
        NB_SH(sh, nbk::launch_pack(sh->count, sh->stage, sh->vel, sh->stream));
        NB_SH(sh, hipStreamSynchronize(sh->stream));
    }
    sh->uploaded = true;
    sh->velfull_valid = false;
    sh->own_ready = false;
    sh->steps = 0;
    return NB_OK;
}

NB_EXPORT int nb_shard_step(nb_shard *sh, uint32_t k)
{
    int rc = shard_ready(sh, "nb_shard_step");
    if (rc != NB_OK) return rc;
    RoctxRange range("nb_shard_step");
    // A real multi-GPU communicator whose host has not said which form to take: before the first step relies on them, both exchanges
    // move a known pattern (a mismatch moves them to their fallbacks), and where the pairs form is planned the machine is asked which
    // form is fastest HERE (ADVICE r04: the library's own line was drawn on one GPU).  Collective: every rank's first step comes here.
    if (k && sh->world > 1 && sh->comm && !sh->rccl_solo && !sh->in_choose) {
        if (!sh->exchanges_verified) {
            rc = nb_shard_verify_exchanges(sh, nullptr, nullptr);
            if (rc != NB_OK) return rc;
        }
        if (!sh->form_decided && shard_ring_active(sh)) {
            rc = nb_shard_choose_form(sh, 4u, nullptr, nullptr);
            if (rc != NB_OK) return rc;
        }
    }
    for (uint32_t s = 0; s < k; ++s) {
        float4 *src = sh->pos[sh->cur], *dst = sh->pos[sh->cur ^ 1];
        if (shard_ring_active(sh) && sh->overlap && sh->ring.phased) {
            // The same in phases (round 5): pairs inside the rank's own slot while the last step's all-gather is still landing on
            // xstream, every other pair, the sums, the second exchange, finish, and the positions leave on xstream while the next
            // step begins.  The second exchange stays on the shard's own stream: handing it to xstream and back costs two cross-stream
            // waits (~25 us on a one-rank communicator, profiles/r05/step_overhead.log) to hide 9 us of reduce -- the all-gather's
            // two waits hide behind the own-slot pairs.
            // The finish is the fused one: it adds the rank's own records itself (no NB_RING_SUMS launch) and leaves the planes of the new
            // own slot, so every step but the first of a run starts with its sweep (two small launches fewer: ~5 us each).
            rc = launch_ring_phase_planned(sh->p, sh->ring, sh->n, sh->first, sh->count, sh->own_ready ? NB_RING_OWN_READY : NB_RING_OWN, src, sh->sums,
                                           sh->scratch, sh->stream, &sh->err);
            sh->own_ready = false;
            if (rc != NB_OK) return rc;
            rc = shard_join_exchange(sh);
            if (rc != NB_OK) return rc;
            rc = launch_ring_phase_planned(sh->p, sh->ring, sh->n, sh->first, sh->count, NB_RING_REST, src, sh->sums, sh->scratch, sh->stream, &sh->err);
            if (rc != NB_OK) return rc;
            rc = shard_ring_exchange(sh);
            if (rc != NB_OK) return rc;
            rc = launch_ring_finish_phase_planned(sh->p, sh->ring, sh->n, sh->first, sh->count, src, dst, sh->vel, nullptr, sh->recv, sh->scratch,
                                                  sh->stream, &sh->err);
            if (rc != NB_OK) return rc;
            sh->own_ready = true;
            if (sh->peers_on) {  // pulls: the signal now, the waits and the copy behind the next step's own-slot pairs -- one stream, no gaps
                if (nb_peers_signal(sh->peers, 0, (void *)sh->stream) != NB_OK) {
                    sh->err = std::string("nb_peers_signal: ") + nb_peers_last_error(sh->peers);
                    return NB_ERR_STATE;
                }
                sh->peers_pending = sh->cur ^ 1;
            } else {
                NB_SH(sh, hipEventRecord(sh->ev_step, sh->stream));
                NB_SH(sh, hipStreamWaitEvent(sh->xstream, sh->ev_step, 0));
                rc = shard_exchange(sh, dst, sh->xstream);
                if (rc != NB_OK) return rc;
                NB_SH(sh, hipEventRecord(sh->ev_gather, sh->xstream));
                sh->gather_pending = true;
            }
            sh->velfull_valid = false;
            sh->cur ^= 1;
            sh->steps++;
            continue;
        }
        sh->own_ready = false;  // (every other form of a step uses `scratch` its own way)
        if (shard_ring_active(sh)) {  // every unordered pair once: fold, the halves of the ranks in front leave, finish, the positions
            rc = shard_join_exchange(sh);
            if (rc != NB_OK) return rc;
            rc = launch_ring_fold_planned(sh->p, sh->ring, sh->n, sh->first, sh->count, src, sh->sums, sh->scratch, sh->stream, &sh->err);
            if (rc != NB_OK) return rc;
            rc = shard_ring_exchange(sh);
            if (rc != NB_OK) return rc;
            rc = launch_ring_finish_planned(sh->p, sh->ring, sh->n, sh->first, sh->count, src, dst, sh->vel, sh->sums, sh->recv, sh->stream,
                                            &sh->err);
            if (rc != NB_OK) return rc;
            rc = shard_exchange(sh, dst);
            if (rc != NB_OK) return rc;
            sh->velfull_valid = false;
            sh->cur ^= 1;
            sh->steps++;
            continue;
        }
        if (sh->overlap) {
            // src's other slots may still be landing (xstream); this rank's own slot of src was written by its own last step
            if (sh->count) {
                rc = launch_phase_planned(sh->p, sh->phases, sh->n, sh->first, sh->count, sh->first, NB_PHASE_RANGE, src, dst, sh->vel,
                                          sh->scratch, sh->stream, &sh->err);
                if (rc != NB_OK) return rc;
            }
            rc = shard_join_exchange(sh);
            if (rc != NB_OK) return rc;
            if (sh->count) {
                rc = launch_phase_planned(sh->p, sh->phases, sh->n, sh->first, sh->count, sh->first, NB_PHASE_REST, src, dst, sh->vel,
                                          sh->scratch, sh->stream, &sh->err);
                if (rc != NB_OK) return rc;
            }
            if (sh->peers_on) {
                if (nb_peers_signal(sh->peers, 0, (void *)sh->stream) != NB_OK) {
                    sh->err = std::string("nb_peers_signal: ") + nb_peers_last_error(sh->peers);
                    return NB_ERR_STATE;
                }
                sh->peers_pending = sh->cur ^ 1;
            } else {
                NB_SH(sh, hipEventRecord(sh->ev_step, sh->stream));
                NB_SH(sh, hipStreamWaitEvent(sh->xstream, sh->ev_step, 0));
                rc = shard_exchange(sh, dst, sh->xstream);
                if (rc != NB_OK) return rc;
                NB_SH(sh, hipEventRecord(sh->ev_gather, sh->xstream));
                sh->gather_pending = true;
            }
            sh->velfull_valid = false;
            sh->cur ^= 1;
            sh->steps++;
            continue;
        }
        if (sh->count) {
            rc = launch_step_planned(sh->p, sh->plan, sh->n, sh->first, sh->count, src, dst, sh->vel, sh->scratch, sh->stream,
                                     &sh->err, &sh->status);
            if (rc != NB_OK) return rc;
        }
        rc = shard_exchange(sh, dst);
        if (rc != NB_OK) return rc;
        sh->velfull_valid = false;  // the velocity replica (boids only) no longer matches the local velocities
        sh->cur ^= 1;
        sh->steps++;
    }
    return NB_OK;
}

NB_EXPORT int nb_shard_step_boids(nb_shard *sh, uint32_t k, const nb_boids_params *params)
{
    int rc = shard_ready(sh, "nb_shard_step_boids");
    if (rc != NB_OK) return rc;
    sh->own_ready = false;
    rc = shard_join_exchange(sh);
    if (rc != NB_OK) return rc;
    const nb_boids_params bp = boids_params_or_default(params);
    const size_t padded = (size_t)sh->slot * sh->world * sizeof(float4);
    const size_t lo = (size_t)sh->rank * sh->slot;
    for (int i = 0; i < 2; ++i)
        if (!sh->velfull[i]) {
            NB_SH(sh, hipMalloc((void **)&sh->velfull[i], padded));
            NB_SH(sh, hipMemsetAsync(sh->velfull[i], 0, padded, sh->stream));
        }
    nbk::BoidsArgs a{};
    uint32_t tile = 0;
    if (sh->count) {
        rc = make_boids_args(bp, sh->n, sh->first, sh->count, &a, &tile, &sh->err);
        if (rc != NB_OK) return rc;
    }
    uint32_t split_slices = 0, split_chunk = 0;
    if (sh->boids_split && sh->count) {
        boids_split_shape(sh->n, sh->count, tile, &split_slices, &split_chunk);
        const size_t need = boids_split_bytes(sh->n, sh->count, split_slices);
        if (need > sh->boids_partial_bytes) {
            NB_SH(sh, hipStreamSynchronize(sh->stream));
            if (sh->boids_partial) (void)hipFree(sh->boids_partial);
            sh->boids_partial = nullptr;
            sh->boids_partial_bytes = 0;
            NB_SH(sh, hipMalloc((void **)&sh->boids_partial, need));
            sh->boids_partial_bytes = need;
        }
        boids_split_pointers(&a, sh->boids_partial, split_slices, split_chunk);
    }
    if (!sh->velfull_valid) {  // (re)build the replica from the local velocities (n-body steps keep only those)
        float4 *vf = sh->velfull[sh->cur];
        if (sh->count)
            NB_SH(sh, hipMemcpyAsync(vf + lo, sh->vel, (size_t)sh->count * sizeof(float4), hipMemcpyDeviceToDevice, sh->stream));
        rc = shard_exchange(sh, vf);
        if (rc != NB_OK) return rc;
        sh->velfull_valid = true;
    }
    // A world above one exchanges BOTH outputs of a step in ONE all-gather: the kernel writes this rank's new positions and
    // velocities straight into its slot of the staging buffer ([pos slot | vel slot]: the output pointers are offset so that
    // record first + l lands there), the slots are gathered in place, and one small kernel deals them out to the replicas.
    const bool staged = sh->world > 1 || sh->rccl_solo;
    if (staged && !sh->pvstage) {
        NB_SH(sh, hipMalloc((void **)&sh->pvstage, 2 * padded));
        NB_SH(sh, hipMemsetAsync(sh->pvstage, 0, 2 * padded, sh->stream));
    }
    for (uint32_t s = 0; s < k; ++s) {
        float4 *pdst = sh->pos[sh->cur ^ 1], *vdst = sh->velfull[sh->cur ^ 1];
        if (sh->count) {
            a.pos_in = sh->pos[sh->cur];
            a.vel_in = sh->velfull[sh->cur];
            // staged: first == rank * slot for every non-empty rank, so (mine + l) == (out + first + l) with out = mine - first
            float4 *mine = staged ? sh->pvstage + (size_t)sh->rank * 2u * sh->slot : nullptr;
            a.pos_out = staged ? mine - sh->first : pdst;
            a.vel_out = staged ? mine + sh->slot - sh->first : vdst;
            if (split_slices)
                NB_SH(sh, nbk::launch_boids_split(a, tile, split_slices, sh->stream));
            else
                NB_SH(sh, nbk::launch_boids(a, tile, boids_form(a.count), sh->stream));
        }
        if (staged) {
            rc = shard_exchange(sh, sh->pvstage, nullptr, 2u * (size_t)sh->slot);
            if (rc == NB_OK) NB_SH(sh, nbk::launch_unstage(sh->slot, (uint32_t)sh->world, sh->pvstage, pdst, vdst, sh->stream));
        }
        if (rc != NB_OK) {
            sh->velfull_valid = false;
            return rc;
        }
        sh->cur ^= 1;
        sh->steps++;
    }
    if (sh->count && k)  // keep the local velocities current for n-body steps and downloads
        NB_SH(sh, hipMemcpyAsync(sh->vel, sh->velfull[sh->cur] + lo, (size_t)sh->count * sizeof(float4), hipMemcpyDeviceToDevice,
                                 sh->stream));
    return NB_OK;
}

NB_EXPORT int nb_shard_download(nb_shard *sh, float *pos_xyz, float *vel_xyz_local, float *inst_16n_local)
{
    int rc = shard_ready(sh, "nb_shard_download");
    if (rc != NB_OK) return rc;
    rc = shard_join_exchange(sh);
    if (rc != NB_OK) return rc;
    if (pos_xyz) {
        NB_SH(sh, nbk::launch_unpack(sh->n, sh->pos[sh->cur], sh->stage, sh->stream));
        NB_SH(sh, hipMemcpyAsync(pos_xyz, sh->stage, (size_t)sh->n * 3 * sizeof(float), hipMemcpyDeviceToHost, sh->stream));
        NB_SH(sh, hipStreamSynchronize(sh->stream));
    }
    if (vel_xyz_local && sh->count) {
        NB_SH(sh, nbk::launch_unpack(sh->count, sh->vel, sh->stage, sh->stream));
        NB_SH(sh, hipMemcpyAsync(vel_xyz_local, sh->stage, (size_t)sh->count * 3 * sizeof(float), hipMemcpyDeviceToHost, sh->stream));
        NB_SH(sh, hipStreamSynchronize(sh->stream));
    }
    if (inst_16n_local && sh->count) {
        if (!sh->inst) NB_SH(sh, hipMalloc((void **)&sh->inst, (size_t)sh->slot * 16 * sizeof(float)));
        NB_SH(sh, nbk::launch_instances(sh->count, sh->pos[sh->cur] + sh->first, sh->vel, sh->inst, sh->stream, overrides().inst_device_libm.on() ? 1u : 0u));
        NB_SH(sh, hipMemcpyAsync(inst_16n_local, sh->inst, (size_t)sh->count * 16 * sizeof(float), hipMemcpyDeviceToHost, sh->stream));
        NB_SH(sh, hipStreamSynchronize(sh->stream));
    }
    NB_SH(sh, hipStreamSynchronize(sh->stream));
    return check_status(&sh->status, &sh->err);
}

NB_EXPORT int nb_shard_sync(nb_shard *sh)
{
    if (!sh) {
        g_tls_error = "nb_shard_sync: shard is null";
        return NB_ERR_INVALID;
    }
    int rc = shard_join_exchange(sh);
    if (rc != NB_OK) return rc;
    NB_SH(sh, hipStreamSynchronize(sh->stream));
    return check_status(&sh->status, &sh->err);
}
