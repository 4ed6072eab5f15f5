// Multi-GPU exchange steps behind the C ABI: RCCL collectives on DEVICE buffers, issued by the host that drives
// the handle (a C++ service, or the Python shim through ctypes) -- no torch, no host staging of the payload.
//
//   scene per GPU (configs[3]): the build has no collective; for cross-scene retrieval every rank contributes its node
//     table (embeddings f32 [n][D] gathered on the device + the parent room of every node) and receives the global table
//     as a resident retrieval index: counts first (one 16-byte all-gather), then the payload padded to the largest table
//     (ncclAllGather straight out of / into HBM).  Global node index = prefix offset of the owning rank + local index, room
//     ids shifted the same way -- the index answers exactly like one built from the concatenated tables.
//   one episode over several GPUs (configs[4]): the per-voxel feature sums and frame counters of the ranks' frame windows
//     are all-reduced in place (graph.py:410-415: sums and counts add).
//
// librccl is loaded on first use (dlopen): a single-GPU process never needs it, and the kernel simulator build has none.
#include "hmsg_boundary.h"

#include <dlfcn.h>

#include <algorithm>

#include <functional>
#include <mutex>

// (device code is not linked across translation units: the two small kernels this file needs are stated here)
__global__ void k_cm_gather_rows(const float* __restrict__ src, const int* __restrict__ row, int n, int D, float* __restrict__ dst) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)n * D) return;
    dst[t] = src[(size_t)row[t / D] * D + t % D];
}
// graph.py:413-415 after the sums changed: feats = sum / (count, or 1e-5 where no frame saw the voxel)
__global__ void k_cm_feats_refresh(const float* __restrict__ sum, const unsigned* __restrict__ cnt, long long V, int D, float* __restrict__ feats) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)V * D) return;
    const unsigned c = cnt[t / D];
    const float d = c == 0u ? 1e-5f : (float)c;
    feats[t] = __fdiv_rn(sum[t], d);
}

namespace {

// the part of rccl.h this file needs (opaque communicator, 128-byte id, type / op codes as rccl.h:455-480 numbers them)
typedef void* rcclComm_t;
struct rcclUniqueId {
    char internal[128];
};
enum { RCCL_INT8 = 0, RCCL_INT32 = 2, RCCL_UINT32 = 3, RCCL_INT64 = 4, RCCL_FLOAT32 = 7, RCCL_FLOAT64 = 8, RCCL_SUM = 0 };

struct RcclApi {
    void* lib = nullptr;
    int (*GetUniqueId)(rcclUniqueId*) = nullptr;
    int (*CommInitRank)(rcclComm_t*, int, rcclUniqueId, int) = nullptr;
    int (*CommDestroy)(rcclComm_t) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, rcclComm_t, hipStream_t) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, rcclComm_t, hipStream_t) = nullptr;
    int (*Send)(const void*, size_t, int, int, rcclComm_t, hipStream_t) = nullptr;     // (point to point: the merge tree's joins)
    int (*Recv)(void*, size_t, int, int, rcclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    std::string why;
};
RcclApi& rccl() {
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        // HMSG_RCCL_LIB: another library with the same six symbols (tests: tests/rccl_double, a shared-memory stand-in that lets
        // the two exchange steps run with world > 1 on the kernel simulator)
        const char* over = getenv("HMSG_RCCL_LIB");
        const char* names[] = {over ? over : "librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"};
        for (const char* n : names) {
            api.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
            if (api.lib || over) break;
        }
        if (!api.lib) {
            api.why = std::string("librccl.so could not be loaded: ") + (dlerror() ? dlerror() : "?");
            return;
        }
        auto sym = [&](const char* s) {
            void* p = dlsym(api.lib, s);
            if (!p) api.why = std::string("librccl.so lacks ") + s;
            return p;
        };
        api.GetUniqueId = (int (*)(rcclUniqueId*))sym("ncclGetUniqueId");
        api.CommInitRank = (int (*)(rcclComm_t*, int, rcclUniqueId, int))sym("ncclCommInitRank");
        api.CommDestroy = (int (*)(rcclComm_t))sym("ncclCommDestroy");
        api.AllGather = (int (*)(const void*, void*, size_t, int, rcclComm_t, hipStream_t))sym("ncclAllGather");
        api.AllReduce = (int (*)(const void*, void*, size_t, int, int, rcclComm_t, hipStream_t))sym("ncclAllReduce");
        api.GetErrorString = (const char* (*)(int))sym("ncclGetErrorString");
        api.Send = (int (*)(const void*, size_t, int, int, rcclComm_t, hipStream_t))sym("ncclSend");
        api.Recv = (int (*)(void*, size_t, int, int, rcclComm_t, hipStream_t))sym("ncclRecv");
    });
    return api;
}
void rccl_need() {
    RcclApi& a = rccl();
    if (!a.why.empty() || !a.lib) throw hmsg_error{HMSG_ERR_UNSUPPORTED, a.why.empty() ? "RCCL not available" : a.why};
}
void rccl_try(int rc, const char* what) {
    if (rc == 0) return;
    RcclApi& a = rccl();
    throw hmsg_error{HMSG_ERR_HIP, std::string(what) + ": " + (a.GetErrorString ? a.GetErrorString(rc) : "RCCL error")};
}

}  // namespace

#define HMSG_COMM_HDR_BYTES 128
struct hmsg_comm {
    rcclComm_t comm = nullptr;
    int rank = 0, world = 1, device = 0;
    std::string err;
    unsigned* flag = nullptr;       // 4 bytes of HBM for the ranks' agreement (made with the communicator: agreeing must not need an allocation)
    char* hdr = nullptr;            // [world][HMSG_COMM_HDR_BYTES] of HBM for the sharded query's header exchange (the same reason)
};

namespace {
// the message of a failed hmsg_comm_unique_id / hmsg_comm_create (no communicator to keep it in): hmsg_comm_last_error(NULL)
thread_local std::string g_comm_err;

// Every rank must reach every collective, or the others wait for ever: a rank that finds something wrong with its OWN inputs
// (a node whose room lies outside the table, a failed allocation) does not return before the first collective -- the ranks
// first agree (a 4-byte all-reduce of an ok flag) and then fail together.
bool all_ranks_ok(hmsg_comm* c, bool mine_ok, hipStream_t s) {
    if (!c->comm) return mine_ok;
    const unsigned v = mine_ok ? 0u : 1u;
    unsigned sum = 0u;
    HIP_TRY(hipMemcpyAsync(c->flag, &v, 4, hipMemcpyHostToDevice, s));
    rccl_try(rccl().AllReduce(c->flag, c->flag, 1, RCCL_UINT32, RCCL_SUM, c->comm, s), "ncclAllReduce (ok flag)");
    HIP_TRY(hipMemcpyAsync(&sum, c->flag, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return sum == 0u;
}
// a rank-local phase between two collectives: what it throws is kept, the ranks agree, and then all of them fail together (the rank
// with the error reports it, the others that another rank failed) -- nobody is left waiting in the next collective
template <typename F>
void local_phase_then_agree(hmsg_comm* c, hipStream_t s, const char* what, F&& f) {
    std::string mine;
    int code = HMSG_OK;
    try {
        f();
    } catch (...) {      // (whatever it is: this rank must still reach the agreement below)
        hmsg_error e = hmsg_current_error();
        mine.swap(e.msg);
        code = e.code;
        if (mine.empty()) mine = what;
    }
    if (!all_ranks_ok(c, mine.empty(), s))
        throw hmsg_error{mine.empty() ? HMSG_ERR_INVALID : code, mine.empty() ? std::string(what) + ": another rank failed (see its hmsg_last_error)" : mine};
}
}  // namespace

extern "C" {

int hmsg_comm_unique_id(uint8_t* out_id) {
    if (!out_id) return HMSG_ERR_INVALID;
    return hmsg_boundary(&g_comm_err, -1, [&] {
        rccl_need();
        rcclUniqueId id;
        rccl_try(rccl().GetUniqueId(&id), "ncclGetUniqueId");
        memcpy(out_id, id.internal, sizeof(id.internal));
    });
}

int hmsg_comm_create(const uint8_t* id, int32_t rank, int32_t world, int32_t device_id, hmsg_comm_t** out) {
    if (!out) return HMSG_ERR_INVALID;
    *out = nullptr;
    if (world < 1 || rank < 0 || rank >= world) return HMSG_ERR_INVALID;
    hmsg_comm* c = nullptr;
    const int rc = hmsg_boundary(&g_comm_err, -1, [&] {
        c = new hmsg_comm();
        c->rank = rank;
        c->world = world;
        c->device = device_id;
        if (id == nullptr) {                   // one rank and no id: no communicator needed (every collective is the identity)
            HMSG_REQUIRE(world == 1, HMSG_ERR_INVALID, "hmsg_comm_create: more than one rank needs the id of hmsg_comm_unique_id");
            return;
        }
        rccl_need();
        HIP_TRY(hipSetDevice(device_id));
        rcclUniqueId uid;
        memcpy(uid.internal, id, sizeof(uid.internal));
        rccl_try(rccl().CommInitRank(&c->comm, world, uid, rank), "ncclCommInitRank");
        HIP_TRY(hipMalloc((void**)&c->flag, 64));
        HIP_TRY(hipMalloc((void**)&c->hdr, (size_t)world * HMSG_COMM_HDR_BYTES));
    });
    if (rc != HMSG_OK) {
        delete c;
        return rc;
    }
    *out = c;
    return HMSG_OK;
}

void hmsg_comm_destroy(hmsg_comm_t* c) {
    if (!c) return;
    if (c->comm) (void)rccl().CommDestroy(c->comm);
    if (c->flag) (void)hipFree(c->flag);
    if (c->hdr) (void)hipFree(c->hdr);
    delete c;
}

/* c == NULL: the message of this thread's last failed hmsg_comm_unique_id / hmsg_comm_create */
const char* hmsg_comm_last_error(const hmsg_comm_t* c) { return c ? c->err.c_str() : g_comm_err.c_str(); }

int hmsg_allgather_nodes(hmsg_t* h, hmsg_comm_t* c, int32_t n_rooms_local, hmsg_index_t** out_index, int64_t* node_off, int64_t* room_off) {
    if (!h || !c || !out_index) return HMSG_ERR_INVALID;
    *out_index = nullptr;
    int rc_index = HMSG_OK;
    const int rc = hmsg_boundary(h, [&] {
        hipStream_t s = h->stream;
        const int W = c->world, D = h->cfg.feat_dim;
        const long long n = (long long)h->nodes.size();
        // everything that can be wrong with THIS rank's inputs is looked at before the first collective, and the ranks agree
        std::string mine;
        if (n_rooms_local < 0) mine = "hmsg_allgather_nodes: negative room count";
        for (long long k = 0; k < n && mine.empty(); ++k)
            if (h->nodes[(size_t)k].room < 0 || h->nodes[(size_t)k].room >= n_rooms_local) mine = "hmsg_allgather_nodes: a node's room lies outside n_rooms_local";
        if (n && !h->pooled) mine = "hmsg_allgather_nodes: run hmsg_pool_instances first";
        if (!all_ranks_ok(c, mine.empty(), s))
            throw hmsg_error{HMSG_ERR_INVALID, mine.empty() ? "hmsg_allgather_nodes: another rank's node table is invalid (see its hmsg_last_error)" : mine};
        // 1. counts (nodes, rooms) of every rank
        std::vector<long long> meta((size_t)W * 2, 0);
        meta[(size_t)c->rank * 2] = n;
        meta[(size_t)c->rank * 2 + 1] = n_rooms_local;
        if (c->comm) {
            DevBuf<long long> dm;
            dm.alloc((size_t)W * 2);
            HIP_TRY(hipMemcpyAsync(dm.p + (size_t)c->rank * 2, meta.data() + (size_t)c->rank * 2, 16, hipMemcpyHostToDevice, s));
            rccl_try(rccl().AllGather(dm.p + (size_t)c->rank * 2, dm.p, 2, RCCL_INT64, c->comm, s), "ncclAllGather (counts)");
            HIP_TRY(hipMemcpyAsync(meta.data(), dm.p, (size_t)W * 16, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
        std::vector<long long> noff((size_t)W + 1, 0), roff((size_t)W + 1, 0);
        long long nmax = 1;
        for (int r = 0; r < W; ++r) {
            noff[(size_t)r + 1] = noff[(size_t)r] + meta[(size_t)r * 2];
            roff[(size_t)r + 1] = roff[(size_t)r] + meta[(size_t)r * 2 + 1];
            nmax = std::max(nmax, meta[(size_t)r * 2]);
        }
        const long long N = noff[(size_t)W];
        if (node_off) for (int r = 0; r <= W; ++r) node_off[r] = noff[(size_t)r];
        if (room_off) for (int r = 0; r <= W; ++r) room_off[r] = roff[(size_t)r];
        HMSG_REQUIRE(N > 0, HMSG_ERR_INVALID, "hmsg_allgather_nodes: no nodes on any rank (hmsg_build_object_nodes)");
        // 2. payload: every rank's slot is nmax rows of D floats + nmax room ids, padded; mine is gathered on the device
        DevBuf<float> emb;                       // [W][nmax][D]
        DevBuf<int> room;                        // [W][nmax]
        float* my_emb = nullptr;
        int* my_room = nullptr;
        local_phase_then_agree(c, s, "hmsg_allgather_nodes", [&] {
        emb.alloc((size_t)W * nmax * D);
        room.alloc((size_t)W * nmax);
        my_emb = emb.p + (size_t)c->rank * nmax * D;
        my_room = room.p + (size_t)c->rank * nmax;
        if (n) {
            std::vector<int> inst((size_t)n), rm((size_t)n);
            for (long long k = 0; k < n; ++k) {
                inst[(size_t)k] = h->nodes[(size_t)k].instance;
                rm[(size_t)k] = h->nodes[(size_t)k].room + (int)roff[(size_t)c->rank];        // global room id
            }
            DevBuf<int> d_inst;
            d_inst.alloc((size_t)n);
            HIP_TRY(hipMemcpyAsync(d_inst.p, inst.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(my_room, rm.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(k_cm_gather_rows, dim3(cdiv((size_t)n * D, 256)), dim3(256), 0, s, (const float*)h->inst_feats.p, (const int*)d_inst.p,
                               (int)n, D, my_emb);
            HMSG_CHECK_LAUNCH();
            HIP_TRY(hipStreamSynchronize(s));    // (inst / rm are stack vectors)
        }
        });
        if (c->comm) {
            rccl_try(rccl().AllGather(my_emb, emb.p, (size_t)nmax * D, RCCL_FLOAT32, c->comm, s), "ncclAllGather (embeddings)");
            rccl_try(rccl().AllGather(my_room, room.p, (size_t)nmax, RCCL_INT32, c->comm, s), "ncclAllGather (rooms)");
        }
        // 3. drop the padding (device copies), hand the packed table to the index
        DevBuf<float> packed;
        DevBuf<int> proom;
        packed.alloc((size_t)N * D);
        proom.alloc((size_t)N);
        for (int r = 0; r < W; ++r) {
            const long long nr = meta[(size_t)r * 2];
            if (!nr) continue;
            HIP_TRY(hipMemcpyAsync(packed.p + (size_t)noff[(size_t)r] * D, emb.p + (size_t)r * nmax * D, (size_t)nr * D * 4, hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipMemcpyAsync(proom.p + (size_t)noff[(size_t)r], room.p + (size_t)r * nmax, (size_t)nr * 4, hipMemcpyDeviceToDevice, s));
        }
        HIP_TRY(hipStreamSynchronize(s));
        rc_index = hmsg_index_create(h->cfg.device_id, D, N, packed.p, 0, proom.p, out_index);
        if (rc_index != HMSG_OK) throw hmsg_error{rc_index, "hmsg_allgather_nodes: hmsg_index_create failed"};
    });
    if (rc != HMSG_OK) c->err = h->err;
    return rc;
}

int hmsg_allreduce_feature_sums(hmsg_t* h, hmsg_comm_t* c) {
    if (!h || !c) return HMSG_ERR_INVALID;
    const int rc = hmsg_boundary(h, [&] {
        hipStream_t s = h->stream;
        std::string mine;
        if (h->restored) mine = "hmsg_allreduce_feature_sums: the handle was restored from stage artefacts (hmsg_restore_stage): no feature sums";
        else if (!h->feats_final) mine = "hmsg_allreduce_feature_sums: run hmsg_fuse_frames first";
        else if (h->pooled) mine = "hmsg_allreduce_feature_sums after hmsg_pool_instances";
        if (!all_ranks_ok(c, mine.empty(), s))
            throw hmsg_error{HMSG_ERR_INVALID, mine.empty() ? "hmsg_allreduce_feature_sums: another rank is not ready (see its hmsg_last_error)" : mine};
        const size_t n = (size_t)h->V * h->cfg.feat_dim;
        if (c->comm && n) {
            rccl_try(rccl().AllReduce(h->sum.p, h->sum.p, n, RCCL_FLOAT32, RCCL_SUM, c->comm, s), "ncclAllReduce (feature sums)");
            rccl_try(rccl().AllReduce(h->cnt.p, h->cnt.p, (size_t)h->V, RCCL_UINT32, RCCL_SUM, c->comm, s), "ncclAllReduce (frame counters)");
        }
        if (n) hipLaunchKernelGGL(k_cm_feats_refresh, dim3(cdiv(n, 256)), dim3(256), 0, s, (const float*)h->sum.p, (const unsigned*)h->cnt.p,
                                  (long long)h->V, h->cfg.feat_dim, h->feats.p);
        HMSG_CHECK_LAUNCH();
        HIP_TRY(hipStreamSynchronize(s));
    });
    if (rc != HMSG_OK) c->err = h->err;
    return rc;
}

}  // extern "C"

// all-gather of one byte string per rank (lengths first, then the payload padded to the longest): the small host-side tables that
// travel with the node tables (hmsg_graph_allgather_index).  all[r] = rank r's bytes, on every rank.
void hmsg_comm_allgather_bytes(hmsg_ctx* h, hmsg_comm* c, const void* mine, size_t my_bytes, std::vector<std::vector<char>>& all) {
    const int W = c->world;
    all.assign((size_t)W, std::vector<char>());
    if (!c->comm) {
        all[0].assign((const char*)mine, (const char*)mine + my_bytes);
        return;
    }
    hipStream_t s = h->stream;
    std::vector<long long> len((size_t)W, 0);
    len[(size_t)c->rank] = (long long)my_bytes;
    DevBuf<long long> dl;
    dl.alloc((size_t)W);
    HIP_TRY(hipMemcpyAsync(dl.p + c->rank, &len[(size_t)c->rank], 8, hipMemcpyHostToDevice, s));
    rccl_try(rccl().AllGather(dl.p + c->rank, dl.p, 1, RCCL_INT64, c->comm, s), "ncclAllGather (table lengths)");
    HIP_TRY(hipMemcpyAsync(len.data(), dl.p, (size_t)W * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    long long mx = 1;
    for (long long v : len) mx = std::max(mx, v);
    mx = (mx + 15) & ~15ll;
    DevBuf<char> buf;
    buf.alloc((size_t)W * (size_t)mx);
    if (my_bytes) HIP_TRY(hipMemcpyAsync(buf.p + (size_t)c->rank * (size_t)mx, mine, my_bytes, hipMemcpyHostToDevice, s));
    rccl_try(rccl().AllGather(buf.p + (size_t)c->rank * (size_t)mx, buf.p, (size_t)mx, RCCL_INT8, c->comm, s), "ncclAllGather (tables)");
    std::vector<char> hostbuf((size_t)W * (size_t)mx);
    HIP_TRY(hipMemcpyAsync(hostbuf.data(), buf.p, hostbuf.size(), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int r = 0; r < W; ++r) all[(size_t)r].assign(hostbuf.begin() + (ptrdiff_t)((size_t)r * (size_t)mx), hostbuf.begin() + (ptrdiff_t)((size_t)r * (size_t)mx + (size_t)len[(size_t)r]));
}
int hmsg_comm_rank(const hmsg_comm* c) { return c->rank; }
int hmsg_comm_world(const hmsg_comm* c) { return c->world; }
void hmsg_comm_set_error(hmsg_comm* c, const std::string& e) { c->err = e; }
int hmsg_comm_device(const hmsg_comm* c) { return c->device; }
// (hmsg_query_sharded.hip) local_phase_then_agree for another translation unit (no communicator at all: f runs, what it throws
// passes through); an all-gather of `slot_bytes` per rank IN PLACE on the device: buf = [world][slot_bytes] with this rank's slot
// filled (ncclAllGather from buf + rank * slot_bytes; no communicator: the identity); and the header exchange: `bytes` (at most
// HMSG_COMM_HDR_BYTES) of this rank's host words -> every rank's, through the buffer made with the communicator (no allocation)
void hmsg_comm_local_phase_then_agree(hmsg_comm* c, hipStream_t s, const char* what, const std::function<void()>& f) {
    if (!c) {
        f();
        return;
    }
    local_phase_then_agree(c, s, what, f);
}
void hmsg_comm_allgather_header(hmsg_comm* c, const void* mine, size_t bytes, void* all, hipStream_t s) {
    if (bytes > HMSG_COMM_HDR_BYTES) throw hmsg_error{HMSG_ERR_INVALID, "hmsg_comm_allgather_header: header too long"};
    if (!c->comm) {
        memcpy(all, mine, bytes);
        return;
    }
    HIP_TRY(hipMemcpyAsync(c->hdr + (size_t)c->rank * HMSG_COMM_HDR_BYTES, mine, bytes, hipMemcpyHostToDevice, s));
    rccl_try(rccl().AllGather(c->hdr + (size_t)c->rank * HMSG_COMM_HDR_BYTES, c->hdr, HMSG_COMM_HDR_BYTES, RCCL_INT8, c->comm, s), "ncclAllGather (header)");
    std::vector<char> h((size_t)c->world * HMSG_COMM_HDR_BYTES);
    HIP_TRY(hipMemcpyAsync(h.data(), c->hdr, h.size(), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int r = 0; r < c->world; ++r) memcpy((char*)all + (size_t)r * bytes, h.data() + (size_t)r * HMSG_COMM_HDR_BYTES, bytes);
}
void hmsg_comm_allgather_inplace(hmsg_comm* c, void* buf, size_t slot_bytes, hipStream_t s) {
    if (!c->comm || !slot_bytes) return;
    char* b = (char*)buf;
    rccl_try(rccl().AllGather(b + (size_t)c->rank * slot_bytes, b, slot_bytes, RCCL_INT8, c->comm, s), "ncclAllGather (sharded query)");
}

extern "C" {

/* ---- point to point: `bytes` of a DEVICE buffer to / from another rank (ncclSend / ncclRecv on the handle's stream; returns when
 * the transfer has completed).  What the cross-rank joins of the sharded merge tree are made of; a host that schedules them itself
 * can use the pair directly. */
int hmsg_comm_send(hmsg_t* h, hmsg_comm_t* c, const void* dev_buf, int64_t bytes, int32_t dst) {
    if (!h || !c || bytes < 0 || (bytes && !dev_buf) || dst < 0 || dst >= c->world || dst == c->rank) return HMSG_ERR_INVALID;
    const int rc = hmsg_boundary(&h->err, -1, [&] {
        HMSG_REQUIRE(c->comm, HMSG_ERR_INVALID, "hmsg_comm_send: a communicator of one rank has nobody to send to");
        HIP_TRY(hipSetDevice(h->cfg.device_id));
        if (bytes) rccl_try(rccl().Send(dev_buf, (size_t)bytes, RCCL_INT8, dst, c->comm, h->stream), "ncclSend");
        HIP_TRY(hipStreamSynchronize(h->stream));
    });
    if (rc != HMSG_OK) c->err = h->err;
    return rc;
}
int hmsg_comm_recv(hmsg_t* h, hmsg_comm_t* c, void* dev_buf, int64_t bytes, int32_t src) {
    if (!h || !c || bytes < 0 || (bytes && !dev_buf) || src < 0 || src >= c->world || src == c->rank) return HMSG_ERR_INVALID;
    const int rc = hmsg_boundary(&h->err, -1, [&] {
        HMSG_REQUIRE(c->comm, HMSG_ERR_INVALID, "hmsg_comm_recv: a communicator of one rank has nobody to receive from");
        HIP_TRY(hipSetDevice(h->cfg.device_id));
        if (bytes) rccl_try(rccl().Recv(dev_buf, (size_t)bytes, RCCL_INT8, src, c->comm, h->stream), "ncclRecv");
        HIP_TRY(hipStreamSynchronize(h->stream));
    });
    if (rc != HMSG_OK) c->err = h->err;
    return rc;
}

/* ---- hierarchical_merge (graph_utils.py:989-1012) of ONE episode whose frame windows are spread over the ranks, in one call per
 * rank (configs[4]; until round 5 the schedule was Python: holoagent_amd/dist.py sharded_hierarchical_merge over torch.distributed):
 *   1. hmsg_merge_tree_local: the levels inside this rank's window;
 *   2. all-gather of (lists, index): the ranks agree on the level they meet at -- a rank that stopped lower holds the last, unpaired
 *      list of its level and carries it up unchanged, as merge_adjacent_frames does with an odd last list;
 *   3. level by level: the owner of list 2k + 1 sends its clouds (count, sizes, points: HBM to HBM, ncclSend / ncclRecv) to the
 *      owner of list 2k, which merges [mine ++ theirs] (hmsg_merge_tree_join; the last join runs the final pass).  Owners are
 *      tracked per list: any number of ranks.
 * holds_result = 1 on the rank that ends with the episode's instances (rank 0's window starts the episode), bit-identical to a
 * one-process hmsg_merge_instances. */
int hmsg_merge_tree_sharded(hmsg_t* h, hmsg_comm_t* c, int32_t total_frames, int32_t* holds_result) {
    if (!h || !c || !holds_result) return HMSG_ERR_INVALID;
    *holds_result = 0;
    const int rc = hmsg_boundary(h, [&] {
        hipStream_t s = h->stream;
        const int W = c->world, me = c->rank;
        const double factor = h->cfg.overlap_thresh_factor;
        auto next_th = [&](double th, long long lists) { return lists > 1 ? th - factor * (double)(lists - 2) / (double)std::max<long long>(1, lists - 1) : th; };
        double th = 0.0;
        int64_t lists = 0, idx = 0;
        const int rc_local = hmsg_merge_tree_local(h, total_frames, &th, &lists, &idx);
        // (a rank whose local levels failed must not leave the others in the collective below: agree first)
        if (!all_ranks_ok(c, rc_local == HMSG_OK, s))
            throw hmsg_error{rc_local != HMSG_OK ? rc_local : HMSG_ERR_INVALID,
                             rc_local != HMSG_OK ? h->err : std::string("hmsg_merge_tree_sharded: another rank's local merge failed (see its hmsg_last_error)")};
        std::vector<long long> meta((size_t)W * 2, 0);
        meta[(size_t)me * 2] = lists;
        meta[(size_t)me * 2 + 1] = idx;
        if (c->comm) {
            DevBuf<long long> dm;
            dm.alloc((size_t)W * 2);
            HIP_TRY(hipMemcpyAsync(dm.p + (size_t)me * 2, meta.data() + (size_t)me * 2, 16, hipMemcpyHostToDevice, s));
            rccl_try(rccl().AllGather(dm.p + (size_t)me * 2, dm.p, 2, RCCL_INT64, c->comm, s), "ncclAllGather (tree levels)");
            HIP_TRY(hipMemcpyAsync(meta.data(), dm.p, (size_t)W * 16, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
        long long target = meta[0];
        for (int r = 0; r < W; ++r) target = std::min(target, meta[(size_t)r * 2]);
        std::vector<int> owner;                  // list index at the common level -> rank (every rank derives the same table)
        for (int r = 0; r < W; ++r) {
            long long l = meta[(size_t)r * 2], i = meta[(size_t)r * 2 + 1];
            double t = th;
            while (l > target) {
                HMSG_REQUIRE(i == l - 1 && l % 2 == 1, HMSG_ERR_INVALID,
                             "hmsg_merge_tree_sharded: rank " + std::to_string(r) + "'s frame window is not a subtree of the merge tree");
                i /= 2;
                l = (l + 1) / 2;
                t = next_th(t, l);
            }
            if ((long long)owner.size() <= i) owner.resize((size_t)i + 1, -1);
            HMSG_REQUIRE(owner[(size_t)i] < 0, HMSG_ERR_INVALID, "hmsg_merge_tree_sharded: two ranks hold list " + std::to_string(i));
            owner[(size_t)i] = r;
            if (r == me) {
                th = t;
                lists = l;
                idx = i;
            }
        }
        HMSG_REQUIRE((long long)owner.size() == lists && std::find(owner.begin(), owner.end(), -1) == owner.end(), HMSG_ERR_INVALID,
                     "hmsg_merge_tree_sharded: the ranks' windows do not cover the lists of their common level");
        if (lists == 1) {                        // one rank held every frame
            if (owner[0] == me) {
                const int rj = hmsg_merge_tree_join(h, 0, nullptr, nullptr, th, 1);
                if (rj != HMSG_OK) throw hmsg_error{rj, h->err};
                *holds_result = 1;
            }
            return;
        }
        bool active = true;
        DevBuf<long long> d_n, d_sizes;
        DevBuf<double> d_pts;
        d_n.alloc(1);
        while (lists > 1) {
            const long long nxt = (lists + 1) / 2;
            if (active && idx % 2 == 1) {        // my list is the odd one of its pair: it travels
                const int dst = owner[(size_t)idx - 1];
                const long long n = hmsg_num_instances(h);
                std::vector<int64_t> sizes((size_t)std::max<long long>(n, 1));
                if (n && hmsg_get_instance_sizes(h, sizes.data()) != HMSG_OK) throw hmsg_error{HMSG_ERR_INVALID, h->err};
                long long total = 0;
                for (long long k = 0; k < n; ++k) total += sizes[(size_t)k];
                HIP_TRY(hipMemcpyAsync(d_n.p, &n, 8, hipMemcpyHostToDevice, s));
                rccl_try(rccl().Send(d_n.p, 1, RCCL_INT64, dst, c->comm, s), "ncclSend (count)");
                if (n) {
                    d_sizes.ensure((size_t)n);
                    HIP_TRY(hipMemcpyAsync(d_sizes.p, sizes.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
                    rccl_try(rccl().Send(d_sizes.p, (size_t)n, RCCL_INT64, dst, c->comm, s), "ncclSend (sizes)");
                    if (total) {
                        d_pts.ensure((size_t)total * 3);
                        if (hmsg_get_instance_points(h, d_pts.p) != HMSG_OK) throw hmsg_error{HMSG_ERR_INVALID, h->err};      // HBM -> HBM
                        rccl_try(rccl().Send(d_pts.p, (size_t)total * 3, RCCL_FLOAT64, dst, c->comm, s), "ncclSend (points)");
                    }
                }
                HIP_TRY(hipStreamSynchronize(s));
                active = false;
            } else if (active && idx + 1 < lists) {      // I hold the even one: merge [mine ++ theirs]
                const int src = owner[(size_t)idx + 1];
                long long n = 0;
                rccl_try(rccl().Recv(d_n.p, 1, RCCL_INT64, src, c->comm, s), "ncclRecv (count)");
                HIP_TRY(hipMemcpyAsync(&n, d_n.p, 8, hipMemcpyDeviceToHost, s));
                HIP_TRY(hipStreamSynchronize(s));
                std::vector<int64_t> sizes((size_t)std::max<long long>(n, 1));
                long long total = 0;
                if (n) {
                    d_sizes.ensure((size_t)n);
                    rccl_try(rccl().Recv(d_sizes.p, (size_t)n, RCCL_INT64, src, c->comm, s), "ncclRecv (sizes)");
                    HIP_TRY(hipMemcpyAsync(sizes.data(), d_sizes.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
                    HIP_TRY(hipStreamSynchronize(s));
                    for (long long k = 0; k < n; ++k) total += sizes[(size_t)k];
                    if (total) {
                        d_pts.ensure((size_t)total * 3);
                        rccl_try(rccl().Recv(d_pts.p, (size_t)total * 3, RCCL_FLOAT64, src, c->comm, s), "ncclRecv (points)");
                        HIP_TRY(hipStreamSynchronize(s));
                    }
                }
                const int rj = hmsg_merge_tree_join(h, (int32_t)n, sizes.data(), total ? d_pts.p : nullptr, th, nxt == 1 ? 1 : 0);   // (reads the receive buffer in place)
                if (rj != HMSG_OK) throw hmsg_error{rj, h->err};
            }
            // (an even list without a partner is carried to the next level unchanged)
            std::vector<int> up((size_t)nxt, -1);
            for (long long k = 0; k < lists; k += 2) up[(size_t)(k / 2)] = owner[(size_t)k];
            owner.swap(up);
            idx /= 2;
            lists = nxt;
            th = next_th(th, lists);
        }
        *holds_result = active ? 1 : 0;
    });
    if (rc != HMSG_OK) c->err = h->err;
    return rc;
}

}  // extern "C"
