// The coarse-to-fine query (hmsg_query_hier) over scene graphs that stay where they are (scene per GPU): tables stay
// sharded, the queries go to every shard, each shard scores only its own rooms and nodes, and what crosses between shards is a
// row per (query, room) and k candidates per query -- never a table.
//
// The answer is that of hmsg_query_hier on ONE index over the concatenated tables (hmsg_graph_allgather_index's index), bit for bit:
//   room stage   every shard reduces its own room-stage GEMMs to one float64 per (query, local room) -- the name similarity (label
//                mode) and the largest similarity over the room's views (view modes; a maximum does not depend on the order) --
//                plus its floor lists, room keys and view counts.  After the exchange every shard runs the GLOBAL room selection
//                (k_sh_room_select: k_room_select's rules on room-level rows) and so holds the same sel / nsel;
//   object stage every shard scores its own nodes (the same f64 GEMM), walks the rooms of the global sel that it owns and keeps
//                its top k by (score desc, key asc) twice -- plain and negative-filtered -- with the count of filtered candidates.
//                key = (position in sel, node position in the room): the candidate order of k_query_topk ("room order, then node
//                order", hmsg_query.hip), so ties break as there.  After the exchange k_sh_merge picks the filtered lists when
//                negatives are on and any shard had a filtered candidate, and merges the shards' lists into the top k.
// Each S[q][n] is the same float64 whichever GEMM kernel computed it (hmsg_query.h: hmsg_gemm_f64), so a shard's smaller table
// scores exactly like its rows of the concatenated one.
#include "hmsg_boundary.h"
#include "hmsg_query_rules.h"

#include <algorithm>
#include <functional>
#include <optional>

// (hmsg_scene_graph.hip)
struct hmsg_graph;
struct hmsg_shard_ws;
hmsg_index_t* hmsg_graph_shard_index(hmsg_graph* g, int* n_floor_rooms);
hmsg_shard_ws*& hmsg_graph_shard_ws(hmsg_graph* g);
int hmsg_graph_device(const hmsg_graph* g);
void hmsg_graph_set_error(hmsg_graph* g, const std::string& e);
// (hmsg_comm.hip)
struct hmsg_comm;
int hmsg_comm_rank(const hmsg_comm* c);
int hmsg_comm_world(const hmsg_comm* c);
int hmsg_comm_device(const hmsg_comm* c);
void hmsg_comm_set_error(hmsg_comm* c, const std::string& e);
void hmsg_comm_local_phase_then_agree(hmsg_comm* c, hipStream_t s, const char* what, const std::function<void()>& f);
void hmsg_comm_allgather_inplace(hmsg_comm* c, void* buf, size_t slot_bytes, hipStream_t s);
void hmsg_comm_allgather_header(hmsg_comm* c, const void* mine, size_t bytes, void* all, hipStream_t s);

// one candidate of a shard's list: score, global tie key, global node index, global room id (key LLONG_MAX: no candidate)
struct ShRec {
    double s;
    long long key;
    int node, room;
};

// where the sections of one shard's slot of the room exchange lie (bytes from the slot's start)
struct ShRoomLayout {
    long long o_lab, o_view, o_fro, o_fr, o_key, o_vcnt, bytes;
    int Rmax, Fmax, NFRmax;
};

// name similarities [Q][R] -> the slot's rows [Q][Rmax]
__global__ void k_sh_pad_rows(const double* __restrict__ src, int Q, int R, int Rmax, double* __restrict__ dst) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)Q * R) return;
    const size_t q = i / (size_t)R, r = i % (size_t)R;
    dst[q * (size_t)Rmax + r] = src[i];
}

// per (query, room): the largest similarity over the room's views, in k_room_select's fmax chain from -1e308 (a maximum: the
// same value in any order); no view leaves -1e308 and a view count of 0, which the global selection turns into the error
__global__ void k_sh_view_max(const double* __restrict__ S_view, long long NV, const int* __restrict__ view_off, int Q, int R, int Rmax,
                              double* __restrict__ dst) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)Q * R) return;
    const size_t q = i / (size_t)R;
    const int r = (int)(i % (size_t)R);
    double mx = -1e308;
    for (int v = view_off[r]; v < view_off[r + 1]; ++v) mx = fmax(mx, S_view[q * (size_t)NV + v]);
    dst[q * (size_t)Rmax + r] = mx;
}

// the shard's levels above the nodes into its slot: floor CSR, room keys, view counts (local ids)
__global__ void k_sh_tables(const int* __restrict__ floor_room_off, int F, const int* __restrict__ floor_rooms, int NFR,
                            const int* __restrict__ room_key, const int* __restrict__ view_off, int R, int* __restrict__ fro,
                            int* __restrict__ fr, int* __restrict__ key, int* __restrict__ vcnt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= F) fro[i] = floor_room_off[i];
    if (i < NFR) fr[i] = floor_rooms[i];
    if (i < R) {
        key[i] = room_key[i];
        vcnt[i] = view_off[i + 1] - view_off[i];
    }
}

// the room level of every shard's slot of the room exchange, as room_select sees it for query q.  Room r (global) lives in the slot
// of the shard s with roff[s] <= r < roff[s + 1], as local room r - roff[s]; floor f (global) likewise by foff.
struct ShardRooms {
    const char* rb;
    long long slot;
    ShRoomLayout lay;
    const int* roff;
    const int *fro, *frs;                // the floor's list in its shard's slot (local room ids from room0), or NULL for all rooms in order
    int W, q, room0, L;
    bool bad_floor;
    __device__ int shard_of(int r) const {
        int s = 0;
        while (s + 1 < W && r >= roff[s + 1]) ++s;
        return s;
    }
    __device__ double row(long long off, int r) const {      // the f64 row entry of (q, global room r)
        const int s = shard_of(r);
        return ((const double*)(rb + (size_t)s * slot + off))[(size_t)q * lay.Rmax + (r - roff[s])];
    }
    __device__ int tab(long long off, int r) const {         // the int table entry of global room r
        const int s = shard_of(r);
        return ((const int*)(rb + (size_t)s * slot + off))[r - roff[s]];
    }
    __device__ int room_at(int i) const { return frs ? room0 + frs[i] : i; }
    __device__ double name_sim(int i) const { return row(lay.o_lab, room_at(i)); }
    __device__ double view_max(int i) const { return row(lay.o_view, room_at(i)); }      // (k_sh_view_max, on the owning shard)
    __device__ bool has_views(int i) const { return tab(lay.o_vcnt, room_at(i)) != 0; }
    __device__ int room_key(int r) const { return tab(lay.o_key, r); }
};
// The GLOBAL room selection (hmsg_query_rules.h) on the gathered room-level rows, one workgroup per query.  sel / nsel / err as
// k_room_select; q_rooms [Q][max_sel]: global room ids.
__global__ void __launch_bounds__(256) k_sh_room_select(const char* __restrict__ rb, long long slot, ShRoomLayout lay, int W,
                                                        const int* __restrict__ roff, const int* __restrict__ foff,
                                                        const int* __restrict__ floor_id, const int* __restrict__ mode, int max_sel,
                                                        int* __restrict__ sel, int* __restrict__ nsel, int* __restrict__ q_rooms,
                                                        int* __restrict__ err) {
    const int q = blockIdx.x, f = floor_id[q];
    __shared__ int s_fs;                          // the shard of floor f
    if (threadIdx.x == 0) {
        int fs = -1;
        for (int s = 0; s < W && f >= 0; ++s)
            if (f >= foff[s] && f < foff[s + 1]) fs = s;
        s_fs = fs;
    }
    __syncthreads();
    const int fs = s_fs;
    ShardRooms src;
    src.rb = rb;
    src.slot = slot;
    src.lay = lay;
    src.roff = roff;
    src.W = W;
    src.q = q;
    src.bad_floor = f >= foff[W];
    src.fro = src.frs = nullptr;
    src.room0 = 0;
    src.L = f < 0 ? roff[W] : 0;
    if (fs >= 0) {
        const int* fro = (const int*)(rb + (size_t)fs * slot + lay.o_fro) + (f - foff[fs]);
        src.frs = (const int*)(rb + (size_t)fs * slot + lay.o_fr) + fro[0];
        src.room0 = roff[fs];
        src.L = fro[1] - fro[0];
    }
    room_select(src, mode[q], max_sel, sel + (size_t)q * max_sel, nsel + q, q_rooms + (size_t)q * max_sel, err + q);
}

// One shard's candidates, one workgroup per query: the nodes of the rooms of q_rooms that this shard owns (global ids in
// [room0, room0 + n_rooms_nodes)), in sel order then node order.  Out: recs [Q][2k] (the exact top k of hmsg_query_rules.h, then
// the top k of the candidates whose arg-max class is the query's) and cnt [Q] (how many of those there are).
__global__ void __launch_bounds__(256) k_sh_candidates(const double* __restrict__ S, long long N, int C, const int* __restrict__ qid,
                                                       const int* __restrict__ q_rooms, int max_sel, const int* __restrict__ room_off,
                                                       const int* __restrict__ room_nodes, int room0, int n_rooms_nodes, int node0, int k,
                                                       int use_neg, ShRec* __restrict__ recs, int* __restrict__ cnt) {
    __shared__ double sh_s[128];
    __shared__ long long sh_k[128];
    __shared__ int sh_n[256];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int myq = qid[q];
    const double* Sq = S + (size_t)q * C * N;
    const int* rq = q_rooms + (size_t)q * max_sel;
    // this thread's nodes of the query's rooms held here: f(key, node)
    auto each_node = [&](auto&& f) {
        for (int j = 0; j < max_sel; ++j) {
            const int lr = rq[j] - room0;
            if (rq[j] < 0 || lr < 0 || lr >= n_rooms_nodes) continue;
            const int b = room_off[lr];
            for (int t = b + tid; t < room_off[lr + 1]; t += 256) f(qkey(j, t - b), room_nodes[t]);
        }
    };
    // the count of filtered candidates
    int mine = 0;
    if (use_neg) each_node([&](long long, int node) { mine += argmax_class_is(Sq, N, C, node, myq) ? 1 : 0; });
    sh_n[tid] = mine;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) sh_n[tid] += sh_n[tid + o];
        __syncthreads();
    }
    if (tid == 0) cnt[q] = sh_n[0];
    ShRec* out = recs + (size_t)q * 2 * k;
    for (int list = 0; list < 2; ++list) {
        const bool filtered = list == 1;
        pick_top_k<256>(
            k, sh_s, sh_k,
            [&](auto&& offer) {
                if (filtered && !use_neg) return;
                each_node([&](long long key, int node) {
                    if (!filtered || argmax_class_is(Sq, N, C, node, myq)) offer(Sq[(size_t)myq * N + node], key);
                });
            },
            [&](int round, double s, long long key, bool) {
                if (tid != 0) return;
                ShRec rec{0.0, QKEY_NONE, -1, -1};
                if (key != QKEY_NONE) {
                    rec.s = s;
                    rec.key = key;
                    rec.room = rq[qkey_j(key)];
                    rec.node = node0 + room_nodes[room_off[rec.room - room0] + qkey_place(key)];
                }
                out[(size_t)list * k + round] = rec;
            });
    }
}

// The shards' lists into the answer, one wave per query: the filtered lists when negatives are on and any shard counted a
// filtered candidate (k_query_topk's `filtered`), else the plain ones; the exact top k of the W * k records.
__global__ void __launch_bounds__(64) k_sh_merge(const char* __restrict__ cb, long long slot, long long o_cnt, int W, int Q, int k, int use_neg,
                                                 int* __restrict__ out_idx, int* __restrict__ out_room, double* __restrict__ out_score) {
    __shared__ double sh_s[32];
    __shared__ long long sh_k[32];
    __shared__ int sh_list;
    const int q = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        long long total = 0;
        for (int s = 0; s < W; ++s) total += ((const int*)(cb + (size_t)s * slot + o_cnt))[q];
        sh_list = (use_neg && total > 0) ? 1 : 0;
    }
    __syncthreads();
    const int list = sh_list;
    auto rec = [&](int i) {                       // record i of the W * k of this query's chosen lists
        const int s = i / k, r = i % k;
        return ((const ShRec*)(cb + (size_t)s * slot))[((size_t)q * 2 + list) * k + r];
    };
    int bi = -1;                                  // this thread's best record of the round
    pick_top_k<64>(
        k, sh_s, sh_k,
        [&](auto&& offer) {
            for (int i = tid; i < W * k; i += 64) {
                const ShRec c = rec(i);
                if (c.key != QKEY_NONE && offer(c.s, c.key)) bi = i;
            }
        },
        [&](int round, double, long long key, bool mine) {
            const size_t o = (size_t)q * k + round;
            if (mine) {
                const ShRec c = rec(bi);
                out_idx[o] = c.node;
                out_room[o] = c.room;
                out_score[o] = c.s;
            } else if (tid == 0 && key == QKEY_NONE) {
                out_idx[o] = -1;
                out_room[o] = -1;
                out_score[o] = 0.0;
            }
        });
}

namespace {

long long al16(long long b) { return (b + 15) & ~15ll; }

}  // namespace

// the sharded path's scratch, kept on each graph between calls (ensure(): grown, never shrunk, freed with the graph); the buffers
// of the exchange belong to the first shard's graph, the GEMM outputs to every shard's own
struct hmsg_shard_ws {
    DevBuf<char> out, room, cand;
    DevBuf<int> qin, qrooms;
    DevBuf<double> T64, Tr64, names, S_room, S_view, S;
    DevBuf<float> Tf, Trf;
};
void hmsg_shard_ws_free(hmsg_shard_ws* w) { delete w; }

namespace {

// one shard held by this process
struct Shard {
    hmsg_index* ix = nullptr;
    const double* names = nullptr;          // [R][D] f64, host or device, or NULL
    int nfr = 0;                            // floor_room_off[n_floors]
    hmsg_shard_ws* ws = nullptr;
};
// the per-shard header of the first exchange (HMSG_COMM_HDR_BYTES at most): what the offsets, the slot sizes and the agreement need --
// the shard's counts and preconditions, and the query arguments every rank must pass alike (a hash of the floor ids and room modes)
enum { M_N, M_R, M_F, M_NFR, M_NV, M_D, M_NAMES, M_OK, M_Q, M_C, M_K, M_RM, M_NEG, M_LABEL, M_VIEW, M_HASH, M_WORDS };
static_assert(M_WORDS * 8 <= 128, "the header exchange carries 128 bytes per rank");

struct Query {
    int Q, C;
    const float *T_obj, *T_room;
    const int *qid, *floor_id, *room_mode;
    int k, use_neg, max_rooms;
    int *out_sel, *out_nsel, *out_idx, *out_room;
    double* out_score;
    int64_t *node_off, *room_off, *floor_off;
};

long long words_hash(const int* a, int n, unsigned long long h) {     // FNV-1a over the words
    for (int i = 0; i < n; ++i) {
        h ^= (unsigned)a[i];
        h *= 1099511628211ull;
    }
    return (long long)(h >> 1);
}

// The sharded query over W shards of which `local` are held here, in slots first .. first + local.size() - 1 (the communicator's
// path: one shard, slot = rank; hmsg_graphs_query: every shard, no communicator, the slots are filled in place).  `pre` holds the
// error of a shard that could not take part (its precondition failed), folded into the first exchange.  Q = 0: the header exchange
// only (the offsets).
void run_sharded(std::vector<Shard>& local, const std::vector<std::string>& pre, int W, int first, hmsg_comm* c, hipStream_t st, const Query& a) {
    const int Q = a.Q, C = a.C, k = a.k, RM = a.max_rooms;
    const QueryScan sc = hmsg_query_scan(Q, a.room_mode, a.floor_id);
    const bool need_label = sc.need_label, need_view = sc.need_view;
    // 1. the header exchange = the agreement on every shard's preconditions and on the query arguments (before any payload collective;
    //    through a buffer made with the communicator: agreeing needs no allocation)
    std::vector<long long> meta((size_t)W * M_WORDS, 0);
    std::vector<std::string> why(local.size());
    for (size_t i = 0; i < local.size(); ++i) {
        long long* m = &meta[(size_t)(first + i) * M_WORDS];
        why[i] = pre[i];
        // (the floors of all shards are not known before the exchange: the floor ids are checked against them after it)
        if (why[i].empty()) why[i] = hmsg_query_precondition("hmsg_graph_query_sharded", sc, -1, a.T_room != nullptr, local[i].names != nullptr);
        m[M_OK] = why[i].empty() ? 1 : 0;
        m[M_Q] = Q;
        m[M_C] = C;
        m[M_K] = k;
        m[M_RM] = RM;
        m[M_NEG] = a.use_neg != 0;
        m[M_LABEL] = need_label;
        m[M_VIEW] = need_view;
        m[M_HASH] = words_hash(a.room_mode, Q, words_hash(a.floor_id, Q, 1469598103934665603ull));
        if (!why[i].empty()) continue;
        hmsg_index* ix = local[i].ix;
        m[M_N] = ix->N;
        m[M_R] = ix->h_rooms;
        m[M_F] = ix->n_floors;
        m[M_NFR] = local[i].nfr;
        m[M_NV] = ix->n_views;
        m[M_D] = ix->D;
        m[M_NAMES] = local[i].names ? 1 : 0;
    }
    if (c) {
        std::vector<long long> all((size_t)W * M_WORDS);
        hmsg_comm_allgather_header(c, &meta[(size_t)first * M_WORDS], M_WORDS * 8, all.data(), st);
        meta.swap(all);
    }
    for (size_t i = 0; i < local.size(); ++i)
        if (!why[i].empty()) throw hmsg_error{HMSG_ERR_INVALID, why[i]};
    for (int s = 0; s < W; ++s)
        HMSG_REQUIRE(meta[(size_t)s * M_WORDS + M_OK], HMSG_ERR_INVALID, "hmsg_graph_query_sharded: shard " + std::to_string(s) + " cannot take part (see its last error)");
    for (int s = 1; s < W; ++s)
        for (int w = M_Q; w < M_WORDS; ++w)
            HMSG_REQUIRE(meta[(size_t)s * M_WORDS + w] == meta[(size_t)w], HMSG_ERR_INVALID,
                         "hmsg_graph_query_sharded: the ranks' queries differ (Q, C, k, max_rooms, use_negatives, floor ids or room modes)");
    // (from here on every rank holds the same headers: what is decided on them is decided alike everywhere)
    const int D = (int)meta[M_D];
    std::vector<int> noff((size_t)W + 1, 0), roff((size_t)W + 1, 0), foff((size_t)W + 1, 0);
    ShRoomLayout lay{};
    lay.Rmax = lay.Fmax = lay.NFRmax = 1;
    for (int s = 0; s < W; ++s) {
        const long long* m = &meta[(size_t)s * M_WORDS];
        HMSG_REQUIRE(m[M_D] == D, HMSG_ERR_INVALID, "hmsg_graph_query_sharded: the shards' embeddings differ in length");
        HMSG_REQUIRE(noff[(size_t)s] + m[M_N] < INT_MAX && roff[(size_t)s] + m[M_R] < INT_MAX, HMSG_ERR_INVALID, "hmsg_graph_query_sharded: too many nodes");
        noff[(size_t)s + 1] = noff[(size_t)s] + (int)m[M_N];
        roff[(size_t)s + 1] = roff[(size_t)s] + (int)m[M_R];
        foff[(size_t)s + 1] = foff[(size_t)s] + (int)m[M_F];
        lay.Rmax = std::max(lay.Rmax, (int)m[M_R]);
        lay.Fmax = std::max(lay.Fmax, (int)m[M_F]);
        lay.NFRmax = std::max(lay.NFRmax, (int)m[M_NFR]);
    }
    for (int s = 0; s <= W; ++s) {
        if (a.node_off) a.node_off[s] = noff[(size_t)s];
        if (a.room_off) a.room_off[s] = roff[(size_t)s];
        if (a.floor_off) a.floor_off[s] = foff[(size_t)s];
    }
    if (Q == 0) return;
    const std::string why_floor = hmsg_query_precondition("hmsg_graph_query_sharded", sc, foff[(size_t)W], true, true);
    HMSG_REQUIRE(why_floor.empty(), HMSG_ERR_INVALID, why_floor);
    // slot layouts of the two payload exchanges
    const long long rows = (long long)Q * lay.Rmax * 8;
    lay.o_lab = 0;
    lay.o_view = lay.o_lab + (need_label ? al16(rows) : 0);
    lay.o_fro = lay.o_view + (need_view ? al16(rows) : 0);
    lay.o_fr = lay.o_fro + al16((long long)(lay.Fmax + 1) * 4);
    lay.o_key = lay.o_fr + al16((long long)lay.NFRmax * 4);
    lay.o_vcnt = lay.o_key + al16((long long)lay.Rmax * 4);
    lay.bytes = lay.o_vcnt + al16((long long)lay.Rmax * 4);
    const long long c_cnt = al16((long long)Q * 2 * k * (long long)sizeof(ShRec)), c_bytes = c_cnt + al16((long long)Q * 4);
    const QueryOut out(Q, k, RM);
    hmsg_shard_ws& G = *local[0].ws;              // the exchange's buffers
    int *d_floor = nullptr, *d_mode = nullptr, *d_qid = nullptr, *d_roff = nullptr, *d_foff = nullptr;
    // 2. the local room and object stages of every shard held here
    hmsg_comm_local_phase_then_agree(c, st, "hmsg_graph_query_sharded", [&] {
        // per-query words and offsets: one upload (floor | mode | qid | roff | foff)
        std::vector<int> qin((size_t)Q * 3 + 2 * ((size_t)W + 1));
        const bool qid_dev = hmsg_query_pack_words(qin.data(), Q, a.floor_id, a.room_mode, a.qid);
        memcpy(qin.data() + 3 * (size_t)Q, roff.data(), ((size_t)W + 1) * 4);
        memcpy(qin.data() + 3 * (size_t)Q + W + 1, foff.data(), ((size_t)W + 1) * 4);
        G.qin.ensure(qin.size());
        HIP_TRY(hipMemcpyAsync(G.qin.p, qin.data(), qin.size() * 4, hipMemcpyHostToDevice, st));
        d_floor = G.qin.p;
        d_mode = G.qin.p + Q;
        d_qid = G.qin.p + 2 * (size_t)Q;
        d_roff = G.qin.p + 3 * (size_t)Q;
        d_foff = d_roff + W + 1;
        if (qid_dev) HIP_TRY(hipMemcpyAsync(d_qid, a.qid, (size_t)Q * 4, hipMemcpyDeviceToDevice, st));
        G.out.ensure(out.bytes);
        G.room.ensure((size_t)W * (size_t)lay.bytes);
        G.cand.ensure((size_t)W * (size_t)c_bytes);
        G.qrooms.ensure((size_t)Q * RM);
        hmsg_text_rows_to_f64(st, a.T_obj, (size_t)Q * C * D, G.Tf, G.T64);
        if (need_label || need_view) hmsg_text_rows_to_f64(st, a.T_room, (size_t)Q * D, G.Trf, G.Tr64);
        for (size_t i = 0; i < local.size(); ++i) {
            Shard& sh = local[i];
            hmsg_shard_ws& L = *sh.ws;
            hmsg_index* ix = sh.ix;
            const int R = ix->h_rooms, F = ix->n_floors;
            char* slot = G.room.p + (size_t)(first + i) * (size_t)lay.bytes;
            if (need_label && R) {
                const double* names = stage_in(L.names, sh.names, (size_t)R * D, st, Up::bounce, true);
                L.S_room.ensure((size_t)Q * R);
                hmsg_gemm_f64(G.Tr64.p, Q, names, R, D, L.S_room.p, st);
                hipLaunchKernelGGL(k_sh_pad_rows, dim3(cdiv((size_t)Q * R, 256)), dim3(256), 0, st, (const double*)L.S_room.p, Q, R, lay.Rmax,
                                   (double*)(slot + lay.o_lab));
                HMSG_CHECK_LAUNCH();
            }
            if (need_view && R) {
                L.S_view.ensure((size_t)Q * std::max<long long>(ix->n_views, 1));
                hmsg_gemm_f64(G.Tr64.p, Q, ix->view_emb.p, ix->n_views, D, L.S_view.p, st);
                hipLaunchKernelGGL(k_sh_view_max, dim3(cdiv((size_t)Q * R, 256)), dim3(256), 0, st, (const double*)L.S_view.p, ix->n_views,
                                   (const int*)ix->view_off.p, Q, R, lay.Rmax, (double*)(slot + lay.o_view));
                HMSG_CHECK_LAUNCH();
            }
            const int nt = std::max(std::max(R, F + 1), sh.nfr);
            hipLaunchKernelGGL(k_sh_tables, dim3(cdiv((size_t)nt, 256)), dim3(256), 0, st, (const int*)ix->floor_room_off.p, F,
                               (const int*)ix->floor_rooms.p, sh.nfr, (const int*)ix->room_key.p, (const int*)ix->view_off.p, R,
                               (int*)(slot + lay.o_fro), (int*)(slot + lay.o_fr), (int*)(slot + lay.o_key), (int*)(slot + lay.o_vcnt));
            HMSG_CHECK_LAUNCH();
            if (ix->N) {                           // (the object GEMM does not wait for the room exchange)
                L.S.ensure((size_t)Q * C * ix->N);
                hmsg_gemm_f64(G.T64.p, Q * C, ix->E.p, ix->N, D, L.S.p, st);
            }
        }
    });
    // 3. room rows + tables of every shard to every shard
    if (c) hmsg_comm_allgather_inplace(c, G.room.p, (size_t)lay.bytes, st);
    // 4. the global room selection, the same on every rank; every shard's candidates in the rooms it owns
    hmsg_comm_local_phase_then_agree(c, st, "hmsg_graph_query_sharded", [&] {
        hipLaunchKernelGGL(k_sh_room_select, dim3(Q), dim3(256), 0, st, (const char*)G.room.p, lay.bytes, lay, W, (const int*)d_roff,
                           (const int*)d_foff, (const int*)d_floor, (const int*)d_mode, RM, out.sel(G.out.p), out.nsel(G.out.p), G.qrooms.p, out.err(G.out.p));
        HMSG_CHECK_LAUNCH();
        for (size_t i = 0; i < local.size(); ++i) {
            hmsg_index* ix = local[i].ix;
            const int s = first + (int)i;
            char* slot = G.cand.p + (size_t)s * (size_t)c_bytes;
            hipLaunchKernelGGL(k_sh_candidates, dim3(Q), dim3(256), 0, st, (const double*)local[i].ws->S.p, ix->N, C, (const int*)d_qid,
                               (const int*)G.qrooms.p, RM, (const int*)ix->room_off.p, (const int*)ix->room_nodes.p, roff[(size_t)s], ix->n_rooms,
                               noff[(size_t)s], k, a.use_neg, (ShRec*)slot, (int*)(slot + c_cnt));
            HMSG_CHECK_LAUNCH();
        }
    });
    // 5. the candidates to every shard; the merge (no collective follows: what fails from here on fails on its own rank only)
    if (c) hmsg_comm_allgather_inplace(c, G.cand.p, (size_t)c_bytes, st);
    hipLaunchKernelGGL(k_sh_merge, dim3(Q), dim3(64), 0, st, (const char*)G.cand.p, c_bytes, c_cnt, W, Q, k, a.use_neg, out.idx(G.out.p),
                       out.room(G.out.p), out.score(G.out.p));
    HMSG_CHECK_LAUNCH();
    std::vector<char> h_out(out.bytes);
    HIP_TRY(hipMemcpyAsync(h_out.data(), G.out.p, out.bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    out.give("hmsg_graph_query_sharded", st, G.out.p, h_out.data(), a.out_score, a.out_sel, a.out_nsel, a.out_idx, a.out_room);
}

// a graph as a shard: its resident index and scratch (what fails here is folded into the agreement, not thrown)
void shard_of_graph(hmsg_graph* g, const double* names, Shard& sh, std::string& why) {
    try {
        hmsg_shard_ws*& w = hmsg_graph_shard_ws(g);
        if (!w) w = new hmsg_shard_ws();
        sh.ws = w;
        sh.ix = hmsg_graph_shard_index(g, &sh.nfr);
        sh.names = names;
    } catch (...) {
        why = hmsg_current_error().msg;
    }
    if (why.empty() && !sh.ix) why = "hmsg_graph_query_sharded: no index";
}
// (Q = 0: no query array is read -- the call is the header exchange, the offsets)
bool query_args_ok(const Query& a) {
    if (a.Q < 0 || a.C < 1 || a.k < 1 || a.max_rooms < 1) return false;
    return a.Q == 0 || (a.T_obj && a.qid && a.floor_id && a.room_mode && a.out_sel && a.out_nsel && a.out_idx && a.out_room && a.out_score);
}

}  // namespace

extern "C" {

int hmsg_graph_query_sharded(hmsg_graph_t* g, hmsg_comm_t* c, const double* room_name_emb, int32_t Q, int32_t C, const float* T_obj,
                             const int32_t* qid, const float* T_room, const int32_t* floor_id, const int32_t* room_mode, int32_t k,
                             int32_t use_negatives, int32_t max_rooms, int32_t* out_sel, int32_t* out_nsel, int32_t* out_idx, int32_t* out_room,
                             double* out_score, int64_t* node_off, int64_t* room_off, int64_t* floor_off) {
    if (!g || !c) return HMSG_ERR_INVALID;
    const Query a{Q, C, T_obj, T_room, qid, floor_id, room_mode, k, use_negatives, max_rooms, out_sel, out_nsel, out_idx, out_room, out_score,
                  node_off, room_off, floor_off};
    std::string err;
    const int rc = hmsg_boundary(&err, hmsg_comm_device(c), [&] {
        std::vector<Shard> local(1);
        std::vector<std::string> pre(1);
        // (bad arguments, like every other local failure, travel in the header: the other ranks fail with this one)
        if (!query_args_ok(a)) pre[0] = "hmsg_graph_query_sharded: bad argument";
        else if (hmsg_graph_device(g) != hmsg_comm_device(c)) pre[0] = "hmsg_graph_query_sharded: the graph and the communicator are on different devices";
        else shard_of_graph(g, room_name_emb, local[0], pre[0]);
        // (a rank without an index still takes part in the header exchange: on a stream of its own)
        hipStream_t st = local[0].ix ? local[0].ix->stream : nullptr;
        std::optional<ScopedStream> own;
        if (!st) st = own.emplace(hipStreamNonBlocking);
        Query b = a;
        if (!pre[0].empty()) b.Q = 0;                   // (no query array of a bad call is read)
        run_sharded(local, pre, hmsg_comm_world(c), hmsg_comm_rank(c), c, st, b);
    });
    if (rc != HMSG_OK) {
        hmsg_graph_set_error(g, err);
        hmsg_comm_set_error(c, err);
    }
    return rc;
}

int hmsg_graphs_query(int32_t n, hmsg_graph_t* const* graphs, const double* const* room_name_embs, int32_t Q, int32_t C, const float* T_obj,
                      const int32_t* qid, const float* T_room, const int32_t* floor_id, const int32_t* room_mode, int32_t k, int32_t use_negatives,
                      int32_t max_rooms, int32_t* out_sel, int32_t* out_nsel, int32_t* out_idx, int32_t* out_room, double* out_score,
                      int64_t* node_off, int64_t* room_off, int64_t* floor_off) {
    if (n < 1 || !graphs) return HMSG_ERR_INVALID;
    for (int i = 0; i < n; ++i)
        if (!graphs[i]) return HMSG_ERR_INVALID;
    const Query a{Q, C, T_obj, T_room, qid, floor_id, room_mode, k, use_negatives, max_rooms, out_sel, out_nsel, out_idx, out_room, out_score,
                  node_off, room_off, floor_off};
    if (!query_args_ok(a)) return HMSG_ERR_INVALID;
    std::string err;
    const int dev = hmsg_graph_device(graphs[0]);
    const int rc = hmsg_boundary(&err, dev, [&] {
        std::vector<Shard> local((size_t)n);
        std::vector<std::string> pre((size_t)n);
        for (int i = 0; i < n; ++i) {
            std::string why;
            if (hmsg_graph_device(graphs[i]) != dev) why = "hmsg_graphs_query: the graphs are on different devices";
            else shard_of_graph(graphs[i], room_name_embs ? room_name_embs[i] : nullptr, local[(size_t)i], why);
            if (!why.empty()) throw hmsg_error{HMSG_ERR_INVALID, "hmsg_graphs_query: graph " + std::to_string(i) + ": " + why};
        }
        run_sharded(local, pre, n, 0, nullptr, local[0].ix->stream, a);
    });
    if (rc != HMSG_OK) hmsg_graph_set_error(graphs[0], err);
    return rc;
}

}  // extern "C"
