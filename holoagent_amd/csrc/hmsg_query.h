// The resident retrieval index (hmsg_query.hip) as the other translation units that work on it see it: the sharded query
// (hmsg_query_sharded.hip) runs its stages on every shard's own index.  Shared here is the host side of a query: the struct, the
// float64 GEMM dispatch, and what hmsg_query_hier and the sharded query do alike around their kernels (argument scan, text rows,
// packed words in, packed results out).  The device-side rules both instantiate are in hmsg_query_rules.h.
#pragma once
#include "hmsg_common.h"

typedef double f64x4 __attribute__((ext_vector_type(4)));

struct hmsg_index {
    int device = 0;
    int D = 0;
    long long N = 0;
    int n_rooms = 0;
    hipStream_t stream = nullptr;
    std::string err;
    DevBuf<double> E;            // [N][D]
    DevBuf<int> room_of;         // [N]
    DevBuf<int> room_off;        // [n_rooms + 1]   CSR room -> nodes (ascending node index)
    DevBuf<int> room_nodes;      // [N]
    std::vector<int> h_room_cnt;
    DevBuf<double> T64, S;       // scratch: text rows in f64, similarity matrix
    DevBuf<float> Tf;
    DevBuf<int> d_qid, d_roff, d_rooms, d_oidx, d_oroom;
    DevBuf<double> d_oscore;
    // the hierarchy above the nodes (hmsg_index_set_hierarchy): floors -> rooms, room name / view embeddings
    bool have_hier = false;
    int n_floors = 0, h_rooms = 0;
    long long n_views = 0;
    DevBuf<double> room_name_emb;   // [n_rooms][D]  CLIP text embedding of the room's name (label mode)
    DevBuf<double> view_emb;        // [n_views][D]  room.embeddings (view mode)
    DevBuf<int> view_off;           // [n_rooms + 1]
    DevBuf<int> room_key;           // [n_rooms]     int(room_id.split("_")[-1]): what the view mode returns
    DevBuf<int> floor_room_off;     // [n_floors + 1]
    DevBuf<int> floor_rooms;        // rooms of floor f in floors[f].rooms order (global room ids)
    DevBuf<double> S_room, S_view;  // scratch
    DevBuf<float> Tr;
    DevBuf<double> Tr64;
    // hmsg_query_hier: the per-query words in (floor | mode | qid) and every result out (score | sel | nsel | err | idx | room) travel as
    // ONE packed copy each way through pinned memory (round 5: three pageable uploads and six pageable read-backs per call)
    PinnedBuf<int> h_qin;
    DevBuf<int> d_qin;
    PinnedBuf<char> h_qout;
    DevBuf<char> d_qout;
    // the view level below the rooms (hmsg_index_set_views, hmsg_query_views.hip): CSR view -> nodes in view.object_ids order
    long long n_obj_views = -1;     // -1: not set
    std::vector<long long> h_vo_off;
    DevBuf<long long> vo_off;       // [n_obj_views + 1]
    DevBuf<int> vo_nodes;
    DevBuf<int> d_view, d_vnode;    // scratch of hmsg_rematch_in_views
    DevBuf<double> d_vscore;
    Prof prof;                   // live timing of the GEMM (hmsg_index_set_profiling)
};

// S[M][N] = A[M][D] . B[N][D]^T in float64 on stream s, with the kernel choice of the index's own GEMM: the 128x128-tiled
// kernel when M >= 64 and N >= 64, the one-wave-per-16x16-tile kernel otherwise.  Both chain the same v_mfma_f64_16x16x4_f64
// k-steps (k = 0, 4, 8, ... from a zero accumulator; the tiled kernel adds zero products past D up to its 16-wide step), so an
// entry S[m][n] has the same bits whichever kernel computed it and wherever its rows sit in A and B.
// One wave's 16x16 tile of that product: the chain of v_mfma_f64_16x16x4_f64 steps k = 0, 4, 8, ... from a zero accumulator.  Lane l
// feeds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15] (ap / bp: the lane's row of A / B, a_ok / b_ok: whether that row
// exists -- a missing row feeds zeros); result register r of lane l is C[row = (l >> 4) + 4 r][col = l & 15].  Every kernel that
// must give hmsg_similarity's bits for an entry (the one-wave-per-tile GEMM, the re-match of hmsg_query_views.hip) goes through it.
__device__ __forceinline__ f64x4 gemm_f64_tile16(const double* __restrict__ ap, bool a_ok, const double* __restrict__ bp, bool b_ok, int D) {
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    const int kq = (threadIdx.x & 63) >> 4;
    for (int k0 = 0; k0 < D; k0 += 4) {
        const int k = k0 + kq;
        const double a = (k < D && a_ok) ? ap[k] : 0.0;
        const double b = (k < D && b_ok) ? bp[k] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    }
    return acc;
}
void hmsg_gemm_f64(const double* A, int M, const double* B, long long N, int D, double* S, hipStream_t s);
// an index without a node table, for hmsg_index_set_hierarchy only: a shard whose rooms hold no object (hmsg_query_sharded.hip)
hmsg_index* hmsg_index_create_rooms_only(int device, int D);

// ---- the host side of a coarse-to-fine query, shared by hmsg_query_hier and the sharded query ----
// `who` is the caller's message prefix ("hmsg_query_hier", "hmsg_graph_query_sharded").

// what the Q room modes / floor ids ask for
struct QueryScan {
    bool need_label = false, need_view = false;     // a query in label mode (1) / a view mode (2, 3)
    bool in_range = true;                           // every mode in 0..3, every floor id >= -1
    int max_floor = -1;
};
QueryScan hmsg_query_scan(int Q, const int* room_mode, const int* floor_id);
// the failed precondition of a query with this scan on tables with n_floors floors, or "" (n_floors < 0: not known yet)
std::string hmsg_query_precondition(const char* who, const QueryScan& sc, int n_floors, bool have_room_text, bool have_room_names);
// n float32 text rows values (host or device) -> dst as float64, through tmp when they come from the host
void hmsg_text_rows_to_f64(hipStream_t s, const float* src, size_t n, DevBuf<float>& tmp, DevBuf<double>& dst);
// the per-query words, packed for one upload: h_words [floor Q | mode Q | qid Q].  Returns whether qid is device memory: then its
// third is left out, and the caller copies qid there on the device once the words are up.
bool hmsg_query_pack_words(int* h_words, int Q, const int* floor_id, const int* room_mode, const int* qid);
// every result of a query as ONE packed buffer: [score f64 Q*k | sel Q*max_rooms | nsel Q | err Q | idx Q*k | room Q*k]
struct QueryOut {
    int Q, k, max_rooms;
    size_t o_sel, o_nsel, o_err, o_idx, o_room, bytes;
    QueryOut(int Q_, int k_, int max_rooms_)
        : Q(Q_), k(k_), max_rooms(max_rooms_), o_sel((size_t)Q_ * k_ * 8), o_nsel(o_sel + (size_t)Q_ * max_rooms_ * 4), o_err(o_nsel + (size_t)Q_ * 4),
          o_idx(o_err + (size_t)Q_ * 4), o_room(o_idx + (size_t)Q_ * k_ * 4), bytes(o_room + (size_t)Q_ * k_ * 4) {}
    double* score(char* base) const { return (double*)base; }
    int* sel(char* base) const { return (int*)(base + o_sel); }
    int* nsel(char* base) const { return (int*)(base + o_nsel); }
    int* err(char* base) const { return (int*)(base + o_err); }
    int* idx(char* base) const { return (int*)(base + o_idx); }
    int* room(char* base) const { return (int*)(base + o_room); }
    // The results into the caller's arrays (host memory, or device memory -- the reference's callers take numpy arrays) from the
    // device buffer d and its host copy h, then the room stage's verdict: throws when a query's err word is set.
    void give(const char* who, hipStream_t s, const char* d, const char* h, double* out_score, int* out_sel, int* out_nsel, int* out_idx,
              int* out_room) const;
};
