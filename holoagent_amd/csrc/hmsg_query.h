// The resident retrieval index (hmsg_query.hip) as the other translation units that work on it see it: the sharded query
// (hmsg_query_sharded.hip) runs its stages on every shard's own index.  Device code is not linked across translation units,
// so what is shared here is host-side: the struct and the float64 GEMM dispatch.
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
    DevBuf<int> d_floor, d_mode, d_sel, d_nsel, d_err;
    // hmsg_query_hier: the per-query words in (floor | mode | qid) and every result out (score | sel | nsel | err | idx | room) travel as
    // ONE packed copy each way through pinned memory (round 5: three pageable uploads and six pageable read-backs per call)
    PinnedBuf<int> h_qin;
    DevBuf<int> d_qin;
    PinnedBuf<char> h_qout;
    DevBuf<char> d_qout;
    Prof prof;                   // live timing of the GEMM (hmsg_index_set_profiling)
};

// S[M][N] = A[M][D] . B[N][D]^T in float64 on stream s, with the kernel choice of the index's own GEMM: the 128x128-tiled
// kernel when M >= 64 and N >= 64, the one-wave-per-16x16-tile kernel otherwise.  Both chain the same v_mfma_f64_16x16x4_f64
// k-steps (k = 0, 4, 8, ... from a zero accumulator; the tiled kernel adds zero products past D up to its 16-wide step), so an
// entry S[m][n] has the same bits whichever kernel computed it and wherever its rows sit in A and B.
void hmsg_gemm_f64(const double* A, int M, const double* B, long long N, int D, double* S, hipStream_t s);
// an index without a node table, for hmsg_index_set_hierarchy only: a shard whose rooms hold no object (hmsg_query_sharded.hip)
hmsg_index* hmsg_index_create_rooms_only(int device, int D);
