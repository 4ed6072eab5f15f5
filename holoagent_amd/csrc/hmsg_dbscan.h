// The batched cosine DBSCAN of feats_denoise_dbscan (utils/graph_utils.py:682-728) as the pooling runs it (hmsg_pool.hip), shared
// with the room naming (hmsg_roomnames.hip).  Rows of many sets are concatenated; every set has its own adjacency bit matrix
// (n x ceil(n / 32) u32 words, row-major) and its own range of Gram tiles.  The kernels live in hmsg_pool.hip; these are the
// launches the room naming reuses unchanged.
#pragma once
#include "hmsg_common.h"

#include <vector>

struct PoolSeg {            // one instance / set
    long long row_base;     // first row in the concatenated feature matrix
    long long bit_base;     // first u32 word of its adjacency bit matrix
    int n;                  // rows (valid points)
    int nw;                 // u32 words per row = ceil(n / 32)
    long long tile_base;    // first Gram tile id (upper triangle, super-tile order: gram_tile_of)
    int nt;                 // Gram tiles per side = ceil(n / GRAM_T)
    int pad;
};

#define GRAM_T 128

// k_pool_gram: float32 MFMA Gram of the L2-normalised rows Xn -> adjacency bits (d = 1 - s clipped to [0, 2], diagonal 0,
// neighbour iff d <= eps) + per-row neighbour counts.  `tiles` = sum over sets of nt (nt + 1) / 2.  adj / ncount zeroed.
void pool_launch_gram_f32(hipStream_t s, const float* Xn, int D, const PoolSeg* d_ps, int K, long long tiles, float eps, unsigned* adj,
                          unsigned* ncount);
// k_seg_rows: seg_of_row[row] = its set (maxn: rows of the largest set)
void pool_launch_seg_rows(hipStream_t s, const PoolSeg* d_ps, int K, int maxn, int* seg_of_row);
// core rows (ncount >= minpts), label propagation to the smallest core row of each component, border rows to the smallest adjacent
// cluster label (sklearn's dbscan_inner), cluster sizes / first rows and per set the largest cluster (ties: the first to appear in
// row order, Counter.most_common).  Caller state: seg_first memset 0x7f, csize and best zeroed, cfirst memset 0xff.
// best[k] = (size << 32) | (0xffffffff - first row), 0 when the set has no cluster.
void pool_cluster(hipStream_t s, const PoolSeg* d_ps, long long R, int minpts, const unsigned* adj, const unsigned* ncount,
                  const int* seg_of_row, int* label, int* seg_first, int* d_changed, int* flabel, unsigned* csize, unsigned* cfirst,
                  unsigned long long* best, DbgLaps* laps = nullptr);
// k_pool_mean: per set the float32 mean of the largest cluster's rows in row order (all rows without a cluster)
void pool_launch_mean_f32(hipStream_t s, const float* X, int D, const PoolSeg* d_ps, int K, const int* flabel, const unsigned* csize,
                          const unsigned* cfirst, const unsigned long long* best, float* out);

// ---- hmsg_roomnames.hip (the room naming of room.py:131-172, 237-308 on the device; include/hmsg.h hmsg_denoise_feats_batch)
// feats_denoise_dbscan over the sets off[k] .. off[k + 1] of the device rows X ([off.back()][D], float32 or float64); every set has at
// least one row.  out: device [K][D] in the input dtype; n_in_cluster (host, optional): rows of the chosen cluster, 0 = none.
void rn_denoise(hipStream_t s, const void* X, bool f64, int D, const std::vector<long long>& off, double eps, int min_samples, void* out,
                int* n_in_cluster);
// first arg-max over types of rows[k] . T[t] (float64 products of the exact inputs); rows device [K][D], T device f32 [n_types][D]
void rn_choose(hipStream_t s, const void* rows, bool f64, long long K, int D, const float* T, int n_types, int* d_type);
// majority vote of the views' arg-max types per room (np.unique order: ties to the smallest type id); -1 for a room without views
void rn_vote(hipStream_t s, const int* d_view_type, const std::vector<long long>& voff, int n_types, int* type_of_room /*host*/);
// device gather of float32 rows: dst[i] = src[rows[i]]
void rn_gather_rows_f32(hipStream_t s, const float* src, const std::vector<int>& rows, int D, float* dst);
