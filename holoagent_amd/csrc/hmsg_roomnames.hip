// Room names on the device: Graph.generate_room_names (fsr_vln/memory/hmsg/graph/graph.py:2146-2187) with
//   "obj_embedding"  Room.infer_room_type_from_objects (room.py:237-308): feats_denoise_dbscan (utils/graph_utils.py:682-728; eps 0.02,
//                    min_samples 2, cosine, sklearn 1.7.2) over the embeddings of the room's objects, then
//                    argmax(represent . type_feats^T) (first maximum);
//   "view_embedding" Room.infer_room_type_from_view_embedding (room.py:131-172): per view the arg-max over the types, then the
//                    majority vote (np.unique order: ties to the smallest type id).
//
// MI355X design.  All rooms go through ONE batched DBSCAN, the same one the pooling runs (hmsg_pool.hip, hmsg_dbscan.h):
//   rows L2-normalised as sklearn.preprocessing.normalize does it (a zero row stays zero) -> Gram on the matrix cores, thresholded in
//   registers to one adjacency BIT per pair plus per-row neighbour counts -> label propagation over the bits (cores: the smallest core
//   row of the component; borders: the smallest adjacent cluster, dbscan_inner) -> the largest cluster (Counter.most_common: the first
//   to appear in row order on a tie) -> the mean over its rows, added in row order and divided once (np.mean(axis=0) of a C-contiguous
//   array).  float32 input uses the pooling's float32 Gram (v_mfma_f32_32x32x2_f32) and mean unchanged.  float64 input -- a LOADED graph
//   holds json.load's float64 embeddings (object.py:71,88) -- has its own Gram on v_mfma_f64_16x16x4_f64 and a float64 mean.
//   Scores against the type table are float64 sums of the exact products (a wave per row), whatever the input dtype.
#include "hmsg_boundary.h"
#include "hmsg_dbscan.h"

#include <algorithm>
#include <cmath>

typedef double rn_f64x4 __attribute__((ext_vector_type(4)));

namespace {

__device__ __forceinline__ double rn_wave_sum_f64(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---- row L2 normalisation (sklearn normalize: norms of 0 are replaced by 1), one wave per row
template <typename T>
__global__ void k_rn_normalize(const T* __restrict__ X, long long N, int D, T* __restrict__ Xn) {
    const int lane = threadIdx.x & 63;
    const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (i >= N) return;
    const T* x = X + (size_t)i * D;
    T n2 = 0;
    for (int e = lane; e < D; e += 64) n2 += x[e] * x[e];
    T nrm;
    if (sizeof(T) == 8) {
        nrm = (T)__dsqrt_rn((double)rn_wave_sum_f64((double)n2));
    } else {
        nrm = (T)__fsqrt_rn(wave_sum_f32((float)n2));
    }
    if (nrm == (T)0) nrm = (T)1;
    for (int e = lane; e < D; e += 64) Xn[(size_t)i * D + e] = x[e] / nrm;
}

// ---- float64 Gram -> adjacency bits + neighbour counts (the bit layout of k_pool_gram: per set n rows of nw u32 words)
// A 256-thread workgroup owns a 64x64 tile of one set's X^ X^T, each wave a 32x32 quadrant = 2x2 accumulators of 16x16
// (v_mfma_f64_16x16x4_f64: lane l feeds A[i = l&15][k = l>>4], B[k = l>>4][j = l&15]; result reg r of lane l is
// C[row = (l>>4) + 4r][col = l&15], as in hmsg_query.hip).  Fragments come straight from global memory (L2-resident: a set is at most a
// few MB); rows past the set's end are clamped to its last row and masked in the epilogue.  The full square is computed (no mirrored
// writes): a pair's two products are the same numbers in the same k order, so the relation stays symmetric.  One 32-bit word of the
// bit matrix = one row of the quadrant: the two column halves are the j = 0 / j = 1 ballots.
__global__ void __launch_bounds__(256) k_rn_gram_f64(const double* __restrict__ Xn, int D, const PoolSeg* __restrict__ segs,
                                                     const long long* __restrict__ tile_base, int K, double eps,
                                                     unsigned* __restrict__ adj, unsigned* __restrict__ ncount) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, wr = wv >> 1, wc = wv & 1;
    const long long tile = blockIdx.x;
    int lo = 0, hi = K - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tile_base[mid] <= tile) lo = mid; else hi = mid - 1;
    }
    const PoolSeg sg = segs[lo];
    const int nt = (sg.n + 63) / 64;
    const long long t = tile - tile_base[lo];
    const int r0 = (int)(t / nt) * 64 + wr * 32, c0 = (int)(t % nt) * 64 + wc * 32;
    if (r0 >= sg.n || c0 >= sg.n) return;                     // wave-uniform; no LDS, no barrier
    const double* base = Xn + (size_t)sg.row_base * D;
    const int li = lane & 15, kq = lane >> 4;
    const double* pa0 = base + (size_t)min(r0 + li, sg.n - 1) * D;
    const double* pa1 = base + (size_t)min(r0 + 16 + li, sg.n - 1) * D;
    const double* pb0 = base + (size_t)min(c0 + li, sg.n - 1) * D;
    const double* pb1 = base + (size_t)min(c0 + 16 + li, sg.n - 1) * D;
    rn_f64x4 acc[2][2];
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) acc[i][j] = rn_f64x4{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < D; k0 += 4) {
        const int k = k0 + kq;
        const bool in = k < D;
        const double a0 = in ? pa0[k] : 0.0, a1 = in ? pa1[k] : 0.0, b0 = in ? pb0[k] : 0.0, b1 = in ? pb1[k] : 0.0;
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
    // epilogue: d = 1 - s, clipped to [0, 2], diagonal 0; neighbour iff d <= eps
    for (int i = 0; i < 2; ++i)
        for (int r = 0; r < 4; ++r) {
            const int row = r0 + i * 16 + kq + 4 * r;
            unsigned long long m[2];
            for (int j = 0; j < 2; ++j) {
                const int col = c0 + j * 16 + li;
                double d = __dadd_rn(-acc[i][j][r], 1.0);
                d = fmin(fmax(d, 0.0), 2.0);
                if (row == col) d = 0.0;
                m[j] = __ballot(row < sg.n && col < sg.n && d <= eps);
            }
            if (lane == 0)
                for (int q = 0; q < 4; ++q) {
                    const int rq = r0 + i * 16 + q + 4 * r;
                    const unsigned word = (unsigned)((m[0] >> (16 * q)) & 0xffffull) | ((unsigned)((m[1] >> (16 * q)) & 0xffffull) << 16);
                    if (rq < sg.n && word) {
                        adj[sg.bit_base + (size_t)rq * sg.nw + (c0 >> 5)] = word;
                        atomicAdd(&ncount[sg.row_base + rq], (unsigned)__popc(word));
                    }
                }
        }
}

// ---- float64 mean over the chosen rows in row order, then / n (np.mean(axis=0): sequential adds, one true division)
__global__ void k_rn_mean_f64(const double* __restrict__ X, int D, const PoolSeg* __restrict__ segs, const int* __restrict__ final_label,
                              const unsigned long long* __restrict__ best, double* __restrict__ out) {
    const int k = blockIdx.y;
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= D) return;
    const PoolSeg sg = segs[k];
    int want = -2;                                            // -2: every row (no cluster)
    const unsigned long long key = best[k];
    if (key) want = final_label[sg.row_base + (0xffffffffu - (unsigned)(key & 0xffffffffull))];
    double acc = 0.0;
    unsigned cnt = 0;
    const double* xb = X + (size_t)sg.row_base * D + d;
    const int* lb = final_label + sg.row_base;
    for (int r = 0; r < sg.n; ++r)
        if (want == -2 || lb[r] == want) {
            acc = __dadd_rn(acc, xb[(size_t)r * D]);
            ++cnt;
        }
    out[(size_t)k * D + d] = cnt > 1 ? __ddiv_rn(acc, (double)cnt) : acc;
}

// ---- first arg-max over the type table of every row, float64 sums of the exact products; one wave per row
template <typename T>
__global__ void k_rn_choose(const T* __restrict__ rows, long long K, int D, const float* __restrict__ Tt, int n_types, int* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long k = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (k >= K) return;
    const T* x = rows + (size_t)k * D;
    double best = 0.0;
    int bi = 0;
    for (int t = 0; t < n_types; ++t) {
        double s = 0.0;
        for (int e = lane; e < D; e += 64) s = fma((double)x[e], (double)Tt[(size_t)t * D + e], s);
        s = rn_wave_sum_f64(s);
        if (t == 0 || s > best) {
            best = s;
            bi = t;
        }
    }
    if (lane == 0) out[k] = bi;
}

// ---- per room: the most frequent view type, the smallest id on a tie; -1 without views
__global__ void k_rn_vote(const int* __restrict__ vt, const long long* __restrict__ voff, int R, int n_types, int* __restrict__ out) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const long long a = voff[r], b = voff[r + 1];
    int best = -1, bc = 0;
    for (int t = 0; t < n_types; ++t) {
        int c = 0;
        for (long long v = a; v < b; ++v) c += vt[v] == t;
        if (c > bc) {
            bc = c;
            best = t;
        }
    }
    out[r] = best;
}

__global__ void k_rn_gather_f32(const float* __restrict__ src, const int* __restrict__ row, int n, int D, float* __restrict__ dst) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)n * D) return;
    dst[t] = src[(size_t)row[t / D] * D + t % D];
}

}  // namespace

void rn_denoise(hipStream_t s, const void* X, bool f64, int D, const std::vector<long long>& off, double eps, int min_samples, void* out,
                int* n_in_cluster) {
    const int K = (int)off.size() - 1;
    if (K <= 0) return;
    const long long N = off.back();
    std::vector<PoolSeg> ps((size_t)K);
    std::vector<long long> tb64((size_t)K);
    long long bitw = 0, tiles32 = 0, tiles64 = 0;
    int maxn = 0;
    for (int k = 0; k < K; ++k) {
        PoolSeg& g = ps[(size_t)k];
        g.row_base = off[(size_t)k];
        g.n = (int)(off[(size_t)k + 1] - off[(size_t)k]);
        HMSG_REQUIRE(g.n >= 1, HMSG_ERR_INVALID, "feats_denoise_dbscan of an empty set");
        g.nw = (g.n + 31) / 32;
        g.nt = (g.n + GRAM_T - 1) / GRAM_T;
        g.bit_base = bitw;
        g.tile_base = tiles32;
        g.pad = 0;
        tb64[(size_t)k] = tiles64;
        bitw += (long long)g.n * g.nw;
        tiles32 += (long long)g.nt * (g.nt + 1) / 2;
        const long long t64 = (g.n + 63) / 64;
        tiles64 += t64 * t64;
        maxn = std::max(maxn, g.n);
    }
    DevBuf<PoolSeg> d_ps;
    DevBuf<long long> d_tb;
    d_ps.alloc((size_t)K);
    d_tb.alloc((size_t)K);
    HIP_TRY(hipMemcpyAsync(d_ps.p, ps.data(), (size_t)K * sizeof(PoolSeg), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_tb.p, tb64.data(), (size_t)K * 8, hipMemcpyHostToDevice, s));
    const size_t esz = f64 ? 8 : 4;
    DevBuf<char> Xn;
    DevBuf<unsigned> adj, ncount, csize, cfirst;
    DevBuf<int> label, flabel, seg_of_row, d_changed, seg_first;
    DevBuf<unsigned long long> best;
    Xn.alloc((size_t)N * D * esz);
    adj.alloc((size_t)std::max<long long>(bitw, 1));
    ncount.alloc((size_t)N);
    csize.alloc((size_t)N);
    cfirst.alloc((size_t)N);
    label.alloc((size_t)N);
    flabel.alloc((size_t)N);
    seg_of_row.alloc((size_t)N);
    d_changed.alloc(1);
    seg_first.alloc((size_t)K);
    best.alloc((size_t)K);
    HIP_TRY(hipMemsetAsync(seg_first.p, 0x7f, (size_t)K * 4, s));
    adj.zero(s);
    ncount.zero(s);
    csize.zero(s);
    HIP_TRY(hipMemsetAsync(cfirst.p, 0xff, (size_t)N * 4, s));
    best.zero(s);
    const unsigned nb = cdiv((size_t)N * 64, 256);
    if (f64)
        hipLaunchKernelGGL(k_rn_normalize<double>, dim3(nb), dim3(256), 0, s, (const double*)X, N, D, (double*)Xn.p);
    else
        hipLaunchKernelGGL(k_rn_normalize<float>, dim3(nb), dim3(256), 0, s, (const float*)X, N, D, (float*)Xn.p);
    HMSG_CHECK_LAUNCH();
    pool_launch_seg_rows(s, d_ps.p, K, maxn, seg_of_row.p);
    if (f64) {
        hipLaunchKernelGGL(k_rn_gram_f64, dim3((unsigned)tiles64), dim3(256), 0, s, (const double*)Xn.p, D, (const PoolSeg*)d_ps.p,
                           (const long long*)d_tb.p, K, eps, adj.p, ncount.p);
        HMSG_CHECK_LAUNCH();
    } else {
        pool_launch_gram_f32(s, (const float*)Xn.p, D, d_ps.p, K, tiles32, (float)eps, adj.p, ncount.p);
    }
    pool_cluster(s, d_ps.p, N, min_samples, adj.p, ncount.p, seg_of_row.p, label.p, seg_first.p, d_changed.p, flabel.p, csize.p, cfirst.p,
                 best.p);
    if (f64) {
        hipLaunchKernelGGL(k_rn_mean_f64, dim3(cdiv(D, 64), K), dim3(64), 0, s, (const double*)X, D, (const PoolSeg*)d_ps.p,
                           (const int*)flabel.p, (const unsigned long long*)best.p, (double*)out);
        HMSG_CHECK_LAUNCH();
    } else {
        pool_launch_mean_f32(s, (const float*)X, D, d_ps.p, K, flabel.p, csize.p, cfirst.p, best.p, (float*)out);
    }
    if (n_in_cluster) {
        std::vector<unsigned long long> hb((size_t)K);
        HIP_TRY(hipMemcpyAsync(hb.data(), best.p, (size_t)K * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (int k = 0; k < K; ++k) n_in_cluster[k] = (int)(hb[(size_t)k] >> 32);
    }
    HIP_TRY(hipStreamSynchronize(s));
}

void rn_choose(hipStream_t s, const void* rows, bool f64, long long K, int D, const float* T, int n_types, int* d_type) {
    if (K <= 0) return;
    const unsigned nb = cdiv((size_t)K * 64, 256);
    if (f64)
        hipLaunchKernelGGL(k_rn_choose<double>, dim3(nb), dim3(256), 0, s, (const double*)rows, K, D, T, n_types, d_type);
    else
        hipLaunchKernelGGL(k_rn_choose<float>, dim3(nb), dim3(256), 0, s, (const float*)rows, K, D, T, n_types, d_type);
    HMSG_CHECK_LAUNCH();
}

void rn_vote(hipStream_t s, const int* d_view_type, const std::vector<long long>& voff, int n_types, int* type_of_room) {
    const int R = (int)voff.size() - 1;
    if (R <= 0) return;
    DevBuf<long long> d_off;
    DevBuf<int> d_out;
    d_off.alloc(voff.size());
    d_out.alloc((size_t)R);
    HIP_TRY(hipMemcpyAsync(d_off.p, voff.data(), voff.size() * 8, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_rn_vote, dim3(cdiv((size_t)R, 64)), dim3(64), 0, s, d_view_type, (const long long*)d_off.p, R, n_types, d_out.p);
    HMSG_CHECK_LAUNCH();
    HIP_TRY(hipMemcpyAsync(type_of_room, d_out.p, (size_t)R * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
}

void rn_gather_rows_f32(hipStream_t s, const float* src, const std::vector<int>& rows, int D, float* dst) {
    if (rows.empty()) return;
    DevBuf<int> d_rows;
    d_rows.alloc(rows.size());
    HIP_TRY(hipMemcpyAsync(d_rows.p, rows.data(), rows.size() * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_rn_gather_f32, dim3(cdiv(rows.size() * (size_t)D, 256)), dim3(256), 0, s, src, (const int*)d_rows.p, (int)rows.size(), D,
                       dst);
    HMSG_CHECK_LAUNCH();
    HIP_TRY(hipStreamSynchronize(s));
}

/* include/hmsg.h: hmsg_denoise_feats_batch */
extern "C" int hmsg_denoise_feats_batch(int32_t device_id, int32_t n_sets, const int64_t* set_off, const void* feats, int32_t feats_is_f64,
                                        int32_t dim, double eps, int32_t min_samples, void* out, int32_t* n_in_cluster) {
    if (n_sets < 0 || (n_sets > 0 && (!set_off || !feats || !out)) || dim <= 0 || !(eps > 0.0) || min_samples < 1) return HMSG_ERR_INVALID;
    if (n_sets == 0) return HMSG_OK;
    return hmsg_boundary("hmsg_denoise_feats_batch", -1, [&] {
        std::vector<long long> off((size_t)n_sets + 1);
        for (int k = 0; k <= n_sets; ++k) off[(size_t)k] = (long long)set_off[k] - (long long)set_off[0];
        for (int k = 0; k < n_sets; ++k)
            HMSG_REQUIRE(off[(size_t)k + 1] > off[(size_t)k], HMSG_ERR_INVALID,
                         "set " + std::to_string(k) + " is empty (feats_denoise_dbscan of an empty array raises)");
        HMSG_REQUIRE(off.back() < (1ll << 31), HMSG_ERR_UNSUPPORTED, "more than 2^31 rows");
        HIP_TRY(hipSetDevice(device_id));
        const size_t esz = feats_is_f64 ? 8 : 4, in_bytes = (size_t)off.back() * dim * esz, out_bytes = (size_t)n_sets * dim * esz;
        const char* src = (const char*)feats + (size_t)set_off[0] * dim * esz;
        hipStream_t s = nullptr;
        DevBuf<char> d_in, d_out;
        const char* X = stage_in(d_in, src, in_bytes, s, Up::direct);
        char* Y = stage_out(d_out, (char*)out, out_bytes);
        rn_denoise(s, X, feats_is_f64 != 0, dim, off, eps, min_samples, Y, n_in_cluster);
        unstage_out((char*)out, Y, out_bytes, s);
        HIP_TRY(hipStreamSynchronize(s));
    });
}
