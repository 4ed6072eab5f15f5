// The open-vocabulary 3-D semantic segmentation score of a feature map (memory/hmsg/utils/eval_utils.py, utils/metric.py).
//
//   hmsg_semseg_instance_labels   text_prompt (eval_utils.py:80-95) + sim_2_label (:285-293): per instance the class whose text row
//                                 has the largest float32 cosine.
//   hmsg_knn_labels               knn_interpolation (:308-339; Tree_interpolation, :296-305, is its k = 1 form): the labels of a
//                                 labelled cloud carried onto a query cloud by an exact k-nearest-neighbour vote.
//   hmsg_semseg_confusion         the confusion matrix every number of metric.py can be read from.
//   hmsg_semseg_metrics           metric.py's five numbers from that matrix, float64 on the host (hmsg_eval_metrics_host.h).
//   hmsg_evaluate_semseg          the four of them on the scene's pooled instances, nothing of the scene leaving the device.
//
// The k-NN search, exact throughout.  The order of candidates is (d2, index): d2 = ((dx*dx) + (dy*dy)) + (dz*dz) in float64 without
// contraction -- the rdist sklearn's Euclidean metric accumulates -- and index = the row's position after the rows with label -1
// were dropped.  The labelled rows are sorted ONCE by the cell of a uniform lattice over their bounding box (hmsg_sort.hip, stable:
// a cell's rows stay in index order); the cell side comes from the cloud's density, 2k rows per cell of the box's volume, so the
// lattice has about n / 2k cells and a dense table of cell starts is small.
//   phase 1  a lane per query walks the cube shells ("rings") around the query's cell outward; a row of cells along x is one
//            contiguous range of the sorted array.  The k best so far live in registers, kept sorted by compare-and-swap chains that
//            are unrolled for the template's width (a runtime index into the list would send it to scratch memory).  After ring r every
//            row not yet seen lies outside the cube of 2r + 1 cells: the search ends when the k-th best d2 is BELOW the squared
//            distance to the nearest face of that cube which still has lattice behind it (less a slack for the rounding of the
//            binning; strictly below, so an unseen row at the same d2 with a smaller index cannot exist), or when the cube covers
//            the lattice.  SS_MAX_RING rings at most.
//   phase 2  the queries that reached the cap -- vertices of the ground truth where nothing was mapped are the normal case -- are
//            compacted into a list and finished by scan: a wave per query, every lane a private top-k over a stride of the labelled
//            rows, the 64 sorted lists laid into LDS and merged by k rounds of "smallest head of the 64".
// Both phases produce the k rows in (d2, index) order, so they agree bit for bit (HMSG_DEBUG_KNN_BRUTE=1 sends every query through
// phase 2).  The vote compares the k kept labels pairwise: no table over the label range.
//
// Bound (derived, not measured): with c rows per occupied cell, a phase-1 query that ends after ring 1 reads at most 27 c rows of
// 28 bytes (three float64 and the index) plus <= 13 cell-table entries of 4 bytes; a phase-2 query reads all n rows (24 bytes each).
#include "hmsg_boundary.h"
#include "hmsg_eval_metrics_host.h"

#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

namespace {

enum { SS_MAX_RING = 8 };

// numpy's order of float32 values as an unsigned key: NaN above every number (np.argmax returns the first NaN), -0 equal to +0
__device__ __forceinline__ unsigned ss_key(float v) {
    if (v != v) return 0xFFFFFFFFu;
    if (v == 0.0f) v = 0.0f;
    const unsigned u = __float_as_uint(v);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}

// ================================================================================ a. instance labels
// One workgroup per instance: the embedding in float32 divided by max(||x||, 1e-8), then a wave per class: the text row's norm
// (clamped likewise) and the dot product of the two normalised rows.  Every class runs the same lane-strided loops and the same
// butterfly, so rows of the same bits give similarities of the same bits and the smaller index wins among them.
__global__ void __launch_bounds__(256) k_ss_inst_labels(const void* __restrict__ emb, int emb_f64, int D, const float* __restrict__ text, int C,
                                                        const int* __restrict__ class_label, int* __restrict__ label) {
    HIP_DYNAMIC_SHARED(float, xn)                        // [D]
    __shared__ float red[4];
    __shared__ unsigned bkey[4];
    __shared__ int bcls[4];
    const int i = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float ss = 0.0f;
    for (int d = tid; d < D; d += 256) {
        const float x = emb_f64 ? (float)((const double*)emb)[(size_t)i * D + d] : ((const float*)emb)[(size_t)i * D + d];
        xn[d] = x;
        ss = __fadd_rn(ss, __fmul_rn(x, x));
    }
    ss = wave_sum_f32(ss);
    if (lane == 0) red[wave] = ss;
    __syncthreads();
    const float nrm = fmaxf(__fsqrt_rn(__fadd_rn(__fadd_rn(red[0], red[1]), __fadd_rn(red[2], red[3]))), 1e-8f);
    for (int d = tid; d < D; d += 256) xn[d] = __fdiv_rn(xn[d], nrm);
    __syncthreads();
    unsigned bk = 0u;
    int bc = INT_MAX;
    for (int c = wave; c < C; c += 4) {
        const float* t = text + (size_t)c * D;
        float ts = 0.0f;
        for (int d = lane; d < D; d += 64) ts = __fadd_rn(ts, __fmul_rn(t[d], t[d]));
        const float tn = fmaxf(__fsqrt_rn(wave_sum_f32(ts)), 1e-8f);
        float dot = 0.0f;
        for (int d = lane; d < D; d += 64) dot = __fadd_rn(dot, __fmul_rn(xn[d], __fdiv_rn(t[d], tn)));
        const unsigned key = ss_key(wave_sum_f32(dot));
        if (bc == INT_MAX || key > bk) bk = key, bc = c;        // (ascending c: the first of equal keys stays)
    }
    if (lane == 0) bkey[wave] = bk, bcls[wave] = bc;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w)
            if (bcls[w] != INT_MAX && (bkey[w] > bk || (bkey[w] == bk && bcls[w] < bc))) bk = bkey[w], bc = bcls[w];
        label[i] = class_label[bc];
    }
}

// ================================================================================ b. the k-NN label vote
struct SsGrid {
    double o[3], cell, slack;
    int n[3], pad;
};
enum { SS_BAD_LABEL = 1, SS_BAD_POINT = 2, SS_BAD_QUERY = 4 };

__device__ __forceinline__ bool ss_finite3(const double* p) {
    return fabs(p[0]) <= 1.7976931348623157e308 && fabs(p[1]) <= 1.7976931348623157e308 && fabs(p[2]) <= 1.7976931348623157e308;
}

// per labelled row: keep flag (label != -1), the refusals (a label below -1 anywhere, a non-finite coordinate in a KEPT row), and the
// bounding box of the kept rows (order-preserving integer keys)
__global__ void __launch_bounds__(256) k_ss_scan_rows(const double* __restrict__ lp, const int* __restrict__ lab, long long n,
                                                      unsigned* __restrict__ keep, unsigned* __restrict__ status,
                                                      unsigned long long* __restrict__ box) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    unsigned long long mn[3] = {~0ull, ~0ull, ~0ull}, mx[3] = {0ull, 0ull, 0ull};
    unsigned bad = 0u;
    if (i < n) {
        const int l = lab[i];
        if (l < -1) bad |= SS_BAD_LABEL;
        if (l != -1 && !ss_finite3(lp + i * 3)) bad |= SS_BAD_POINT;      // (a dropped row never reaches the reference's tree either)
        keep[i] = l != -1 ? 1u : 0u;
        if (l != -1)
            for (int a = 0; a < 3; ++a) mn[a] = mx[a] = enc_f64(lp[i * 3 + a]);
    }
    for (int a = 0; a < 3; ++a) {
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long pmn = __shfl_xor(mn[a], o), pmx = __shfl_xor(mx[a], o);
            mn[a] = pmn < mn[a] ? pmn : mn[a];
            mx[a] = pmx > mx[a] ? pmx : mx[a];
        }
        if ((threadIdx.x & 63) == 0 && mn[a] <= mx[a]) {
            atomicMin(&box[a], mn[a]);
            atomicMax(&box[3 + a], mx[a]);
        }
    }
    if (bad) atomicOr(status, bad);
}
__global__ void __launch_bounds__(256) k_ss_check_queries(const double* __restrict__ q, long long m, unsigned* __restrict__ status) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j < m && !ss_finite3(q + j * 3)) atomicOr(status, (unsigned)SS_BAD_QUERY);
}

__device__ __forceinline__ int ss_cell(const SsGrid& g, double v, int a) {
    return (int)floor(__ddiv_rn(__dsub_rn(v, g.o[a]), g.cell));
}
// the kept rows in order (points, labels) and their sort records: key = cell key (cz NY + cy) NX + cx, value = position after the drop
__global__ void __launch_bounds__(256) k_ss_compact(const double* __restrict__ lp, const int* __restrict__ lab, long long n,
                                                    const unsigned* __restrict__ keep, const unsigned* __restrict__ pos, SsGrid g,
                                                    double* __restrict__ cp, int* __restrict__ cl, unsigned* __restrict__ keys,
                                                    unsigned long long* __restrict__ vals) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !keep[i]) return;
    const size_t p = pos[i];
    int c[3];
    for (int a = 0; a < 3; ++a) {
        const double v = lp[i * 3 + a];
        cp[p * 3 + a] = v;
        c[a] = min(max(ss_cell(g, v, a), 0), g.n[a] - 1);
    }
    cl[p] = lab[i];
    keys[p] = (unsigned)((c[2] * g.n[1] + c[1]) * g.n[0] + c[0]);
    vals[p] = (unsigned long long)p;
}
__global__ void __launch_bounds__(256) k_ss_gather(const double* __restrict__ cp, const unsigned long long* __restrict__ vals, long long n,
                                                   double* __restrict__ sp, int* __restrict__ sidx) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t p = (size_t)vals[i];
    sidx[i] = (int)p;
    for (int a = 0; a < 3; ++a) sp[i * 3 + a] = cp[p * 3 + a];
}
// cs[c] = first sorted row of a cell >= c, cs[ncells] = n: the row that opens cell k fills the entries of the empty cells before it
__global__ void __launch_bounds__(256) k_ss_cell_starts(const unsigned* __restrict__ skey, long long n, unsigned ncells, unsigned* __restrict__ cs) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned k = skey[i];
    const long long prev = i ? (long long)skey[i - 1] : -1;
    for (long long c = prev + 1; c <= (long long)k; ++c) cs[c] = (unsigned)i;
    if (i == n - 1)
        for (unsigned c = k + 1; c <= ncells; ++c) cs[c] = (unsigned)n;
}

// the K best (d2, index) so far, ascending; every loop over the list is unrolled so that it stays in registers
template <int K>
__device__ __forceinline__ void ss_topk_init(double (&d)[K], int (&ix)[K]) {
#pragma unroll
    for (int j = 0; j < K; ++j) d[j] = INFINITY, ix[j] = INT_MAX;
}
template <int K>
__device__ __forceinline__ void ss_topk_push(double (&d)[K], int (&ix)[K], double nd, int ni) {
    if (!(nd < d[K - 1] || (nd == d[K - 1] && ni < ix[K - 1]))) return;
    d[K - 1] = nd;
    ix[K - 1] = ni;
#pragma unroll
    for (int j = K - 1; j > 0; --j) {
        const bool sw = d[j] < d[j - 1] || (d[j] == d[j - 1] && ix[j] < ix[j - 1]);
        const double da = d[j - 1], db = d[j];
        const int ia = ix[j - 1], ib = ix[j];
        d[j - 1] = sw ? db : da;
        d[j] = sw ? da : db;
        ix[j - 1] = sw ? ib : ia;
        ix[j] = sw ? ia : ib;
    }
}
__device__ __forceinline__ double ss_d2(double qx, double qy, double qz, const double* __restrict__ p) {
    const double dx = __dsub_rn(qx, p[0]), dy = __dsub_rn(qy, p[1]), dz = __dsub_rn(qz, p[2]);
    return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}
// np.bincount(labels[:k]).argmax(): the most frequent label, the smallest among equally frequent ones
template <int K>
__device__ __forceinline__ int ss_vote(const int (&l)[K], int k) {
    int best = INT_MAX, best_n = 0;
#pragma unroll
    for (int a = 0; a < K; ++a) {
        int cnt = 0;
#pragma unroll
        for (int b = 0; b < K; ++b) cnt += (b < k && l[b] == l[a]) ? 1 : 0;
        if (a < k && (cnt > best_n || (cnt == best_n && l[a] < best))) best = l[a], best_n = cnt;
    }
    return best;
}
template <int K>
__device__ __forceinline__ void ss_finish(const int (&ix)[K], int k, long long j, const int* __restrict__ cl, int* __restrict__ out_label,
                                          int* __restrict__ out_nn) {
    int l[K];
#pragma unroll
    for (int a = 0; a < K; ++a) l[a] = a < k ? cl[ix[a]] : 0;
    out_label[j] = ss_vote<K>(l, k);
    if (out_nn) {
#pragma unroll
        for (int a = 0; a < K; ++a)
            if (a < k) out_nn[j * k + a] = ix[a];
    }
}

// phase 1: a lane per query, rings of cells outward (see the head of the file); a query that is not done at the cap goes to `todo`
template <int K>
__global__ void __launch_bounds__(256) k_ss_knn_rings(const double* __restrict__ sp, const int* __restrict__ sidx, const unsigned* __restrict__ cs,
                                                      SsGrid g, const double* __restrict__ q, long long m, int k, const int* __restrict__ cl,
                                                      int* __restrict__ out_label, int* __restrict__ out_nn, unsigned* __restrict__ todo,
                                                      unsigned* __restrict__ n_todo) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const double qv[3] = {q[j * 3], q[j * 3 + 1], q[j * 3 + 2]};
    int c[3];
    bool far = false;
    for (int a = 0; a < 3; ++a) {
        const double t = floor(__ddiv_rn(__dsub_rn(qv[a], g.o[a]), g.cell));
        far = far || t < -(double)(SS_MAX_RING + 1) || t > (double)(g.n[a] + SS_MAX_RING);   // (no ring reaches the lattice)
        c[a] = far ? 0 : (int)t;
    }
    double d[K];
    int ix[K];
    ss_topk_init<K>(d, ix);
    bool done = false;
    for (int r = 0; r <= SS_MAX_RING && !far && !done; ++r) {
        const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, g.n[2] - 1), y0 = max(c[1] - r, 0), y1 = min(c[1] + r, g.n[1] - 1);
        for (int z = z0; z <= z1; ++z)
            for (int y = y0; y <= y1; ++y) {
                const bool shell = z - c[2] == r || c[2] - z == r || y - c[1] == r || c[1] - y == r;
                const unsigned row = (unsigned)((z * g.n[1] + y) * g.n[0]);
                // a shell row is the whole run of cells along x; an inner row has the two cells at distance r
                for (int half = 0; half < (shell ? 1 : 2); ++half) {
                    const int xa = shell ? c[0] - r : (half ? c[0] + r : c[0] - r), xb = shell ? c[0] + r : xa;
                    const int x0 = max(xa, 0), x1 = min(xb, g.n[0] - 1);
                    if (x0 > x1) continue;
                    const unsigned e = cs[row + (unsigned)x1 + 1u];
                    for (unsigned p = cs[row + (unsigned)x0]; p < e; ++p)
                        ss_topk_push<K>(d, ix, ss_d2(qv[0], qv[1], qv[2], sp + (size_t)p * 3), sidx[p]);
                }
            }
        double b = INFINITY;
        for (int a = 0; a < 3; ++a) {
            if (c[a] - r > 0) b = fmin(b, __dsub_rn(qv[a], __dadd_rn(g.o[a], __dmul_rn((double)(c[a] - r), g.cell))));
            if (c[a] + r < g.n[a] - 1) b = fmin(b, __dsub_rn(__dadd_rn(g.o[a], __dmul_rn((double)(c[a] + r + 1), g.cell)), qv[a]));
        }
        double kth = INFINITY;
#pragma unroll
        for (int a = 0; a < K; ++a) kth = a == k - 1 ? d[a] : kth;
        if (b == INFINITY) done = true;                       // the cube covers the lattice: every row was seen
        else {
            b = fmax(__dsub_rn(b, g.slack), 0.0);
            done = kth < __dmul_rn(b, b);
        }
    }
    if (done) ss_finish<K>(ix, k, j, cl, out_label, out_nn);
    else todo[atomicAdd(n_todo, 1u)] = (unsigned)j;
}

// phase 2: a wave (= a workgroup) per query of the list (todo == nullptr: every query)
template <int K>
__global__ void __launch_bounds__(64) k_ss_knn_scan(const double* __restrict__ cp, long long n, const int* __restrict__ cl, const double* __restrict__ q,
                                                    const unsigned* __restrict__ todo, long long cnt, int k, int* __restrict__ out_label,
                                                    int* __restrict__ out_nn) {
    __shared__ double sd[K * 64];
    __shared__ int si[K * 64];
    __shared__ int win[16];
    const int lane = (int)threadIdx.x;
    for (long long t = blockIdx.x; t < cnt; t += gridDim.x) {
        const long long j = todo ? (long long)todo[t] : t;
        const double qx = q[j * 3], qy = q[j * 3 + 1], qz = q[j * 3 + 2];
        double d[K];
        int ix[K];
        ss_topk_init<K>(d, ix);
        for (long long i = lane; i < n; i += 64) ss_topk_push<K>(d, ix, ss_d2(qx, qy, qz, cp + i * 3), (int)i);
#pragma unroll
        for (int a = 0; a < K; ++a) sd[a * 64 + lane] = d[a], si[a * 64 + lane] = ix[a];
        __syncthreads();
        int head = 0;
        for (int r = 0; r < k; ++r) {
            const double hd = head < K ? sd[head * 64 + lane] : INFINITY;
            const int hi = head < K ? si[head * 64 + lane] : INT_MAX;
            double md = hd;
            int mi = hi;
            for (int o = 32; o > 0; o >>= 1) {
                const double od = __shfl_xor(md, o);
                const int oi = __shfl_xor(mi, o);
                if (od < md || (od == md && oi < mi)) md = od, mi = oi;
            }
            if (hd == md && hi == mi) ++head;                 // (indices are distinct: one lane's head is the smallest)
            if (lane == 0) win[r] = mi;
        }
        __syncthreads();
        if (lane == 0) {
            int w[K];
#pragma unroll
            for (int a = 0; a < K; ++a) w[a] = a < k ? win[a] : 0;
            ss_finish<K>(w, k, j, cl, out_label, out_nn);
        }
        __syncthreads();
    }
}

// one instance's label on each of its pool points (instances in order, duplicates kept)
__global__ void __launch_bounds__(256) k_ss_paint(const long long* __restrict__ off, int n_inst, const int* __restrict__ inst_label, long long total,
                                                  int* __restrict__ lab) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    int lo = 0, hi = n_inst - 1;                            // the last instance that starts at or before i (it is not empty)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    lab[i] = inst_label[lo];
}

// ================================================================================ c. confusion matrix
__global__ void __launch_bounds__(256) k_ss_check_labels(const int* __restrict__ gt, const int* __restrict__ pred, long long m, int L,
                                                         unsigned* __restrict__ status) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j < m && (gt[j] < 0 || gt[j] >= L || pred[j] < 0 || pred[j] >= L)) atomicOr(status, 1u);
}
// LDS: a workgroup counts its share of the points in a histogram of its own and adds the cells it touched to the matrix
template <bool LDS>
__global__ void __launch_bounds__(256) k_ss_confusion(const int* __restrict__ gt, const int* __restrict__ pred, long long m, int L,
                                                      unsigned long long* __restrict__ conf) {
    HIP_DYNAMIC_SHARED(unsigned, hist)                   // [L * L] in the LDS form
    const int cells = L * L;
    if (LDS) {
        for (int c = (int)threadIdx.x; c < cells; c += 256) hist[c] = 0u;
        __syncthreads();
    }
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < m; j += (long long)gridDim.x * 256) {
        const size_t c = (size_t)gt[j] * (size_t)L + (size_t)pred[j];
        if (LDS) atomicAdd(&hist[c], 1u);
        else atomicAdd(&conf[c], 1ull);
    }
    if (LDS) {
        __syncthreads();
        for (int c = (int)threadIdx.x; c < cells; c += 256)
            if (hist[c]) atomicAdd(&conf[c], (unsigned long long)hist[c]);
    }
}

// ================================================================================ host side
long long g_last_phase2 = 0;       // queries the last hmsg_knn_labels call finished in phase 2 (hmsg_test_knn_last_phase2)

void ss_instance_labels(hmsg_ctx* h, int32_t n, const void* emb, int32_t emb_is_f64, int32_t D, int32_t C, const float* text,
                        const int32_t* class_label, int32_t* label_out) {
    hipStream_t s = h->stream;
    HMSG_REQUIRE(n >= 0 && D > 0 && C > 0, HMSG_ERR_INVALID, "hmsg_semseg_instance_labels: bad shape");
    HMSG_REQUIRE(D <= 8192, HMSG_ERR_UNSUPPORTED, "hmsg_semseg_instance_labels: embeddings of more than 8192 components");
    HMSG_REQUIRE(text && class_label && (n == 0 || (emb && label_out)), HMSG_ERR_INVALID, "hmsg_semseg_instance_labels: null argument");
    if (n == 0) return;
    DevBuf<float> uf, ut;
    DevBuf<double> ud;
    DevBuf<int32_t> uc, own;
    const void* de = emb_is_f64 ? (const void*)stage_in(ud, (const double*)emb, (size_t)n * D, s, Up::direct)
                                : (const void*)stage_in(uf, (const float*)emb, (size_t)n * D, s, Up::direct);
    const float* dt = stage_in(ut, text, (size_t)C * D, s, Up::direct);
    const int32_t* dc = stage_in(uc, class_label, (size_t)C, s, Up::direct);
    int32_t* dl = stage_out(own, label_out, (size_t)n);
    {
        ProfScope ps(h->prof, s, "k_ss_inst_labels", (double)n * ((double)C * D * 4 + (double)D * 8));
        hipLaunchKernelGGL(k_ss_inst_labels, dim3((unsigned)n), dim3(256), (size_t)D * 4, s, de, (int)(emb_is_f64 != 0), (int)D, dt, (int)C,
                           (const int*)dc, (int*)dl);
        HMSG_CHECK_LAUNCH();
    }
    unstage_out(label_out, dl, (size_t)n, s);
    HIP_TRY(hipStreamSynchronize(s));
}

template <int K>
void ss_knn_launch(hmsg_ctx* h, bool brute, const double* sp, const int* sidx, const unsigned* cs, const SsGrid& g, const double* cp,
                   long long nk, const int* cl, const double* dq, long long m, int k, int* dl, int* dnn) {
    hipStream_t s = h->stream;
    long long n2 = m;
    DevBuf<unsigned> todo, cnt;
    if (!brute) {
        todo.alloc((size_t)m);
        cnt.alloc(1);
        cnt.zero(s);
        {
            ProfScope ps(h->prof, s, "k_ss_knn_rings", (double)m * (24.0 + 4.0 + 4.0 * k));
            hipLaunchKernelGGL(k_ss_knn_rings<K>, dim3(cdiv((size_t)m, 256)), dim3(256), 0, s, sp, sidx, cs, g, dq, m, k, cl, dl, dnn, todo.p, cnt.p);
            HMSG_CHECK_LAUNCH();
        }
        unsigned got = 0;
        HIP_TRY(hipMemcpyAsync(&got, cnt.p, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        n2 = (long long)got;
    }
    g_last_phase2 = n2;
    if (n2 > 0) {
        ProfScope ps(h->prof, s, "k_ss_knn_scan", (double)n2 * (double)nk * 24.0);
        hipLaunchKernelGGL(k_ss_knn_scan<K>, dim3((unsigned)std::min<long long>(n2, 65536)), dim3(64), 0, s, cp, nk, cl, dq,
                           brute ? (const unsigned*)nullptr : (const unsigned*)todo.p, n2, k, dl, dnn);
        HMSG_CHECK_LAUNCH();
    }
    HIP_TRY(hipStreamSynchronize(s));
}

void ss_knn_labels(hmsg_ctx* h, int64_t n, const double* lp, const int32_t* lab, int64_t m, const double* q, int32_t k, int32_t* out_label,
                   int32_t* out_nn) {
    hipStream_t s = h->stream;
    HMSG_REQUIRE(k >= 1 && k <= 16, HMSG_ERR_INVALID, "hmsg_knn_labels: k outside 1 .. 16");
    HMSG_REQUIRE(n >= 0 && m >= 0 && (n == 0 || (lp && lab)) && (m == 0 || (q && out_label)), HMSG_ERR_INVALID,
                 "hmsg_knn_labels: bad shape or null argument");
    HMSG_REQUIRE(n < (1ll << 31) && m < (1ll << 31) && (long long)m * k < (1ll << 40), HMSG_ERR_UNSUPPORTED, "hmsg_knn_labels: 2^31 rows or more");
    if (m == 0) return;
    HMSG_REQUIRE(n >= k, HMSG_ERR_INVALID, "hmsg_knn_labels: fewer than k labelled rows (sklearn raises)");
    g_last_phase2 = 0;
    DevBuf<double> up, uq;
    DevBuf<int32_t> ul;
    const double* dp = stage_in(up, lp, (size_t)n * 3, s, Up::bounce);
    const int32_t* dlab = stage_in(ul, lab, (size_t)n, s, Up::direct);
    const double* dq = stage_in(uq, q, (size_t)m * 3, s, Up::bounce);
    // pass 1: keep flags, refusals, bounding box -- nothing of the outputs is written before the host has seen them
    DevBuf<unsigned> keep, pos, status;
    DevBuf<unsigned long long> box;
    keep.alloc((size_t)n);
    pos.alloc((size_t)n);
    status.alloc(1);
    status.zero(s);
    box.alloc(6);
    const unsigned long long init[6] = {~0ull, ~0ull, ~0ull, 0ull, 0ull, 0ull};
    HIP_TRY(hipMemcpyAsync(box.p, init, sizeof(init), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_ss_scan_rows, dim3(cdiv((size_t)n, 256)), dim3(256), 0, s, dp, (const int*)dlab, (long long)n, keep.p, status.p, box.p);
    HMSG_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_ss_check_queries, dim3(cdiv((size_t)m, 256)), dim3(256), 0, s, dq, (long long)m, status.p);
    HMSG_CHECK_LAUNCH();
    unsigned long long nkept = 0;
    hmsg_scan_u32(keep.p, pos.p, (size_t)n, s, h->scan_tmp, &nkept);
    unsigned st = 0;
    unsigned long long hb[6];
    HIP_TRY(hipMemcpyAsync(&st, status.p, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(hb, box.p, sizeof(hb), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    HMSG_REQUIRE(!(st & SS_BAD_LABEL), HMSG_ERR_INVALID, "hmsg_knn_labels: a label below -1");
    HMSG_REQUIRE(!(st & (SS_BAD_POINT | SS_BAD_QUERY)), HMSG_ERR_INVALID, "hmsg_knn_labels: a coordinate is not finite");
    const long long nk = (long long)nkept;
    HMSG_REQUIRE(nk >= k, HMSG_ERR_INVALID, "hmsg_knn_labels: fewer than k labelled rows once label -1 is dropped (sklearn raises)");
    // the lattice: 2k rows per cell of the box's volume (an axis thinner than a thousandth of the longest counts as that thick), at most
    // 1024 cells along an axis
    SsGrid g;
    double ext[3], emax = 0.0, amax = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double lo = dec_f64(hb[a]), hi = dec_f64(hb[3 + a]);
        g.o[a] = lo;
        ext[a] = hi - lo;
        emax = std::max(emax, ext[a]);
        amax = std::max(amax, std::max(std::fabs(lo), std::fabs(hi)));
    }
    HMSG_REQUIRE(std::isfinite(emax), HMSG_ERR_UNSUPPORTED, "hmsg_knn_labels: the labelled cloud's extent overflows");
    if (emax > 0.0) {
        double vol = 1.0;
        for (int a = 0; a < 3; ++a) vol *= std::max(ext[a], emax * 1e-3);
        g.cell = std::max(std::cbrt(vol * (2.0 * k) / (double)nk), emax / 1023.0);
    } else
        g.cell = 1.0;
    unsigned long long ncells = 1;
    for (int a = 0; a < 3; ++a) {
        g.n[a] = (int)std::min(std::floor(ext[a] / g.cell) + 1.0, 1025.0);
        ncells *= (unsigned long long)g.n[a];
    }
    g.pad = 0;
    g.slack = 1e-6 * g.cell + 1e-13 * (amax + (SS_MAX_RING + 2) * g.cell);
    HMSG_REQUIRE(ncells <= (1ull << 27), HMSG_ERR_UNSUPPORTED, "hmsg_knn_labels: the lattice has more than 2^27 cells");
    // pass 2: compact, sort by cell, gather, cell starts
    DevBuf<double> cp, sp;
    DevBuf<int> cl, sidx;
    DevBuf<unsigned> cs;
    cp.alloc((size_t)nk * 3);
    cl.alloc((size_t)nk);
    const bool brute = getenv("HMSG_DEBUG_KNN_BRUTE") != nullptr && atoi(getenv("HMSG_DEBUG_KNN_BRUTE")) != 0;
    {
        SortBufs sb;
        sb.keys.alloc((size_t)nk);
        sb.vals.alloc((size_t)nk);
        ProfScope ps(h->prof, s, "k_ss_compact_sort", (double)n * (24 + 4 + 8) + (double)nk * (24 + 4 + 12 + 28));
        hipLaunchKernelGGL(k_ss_compact, dim3(cdiv((size_t)n, 256)), dim3(256), 0, s, dp, (const int*)dlab, (long long)n, (const unsigned*)keep.p,
                           (const unsigned*)pos.p, g, cp.p, cl.p, sb.keys.p, sb.vals.p);
        HMSG_CHECK_LAUNCH();
        if (!brute) {
            hmsg_sort_pairs(sb, (size_t)nk, bits_for(ncells), s);
            sp.alloc((size_t)nk * 3);
            sidx.alloc((size_t)nk);
            cs.alloc((size_t)ncells + 1);
            hipLaunchKernelGGL(k_ss_gather, dim3(cdiv((size_t)nk, 256)), dim3(256), 0, s, (const double*)cp.p, (const unsigned long long*)sb.res_vals,
                               nk, sp.p, sidx.p);
            HMSG_CHECK_LAUNCH();
            hipLaunchKernelGGL(k_ss_cell_starts, dim3(cdiv((size_t)nk, 256)), dim3(256), 0, s, (const unsigned*)sb.res_keys, nk, (unsigned)ncells, cs.p);
            HMSG_CHECK_LAUNCH();
        }
        HIP_TRY(hipStreamSynchronize(s));                   // (the sort's buffers go back to the cache here)
    }
    DevBuf<int32_t> own_l, own_nn;
    int32_t* dl = stage_out(own_l, out_label, (size_t)m);
    int32_t* dnn = stage_out(own_nn, out_nn, (size_t)m * k);
    const int width = k == 1 ? 1 : k <= 5 ? 5 : k <= 8 ? 8 : 16;
    switch (width) {
    case 1: ss_knn_launch<1>(h, brute, sp.p, sidx.p, cs.p, g, cp.p, nk, cl.p, dq, m, k, dl, dnn); break;
    case 5: ss_knn_launch<5>(h, brute, sp.p, sidx.p, cs.p, g, cp.p, nk, cl.p, dq, m, k, dl, dnn); break;
    case 8: ss_knn_launch<8>(h, brute, sp.p, sidx.p, cs.p, g, cp.p, nk, cl.p, dq, m, k, dl, dnn); break;
    default: ss_knn_launch<16>(h, brute, sp.p, sidx.p, cs.p, g, cp.p, nk, cl.p, dq, m, k, dl, dnn); break;
    }
    unstage_out(out_label, dl, (size_t)m, s);
    if (out_nn) unstage_out(out_nn, dnn, (size_t)m * k, s);
    HIP_TRY(hipStreamSynchronize(s));
}

void ss_confusion(hmsg_ctx* h, int64_t m, const int32_t* gt_label, const int32_t* pred_label, int32_t L, int64_t* conf) {
    hipStream_t s = h->stream;
    HMSG_REQUIRE(L >= 1 && L <= 4096, HMSG_ERR_INVALID, "hmsg_semseg_confusion: L outside 1 .. 4096");
    HMSG_REQUIRE(m >= 0 && conf && (m == 0 || (gt_label && pred_label)), HMSG_ERR_INVALID, "hmsg_semseg_confusion: bad shape or null argument");
    const size_t cells = (size_t)L * L;
    DevBuf<int32_t> ug, upd;
    DevBuf<int64_t> own;
    DevBuf<unsigned> status;
    const int32_t* dg = m ? stage_in(ug, gt_label, (size_t)m, s, Up::bounce) : nullptr;
    const int32_t* dpr = m ? stage_in(upd, pred_label, (size_t)m, s, Up::bounce) : nullptr;
    if (m) {
        status.alloc(1);
        status.zero(s);
        hipLaunchKernelGGL(k_ss_check_labels, dim3(cdiv((size_t)m, 256)), dim3(256), 0, s, (const int*)dg, (const int*)dpr, (long long)m, (int)L, status.p);
        HMSG_CHECK_LAUNCH();
        unsigned st = 0;
        HIP_TRY(hipMemcpyAsync(&st, status.p, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        HMSG_REQUIRE(st == 0, HMSG_ERR_INVALID, "hmsg_semseg_confusion: a label outside [0, L)");
    }
    int64_t* dc = stage_out(own, conf, cells);
    HIP_TRY(hipMemsetAsync(dc, 0, cells * 8, s));
    if (m) {
        const bool lds = cells * 4 <= 48 * 1024;
        const unsigned nblk = std::min<unsigned>(cdiv((size_t)m, 256 * 16), 4096u);
        ProfScope ps(h->prof, s, "k_ss_confusion", (double)m * 8.0 + (double)cells * 8.0);
        if (lds)
            hipLaunchKernelGGL(k_ss_confusion<true>, dim3(nblk), dim3(256), cells * 4, s, (const int*)dg, (const int*)dpr, (long long)m, (int)L,
                               (unsigned long long*)dc);
        else
            hipLaunchKernelGGL(k_ss_confusion<false>, dim3(nblk), dim3(256), 0, s, (const int*)dg, (const int*)dpr, (long long)m, (int)L,
                               (unsigned long long*)dc);
        HMSG_CHECK_LAUNCH();
    }
    unstage_out(conf, dc, cells, s);
    HIP_TRY(hipStreamSynchronize(s));
}

void ss_check_ignore(const char* who, const int32_t* ignore, int32_t n_ignore) {
    HMSG_REQUIRE(n_ignore >= 0 && (n_ignore == 0 || ignore), HMSG_ERR_INVALID, std::string(who) + ": bad ignore list");
}

void ss_evaluate(hmsg_ctx* h, const float* text, int32_t C, const int32_t* class_label, const double* gt_pts, const int32_t* gt_label, int64_t m,
                 int32_t k, int32_t L, const int32_t* ignore, int32_t n_ignore, hmsg_semseg_scores* scores, double* per_class_iou, int64_t* conf) {
    hipStream_t s = h->stream;
    HMSG_REQUIRE(h->merged && h->pooled && h->inst.off.size() > 1, HMSG_ERR_INVALID, "hmsg_evaluate_semseg: no pooled instances (hmsg_pool_instances first)");
    HMSG_REQUIRE(scores && m > 0 && gt_pts && gt_label, HMSG_ERR_INVALID, "hmsg_evaluate_semseg: null argument or no ground-truth points");
    HMSG_REQUIRE(L >= 1 && L <= 4096, HMSG_ERR_INVALID, "hmsg_evaluate_semseg: L outside 1 .. 4096");
    ss_check_ignore("hmsg_evaluate_semseg", ignore, n_ignore);
    const int n_inst = (int)h->inst.off.size() - 1;
    const long long total = h->inst.total;
    DevBuf<int32_t> inst_label, lab, pred;
    DevBuf<long long> doff;
    inst_label.alloc((size_t)n_inst);
    ss_instance_labels(h, n_inst, h->inst_feats.p, 0, h->cfg.feat_dim, C, text, class_label, inst_label.p);
    lab.alloc((size_t)total);
    doff.alloc(h->inst.off.size());
    HIP_TRY(hipMemcpyAsync(doff.p, h->inst.off.data(), h->inst.off.size() * 8, hipMemcpyHostToDevice, s));
    if (total) {
        hipLaunchKernelGGL(k_ss_paint, dim3(cdiv((size_t)total, 256)), dim3(256), 0, s, (const long long*)doff.p, n_inst, (const int*)inst_label.p, total,
                           lab.p);
        HMSG_CHECK_LAUNCH();
    }
    HIP_TRY(hipStreamSynchronize(s));                       // (h->inst.off is the source of an asynchronous copy)
    pred.alloc((size_t)m);
    ss_knn_labels(h, total, h->inst.pts.p, lab.p, m, gt_pts, k, pred.p, nullptr);
    std::vector<int64_t> hc((size_t)L * L);
    ss_confusion(h, m, gt_label, pred.p, L, hc.data());
    eval_metrics::SemsegScores sc = eval_metrics::semseg_metrics(hc.data(), L, ignore, n_ignore, per_class_iou);
    scores->miou = sc.miou, scores->fmiou = sc.fmiou, scores->acc = sc.acc, scores->macc = sc.macc;
    if (conf) write_out(conf, hc.data(), hc.size() * 8);
}

}  // namespace

extern "C" int hmsg_semseg_instance_labels(hmsg_t* h, int32_t n, const void* emb, int32_t emb_is_f64, int32_t D, int32_t C, const float* text,
                                           const int32_t* class_label, int32_t* label_out) {
    if (!h) return HMSG_ERR_INVALID;
    return hmsg_boundary(h, [&] { ss_instance_labels(h, n, emb, emb_is_f64, D, C, text, class_label, label_out); });
}

extern "C" int hmsg_knn_labels(hmsg_t* h, int64_t n, const double* lp, const int32_t* lab, int64_t m, const double* q, int32_t k, int32_t* out_label,
                               int32_t* out_nn_index) {
    if (!h) return HMSG_ERR_INVALID;
    return hmsg_boundary(h, [&] { ss_knn_labels(h, n, lp, lab, m, q, k, out_label, out_nn_index); });
}

extern "C" int64_t hmsg_test_knn_last_phase2(void) { return (int64_t)g_last_phase2; }

extern "C" int hmsg_semseg_confusion(hmsg_t* h, int64_t m, const int32_t* gt_label, const int32_t* pred_label, int32_t L, int64_t* conf) {
    if (!h) return HMSG_ERR_INVALID;
    return hmsg_boundary(h, [&] { ss_confusion(h, m, gt_label, pred_label, L, conf); });
}

extern "C" int hmsg_semseg_metrics(const int64_t* conf, int32_t L, const int32_t* ignore, int32_t n_ignore, hmsg_semseg_scores* out,
                                   double* per_class_iou) {
    return hmsg_boundary("hmsg_semseg_metrics", -1, [&] {
        HMSG_REQUIRE(conf && out && L >= 1 && L <= 4096, HMSG_ERR_INVALID, "null argument, or L outside 1 .. 4096");
        ss_check_ignore("hmsg_semseg_metrics", ignore, n_ignore);
        for (size_t c = 0; c < (size_t)L * L; ++c) HMSG_REQUIRE(conf[c] >= 0, HMSG_ERR_INVALID, "a negative count");
        const eval_metrics::SemsegScores sc = eval_metrics::semseg_metrics(conf, L, ignore, n_ignore, per_class_iou);
        out->miou = sc.miou, out->fmiou = sc.fmiou, out->acc = sc.acc, out->macc = sc.macc;
    });
}

extern "C" int hmsg_evaluate_semseg(hmsg_t* h, const float* text, int32_t C, const int32_t* class_label, const double* gt_pts,
                                    const int32_t* gt_label, int64_t m, int32_t k, int32_t L, const int32_t* ignore, int32_t n_ignore,
                                    hmsg_semseg_scores* scores, double* per_class_iou, int64_t* conf) {
    if (!h) return HMSG_ERR_INVALID;
    return hmsg_boundary(h, [&] {
        ss_evaluate(h, text, C, class_label, gt_pts, gt_label, m, k, L, ignore, n_ignore, scores, per_class_iou, conf);
    });
}
