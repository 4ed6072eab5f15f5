// hmsg_kmeans on the device, for a batch of independent problems ("sets"): hmsg_kmeans_batch (include/hmsg.h) and the test seam
// hmsg_test_kmeans_lloyd (include/hmsg_test.h).  A restatement of hmsg_kmeans.hip, statement by statement, that gives the same
// bits: labels, centres, inertia and n_iter of every set equal hmsg_kmeans called on that set alone.
//
// Why the bits can be equal.  Every sum of hmsg_kmeans.hip is one of two kinds, and both are kept as they are:
//   * float64 sums of products of two float32 values (the E-step, the centre norms, |x|^2, the k-means++ distances): eight
//     running sums over i mod 8, combined ((s0+s1)+(s2+s3))+((s4+s5)+(s6+s7)), then the tail (dots / dot8 below).  The products
//     are exact in float64, so a fused multiply-add gives what a multiply and an add give; only the ORDER of the additions
//     matters.  Plain vector float64 arithmetic, no MFMA (its internal order is not the host's).
//   * float32 sums in a stated order: column means / variances and a cluster's centre sum add rows in ascending row order (one
//     thread per column adds them one after the other), numpy's pairwise sum (pairwise_sum_dev) over D for the tolerance and the
//     relocation distances and over k for the squared shifts, _euclidean_dense_dense four terms per step (euclid_dd_dev).
// The two float64 running sums of k-means++ -- the cumulative sum over `closest` and the potential d @ ones -- add in index order:
// one lane per run does them (runs and sets side by side), no parallel scan.  The random numbers do not depend on the data (one
// draw for the first centre, 2 + int(log k) for each of the others): the host draws them with hmsg_kmeans.hip's MT19937 and
// uploads them once; every set starts from a fresh RandomState(seed).
//
// Shape.  n_sets * n_init independent fits are in flight together; fit f = set * n_init + run.  Nothing waits for another
// workgroup inside a kernel; the steps are cut at kernel boundaries:
//   k_km_colstats, k_km_tol, k_km_center, k_km_xx          once per call: mean / variance / tolerance / centring / |x|^2
//   k_km_pp_dist, k_km_pp_choose                           once per chosen centre (k of each)
//   k_km_estep, k_km_sums, k_km_finalize                   once per Lloyd iteration (max_iter of each are enqueued; a fit that
//                                                          has stopped says so in KmFit::phase and its workgroups return at once)
//   k_km_estep (final), k_km_inertia_rows, k_km_select     once per call
// The host synchronises once, when the outputs are complete.
//
// What bounds each kernel: k_km_estep and k_km_pp_dist are bound by float64 vector arithmetic (n * k * D, resp. n * trials * D
// multiply-adds; one row per thread, the k centres staged in LDS as float32 and taken four at a time: 32 float64 accumulators);
// k_km_sums by its walk over the labels (one workgroup per cluster, members added in row order); k_km_pp_choose and k_km_select by
// the latency of one lane's n dependent additions; the rest are small.
#include "hmsg_boundary.h"

#include <cmath>

// hmsg_kmeans.hip: the host Lloyd iteration (lloyd_iter with update_centers) and `count` consecutive random_sample() draws of
// numpy's RandomState(seed)
void hmsg_kmeans_host_lloyd(const float* X, int n, int D, int k, const float* centers_old, float* centers_new, float* weight, int* labels,
                            float* center_shift);
void hmsg_kmeans_draws(uint32_t seed, size_t count, double* out);

namespace {

constexpr int KM_T = 256;             // threads of a workgroup
constexpr int KM_LDS = 12288;         // floats of staged rows (48 KiB: 24 centres of 512)
constexpr int KM_TILE_ROWS = 256;     // staged rows at most (their norms sit in a second LDS array)
constexpr int KM_MAX_TRIALS = 16;     // 2 + int(log 65536) = 13
constexpr int KM_LAB_TILE = 1024;     // labels staged per step of k_km_sums

struct KmFit {
    int phase;                        // 0: iterating; 1: stopped by the tolerance (the extra E-step is due); 2: stopped with equal labels
    int n_iter;
    float pot;                        // k-means++: current_pot
    float inertia;
    int cand[KM_MAX_TRIALS];          // k-means++: the candidates of the centre being chosen (step 0: the first centre)
};

struct KmProb {
    int n_sets, n_init, D, Dp, k, T;  // Dp: row stride of the staged rows (D rounded up to 4); T: n_local_trials
    long long per_run;                // draws of one run: 1 + (k - 1) * T
    const long long* off;             // [n_sets + 1] rows of the sets, from 0
    const float* X;                   // [N][D] the rows the fits see (centred)
    const double* xx;                 // [N] |x|^2
    const float* tol;                 // [n_sets]
    const double* draws;              // [n_init][per_run]
    float *centers, *centers_new;     // [F][k][D]
    float *weight, *shift;            // [F][k]
    int *labels, *labels_old;         // [n_init * N]: fit (s, r) at off[s] * n_init + r * n_s
    float* closest;                   // [n_init * N], same layout: k-means++ closest distances; later per-row scratch
    float* cand_d;                    // [n_init * N * T]: fit (s, r), trial t at off[s] * n_init * T + (r * T + t) * n_s
    int *empties, *far;               // [F][k]
    KmFit* fit;                       // [F]
};

struct KmWhere {
    int s, r, n;
    long long row0, fo;               // first row of the set; offset of the fit in labels / closest
};
__device__ __forceinline__ KmWhere km_where(const KmProb& p, int f) {
    KmWhere w;
    w.s = f / p.n_init;
    w.r = f - w.s * p.n_init;
    w.row0 = p.off[w.s];
    w.n = (int)(p.off[w.s + 1] - w.row0);
    w.fo = w.row0 * p.n_init + (long long)w.r * w.n;
    return w;
}

// s + a * b with a, b float32 values held as float64: the product is exact, so the fused form gives the bits of a multiply
// followed by an add (the file is built with -ffp-contract=off; the fusion is asked for here, where it changes nothing)
__device__ __forceinline__ double dfma(double a, double b, double s) {
#ifdef HMSG_EMU_BUILD
    return s + a * b;
#else
    return __builtin_fma(a, b, s);
#endif
}
// correctly rounded float32 quotient and square root through float64 (53 >= 2 * 24 + 2 bits: the second rounding is innocuous)
__device__ __forceinline__ float div_f32(float a, float b) { return (float)((double)a / (double)b); }
__device__ __forceinline__ float sqrt_f32(float a) { return (float)sqrt((double)a); }

// dot_f64 of hmsg_kmeans.hip
__device__ __forceinline__ double dot8(const float* a, const float* b, int n) {
    double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int i = 0;
    for (; i + 8 <= n; i += 8)
#pragma unroll
        for (int q = 0; q < 8; ++q) s[q] = dfma((double)a[i + q], (double)b[i + q], s[q]);
    double r = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
    for (; i < n; ++i) r = dfma((double)a[i], (double)b[i], r);
    return r;
}
// dot_f64 of one row x (global memory) with C staged rows (LDS, stride Dp, 16-byte aligned)
template <int C>
__device__ __forceinline__ void dots(const float* __restrict__ x, const float* cs, int D, int Dp, double* out) {
    double s[C][8];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int q = 0; q < 8; ++q) s[c][q] = 0.0;
    const bool v4 = (D & 3) == 0;           // rows of X start on 16 bytes
    int i = 0;
    for (; i + 8 <= D; i += 8) {
        double xd[8];
        if (v4) {
            const float4 a = *(const float4*)(x + i), b = *(const float4*)(x + i + 4);
            xd[0] = (double)a.x, xd[1] = (double)a.y, xd[2] = (double)a.z, xd[3] = (double)a.w;
            xd[4] = (double)b.x, xd[5] = (double)b.y, xd[6] = (double)b.z, xd[7] = (double)b.w;
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) xd[q] = (double)x[i + q];
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float4 a = *(const float4*)(cs + (size_t)c * Dp + i), b = *(const float4*)(cs + (size_t)c * Dp + i + 4);
            s[c][0] = dfma(xd[0], (double)a.x, s[c][0]);
            s[c][1] = dfma(xd[1], (double)a.y, s[c][1]);
            s[c][2] = dfma(xd[2], (double)a.z, s[c][2]);
            s[c][3] = dfma(xd[3], (double)a.w, s[c][3]);
            s[c][4] = dfma(xd[4], (double)b.x, s[c][4]);
            s[c][5] = dfma(xd[5], (double)b.y, s[c][5]);
            s[c][6] = dfma(xd[6], (double)b.z, s[c][6]);
            s[c][7] = dfma(xd[7], (double)b.w, s[c][7]);
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) out[c] = ((s[c][0] + s[c][1]) + (s[c][2] + s[c][3])) + ((s[c][4] + s[c][5]) + (s[c][6] + s[c][7]));
    for (; i < D; ++i) {
        const double xv = (double)x[i];
#pragma unroll
        for (int c = 0; c < C; ++c) out[c] = dfma(xv, (double)cs[(size_t)c * Dp + i], out[c]);
    }
}

// pairwise_sum_f32 of hmsg_kmeans.hip over el(0) .. el(n - 1): the recursion as a loop with a stack of its own
template <typename F>
__device__ __forceinline__ float pairwise_leaf(F el, size_t off, size_t n) {
    if (n < 8) {
        float res = 0.f;
        for (size_t i = 0; i < n; ++i) res += el(off + i);
        return res;
    }
    float r[8];
    for (int q = 0; q < 8; ++q) r[q] = el(off + q);
    size_t i;
    for (i = 8; i < n - (n % 8); i += 8)
        for (int q = 0; q < 8; ++q) r[q] += el(off + i + q);
    float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += el(off + i);
    return res;
}
template <typename F>
__device__ float pairwise_sum_dev(F el, size_t n) {
    if (n <= 128) return pairwise_leaf(el, 0, n);
    struct Frame {
        size_t off, len;
        int stage;
        float left;
    };
    Frame st[40];                  // (a level halves the length: 2^24 elements are 18 levels)
    int sp = 0;
    st[0] = Frame{0, n, 0, 0.f};
    float ret = 0.f;
    while (sp >= 0) {
        Frame& f = st[sp];
        if (f.stage == 0) {
            if (f.len <= 128) {
                ret = pairwise_leaf(el, f.off, f.len);
                --sp;
                continue;
            }
            size_t n2 = f.len / 2;
            n2 -= n2 % 8;
            f.stage = 1;
            st[sp + 1] = Frame{f.off, n2, 0, 0.f};
            ++sp;
        } else if (f.stage == 1) {
            size_t n2 = f.len / 2;
            n2 -= n2 % 8;
            f.left = ret;
            f.stage = 2;
            st[sp + 1] = Frame{f.off + n2, f.len - n2, 0, 0.f};
            ++sp;
        } else {
            ret = f.left + ret;
            --sp;
        }
    }
    return ret;
}

// euclid_dd of hmsg_kmeans.hip
__device__ __forceinline__ float euclid_dd_dev(const float* a, const float* b, int n_features, bool squared) {
    const int n = n_features / 4, rem = n_features % 4;
    float result = 0.f;
    for (int i = 0; i < n; ++i) {
        result += ((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]) +
                   (a[3] - b[3]) * (a[3] - b[3]));
        a += 4;
        b += 4;
    }
    for (int i = 0; i < rem; ++i) result += (a[i] - b[i]) * (a[i] - b[i]);
    return squared ? result : sqrt_f32(result);
}

// ---------------------------------------------------------------------------------------------- once per call
// X.mean(axis = 0) and np.var(X, axis = 0) of every set as the host adds them: one thread per column, rows one after the other
static __global__ void __launch_bounds__(KM_T) k_km_colstats(const float* __restrict__ X, const long long* __restrict__ off, int D,
                                                             float* __restrict__ mean, float* __restrict__ var) {
    const int s = blockIdx.y, q = blockIdx.x * KM_T + threadIdx.x;
    if (q >= D) return;
    const long long r0 = off[s];
    const int n = (int)(off[s + 1] - r0);
    const float* x = X + (size_t)r0 * D + q;
    float m = 0.f;
    int i = 0;
    for (; i + 8 <= n; i += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = x[(size_t)(i + u) * D];
#pragma unroll
        for (int u = 0; u < 8; ++u) m += v[u];
    }
    for (; i < n; ++i) m += x[(size_t)i * D];
    m = div_f32(m, (float)n);
    float a = 0.f;
    for (i = 0; i + 8 <= n; i += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = x[(size_t)(i + u) * D];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const float t = v[u] - m;
            a += t * t;
        }
    }
    for (; i < n; ++i) {
        const float t = x[(size_t)i * D] - m;
        a += t * t;
    }
    mean[(size_t)s * D + q] = m;
    var[(size_t)s * D + q] = div_f32(a, (float)n);
}
// _tolerance: np.mean(var) * 1e-4
static __global__ void k_km_tol(const float* __restrict__ var, int D, float* __restrict__ tol) {
    if (threadIdx.x != 0) return;
    const float* v = var + (size_t)blockIdx.x * D;
    tol[blockIdx.x] = div_f32(pairwise_sum_dev([v](size_t i) { return v[i]; }, (size_t)D), (float)D) * 1e-4f;
}
// X -= X_mean
static __global__ void __launch_bounds__(KM_T) k_km_center(const float* __restrict__ X, const long long* __restrict__ off, int D,
                                                           const float* __restrict__ mean, float* __restrict__ Xc) {
    const int s = blockIdx.y;
    const long long r0 = off[s];
    const size_t cnt = (size_t)(off[s + 1] - r0) * D, e = (size_t)blockIdx.x * KM_T + threadIdx.x;
    if (e >= cnt) return;
    Xc[(size_t)r0 * D + e] = X[(size_t)r0 * D + e] - mean[(size_t)s * D + e % (size_t)D];
}
static __global__ void __launch_bounds__(KM_T) k_km_xx(const float* __restrict__ Xc, long long N, int D, double* __restrict__ xx) {
    const long long i = (long long)blockIdx.x * KM_T + threadIdx.x;
    if (i >= N) return;
    xx[i] = dot8(Xc + (size_t)i * D, Xc + (size_t)i * D, D);
}

// rows src(0) .. src(cnt - 1) into LDS, stride Dp
template <typename Src>
__device__ __forceinline__ void km_stage(float* cs, int cnt, int D, int Dp, Src src) {
    for (int j = 0; j < cnt; ++j) {
        const float* row = src(j);
        for (int q = threadIdx.x; q < D; q += KM_T) cs[(size_t)j * Dp + q] = row[q];
    }
}

// ---------------------------------------------------------------------------------------------- k-means++ (_kmeans_plusplus)
// step c: squared distances (euclid_sq_rows) of every row to the candidates of centre c, min'ed with `closest` (c > 0)
static __global__ void __launch_bounds__(KM_T) k_km_pp_dist(KmProb p, int c) {
    __shared__ __attribute__((aligned(16))) float cs[KM_LDS];
    __shared__ double yys[KM_MAX_TRIALS];
    const int f = blockIdx.y;
    const KmWhere w = km_where(p, f);
    if ((long long)blockIdx.x * KM_T >= w.n) return;
    const int row = blockIdx.x * KM_T + threadIdx.x, Tc = c == 0 ? 1 : p.T;
    const bool active = row < w.n;
    const float* x = p.X + (size_t)(w.row0 + (active ? row : 0)) * p.D;
    const float* Xs = p.X + (size_t)w.row0 * p.D;
    const int* cand = p.fit[f].cand;
    const int tile = min(KM_MAX_TRIALS, KM_LDS / p.Dp);
    const double xxi = p.xx[w.row0 + (active ? row : 0)];
    const float cl = (c > 0 && active) ? p.closest[w.fo + row] : 0.f;
    float* out = p.cand_d + (size_t)w.row0 * p.n_init * p.T + (size_t)w.r * p.T * w.n;
    for (int t0 = 0; t0 < Tc; t0 += tile) {
        const int cnt = min(tile, Tc - t0);
        __syncthreads();
        km_stage(cs, cnt, p.D, p.Dp, [&](int j) { return Xs + (size_t)cand[t0 + j] * p.D; });
        if ((int)threadIdx.x < cnt) yys[threadIdx.x] = p.xx[w.row0 + cand[t0 + threadIdx.x]];
        __syncthreads();
        if (!active) continue;
        for (int j = 0; j < cnt; ++j) {
            double dot;
            dots<1>(x, cs + (size_t)j * p.Dp, p.D, p.Dp, &dot);
            double d = -2.0 * dot;
            d += yys[j];
            d += xxi;
            float v = (float)d;
            v = v > 0.f ? v : 0.f;
            if (c > 0) v = v < cl ? v : cl;                       // np.minimum(closest, distance_to_candidates)
            out[(size_t)(t0 + j) * w.n + row] = v;
        }
    }
}
// step c: the potentials of the candidates (one lane each, in index order), the best of them becomes centre c; then the candidates
// of centre c + 1: searchsorted of rand * current_pot in the running sum of `closest` (one lane per candidate walks the same sum)
static __global__ void __launch_bounds__(KM_T) k_km_pp_choose(KmProb p, int c) {
    __shared__ float pot_s[KM_MAX_TRIALS];
    __shared__ int best_s;
    const int f = blockIdx.x, t = threadIdx.x;
    const KmWhere w = km_where(p, f);
    const int Tc = c == 0 ? 1 : p.T, n = w.n;
    KmFit& st = p.fit[f];
    const float* cd = p.cand_d + (size_t)w.row0 * p.n_init * p.T + (size_t)w.r * p.T * n;
    if (t < Tc) {
        const float* d = cd + (size_t)t * n;
        double s = 0.0;
        int i = 0;
        for (; i + 8 <= n; i += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = d[i + u];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += (double)v[u];
        }
        for (; i < n; ++i) s += (double)d[i];
        pot_s[t] = (float)s;
    }
    __syncthreads();
    if (t == 0) {
        int best = 0;
        for (int u = 1; u < Tc; ++u)
            if (pot_s[u] < pot_s[best]) best = u;                  // np.argmin: first minimum
        best_s = best;
    }
    __syncthreads();
    const int best = best_s, cb = st.cand[best];
    const float pot = pot_s[best];
    float* closest = p.closest + w.fo;
    for (int i = t; i < n; i += KM_T) closest[i] = cd[(size_t)best * n + i];
    const float* xb = p.X + (size_t)(w.row0 + cb) * p.D;
    float* ctr = p.centers + ((size_t)f * p.k + c) * p.D;
    for (int q = t; q < p.D; q += KM_T) ctr[q] = xb[q];
    __syncthreads();
    if (t == 0) st.pot = pot;
    if (c + 1 >= p.k || t >= p.T) return;
    const double rv = p.draws[(size_t)w.r * p.per_run + 1 + (size_t)c * p.T + t] * (double)pot;
    double acc = 0.0;                                             // stable_cumsum(closest)
    int id = n, i = 0;
    for (; i + 8 <= n; i += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = closest[i + u];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            acc += (double)v[u];
            if (id == n && !(acc < rv)) id = i + u;               // searchsorted (side left)
        }
    }
    for (; i < n; ++i) {
        acc += (double)closest[i];
        if (id == n && !(acc < rv)) id = i;
    }
    st.cand[t] = min(id, n - 1);
}

// ---------------------------------------------------------------------------------------------- Lloyd (lloyd_iter)
// E-step: one row per thread against the centres staged in LDS (their norms beside them), four centres at a time.  final_pass: the
// extra E-step of the fits that did not stop with equal labels.
static __global__ void __launch_bounds__(KM_T) k_km_estep(KmProb p, int final_pass) {
    __shared__ __attribute__((aligned(16))) float cs[KM_LDS];
    __shared__ float cn2s[KM_TILE_ROWS];
    const int f = blockIdx.y, phase = p.fit[f].phase;
    if (final_pass ? phase == 2 : phase != 0) return;
    const KmWhere w = km_where(p, f);
    if ((long long)blockIdx.x * KM_T >= w.n) return;
    const int row = blockIdx.x * KM_T + threadIdx.x;
    const bool active = row < w.n;
    const float* x = p.X + (size_t)(w.row0 + (active ? row : 0)) * p.D;
    const float* ctr = p.centers + (size_t)f * p.k * p.D;
    const int tile = min(KM_TILE_ROWS, KM_LDS / p.Dp);
    float min_d = 0.f;
    int label = 0;
    for (int j0 = 0; j0 < p.k; j0 += tile) {
        const int cnt = min(tile, p.k - j0);
        __syncthreads();
        km_stage(cs, cnt, p.D, p.Dp, [&](int j) { return ctr + (size_t)(j0 + j) * p.D; });
        __syncthreads();
        for (int j = threadIdx.x; j < cnt; j += KM_T) cn2s[j] = (float)dot8(cs + (size_t)j * p.Dp, cs + (size_t)j * p.Dp, p.D);
        __syncthreads();
        if (!active) continue;
        int j = 0;
        for (; j + 4 <= cnt; j += 4) {
            double dot[4];
            dots<4>(x, cs + (size_t)j * p.Dp, p.D, p.Dp, dot);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float d = (float)((double)cn2s[j + u] - 2.0 * dot[u]);
                if (j0 + j + u == 0 || d < min_d) {
                    min_d = d;
                    label = j0 + j + u;
                }
            }
        }
        for (; j < cnt; ++j) {
            double dot;
            dots<1>(x, cs + (size_t)j * p.Dp, p.D, p.Dp, &dot);
            const float d = (float)((double)cn2s[j] - 2.0 * dot);
            if (j0 + j == 0 || d < min_d) {
                min_d = d;
                label = j0 + j;
            }
        }
    }
    if (active) p.labels[w.fo + row] = label;
}
// centre sums and weights: one workgroup per (cluster, fit), one thread per column, the member rows added in ascending row order
static __global__ void __launch_bounds__(KM_T) k_km_sums(KmProb p) {
    __shared__ int lab[KM_LAB_TILE];
    const int f = blockIdx.y, j = blockIdx.x;
    if (p.fit[f].phase != 0) return;
    const KmWhere w = km_where(p, f);
    const int* labels = p.labels + w.fo;
    const float* Xs = p.X + (size_t)w.row0 * p.D;
    float* dst = p.centers_new + ((size_t)f * p.k + j) * p.D;
    float members = 0.f;
    for (int q0 = 0; q0 < p.D; q0 += 4 * KM_T) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int i0 = 0; i0 < w.n; i0 += KM_LAB_TILE) {
            const int m = min(KM_LAB_TILE, w.n - i0);
            __syncthreads();
            for (int i = threadIdx.x; i < m; i += KM_T) lab[i] = labels[i0 + i];
            __syncthreads();
            for (int i = 0; i < m; ++i) {
                if (lab[i] != j) continue;
                const float* x = Xs + (size_t)(i0 + i) * p.D;
                if (q0 == 0) members += 1.0f;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int q = q0 + u * KM_T + (int)threadIdx.x;
                    if (q < p.D) acc[u] += x[q];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int q = q0 + u * KM_T + (int)threadIdx.x;
            if (q < p.D) dst[q] = 0.f + acc[u];                   // (the chunk's sums are added to zeroed totals)
        }
    }
    if (threadIdx.x == 0) p.weight[(size_t)f * p.k + j] = 0.f + members;
}
// the rest of an iteration, one workgroup per fit: _relocate_empty_clusters_dense, _average_centers, _center_shift, then the stopping
// rules of _kmeans_single_lloyd.  `it` is the iteration's number (n_iter = it + 1 when the fit stops here).
static __global__ void __launch_bounds__(KM_T) k_km_finalize(KmProb p, int it) {
    __shared__ float red_v[KM_T];
    __shared__ int red_i[KM_T];
    __shared__ int sh_i[2];
    __shared__ float sh_f;
    const int f = blockIdx.x, t = threadIdx.x;
    KmFit& st = p.fit[f];
    if (st.phase != 0) return;
    const KmWhere w = km_where(p, f);
    const int n = w.n, D = p.D, k = p.k;
    const float* Xs = p.X + (size_t)w.row0 * D;
    float* c_old = p.centers + (size_t)f * k * D;
    float* c_new = p.centers_new + (size_t)f * k * D;
    float* weight = p.weight + (size_t)f * k;
    float* shift = p.shift + (size_t)f * k;
    int* labels = p.labels + w.fo;
    int* labels_old = p.labels_old + w.fo;
    int* empties = p.empties + (size_t)f * k;
    int* far = p.far + (size_t)f * k;
    float* dist = p.closest + w.fo;                               // (k-means++ is over: its array is this kernel's scratch)
    if (t == 0) {
        int ne = 0;
        for (int j = 0; j < k; ++j)
            if (weight[j] == 0.f) empties[ne++] = j;
        sh_i[0] = ne;
    }
    __syncthreads();
    const int n_empty = sh_i[0];
    if (n_empty > 0) {
        // distances = ((X - centers_old[labels]) ** 2).sum(axis = 1)
        float mx = 0.f;
        for (int i = t; i < n; i += KM_T) {
            const float* x = Xs + (size_t)i * D;
            const float* c = c_old + (size_t)labels[i] * D;
            const float d = pairwise_sum_dev(
                [x, c](size_t q) {
                    const float u = x[q] - c[q];
                    return u * u;
                },
                (size_t)D);
            dist[i] = d;
            mx = d > mx ? d : mx;
        }
        red_v[t] = mx;
        __syncthreads();
        if (t == 0) {
            float m = 0.f;
            for (int u = 0; u < KM_T; ++u) m = red_v[u] > m ? red_v[u] : m;
            sh_f = m;
        }
        __syncthreads();
        if (sh_f != 0.f) {
            // the n_empty farthest samples, farthest first, equal distances in ascending row order (the host's stable sort)
            for (int e = 0; e < n_empty && e < n; ++e) {
                float bv = -1.f;
                int bi = 0x7fffffff;
                for (int i = t; i < n; i += KM_T) {
                    const float v = dist[i];
                    if (v > bv) {
                        bv = v;
                        bi = i;
                    }
                }
                red_v[t] = bv;
                red_i[t] = bi;
                __syncthreads();
                if (t == 0) {
                    float v = red_v[0];
                    int b = red_i[0];
                    for (int u = 1; u < KM_T; ++u)
                        if (red_v[u] > v || (red_v[u] == v && red_i[u] < b)) {
                            v = red_v[u];
                            b = red_i[u];
                        }
                    if (b >= n) b = 0;                            // (only NaN distances are left: stay inside the arrays)
                    far[e] = b;
                    dist[b] = -2.f;                               // taken
                }
                __syncthreads();
            }
            const int ne = min(n_empty, n);
            for (int q = t; q < D; q += KM_T)
                for (int e = 0; e < ne; ++e) {
                    const int fr = far[e], nw = empties[e], old = labels[fr];
                    const float xv = Xs[(size_t)fr * D + q];
                    c_new[(size_t)old * D + q] -= xv;
                    c_new[(size_t)nw * D + q] = xv;
                }
            if (t == 0)
                for (int e = 0; e < ne; ++e) {
                    weight[empties[e]] = 1.0f;
                    weight[labels[far[e]]] -= 1.0f;
                }
            __syncthreads();
        }
    }
    // _average_centers (clusters in ascending order: an empty one copies the heaviest centre as it is at that moment)
    if (t == 0) {
        int am = 0;
        for (int j = 1; j < k; ++j)
            if (weight[j] > weight[am]) am = j;
        sh_i[1] = am;
    }
    __syncthreads();
    const int argmax_w = sh_i[1];
    for (int q = t; q < D; q += KM_T)
        for (int j = 0; j < k; ++j) {
            const float wj = weight[j];
            if (wj > 0.f) c_new[(size_t)j * D + q] *= div_f32(1.0f, wj);
            else c_new[(size_t)j * D + q] = c_new[(size_t)argmax_w * D + q];
        }
    __syncthreads();
    for (int j = t; j < k; j += KM_T) shift[j] = euclid_dd_dev(c_new + (size_t)j * D, c_old + (size_t)j * D, D, false);
    __syncthreads();
    for (size_t e = t; e < (size_t)k * D; e += KM_T) c_old[e] = c_new[e];          // centers, centers_new = centers_new, centers
    int differ = 0;
    for (int i = t; i < n; i += KM_T) differ |= labels[i] != labels_old[i];
    red_i[t] = differ;
    __syncthreads();
    if (t == 0) {
        int any = 0;
        for (int u = 0; u < KM_T; ++u) any |= red_i[u];
        int stop = 0;
        if (!any) {
            st.phase = 2;
            stop = 1;
        } else {
            const float s2 = pairwise_sum_dev([shift](size_t j) { return shift[j] * shift[j]; }, (size_t)k);
            if (s2 <= p.tol[w.s]) {
                st.phase = 1;
                stop = 1;
            }
        }
        if (stop) st.n_iter = it + 1;
        sh_i[0] = stop;
    }
    __syncthreads();
    if (sh_i[0]) return;
    for (int i = t; i < n; i += KM_T) labels_old[i] = labels[i];
}

// ---------------------------------------------------------------------------------------------- after the fits
// the terms of _inertia_dense, one row per thread (into the fits' scratch rows)
static __global__ void __launch_bounds__(KM_T) k_km_inertia_rows(KmProb p) {
    const int f = blockIdx.y;
    const KmWhere w = km_where(p, f);
    const int row = blockIdx.x * KM_T + threadIdx.x;
    if (row >= w.n) return;
    const int lab = p.labels[w.fo + row];
    p.closest[w.fo + row] = euclid_dd_dev(p.X + (size_t)(w.row0 + row) * p.D, p.centers + ((size_t)f * p.k + lab) * p.D, p.D, true);
}
// one workgroup per set: the inertia of its runs (one lane each, rows in order), the best run as KMeans.fit chooses it (a run wins
// with a smaller inertia unless it is the same clustering), then the outputs
static __global__ void __launch_bounds__(KM_T) k_km_select(KmProb p, const float* __restrict__ mean, int* __restrict__ first,
                                                           int32_t* __restrict__ out_labels, float* __restrict__ out_centers,
                                                           float* __restrict__ out_inertia, int32_t* __restrict__ out_n_iter) {
    __shared__ int sh_same;
    const int s = blockIdx.x, t = threadIdx.x;
    const KmWhere w0 = km_where(p, s * p.n_init);
    const int n = w0.n;
    for (int r = t; r < p.n_init; r += KM_T) {
        const float* term = p.closest + w0.fo + (size_t)r * n;
        float in = 0.f;
        int i = 0;
        for (; i + 8 <= n; i += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = term[i + u];
#pragma unroll
            for (int u = 0; u < 8; ++u) in += v[u];
        }
        for (; i < n; ++i) in += term[i];
        p.fit[s * p.n_init + r].inertia = in;
    }
    __syncthreads();
    int best = 0;
    int* fst = first + (size_t)s * p.k;
    for (int r = 1; r < p.n_init; ++r) {
        if (!(p.fit[s * p.n_init + r].inertia < p.fit[s * p.n_init + best].inertia)) continue;       // (uniform)
        // _is_same_clustering(labels of r, labels of best): every label of r maps to ONE label of best
        const int* a = p.labels + w0.fo + (size_t)r * n;
        const int* b = p.labels + w0.fo + (size_t)best * n;
        if (t == 0) sh_same = 1;
        for (int j = t; j < p.k; j += KM_T) fst[j] = 0x7fffffff;
        __syncthreads();
        for (int i = t; i < n; i += KM_T) atomicMin(&fst[a[i]], i);
        __syncthreads();
        for (int i = t; i < n; i += KM_T)
            if (b[i] != b[fst[a[i]]]) sh_same = 0;
        __syncthreads();
        if (!sh_same) best = r;
        __syncthreads();
    }
    const int fb = s * p.n_init + best;
    const int* lab = p.labels + w0.fo + (size_t)best * n;
    for (int i = t; i < n; i += KM_T) out_labels[w0.row0 + i] = lab[i];
    const float* c = p.centers + (size_t)fb * p.k * p.D;
    for (size_t e = t; e < (size_t)p.k * p.D; e += KM_T) out_centers[(size_t)s * p.k * p.D + e] = c[e] + mean[(size_t)s * p.D + e % (size_t)p.D];
    if (t == 0) {
        if (out_inertia) out_inertia[s] = p.fit[fb].inertia;
        if (out_n_iter) out_n_iter[s] = p.fit[fb].n_iter;
    }
}

// ---------------------------------------------------------------------------------------------- host side
struct KmScratch {
    DevBuf<long long> off;
    DevBuf<float> Xc, mean, var, tol, centers, centers_new, weight, shift, closest, cand_d;
    DevBuf<double> xx, draws;
    DevBuf<int> labels, labels_old, empties, far, first;
    DevBuf<KmFit> fit;
};

// the arrays every kernel sees; n_max: the largest set
KmProb km_problem(KmScratch& w, int n_sets, const std::vector<long long>& off, int D, int k, int n_init, int T, hipStream_t s) {
    const long long N = off.back();
    const size_t F = (size_t)n_sets * n_init;
    w.off.alloc(off.size());
    HIP_TRY(hipMemcpyAsync(w.off.p, off.data(), off.size() * sizeof(long long), hipMemcpyHostToDevice, s));
    w.centers.alloc(F * k * D);
    w.centers_new.alloc(F * k * D);
    w.weight.alloc(F * k);
    w.shift.alloc(F * k);
    w.labels.alloc((size_t)N * n_init);
    w.labels_old.alloc((size_t)N * n_init);
    w.closest.alloc((size_t)N * n_init);
    w.empties.alloc(F * k);
    w.far.alloc(F * k);
    w.fit.alloc(F);
    HIP_TRY(hipMemsetAsync(w.labels_old.p, 0xff, (size_t)N * n_init * sizeof(int), s));      // labels_old = -1
    KmProb p{};
    p.n_sets = n_sets, p.n_init = n_init, p.D = D, p.Dp = (D + 3) & ~3, p.k = k, p.T = T;
    p.per_run = 1 + (long long)(k - 1) * T;
    p.off = w.off.p;
    p.centers = w.centers.p, p.centers_new = w.centers_new.p, p.weight = w.weight.p, p.shift = w.shift.p;
    p.labels = w.labels.p, p.labels_old = w.labels_old.p, p.closest = w.closest.p;
    p.empties = w.empties.p, p.far = w.far.p, p.fit = w.fit.p;
    return p;
}

void km_lloyd_step(const KmProb& p, int n_max, int it, hipStream_t s) {
    const unsigned F = (unsigned)(p.n_sets * p.n_init);
    hipLaunchKernelGGL(k_km_estep, dim3(cdiv((size_t)n_max, KM_T), F), dim3(KM_T), 0, s, p, 0);
    hipLaunchKernelGGL(k_km_sums, dim3((unsigned)p.k, F), dim3(KM_T), 0, s, p);
    hipLaunchKernelGGL(k_km_finalize, dim3(F), dim3(KM_T), 0, s, p, it);
    HMSG_CHECK_LAUNCH();
}

void km_check_shape(int D, int k, int n_sets, int n_init) {
    HMSG_REQUIRE(((D + 3) & ~3) <= KM_LDS, HMSG_ERR_UNSUPPORTED, "hmsg_kmeans_batch: dim above " + std::to_string(KM_LDS));
    HMSG_REQUIRE((long long)n_sets * n_init <= 65535 && k <= 65536, HMSG_ERR_UNSUPPORTED, "hmsg_kmeans_batch: more than 65535 fits in one call");
}

}  // namespace

/* include/hmsg.h: hmsg_kmeans_batch */
extern "C" int hmsg_kmeans_batch(int32_t device_id, int32_t n_sets, const int64_t* set_off, const float* X_in, int32_t D, int32_t k, int32_t n_init,
                                 int32_t max_iter, uint32_t seed, int32_t* out_labels, float* out_centers, float* out_inertia, int32_t* out_n_iter) {
    if (n_sets < 0) return HMSG_ERR_INVALID;
    if (n_sets == 0) return HMSG_OK;
    if (!set_off || !X_in || D <= 0 || k <= 0 || k > 65536 || n_init <= 0 || max_iter <= 0 || !out_labels || !out_centers || set_off[0] != 0)
        return HMSG_ERR_INVALID;
    for (int s = 0; s < n_sets; ++s) {                             // hmsg_kmeans' rules, set by set, before anything is written
        const int64_t n = set_off[s + 1] - set_off[s];
        if (n <= 0 || n > (1 << 24) || k > n) return HMSG_ERR_INVALID;
    }
    return hmsg_boundary("hmsg_kmeans_batch", device_id, [&] {
        km_check_shape(D, k, n_sets, n_init);
        std::vector<long long> off((size_t)n_sets + 1);
        int n_max = 0;
        for (int s = 0; s <= n_sets; ++s) off[(size_t)s] = (long long)set_off[s];
        for (int s = 0; s < n_sets; ++s) n_max = std::max(n_max, (int)(off[(size_t)s + 1] - off[(size_t)s]));
        const long long N = off.back();
        const int T = 2 + (int)std::log((double)k);                // n_local_trials
        const size_t F = (size_t)n_sets * n_init;
        // the random numbers of one set (every set: a fresh RandomState(seed)); the first centre of every fit is
        // random_state.choice(n, p = 1 / n): searchsorted (side right) of the draw in the normalised running sum of float32(1 / n)
        const size_t per_run = 1 + (size_t)(k - 1) * T;
        std::vector<double> draws(per_run * n_init);
        hmsg_kmeans_draws(seed, draws.size(), draws.data());
        std::vector<KmFit> fits(F);
        {
            std::vector<double> cdf;
            for (int s = 0; s < n_sets; ++s) {
                const int n = (int)(off[(size_t)s + 1] - off[(size_t)s]);
                const double pr = (double)(1.0f / (float)n);
                cdf.resize((size_t)n);
                double run = 0.0;
                for (int i = 0; i < n; ++i) {
                    run += pr;
                    cdf[(size_t)i] = run;
                }
                for (int i = 0; i < n; ++i) cdf[(size_t)i] /= run;
                for (int r = 0; r < n_init; ++r) {
                    KmFit& f = fits[(size_t)s * n_init + r];
                    memset(&f, 0, sizeof f);
                    f.n_iter = max_iter;
                    const int id = (int)(std::upper_bound(cdf.begin(), cdf.end(), draws[(size_t)r * per_run]) - cdf.begin());
                    f.cand[0] = std::min(id, n - 1);
                }
            }
        }
        ScopedStream s(hipStreamNonBlocking);
        KmScratch w;
        DevBuf<float> x_own, c_own, in_own;
        DevBuf<int32_t> l_own, it_own;
        try {
            const float* X = stage_in(x_own, X_in, (size_t)N * D, s, Up::bounce);
            int32_t* d_labels = stage_out(l_own, out_labels, (size_t)N);
            float* d_centers = stage_out(c_own, out_centers, (size_t)n_sets * k * D);
            float* d_inertia = stage_out(in_own, out_inertia, (size_t)n_sets);
            int32_t* d_n_iter = stage_out(it_own, out_n_iter, (size_t)n_sets);
            KmProb p = km_problem(w, n_sets, off, D, k, n_init, T, s);
            w.Xc.alloc((size_t)N * D);
            w.xx.alloc((size_t)N);
            w.mean.alloc((size_t)n_sets * D);
            w.var.alloc((size_t)n_sets * D);
            w.tol.alloc((size_t)n_sets);
            w.cand_d.alloc((size_t)N * n_init * T);
            w.draws.alloc(draws.size());
            w.first.alloc((size_t)n_sets * k);
            HIP_TRY(hipMemcpyAsync(w.draws.p, draws.data(), draws.size() * sizeof(double), hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(w.fit.p, fits.data(), F * sizeof(KmFit), hipMemcpyHostToDevice, s));
            p.X = w.Xc.p, p.xx = w.xx.p, p.tol = w.tol.p, p.draws = w.draws.p, p.cand_d = w.cand_d.p;
            // KMeans.fit: the tolerance from the data as given, then X -= X.mean(axis = 0)
            hipLaunchKernelGGL(k_km_colstats, dim3(cdiv((size_t)D, KM_T), (unsigned)n_sets), dim3(KM_T), 0, s, X, p.off, D, w.mean.p, w.var.p);
            hipLaunchKernelGGL(k_km_tol, dim3((unsigned)n_sets), dim3(64), 0, s, w.var.p, D, w.tol.p);
            hipLaunchKernelGGL(k_km_center, dim3(cdiv((size_t)n_max * D, KM_T), (unsigned)n_sets), dim3(KM_T), 0, s, X, p.off, D, w.mean.p, w.Xc.p);
            hipLaunchKernelGGL(k_km_xx, dim3(cdiv((size_t)N, KM_T)), dim3(KM_T), 0, s, w.Xc.p, N, D, w.xx.p);
            HMSG_CHECK_LAUNCH();
            for (int c = 0; c < k; ++c) {
                hipLaunchKernelGGL(k_km_pp_dist, dim3(cdiv((size_t)n_max, KM_T), (unsigned)F), dim3(KM_T), 0, s, p, c);
                hipLaunchKernelGGL(k_km_pp_choose, dim3((unsigned)F), dim3(KM_T), 0, s, p, c);
            }
            HMSG_CHECK_LAUNCH();
            for (int it = 0; it < max_iter; ++it) km_lloyd_step(p, n_max, it, s);
            hipLaunchKernelGGL(k_km_estep, dim3(cdiv((size_t)n_max, KM_T), (unsigned)F), dim3(KM_T), 0, s, p, 1);
            hipLaunchKernelGGL(k_km_inertia_rows, dim3(cdiv((size_t)n_max, KM_T), (unsigned)F), dim3(KM_T), 0, s, p);
            hipLaunchKernelGGL(k_km_select, dim3((unsigned)n_sets), dim3(KM_T), 0, s, p, w.mean.p, w.first.p, d_labels, d_centers, d_inertia, d_n_iter);
            HMSG_CHECK_LAUNCH();
            unstage_out(out_labels, d_labels, (size_t)N, s);
            unstage_out(out_centers, d_centers, (size_t)n_sets * k * D, s);
            if (out_inertia) unstage_out(out_inertia, d_inertia, (size_t)n_sets, s);
            if (out_n_iter) unstage_out(out_n_iter, d_n_iter, (size_t)n_sets, s);
            HIP_TRY(hipStreamSynchronize(s));
        } catch (...) {
            (void)hipStreamSynchronize(s);                         // (the scratch goes back to the allocator: nothing may still run on it)
            throw;
        }
    });
}

/* include/hmsg_test.h: hmsg_test_kmeans_lloyd */
extern "C" int hmsg_test_kmeans_lloyd(int32_t on_device, int32_t device_id, const float* X, int64_t n64, int32_t D, int32_t k, const float* centers_in,
                                      int32_t* labels, float* centers_out, float* shift) {
    if (!X || n64 <= 0 || n64 > (1 << 24) || D <= 0 || k <= 0 || k > n64 || k > 65536 || !centers_in || !labels || !centers_out || !shift)
        return HMSG_ERR_INVALID;
    const int n = (int)n64;
    if (!on_device)
        return hmsg_boundary("hmsg_test_kmeans_lloyd", -1, [&] {
            std::vector<float> weight((size_t)k, 0.f);
            hmsg_kmeans_host_lloyd(X, n, D, k, centers_in, centers_out, weight.data(), labels, shift);
        });
    return hmsg_boundary("hmsg_test_kmeans_lloyd", device_id, [&] {
        km_check_shape(D, k, 1, 1);
        ScopedStream s(hipStreamNonBlocking);
        KmScratch w;
        const std::vector<long long> off{0, (long long)n};
        try {
            KmProb p = km_problem(w, 1, off, D, k, 1, 1, s);
            w.Xc.alloc((size_t)n * D);
            w.tol.alloc(1);
            copy_in(w.Xc.p, X, (size_t)n * D * 4, s, Up::bounce);
            copy_in(w.centers.p, centers_in, (size_t)k * D * 4, s, Up::direct);
            KmFit f;
            memset(&f, 0, sizeof f);
            HIP_TRY(hipMemcpyAsync(w.fit.p, &f, sizeof f, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemsetAsync(w.tol.p, 0, sizeof(float), s));
            p.X = w.Xc.p, p.tol = w.tol.p;
            km_lloyd_step(p, n, 0, s);
            copy_out(labels, w.labels.p, (size_t)n * 4, s);
            copy_out(centers_out, w.centers.p, (size_t)k * D * 4, s);
            copy_out(shift, w.shift.p, (size_t)k * 4, s);
            HIP_TRY(hipStreamSynchronize(s));
        } catch (...) {
            (void)hipStreamSynchronize(s);
            throw;
        }
    });
}
