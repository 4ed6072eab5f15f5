// Evaluation of a graph against ground truth (memory/hmsg/eval/hm3dsem_evaluator.py): the device part and the assignment.
//
//   hmsg_cloud_set_overlaps     find_overlapping_ratio_faiss (utils/graph_utils.py:620-662) for pairs (a, b) of clouds taken from
//                               two SETS, for any radius: counts[p] = (points of A[a] with a point of B[b] whose float32 squared
//                               distance is < (float)(radius * radius), the same the other way round).  evaluate_objects asks it for
//                               every predicted / ground-truth pair whose boxes intersect (radius 0.02), evaluate_rooms for every
//                               room pair (0.05); ground-truth clouds are mesh samples of 10^4 .. 10^5 points, so the exhaustive
//                               scan of hmsg_pair_overlaps (hmsg_objmerge.hip, O(n_A n_B) per pair) is out of the question.
//   hmsg_cloud_set_overlaps_kd  the same probe with find_intersection_share's comparison (utils/graph_utils.py:160-189: a float64
//                               cKDTree query with distance_upper_bound = radius): float64 (dx*dx + dy*dy) + dz*dz < radius * radius,
//                               strict -- the 3-D form of hmsg_room_share_on (hmsg_merge.hip).
//   hmsg_eval_object_matrices   the matrix loop of evaluate_objects (hm3dsem_evaluator.py:429-458): predicted boxes, get_3d_iou, and the
//                               overlap of the pairs with iou > 0 through the counter above.
//   hmsg_lsap                   scipy.optimize.linear_sum_assignment (hmsg_lsap_host.h).
//   hmsg_eval_rooms             the three matrices of evaluate_rooms (:265-341); described where it starts, further down.
//   hmsg_eval_semantic_ranks    the ranks behind object_semantics_eval_tp_auc (:557-589); likewise.
//   hmsg_eval_floors, hmsg_eval_metrics_from_matrix, hmsg_eval_counts_at, hmsg_eval_hydra_means, hmsg_eval_top_k
//                               the numbers behind the matrices, float64 on the host (hmsg_eval_metrics_host.h).
//   (hmsg_graph_evaluate, which composes them for a graph, is in hmsg_scene_graph.hip beside the graph object.)
//
// The probe.  One cell lattice for both sets: origin at the lower corner of all points, cell side from the reach exactly as the
// merge's grids choose it (merger_set_reach, hmsg_merge.hip: reach = radius, or sqrt(radius^2 + E) in faiss's BLAS form, E that
// form's error bound at the scene's coordinates; cell = reach (1 + 1e-3) + 2e-3), so a witness of a query point lies in one of the
// 27 cells around the query's.  Each side is sorted ONCE by (cloud, cell key), cell key = (cz NY + cy) NX + cx (hmsg_sort.hip, stable;
// a CSR cloud keeps its range, sorted by key inside).  A work item is (pair, direction, chunk of 256 query points); a lane takes one
// query point, and for each of the up to 9 (cy, cz) rows around its cell -- the three cells of a row are neighbours in key order --
// finds the row's first point by binary search in the target cloud's key range, walks to the row's last and leaves at the first
// witness.  Rows outside the target cloud's cell box are not searched.  A wave adds its ballot's popcount with one integer atomic:
// no floating-point atomics, every run gives the same counts.
//
// Bound: per query point <= 9 searches of log2(n_target) steps plus the points of 27 cells, against n_target distance
// evaluations of the exhaustive scan.
#include "hmsg_boundary.h"
#include "hmsg_cloudops.h"
#include "hmsg_eval_metrics_host.h"
#include "hmsg_lsap_host.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <deque>
#include <map>
#include <vector>

void hmsg_pair_overlaps(hmsg_ctx* h, const double* points, const long long* start, const int* count, int n_pairs, const int* pa, const int* pb,
                        double radius, double* overlap, unsigned* counts_out);

namespace {

enum { EV_DIRECT = 0, EV_BLAS = 1, EV_KD = 2 };

struct EvGrid {
    double o[3], cell;
    int n[3], pad;
};
struct EvSideDev {           // one set, sorted by (cloud, cell key)
    const void* pts;         // float4 [N] (x, y, z, |p|^2 as hmsg.h states it) | double [N][3] in the kd mode
    const unsigned long long* key;
    const int* cbox;         // [clouds][6]: cell box of every cloud (min xyz, max xyz; min > max: an empty cloud)
};
struct EvTask {              // count the points of cloud qc (set qside) that have a witness in cloud tc (the other set)
    long long q0, t0;        // first points in the sorted arrays
    int nq, nt;
    int qc, tc;
    unsigned blk0;           // first workgroup of the task: ceil(nq / 256) of them, at least one
    int qside;
};

// order-preserving map of a double onto u64 (for integer min / max atomics)
__host__ __device__ inline unsigned long long ev_enc(long long bits) {
    const unsigned long long u = (unsigned long long)bits;
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
inline double ev_dec(unsigned long long e) {
    const unsigned long long u = (e >> 63) ? (e & 0x7fffffffffffffffull) : ~e;
    double d;
    memcpy(&d, &u, 8);
    return d;
}
// the coordinate a mode works on: the float32 cast of the reference's `astype(np.float32)`, or the float64 itself
template <bool KD>
__device__ __forceinline__ double ev_coord(double v) { return KD ? v : (double)(float)v; }

template <bool KD>
__global__ void __launch_bounds__(256) k_ev_bounds(const double* __restrict__ pts, long long n, unsigned long long* __restrict__ box) {
    unsigned long long mn[3] = {~0ull, ~0ull, ~0ull}, mx[3] = {0ull, 0ull, 0ull};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        for (int a = 0; a < 3; ++a) {
            const unsigned long long e = ev_enc(__double_as_longlong(ev_coord<KD>(pts[i * 3 + a])));
            mn[a] = e < mn[a] ? e : mn[a];
            mx[a] = e > mx[a] ? e : mx[a];
        }
    for (int a = 0; a < 3; ++a) {
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long pmn = __shfl_xor(mn[a], o), pmx = __shfl_xor(mx[a], o);
            mn[a] = pmn < mn[a] ? pmn : mn[a];
            mx[a] = pmx > mx[a] ? pmx : mx[a];
        }
        if ((threadIdx.x & 63) == 0) {
            atomicMin(&box[a], mn[a]);
            atomicMax(&box[3 + a], mx[a]);
        }
    }
}

// per point: cloud, cell key (first sort key = its low 32 bits, value = the point's index); per cloud: its cell box
template <bool KD>
__global__ void __launch_bounds__(256) k_ev_cells(const double* __restrict__ pts, long long n, const long long* __restrict__ off, int nclouds,
                                                  EvGrid g, unsigned long long* __restrict__ ck, unsigned* __restrict__ cl,
                                                  unsigned* __restrict__ keys, unsigned long long* __restrict__ vals, int* __restrict__ cbox) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < n;
    int c[3] = {0, 0, 0}, cloud = 0;
    if (live) {
        int lo = 0, hi = nclouds - 1;                   // the last cloud that starts at or before i (it is not empty)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (off[mid] <= i) lo = mid; else hi = mid - 1;
        }
        cloud = lo;
        for (int a = 0; a < 3; ++a) {
            const int k = (int)floor((ev_coord<KD>(pts[i * 3 + a]) - g.o[a]) / g.cell);
            c[a] = min(max(k, 0), g.n[a] - 1);
        }
        const unsigned long long key = ((unsigned long long)c[2] * (unsigned long long)g.n[1] + (unsigned long long)c[1]) * (unsigned long long)g.n[0] +
                                       (unsigned long long)c[0];
        ck[i] = key;
        cl[i] = (unsigned)cloud;
        keys[i] = (unsigned)key;
        vals[i] = (unsigned long long)i;
    }
    // the cell box: a wave that lies inside one cloud (nearly all do) reduces first
    const int cloud0 = __shfl(cloud, 0);
    if (__all(live && cloud == cloud0)) {
        for (int a = 0; a < 3; ++a) {
            int mn = c[a], mx = c[a];
            for (int o = 32; o > 0; o >>= 1) {
                mn = min(mn, __shfl_xor(mn, o));
                mx = max(mx, __shfl_xor(mx, o));
            }
            if ((threadIdx.x & 63) == 0) {
                atomicMin(&cbox[(size_t)cloud * 6 + a], mn);
                atomicMax(&cbox[(size_t)cloud * 6 + 3 + a], mx);
            }
        }
    } else if (live) {
        for (int a = 0; a < 3; ++a) {
            atomicMin(&cbox[(size_t)cloud * 6 + a], c[a]);
            atomicMax(&cbox[(size_t)cloud * 6 + 3 + a], c[a]);
        }
    }
}

// the key of a later sort pass, read through the permutation so far: the cell key's high half, or the cloud
__global__ void __launch_bounds__(256) k_ev_rekey(const unsigned long long* __restrict__ vals, long long n, const unsigned long long* __restrict__ ck,
                                                  const unsigned* __restrict__ cl, int by_cloud, unsigned* __restrict__ keys) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const unsigned long long v = vals[j];
    keys[j] = by_cloud ? cl[v] : (unsigned)(ck[v] >> 32);
}

__device__ __forceinline__ float ev_norm2(float a, float b, float c) { return __fadd_rn(__fadd_rn(__fmul_rn(a, a), __fmul_rn(b, b)), __fmul_rn(c, c)); }

template <bool KD>
__global__ void __launch_bounds__(256) k_ev_gather(const double* __restrict__ pts, const unsigned long long* __restrict__ vals, long long n,
                                                   const unsigned long long* __restrict__ ck, unsigned long long* __restrict__ skey,
                                                   void* __restrict__ spts) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const unsigned long long v = vals[j];
    skey[j] = ck[v];
    const double* p = pts + v * 3;
    if (KD) {
        double* o = (double*)spts + j * 3;
        o[0] = p[0], o[1] = p[1], o[2] = p[2];
    } else {
        const float x = (float)p[0], y = (float)p[1], z = (float)p[2];
        ((float4*)spts)[j] = make_float4(x, y, z, ev_norm2(x, y, z));
    }
}

// MODE EV_DIRECT: (dx*dx + dy*dy) + dz*dz; EV_BLAS: a query cloud of 20 or more points in faiss's expanded form (hmsg.h), a smaller
// one direct; EV_KD: float64.
template <int MODE>
__global__ void __launch_bounds__(256) k_ev_probe(EvSideDev sa, EvSideDev sb, const EvTask* __restrict__ tasks, int ntasks, EvGrid g, float r2f,
                                                  double r2d, unsigned* __restrict__ counts) {
    int lo = 0, hi = ntasks - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tasks[mid].blk0 <= blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const EvTask t = tasks[lo];
    const EvSideDev& Q = t.qside ? sb : sa;
    const EvSideDev& T = t.qside ? sa : sb;
    const int i = (int)(blockIdx.x - t.blk0) * 256 + (int)threadIdx.x;
    bool hit = false;
    if (i < t.nq && t.nt > 0) {
        const int* tb = T.cbox + (size_t)t.tc * 6;
        const unsigned long long NX = (unsigned long long)g.n[0], NY = (unsigned long long)g.n[1];
        const unsigned long long key = Q.key[t.q0 + i];
        const int cx = (int)(key % NX), cy = (int)((key / NX) % NY), cz = (int)(key / (NX * NY));
        const int x0 = max(cx - 1, tb[0]), x1 = min(cx + 1, tb[3]);
        float xf = 0.f, yf = 0.f, zf = 0.f, nf = 0.f;
        double xd = 0.0, yd = 0.0, zd = 0.0;
        if (MODE == EV_KD) {
            const double* p = (const double*)Q.pts + (size_t)(t.q0 + i) * 3;
            xd = p[0], yd = p[1], zd = p[2];
        } else {
            const float4 p = ((const float4*)Q.pts)[t.q0 + i];
            xf = p.x, yf = p.y, zf = p.z, nf = p.w;
        }
        const bool blas = MODE == EV_BLAS && t.nq >= 20;
        const unsigned long long* tk = T.key + t.t0;
        if (x0 <= x1)
            for (int rz = 0; rz < 3 && !hit; ++rz) {
                const int zz = cz + (rz == 0 ? 0 : (rz == 1 ? -1 : 1));         // the query's own row first
                if (zz < tb[2] || zz > tb[5]) continue;
                for (int ry = 0; ry < 3 && !hit; ++ry) {
                    const int yy = cy + (ry == 0 ? 0 : (ry == 1 ? -1 : 1));
                    if (yy < tb[1] || yy > tb[4]) continue;
                    const unsigned long long kb = ((unsigned long long)zz * NY + (unsigned long long)yy) * NX;
                    const unsigned long long klo = kb + (unsigned long long)x0, khi = kb + (unsigned long long)x1;
                    int a = 0, b = t.nt;                                       // first point with key >= klo
                    while (a < b) {
                        const int mid = (int)(((unsigned)a + (unsigned)b) >> 1);
                        if (tk[mid] < klo) a = mid + 1; else b = mid;
                    }
                    for (int k = a; k < t.nt && tk[k] <= khi; ++k) {
                        if (MODE == EV_KD) {
                            const double* q = (const double*)T.pts + (size_t)(t.t0 + k) * 3;
                            const double dx = __dsub_rn(q[0], xd), dy = __dsub_rn(q[1], yd), dz = __dsub_rn(q[2], zd);
                            hit = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz)) < r2d;
                        } else {
                            const float4 q = ((const float4*)T.pts)[t.t0 + k];
                            float d2;
                            if (blas) {
                                const float ip = __fmaf_rn(zf, q.z, __fmaf_rn(yf, q.y, __fmul_rn(xf, q.x)));
                                d2 = __fsub_rn(__fadd_rn(nf, q.w), __fmul_rn(2.0f, ip));
                                d2 = d2 < 0.f ? 0.f : d2;
                            } else {
                                const float dx = __fsub_rn(xf, q.x), dy = __fsub_rn(yf, q.y), dz = __fsub_rn(zf, q.z);
                                d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
                            }
                            hit = d2 < r2f;
                        }
                        if (hit) break;
                    }
                }
            }
    }
    const unsigned long long m = __ballot(hit);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&counts[lo], (unsigned)__popcll(m));
}

struct EvSide {
    int nclouds = 0;
    long long N = 0;
    std::vector<long long> off;
    DevBuf<double> up;
    const double* dpts = nullptr;
    DevBuf<long long> doff;
    DevBuf<unsigned long long> ck, skey;
    DevBuf<unsigned> cl;
    DevBuf<int> cbox;
    DevBuf<unsigned char> spts;
    EvSideDev dev() const { return EvSideDev{spts.p, skey.p, cbox.p}; }
};

void ev_read_side(EvSide& S, const char* which, int32_t n, const double* pts, const int64_t* off) {
    HMSG_REQUIRE(n >= 0 && off, HMSG_ERR_INVALID, std::string("hmsg_cloud_set_overlaps: set ") + which + ": no offsets");
    S.nclouds = n;
    S.off.resize((size_t)n + 1);
    read_in(S.off.data(), off, ((size_t)n + 1) * 8);
    HMSG_REQUIRE(S.off[0] == 0, HMSG_ERR_INVALID, std::string("hmsg_cloud_set_overlaps: set ") + which + ": offsets do not start at 0");
    for (int c = 0; c < n; ++c) {
        HMSG_REQUIRE(S.off[(size_t)c + 1] >= S.off[(size_t)c], HMSG_ERR_INVALID,
                     std::string("hmsg_cloud_set_overlaps: set ") + which + ": offsets decrease at cloud " + std::to_string(c));
        HMSG_REQUIRE(S.off[(size_t)c + 1] - S.off[(size_t)c] < (1ll << 31), HMSG_ERR_UNSUPPORTED,
                     std::string("hmsg_cloud_set_overlaps: set ") + which + ": a cloud of 2^31 points or more");
    }
    S.N = S.off[(size_t)n];
    HMSG_REQUIRE(S.N < (1ll << 32), HMSG_ERR_UNSUPPORTED, std::string("hmsg_cloud_set_overlaps: set ") + which + ": 2^32 points or more");
    HMSG_REQUIRE(S.N == 0 || pts, HMSG_ERR_INVALID, std::string("hmsg_cloud_set_overlaps: set ") + which + ": no points");
}

template <bool KD>
void ev_sort_side(hmsg_ctx* h, EvSide& S, const EvGrid& g, int key_bits) {
    hipStream_t s = h->stream;
    const size_t N = (size_t)S.N;
    const unsigned nblk = cdiv(N, 256);
    std::vector<int> init((size_t)S.nclouds * 6);
    for (int c = 0; c < S.nclouds; ++c)
        for (int a = 0; a < 6; ++a) init[(size_t)c * 6 + a] = a < 3 ? INT_MAX : INT_MIN;
    S.cbox.alloc(init.size());
    if (!init.empty()) HIP_TRY(hipMemcpyAsync(S.cbox.p, init.data(), init.size() * 4, hipMemcpyHostToDevice, s));
    S.doff.alloc(S.off.size());
    HIP_TRY(hipMemcpyAsync(S.doff.p, S.off.data(), S.off.size() * 8, hipMemcpyHostToDevice, s));
    S.ck.alloc(N);
    S.cl.alloc(N);
    S.skey.alloc(N);
    S.spts.alloc(N * (KD ? 24 : 16));
    if (N) {
        SortBufs sb;
        sb.keys.alloc(N);
        sb.vals.alloc(N);
        {
            ProfScope ps(h->prof, s, "k_ev_cells", (double)N * (24 + 8 + 4 + 4 + 8));
            hipLaunchKernelGGL(k_ev_cells<KD>, dim3(nblk), dim3(256), 0, s, S.dpts, (long long)N, (const long long*)S.doff.p, S.nclouds, g, S.ck.p,
                               S.cl.p, sb.keys.p, sb.vals.p, S.cbox.p);
            HMSG_CHECK_LAUNCH();
        }
        // stable passes, least significant key first: cell key (low half, high half), then the cloud
        auto pass = [&](int bits) {
            hmsg_sort_pairs(sb, N, bits, s);
            if (sb.res_keys != sb.keys.p) {
                sb.keys.swap(sb.keys_alt);
                sb.vals.swap(sb.vals_alt);
            }
        };
        auto rekey = [&](int by_cloud) {
            hipLaunchKernelGGL(k_ev_rekey, dim3(nblk), dim3(256), 0, s, (const unsigned long long*)sb.vals.p, (long long)N,
                               (const unsigned long long*)S.ck.p, (const unsigned*)S.cl.p, by_cloud, sb.keys.p);
            HMSG_CHECK_LAUNCH();
        };
        pass(std::min(key_bits, 32));
        if (key_bits > 32) {
            rekey(0);
            pass(key_bits - 32);
        }
        if (S.nclouds > 1) {
            rekey(1);
            pass(bits_for((unsigned long long)S.nclouds));
        }
        ProfScope ps(h->prof, s, "k_ev_gather", (double)N * (8 + 8 + 24 + 8 + (KD ? 24 : 16)));
        hipLaunchKernelGGL(k_ev_gather<KD>, dim3(nblk), dim3(256), 0, s, S.dpts, (const unsigned long long*)sb.vals.p, (long long)N,
                           (const unsigned long long*)S.ck.p, S.skey.p, (void*)S.spts.p);
        HMSG_CHECK_LAUNCH();
        HIP_TRY(hipStreamSynchronize(s));               // (the sort's buffers go back to the cache here)
    }
}

template <bool KD>
void ev_bounds(hmsg_ctx* h, const EvSide* sides, int nsides, double* lo, double* hi) {
    hipStream_t s = h->stream;
    DevBuf<unsigned long long> box;
    box.alloc(6);
    const unsigned long long init[6] = {~0ull, ~0ull, ~0ull, 0ull, 0ull, 0ull};
    HIP_TRY(hipMemcpyAsync(box.p, init, sizeof(init), hipMemcpyHostToDevice, s));
    for (int k = 0; k < nsides; ++k)
        if (sides[k].N) {
            const unsigned nblk = std::min<unsigned>(cdiv((size_t)sides[k].N, 256), 1024u);
            hipLaunchKernelGGL(k_ev_bounds<KD>, dim3(nblk), dim3(256), 0, s, sides[k].dpts, sides[k].N, box.p);
            HMSG_CHECK_LAUNCH();
        }
    unsigned long long got[6];
    HIP_TRY(hipMemcpyAsync(got, box.p, sizeof(got), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int a = 0; a < 3; ++a) {
        lo[a] = ev_dec(got[a]);
        hi[a] = ev_dec(got[3 + a]);
        HMSG_REQUIRE(std::isfinite(lo[a]) && std::isfinite(hi[a]), HMSG_ERR_INVALID, "hmsg_cloud_set_overlaps: a coordinate is not finite");
    }
}

// mode: EV_DIRECT / EV_BLAS (by the handle's overlap_distance_form) or EV_KD
void ev_cloud_set_overlaps(hmsg_ctx* h, int mode, int32_t nA, const double* ptsA, const int64_t* offA, int32_t nB, const double* ptsB,
                           const int64_t* offB, int64_t n_pairs, const int32_t* pairs, double radius, uint32_t* counts) {
    hipStream_t s = h->stream;
    HMSG_REQUIRE(n_pairs >= 0 && (n_pairs == 0 || (pairs && counts)), HMSG_ERR_INVALID, "hmsg_cloud_set_overlaps: no pairs / counts array");
    HMSG_REQUIRE(std::isfinite(radius) && radius > 0.0, HMSG_ERR_INVALID, "hmsg_cloud_set_overlaps: the radius must be positive");
    HMSG_REQUIRE(n_pairs < (1ll << 30), HMSG_ERR_UNSUPPORTED, "hmsg_cloud_set_overlaps: 2^30 pairs or more");
    // everything the host can check is checked before a kernel runs or `counts` is written
    EvSide side[2];
    ev_read_side(side[0], "A", nA, ptsA, offA);
    const bool same = ptsA == ptsB && offA == offB && nA == nB;     // one set against itself: sorted once
    if (!same) ev_read_side(side[1], "B", nB, ptsB, offB);
    EvSide& SA = side[0];
    EvSide& SB = same ? side[0] : side[1];
    std::vector<int32_t> hp((size_t)n_pairs * 2);
    if (n_pairs) read_in(hp.data(), pairs, hp.size() * 4);
    std::vector<EvTask> tasks;
    tasks.reserve(hp.size());
    unsigned long long nblk = 0;
    for (int64_t p = 0; p < n_pairs; ++p) {
        const int a = hp[(size_t)p * 2], b = hp[(size_t)p * 2 + 1];
        HMSG_REQUIRE(a >= 0 && a < nA && b >= 0 && b < nB, HMSG_ERR_INVALID,
                     "hmsg_cloud_set_overlaps: pair " + std::to_string(p) + " names a cloud that does not exist");
        const long long a0 = SA.off[(size_t)a], b0 = SB.off[(size_t)b];
        const int na = (int)(SA.off[(size_t)a + 1] - a0), nb = (int)(SB.off[(size_t)b + 1] - b0);
        tasks.push_back(EvTask{a0, b0, na, nb, a, b, (unsigned)nblk, 0});
        nblk += (unsigned long long)std::max(1, (na + 255) / 256);
        tasks.push_back(EvTask{b0, a0, nb, na, b, a, (unsigned)nblk, 1});
        nblk += (unsigned long long)std::max(1, (nb + 255) / 256);
    }
    HMSG_REQUIRE(nblk < (1ull << 31), HMSG_ERR_UNSUPPORTED, "hmsg_cloud_set_overlaps: more than 2^31 chunks of 256 query points; split the pair list");
    if (n_pairs == 0) return;
    DevBuf<uint32_t> own_counts;
    uint32_t* dcounts = stage_out(own_counts, counts, tasks.size());
    HIP_TRY(hipMemsetAsync(dcounts, 0, tasks.size() * 4, s));
    if (SA.N > 0 && SB.N > 0) {
        SA.dpts = stage_in(SA.up, ptsA, (size_t)SA.N * 3, s, Up::bounce);
        if (!same) SB.dpts = stage_in(SB.up, ptsB, (size_t)SB.N * 3, s, Up::bounce);
        double lo[3], hi[3];
        if (mode == EV_KD) ev_bounds<true>(h, side, same ? 1 : 2, lo, hi);
        else ev_bounds<false>(h, side, same ? 1 : 2, lo, hi);
        // the reach and the cell side: merger_set_reach (hmsg_merge.hip)
        double reach = radius;
        if (mode == EV_BLAS) {
            double m2 = 0.0;
            for (int a = 0; a < 3; ++a) {
                const double v = std::max(std::fabs(lo[a]), std::fabs(hi[a])) + 1.0;
                m2 += v * v;
            }
            reach = std::sqrt(radius * radius + 16.0 * 5.9604644775390625e-08 * m2);
        }
        EvGrid g;
        g.cell = reach * (1.0 + 1e-3) + 2e-3;
        g.pad = 0;
        unsigned long long ncell = 1;
        for (int a = 0; a < 3; ++a) {
            g.o[a] = lo[a];
            const double n = std::floor((hi[a] - lo[a]) / g.cell) + 1.0;
            HMSG_REQUIRE(n < 2097152.0, HMSG_ERR_UNSUPPORTED, "hmsg_cloud_set_overlaps: the clouds span 2^21 cells or more along an axis");
            g.n[a] = (int)n;
            ncell *= (unsigned long long)g.n[a];
        }
        const int key_bits = bits_for(ncell);
        if (mode == EV_KD) {
            ev_sort_side<true>(h, SA, g, key_bits);
            if (!same) ev_sort_side<true>(h, SB, g, key_bits);
        } else {
            ev_sort_side<false>(h, SA, g, key_bits);
            if (!same) ev_sort_side<false>(h, SB, g, key_bits);
        }
        DevBuf<EvTask> dt;
        dt.alloc(tasks.size());
        HIP_TRY(hipMemcpyAsync(dt.p, tasks.data(), tasks.size() * sizeof(EvTask), hipMemcpyHostToDevice, s));
        const float r2f = (float)(radius * radius);       // `D < radius**2` with a float32 D (graph_utils.py:654-655)
        const double r2d = radius * radius;
        const EvSideDev da = SA.dev(), db = SB.dev();
        {
            // algorithmic bytes: every query point and its key once, every point and key of the target cloud once per task, the count
            double work = 0.0;
            for (const EvTask& t : tasks) work += ((double)t.nq + (double)t.nt) * (mode == EV_KD ? 32.0 : 24.0) + 4.0;
            ProfScope ps(h->prof, s, "k_ev_probe", work);
            if (mode == EV_KD)
                hipLaunchKernelGGL(k_ev_probe<EV_KD>, dim3((unsigned)nblk), dim3(256), 0, s, da, db, (const EvTask*)dt.p, (int)tasks.size(), g, r2f, r2d,
                                   dcounts);
            else if (mode == EV_BLAS)
                hipLaunchKernelGGL(k_ev_probe<EV_BLAS>, dim3((unsigned)nblk), dim3(256), 0, s, da, db, (const EvTask*)dt.p, (int)tasks.size(), g, r2f,
                                   r2d, dcounts);
            else
                hipLaunchKernelGGL(k_ev_probe<EV_DIRECT>, dim3((unsigned)nblk), dim3(256), 0, s, da, db, (const EvTask*)dt.p, (int)tasks.size(), g,
                                   r2f, r2d, dcounts);
            HMSG_CHECK_LAUNCH();
        }
        unstage_out(counts, dcounts, tasks.size(), s);
        HIP_TRY(hipStreamSynchronize(s));
        return;
    }
    unstage_out(counts, dcounts, tasks.size(), s);
    HIP_TRY(hipStreamSynchronize(s));
}

// float64 bounding box of every cloud of a CSR set: box[c] = (min xyz, max xyz) in ev_enc's u64 image, initialised by the caller
__global__ void __launch_bounds__(256) k_ev_cloud_box(const double* __restrict__ pts, long long n, const long long* __restrict__ off, int nclouds,
                                                      unsigned long long* __restrict__ box) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < n;
    int cloud = 0;
    unsigned long long e[3] = {0ull, 0ull, 0ull};
    if (live) {
        int lo = 0, hi = nclouds - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (off[mid] <= i) lo = mid; else hi = mid - 1;
        }
        cloud = lo;
        for (int a = 0; a < 3; ++a) e[a] = ev_enc(__double_as_longlong(pts[i * 3 + a]));
    }
    const int cloud0 = __shfl(cloud, 0);
    if (__all(live && cloud == cloud0)) {
        for (int a = 0; a < 3; ++a) {
            unsigned long long mn = e[a], mx = e[a];
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned long long pmn = __shfl_xor(mn, o), pmx = __shfl_xor(mx, o);
                mn = pmn < mn ? pmn : mn;
                mx = pmx > mx ? pmx : mx;
            }
            if ((threadIdx.x & 63) == 0) {
                atomicMin(&box[(size_t)cloud * 6 + a], mn);
                atomicMax(&box[(size_t)cloud * 6 + 3 + a], mx);
            }
        }
    } else if (live) {
        for (int a = 0; a < 3; ++a) {
            atomicMin(&box[(size_t)cloud * 6 + a], e[a]);
            atomicMax(&box[(size_t)cloud * 6 + 3 + a], e[a]);
        }
    }
}

// get_3d_iou (utils/eval_utils.py:169-200) in float64, operation for operation
double ev_iou_3d(const double* c1, const double* d1, const double* c2, const double* d2) {
    double inter = 1.0;
    for (int a = 0; a < 3; ++a) {
        const double e1 = d1[a] / 2, e2 = d2[a] / 2;
        const double mn = std::max(c1[a] - e1, c2[a] - e2), mx = std::min(c1[a] + e1, c2[a] + e2);
        const double side = mx - mn > 0 ? mx - mn : 0.0;
        inter = a == 0 ? side : inter * side;
    }
    const double v1 = d1[0] * d1[1] * d1[2], v2 = d2[0] * d2[1] * d2[2];
    const double uni = v1 + v2 - inter;
    return uni > 0 ? inter / uni : 0.0;
}

// hm3dsem_evaluator.py:429-458: the two association matrices of evaluate_objects
void ev_object_matrices(hmsg_ctx* h, int32_t P, const double* pred_pts, const int64_t* pred_off, int32_t G, const double* gt_pts,
                        const int64_t* gt_off, const double* gt_center, const double* gt_dims, double radius, double* iou_out,
                        double* overlap_out, int64_t* n_gated) {
    hipStream_t s = h->stream;
    HMSG_REQUIRE(P > 0 && G > 0, HMSG_ERR_INVALID, "hmsg_eval_object_matrices: no predicted or no ground-truth objects (the reference divides by zero there)");
    HMSG_REQUIRE(gt_center && gt_dims && (iou_out || overlap_out), HMSG_ERR_INVALID, "hmsg_eval_object_matrices: null boxes / no output");
    EvSide S;
    ev_read_side(S, "pred", P, pred_pts, pred_off);
    // the predicted boxes: min / max of every cloud's float64 points
    std::vector<unsigned long long> hb((size_t)P * 6);
    for (size_t k = 0; k < hb.size(); ++k) hb[k] = (k % 6) < 3 ? ~0ull : 0ull;
    if (S.N) {
        DevBuf<unsigned long long> box;
        box.alloc(hb.size());
        HIP_TRY(hipMemcpyAsync(box.p, hb.data(), hb.size() * 8, hipMemcpyHostToDevice, s));
        S.doff.alloc(S.off.size());
        HIP_TRY(hipMemcpyAsync(S.doff.p, S.off.data(), S.off.size() * 8, hipMemcpyHostToDevice, s));
        const double* dp = stage_in(S.up, pred_pts, (size_t)S.N * 3, s, Up::bounce);
        hipLaunchKernelGGL(k_ev_cloud_box, dim3(cdiv((size_t)S.N, 256)), dim3(256), 0, s, dp, S.N, (const long long*)S.doff.p, P, box.p);
        HMSG_CHECK_LAUNCH();
        HIP_TRY(hipMemcpyAsync(hb.data(), box.p, hb.size() * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    std::vector<double> gc((size_t)G * 3), gd((size_t)G * 3);
    read_in(gc.data(), gt_center, gc.size() * 8);
    read_in(gd.data(), gt_dims, gd.size() * 8);
    std::vector<double> iou((size_t)P * G, 0.0), ov((size_t)P * G, 0.0);
    std::vector<int32_t> pairs;
    for (int p = 0; p < P; ++p) {
        // get_axis_aligned_bounding_box().get_box_points() in Open3D's corner order, then find_box_center_and_dims
        // (utils/eval_utils.py:413-417): np.mean adds the eight corners in order and divides by 8, np.ptp is max - min over them.
        // An empty cloud has Open3D's box at the origin with no extent.
        double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, c[3], d[3];
        if (S.off[(size_t)p + 1] > S.off[(size_t)p])
            for (int a = 0; a < 3; ++a) {
                lo[a] = ev_dec(hb[(size_t)p * 6 + a]);
                hi[a] = ev_dec(hb[(size_t)p * 6 + 3 + a]);
                HMSG_REQUIRE(std::isfinite(lo[a]) && std::isfinite(hi[a]), HMSG_ERR_INVALID, "hmsg_eval_object_matrices: a coordinate is not finite");
            }
        static const int corner[8][3] = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {2, 2, 2}, {0, 1, 1}, {1, 0, 1}, {1, 1, 0}};   // 0 min, 1 min + extent, 2 max
        for (int a = 0; a < 3; ++a) {
            const double ex = hi[a] - lo[a];
            double sum = 0.0, mn = 0.0, mx = 0.0;
            for (int k = 0; k < 8; ++k) {
                const double v = corner[k][a] == 0 ? lo[a] : (corner[k][a] == 1 ? lo[a] + ex : hi[a]);
                sum = k == 0 ? v : sum + v;
                mn = k == 0 ? v : std::min(mn, v);
                mx = k == 0 ? v : std::max(mx, v);
            }
            c[a] = sum / 8.0;
            d[a] = mx - mn;
        }
        for (int g = 0; g < G; ++g) {
            const double v = ev_iou_3d(&gc[(size_t)g * 3], &gd[(size_t)g * 3], c, d);
            iou[(size_t)p * G + g] = v;
            if (v > 0.0) {
                pairs.push_back(p);
                pairs.push_back(g);
            }
        }
    }
    const int64_t np_ = (int64_t)pairs.size() / 2;
    std::vector<uint32_t> counts((size_t)np_ * 2 + 2, 0u);
    const int mode = h->cfg.overlap_distance_form == HMSG_OVERLAP_FAISS_BLAS ? EV_BLAS : EV_DIRECT;
    ev_cloud_set_overlaps(h, mode, P, pred_pts, pred_off, G, gt_pts, gt_off, np_, pairs.data(), radius, counts.data());
    std::vector<long long> goff((size_t)G + 1);
    read_in(goff.data(), gt_off, goff.size() * 8);
    for (int64_t k = 0; k < np_; ++k) {
        const int p = pairs[(size_t)k * 2], g = pairs[(size_t)k * 2 + 1];
        const double n1 = (double)(S.off[(size_t)p + 1] - S.off[(size_t)p]), n2 = (double)(goff[(size_t)g + 1] - goff[(size_t)g]);
        // find_overlapping_ratio_faiss: 0 for an empty cloud, else max of the two ratios
        ov[(size_t)p * G + g] = (n1 == 0 || n2 == 0) ? 0.0 : std::max((double)counts[(size_t)k * 2] / n1, (double)counts[(size_t)k * 2 + 1] / n2);
    }
    if (iou_out) write_out(iou_out, iou.data(), iou.size() * 8);
    if (overlap_out) write_out(overlap_out, ov.data(), ov.size() * 8);
    if (n_gated) *n_gated = np_;
}

}  // namespace

extern "C" int hmsg_eval_object_matrices(hmsg_t* h, int32_t P, const double* pred_pts, const int64_t* pred_off, int32_t G, const double* gt_pts,
                                         const int64_t* gt_off, const double* gt_obb_center, const double* gt_obb_dims, double radius,
                                         double* iou, double* overlap, int64_t* n_gated) {
    if (!h) return HMSG_ERR_INVALID;
    return hmsg_boundary(h, [&] {
        ev_object_matrices(h, P, pred_pts, pred_off, G, gt_pts, gt_off, gt_obb_center, gt_obb_dims, radius, iou, overlap, n_gated);
    });
}

extern "C" int hmsg_cloud_set_overlaps(hmsg_t* h, int32_t nA, const double* ptsA, const int64_t* offA, int32_t nB, const double* ptsB,
                                       const int64_t* offB, int64_t n_pairs, const int32_t* pairs, double radius, uint32_t* counts) {
    if (!h) return HMSG_ERR_INVALID;
    return hmsg_boundary(h, [&] {
        const int mode = h->cfg.overlap_distance_form == HMSG_OVERLAP_FAISS_BLAS ? EV_BLAS : EV_DIRECT;
        ev_cloud_set_overlaps(h, mode, nA, ptsA, offA, nB, ptsB, offB, n_pairs, pairs, radius, counts);
    });
}

extern "C" int hmsg_cloud_set_overlaps_kd(hmsg_t* h, int32_t nA, const double* ptsA, const int64_t* offA, int32_t nB, const double* ptsB,
                                          const int64_t* offB, int64_t n_pairs, const int32_t* pairs, double radius, uint32_t* counts) {
    if (!h) return HMSG_ERR_INVALID;
    return hmsg_boundary(h, [&] { ev_cloud_set_overlaps(h, EV_KD, nA, ptsA, offA, nB, ptsB, offB, n_pairs, pairs, radius, counts); });
}

extern "C" int hmsg_lsap(int32_t nr, int32_t nc, const double* cost, int32_t maximize, int32_t* row_ind, int32_t* col_ind, int32_t* n_assigned) {
    return hmsg_boundary("hmsg_lsap", -1, [&] {
        HMSG_REQUIRE(nr >= 0 && nc >= 0 && n_assigned, HMSG_ERR_INVALID, "negative shape or no n_assigned");
        const int32_t n = std::min(nr, nc);
        HMSG_REQUIRE(n == 0 || (cost && row_ind && col_ind), HMSG_ERR_INVALID, "null cost / row_ind / col_ind");
        std::vector<int64_t> r((size_t)n), c((size_t)n);
        const int rc = lsap_solve(nr, nc, cost, maximize != 0, r.data(), c.data());
        HMSG_REQUIRE(rc != LSAP_INVALID, HMSG_ERR_INVALID, "matrix contains invalid numeric entries");
        HMSG_REQUIRE(rc != LSAP_INFEASIBLE, HMSG_ERR_INVALID, "cost matrix is infeasible");
        for (int32_t i = 0; i < n; ++i) {
            row_ind[i] = (int32_t)r[(size_t)i];
            col_ind[i] = (int32_t)c[(size_t)i];
        }
        *n_assigned = n;
    });
}

// ==================================================================================================== evaluate_rooms (:265-341)
// hmsg_eval_rooms: the three room matrices.  The reference flattens a predicted room onto the ground-truth room's min_height and
// down-samples it for every pair it visits, and replaces the ground-truth room's bev cloud by its own down-sample at every visit
// (include/hmsg.h states the consequences).  Here:
//   - the visit sequence and the gate are planned on the host (a few thousand comparisons);
//   - the ground-truth versions vds^k(gt_g) come from CloudOps::voxel_down_sample, one batch per round over the rooms that still
//     need a further version and have not reached their bitwise fixed point (k_evr_same);
//   - a flattened cloud's voxel grouping does not depend on the ground-truth room (every point has the same y, the origin is per
//     axis), so every predicted room is grouped ONCE: k_evr_keys, a stable sort by (room, x cell, z cell), k_evr_heads, k_evr_walk
//     (per voxel: count and the sequential float64 sums of x and z in input order, / count); k_evr_flatten then writes, per visited
//     pair, the voxel's y = (h + h + ... + h) / count added sequentially -- NOT h for most counts -- beside the shared x and z;
//   - the flattened clouds are set A, the versions set B of one hmsg_cloud_set_overlaps call (loop 1) and one
//     hmsg_cloud_set_overlaps_kd call (loop 2: both directions of find_intersection_share come from the one pair list).
// HMSG_DEBUG_EVAL_ROOMS_PER_PAIR=1 flattens and down-samples the whole predicted cloud for every pair instead (k_evr_copy_flat +
// CloudOps::voxel_down_sample); the results are the same bits.
namespace {

__global__ void __launch_bounds__(256) k_evr_keys(const double* __restrict__ pts, long long n, const long long* __restrict__ off, int nclouds,
                                                  const double* __restrict__ org, double vs, unsigned long long NZ,
                                                  unsigned long long* __restrict__ ck, unsigned* __restrict__ cl, unsigned* __restrict__ keys,
                                                  unsigned long long* __restrict__ vals) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int lo = 0, hi = nclouds - 1;                       // the last cloud that starts at or before i (it is not empty)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    // Open3D's voxel index (o3d_voxel_keys): floor((p - (min_bound - voxel / 2)) / voxel) per axis; y is the same for every point
    const long long ix = (long long)floor(__ddiv_rn(__dsub_rn(pts[i * 3 + 0], org[(size_t)lo * 2 + 0]), vs));
    const long long iz = (long long)floor(__ddiv_rn(__dsub_rn(pts[i * 3 + 2], org[(size_t)lo * 2 + 1]), vs));
    const unsigned long long key = (unsigned long long)ix * NZ + (unsigned long long)iz;
    ck[i] = key;
    cl[i] = (unsigned)lo;
    keys[i] = (unsigned)key;
    vals[i] = (unsigned long long)i;
}

// bit j of the bitmap: sorted position j starts a voxel (another room or another key than position j - 1)
__global__ void __launch_bounds__(256) k_evr_heads(const unsigned long long* __restrict__ vals, long long n, const unsigned long long* __restrict__ ck,
                                                   const unsigned* __restrict__ cl, unsigned long long* __restrict__ bitmap) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    bool head = false;
    if (j < n) {
        const unsigned long long v = vals[j];
        if (j == 0) head = true;
        else {
            const unsigned long long u = vals[j - 1];
            head = cl[v] != cl[u] || ck[v] != ck[u];
        }
    }
    const unsigned long long m = __ballot(head);
    if ((threadIdx.x & 63) == 0) bitmap[j >> 6] = m;    // (the bitmap has a word for every wave of the grid)
}

// the lane of a voxel's first sorted position walks the voxel: count, sequential float64 sums of x and z in input order (the sort
// is stable), / count -- o3d_voxel_down_sample's arithmetic for the two axes the flattening leaves alone
__global__ void __launch_bounds__(256) k_evr_walk(const unsigned long long* __restrict__ vals, long long n, const unsigned long long* __restrict__ bitmap,
                                                  const unsigned* __restrict__ rank, const double* __restrict__ pts, const unsigned* __restrict__ cl,
                                                  const long long* __restrict__ off, double* __restrict__ vx, double* __restrict__ vz,
                                                  unsigned* __restrict__ vcnt, unsigned* __restrict__ vstart) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const unsigned long long w = bitmap[j >> 6];
    if (!((w >> (j & 63)) & 1ull)) return;
    const unsigned slot = rank[j >> 6] + (unsigned)__popcll(w & ((1ull << (j & 63)) - 1ull));
    double sx = 0.0, sz = 0.0;
    long long r = j;
    do {
        const double* p = pts + (size_t)vals[r] * 3;
        sx = __dadd_rn(sx, p[0]);
        sz = __dadd_rn(sz, p[2]);
        ++r;
    } while (r < n && !((bitmap[r >> 6] >> (r & 63)) & 1ull));
    const double cnt = (double)(r - j);
    vx[slot] = __ddiv_rn(sx, cnt);
    vz[slot] = __ddiv_rn(sz, cnt);
    vcnt[slot] = (unsigned)(r - j);
    const unsigned c = cl[vals[j]];
    if (j == off[c]) vstart[c] = slot;                   // (a room's points are one range of the sorted order: the sort's last key is the room)
}

struct EvrFlat {
    long long a0, s0;            // first output point; first source point (k_evr_copy_flat)
    unsigned v0;                 // first voxel slot of the predicted room (k_evr_flatten)
    int n;                       // voxels (k_evr_flatten) | points (k_evr_copy_flat)
    double h;                    // the ground-truth room's min_height
};
// one flattened, down-sampled cloud per visited pair: x and z of the room's voxels, y = count copies of h added one by one / count
__global__ void __launch_bounds__(256) k_evr_flatten(const EvrFlat* __restrict__ tasks, const double* __restrict__ vx, const double* __restrict__ vz,
                                                     const unsigned* __restrict__ vcnt, double* __restrict__ out) {
    const EvrFlat t = tasks[blockIdx.y];
    for (int i = (int)(blockIdx.x * 256 + threadIdx.x); i < t.n; i += (int)(gridDim.x * 256)) {
        const unsigned c = vcnt[t.v0 + (unsigned)i];
        const double sy = repeat_add(0.0, t.h, (int)c);          // c sequential additions of h (hmsg_common.h: the same bits, in closed form)
        double* o = out + (size_t)(t.a0 + i) * 3;
        o[0] = vx[t.v0 + (unsigned)i];
        o[1] = __ddiv_rn(sy, (double)c);
        o[2] = vz[t.v0 + (unsigned)i];
    }
}
// the debug route: the whole predicted cloud with every y set to h, for CloudOps::voxel_down_sample
__global__ void __launch_bounds__(256) k_evr_copy_flat(const EvrFlat* __restrict__ tasks, const double* __restrict__ pts, double* __restrict__ out) {
    const EvrFlat t = tasks[blockIdx.y];
    for (int i = (int)(blockIdx.x * 256 + threadIdx.x); i < t.n; i += (int)(gridDim.x * 256)) {
        const double* p = pts + (size_t)(t.s0 + i) * 3;
        double* o = out + (size_t)(t.a0 + i) * 3;
        o[0] = p[0], o[1] = t.h, o[2] = p[2];
    }
}

struct EvrCmp {
    long long a0, b0;
    int n, pad;
};
// differs[k] = 1 when cloud k of a and of b are not the same bits
__global__ void __launch_bounds__(256) k_evr_same(const double* __restrict__ a, const double* __restrict__ b, const EvrCmp* __restrict__ tasks,
                                                  int* __restrict__ differs) {
    const EvrCmp t = tasks[blockIdx.y];
    const long long n3 = (long long)t.n * 3;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n3; i += (long long)gridDim.x * 256)
        if (__double_as_longlong(a[t.a0 * 3 + i]) != __double_as_longlong(b[t.b0 * 3 + i])) differs[blockIdx.y] = 1;
}

// the boxes of a CSR set's clouds (CloudOps::bounds) with the refusal of coordinates that are not finite
void evr_boxes(CloudOps& ops, const double* dpts, const EvSide& S, std::vector<SegDesc>& segs, const char* what) {
    segs.assign((size_t)S.nclouds, SegDesc());
    for (int c = 0; c < S.nclouds; ++c) {
        segs[(size_t)c].pt_base = S.off[(size_t)c];
        segs[(size_t)c].n = (int)(S.off[(size_t)c + 1] - S.off[(size_t)c]);
    }
    if (S.N == 0) return;
    ops.bounds(dpts, segs);
    for (const SegDesc& sd : segs)
        for (int a = 0; a < 3 && sd.n; ++a)
            HMSG_REQUIRE(std::isfinite(sd.mn[a]) && std::isfinite(sd.mx[a]), HMSG_ERR_INVALID,
                         std::string("hmsg_eval_rooms: a coordinate of the ") + what + " rooms is not finite");
}

struct EvrVersion {
    const double* p;
    int n;
};

void ev_rooms(hmsg_ctx* h, int32_t P, const double* pred_pts, const int64_t* pred_off, const double* zero_level, const double* height, int32_t G,
              const double* gt_pts, const int64_t* gt_off, const double* gt_min_h, const double* gt_max_h, const double* gt_mean_h, int32_t F,
              const double* fl_lower, const double* fl_upper, double voxel, double radius, double* assoc_out, double* over_pred_out,
              double* over_gt_out, int64_t* n_gated) {
    hipStream_t s = h->stream;
    HMSG_REQUIRE(P > 0 && G > 0, HMSG_ERR_INVALID, "hmsg_eval_rooms: no predicted or no ground-truth rooms (the reference divides by zero there)");
    HMSG_REQUIRE(F >= 0 && (F == 0 || (fl_lower && fl_upper)) && zero_level && height && gt_min_h && gt_max_h && gt_mean_h, HMSG_ERR_INVALID,
                 "hmsg_eval_rooms: null argument");
    HMSG_REQUIRE(std::isfinite(voxel) && voxel > 0.0 && std::isfinite(radius) && radius > 0.0, HMSG_ERR_INVALID,
                 "hmsg_eval_rooms: the voxel size and the radius must be positive");
    EvSide SP, SG;
    ev_read_side(SP, "of predicted rooms", P, pred_pts, pred_off);
    ev_read_side(SG, "of ground-truth rooms", G, gt_pts, gt_off);
    std::vector<double> zl((size_t)P), ht((size_t)P), mnh((size_t)G), mxh((size_t)G), meh((size_t)G), lo((size_t)F), up((size_t)F);
    read_in(zl.data(), zero_level, zl.size() * 8);
    read_in(ht.data(), height, ht.size() * 8);
    read_in(mnh.data(), gt_min_h, mnh.size() * 8);
    read_in(mxh.data(), gt_max_h, mxh.size() * 8);
    read_in(meh.data(), gt_mean_h, meh.size() * 8);
    if (F) read_in(lo.data(), fl_lower, lo.size() * 8);
    if (F) read_in(up.data(), fl_upper, up.size() * 8);
    // ---- the visit sequence (:279-299; the second nest :304-341 repeats it).  A cell keeps its LAST visit.
    std::vector<int> visits((size_t)G, 0);
    std::map<std::pair<int, int>, int> last;             // (p, g) -> which visit of g (1 ..) wrote the cell last
    for (int f = 0; f < F; ++f)
        for (int g = 0; g < G; ++g)
            if (meh[(size_t)g] > lo[(size_t)f] && meh[(size_t)g] < up[(size_t)f])
                for (int p = 0; p < P; ++p) {
                    const double pm = zl[(size_t)p] + ht[(size_t)p] / 2;
                    if (pm > mnh[(size_t)g] && pm < mxh[(size_t)g]) last[{p, g}] = ++visits[(size_t)g];
                }
    struct Cell {
        int p, g, j;
    };
    std::vector<Cell> cells;
    for (const auto& kv : last) cells.push_back(Cell{kv.first.first, kv.first.second, kv.second});
    // ---- both sets on the device, their boxes, the finite check
    CloudOps ops;
    ops.s = s;
    const double* dP = SP.N ? stage_in(SP.up, pred_pts, (size_t)SP.N * 3, s, Up::bounce) : nullptr;
    const double* dG = SG.N ? stage_in(SG.up, gt_pts, (size_t)SG.N * 3, s, Up::bounce) : nullptr;
    for (EvSide* S : {&SP, &SG})                          // the refusal of coordinates that are not finite, NaN included (ev_bounds orders them outside +-inf)
        if (S->N) {
            double blo[3], bhi[3];
            S->dpts = S == &SP ? dP : dG;
            ev_bounds<true>(h, S, 1, blo, bhi);
        }
    std::vector<SegDesc> boxP, boxG;
    evr_boxes(ops, dP, SP, boxP, "predicted");
    evr_boxes(ops, dG, SG, boxG, "ground-truth");
    for (const SegDesc& sd : boxP)
        for (int a = 0; a < 3 && sd.n; a += 2)
            HMSG_REQUIRE(std::floor((sd.mx[a] - sd.mn[a]) / voxel) + 3.0 < 2097152.0, HMSG_ERR_UNSUPPORTED,
                         "hmsg_eval_rooms: a predicted room spans 2^21 voxels or more along an axis");
    const size_t PG = (size_t)P * (size_t)G;
    std::vector<double> assoc(PG, 0.0), over_pred(PG, 0.0), over_gt(PG, 0.0);
    const size_t NC = cells.size();
    if (NC) {
        // ---- set A: the flattened, down-sampled predicted cloud of every cell
        std::vector<long long> offA(NC + 1, 0);
        DevBuf<double> A;
        if (getenv("HMSG_DEBUG_EVAL_ROOMS_PER_PAIR") == nullptr) {
            std::vector<unsigned> vstart((size_t)P + 1, 0u);
            DevBuf<double> vx, vz;
            DevBuf<unsigned> vcnt;
            if (SP.N) {
                const size_t N = (size_t)SP.N;
                const unsigned nblk = cdiv(N, 256);
                std::vector<double> org((size_t)P * 2, 0.0);
                unsigned long long NX = 1, NZ = 1;
                for (int p = 0; p < P; ++p) {
                    const SegDesc& sd = boxP[(size_t)p];
                    if (!sd.n) continue;
                    org[(size_t)p * 2 + 0] = sd.mn[0] - voxel * 0.5;
                    org[(size_t)p * 2 + 1] = sd.mn[2] - voxel * 0.5;
                    NX = std::max(NX, (unsigned long long)std::floor((sd.mx[0] - org[(size_t)p * 2 + 0]) / voxel) + 2ull);
                    NZ = std::max(NZ, (unsigned long long)std::floor((sd.mx[2] - org[(size_t)p * 2 + 1]) / voxel) + 2ull);
                }
                DevBuf<double> dorg;
                dorg.alloc(org.size());
                HIP_TRY(hipMemcpyAsync(dorg.p, org.data(), org.size() * 8, hipMemcpyHostToDevice, s));
                SP.doff.alloc(SP.off.size());
                HIP_TRY(hipMemcpyAsync(SP.doff.p, SP.off.data(), SP.off.size() * 8, hipMemcpyHostToDevice, s));
                SP.ck.alloc(N);
                SP.cl.alloc(N);
                SortBufs sb;
                sb.keys.alloc(N);
                sb.vals.alloc(N);
                {
                    ProfScope ps(h->prof, s, "k_evr_keys", (double)N * (24 + 8 + 4 + 4 + 8));
                    hipLaunchKernelGGL(k_evr_keys, dim3(nblk), dim3(256), 0, s, dP, (long long)N, (const long long*)SP.doff.p, (int)P,
                                       (const double*)dorg.p, voxel, NZ, SP.ck.p, SP.cl.p, sb.keys.p, sb.vals.p);
                    HMSG_CHECK_LAUNCH();
                }
                // stable passes, least significant key first: voxel key (low half, high half), then the room
                auto pass = [&](int bits) {
                    hmsg_sort_pairs(sb, N, bits, s);
                    if (sb.res_keys != sb.keys.p) {
                        sb.keys.swap(sb.keys_alt);
                        sb.vals.swap(sb.vals_alt);
                    }
                };
                auto rekey = [&](int by_cloud) {
                    hipLaunchKernelGGL(k_ev_rekey, dim3(nblk), dim3(256), 0, s, (const unsigned long long*)sb.vals.p, (long long)N,
                                       (const unsigned long long*)SP.ck.p, (const unsigned*)SP.cl.p, by_cloud, sb.keys.p);
                    HMSG_CHECK_LAUNCH();
                };
                const int key_bits = bits_for(NX * NZ);
                pass(std::min(key_bits, 32));
                if (key_bits > 32) {
                    rekey(0);
                    pass(key_bits - 32);
                }
                if (P > 1) {
                    rekey(1);
                    pass(bits_for((unsigned long long)P));
                }
                DevBuf<unsigned long long> bitmap;
                DevBuf<unsigned> rank, tmp, dvstart;
                const size_t nwords = (size_t)nblk * 4;
                bitmap.alloc(nwords);
                rank.alloc(nwords);
                hipLaunchKernelGGL(k_evr_heads, dim3(nblk), dim3(256), 0, s, (const unsigned long long*)sb.vals.p, (long long)N,
                                   (const unsigned long long*)SP.ck.p, (const unsigned*)SP.cl.p, bitmap.p);
                HMSG_CHECK_LAUNCH();
                const size_t NV = (size_t)hmsg_bitmap_rank(bitmap.p, rank.p, nwords, s, tmp);
                vx.alloc(NV);
                vz.alloc(NV);
                vcnt.alloc(NV);
                dvstart.alloc((size_t)P);
                {
                    ProfScope ps(h->prof, s, "k_evr_walk", (double)N * (8 + 16) + (double)NV * 20);
                    hipLaunchKernelGGL(k_evr_walk, dim3(nblk), dim3(256), 0, s, (const unsigned long long*)sb.vals.p, (long long)N,
                                       (const unsigned long long*)bitmap.p, (const unsigned*)rank.p, dP, (const unsigned*)SP.cl.p,
                                       (const long long*)SP.doff.p, vx.p, vz.p, vcnt.p, dvstart.p);
                    HMSG_CHECK_LAUNCH();
                }
                HIP_TRY(hipMemcpyAsync(vstart.data(), dvstart.p, (size_t)P * 4, hipMemcpyDeviceToHost, s));
                HIP_TRY(hipStreamSynchronize(s));
                vstart[(size_t)P] = (unsigned)NV;
                for (int p = P - 1; p >= 0; --p)
                    if (!boxP[(size_t)p].n) vstart[(size_t)p] = vstart[(size_t)p + 1];     // (an empty room wrote nothing)
            }
            std::vector<EvrFlat> tasks(NC);
            int maxn = 0;
            for (size_t k = 0; k < NC; ++k) {
                const int p = cells[k].p;
                const int nv = (int)(vstart[(size_t)p + 1] - vstart[(size_t)p]);
                tasks[k] = EvrFlat{offA[k], 0, vstart[(size_t)p], nv, mnh[(size_t)cells[k].g]};
                offA[k + 1] = offA[k] + nv;
                maxn = std::max(maxn, nv);
            }
            A.alloc((size_t)offA[NC] * 3);
            if (offA[NC]) {
                DevBuf<EvrFlat> dt;
                dt.alloc(NC);
                HIP_TRY(hipMemcpyAsync(dt.p, tasks.data(), NC * sizeof(EvrFlat), hipMemcpyHostToDevice, s));
                const unsigned gx = std::max(1u, std::min(cdiv((size_t)maxn, 256), 1024u));
                ProfScope ps(h->prof, s, "k_evr_flatten", (double)offA[NC] * (20 + 24));
                for (size_t k0 = 0; k0 < NC; k0 += 32768) {
                    hipLaunchKernelGGL(k_evr_flatten, dim3(gx, (unsigned)std::min<size_t>(32768, NC - k0)), dim3(256), 0, s, (const EvrFlat*)dt.p + k0,
                                       (const double*)vx.p, (const double*)vz.p, (const unsigned*)vcnt.p, A.p);
                    HMSG_CHECK_LAUNCH();
                }
                HIP_TRY(hipStreamSynchronize(s));        // (dt and the voxel tables leave scope)
            }
        } else {
            // the debug route: every cell's whole cloud, flattened, through the segmented voxel_down_sample
            std::vector<EvrFlat> tasks(NC);
            std::vector<SegDesc> segs(NC);
            long long tot = 0;
            int maxn = 0;
            for (size_t k = 0; k < NC; ++k) {
                const SegDesc& bx = boxP[(size_t)cells[k].p];
                const double hgt = mnh[(size_t)cells[k].g];
                tasks[k] = EvrFlat{tot, bx.pt_base, 0u, bx.n, hgt};
                segs[k].pt_base = tot;
                segs[k].n = bx.n;
                segs[k].mn[0] = bx.mn[0], segs[k].mn[1] = hgt, segs[k].mn[2] = bx.mn[2];
                segs[k].mx[0] = bx.mx[0], segs[k].mx[1] = hgt, segs[k].mx[2] = bx.mx[2];
                tot += bx.n;
                maxn = std::max(maxn, bx.n);
            }
            HMSG_REQUIRE(tot < (1ll << 32), HMSG_ERR_UNSUPPORTED, "hmsg_eval_rooms: the per-pair route has 2^32 points or more");
            A.alloc((size_t)tot * 3);
            if (tot) {
                DevBuf<double> flat;
                flat.alloc((size_t)tot * 3);
                DevBuf<EvrFlat> dt;
                dt.alloc(NC);
                HIP_TRY(hipMemcpyAsync(dt.p, tasks.data(), NC * sizeof(EvrFlat), hipMemcpyHostToDevice, s));
                const unsigned gx = std::max(1u, std::min(cdiv((size_t)maxn, 256), 1024u));
                for (size_t k0 = 0; k0 < NC; k0 += 32768) {
                    hipLaunchKernelGGL(k_evr_copy_flat, dim3(gx, (unsigned)std::min<size_t>(32768, NC - k0)), dim3(256), 0, s, (const EvrFlat*)dt.p + k0, dP,
                                       flat.p);
                    HMSG_CHECK_LAUNCH();
                }
                std::vector<int> out_n;
                ops.voxel_down_sample(flat.p, segs, voxel, A.p, out_n);
                for (size_t k = 0; k < NC; ++k) offA[k + 1] = offA[k] + out_n[k];
            }
        }
        // ---- set B: the versions vds^k(gt_g) the cells read.  Loop 1 reads version j of its visit, loop 2 version visits[g] + j.
        std::vector<int> need((size_t)G, 0);
        for (const Cell& c : cells) need[(size_t)c.g] = std::max(need[(size_t)c.g], visits[(size_t)c.g] + c.j);
        std::vector<std::vector<EvrVersion>> ver((size_t)G);
        std::vector<EvrVersion> cur((size_t)G);
        std::vector<char> fixed((size_t)G, 0);
        for (int g = 0; g < G; ++g) cur[(size_t)g] = EvrVersion{dG ? dG + (size_t)SG.off[(size_t)g] * 3 : nullptr, boxG[(size_t)g].n};
        std::deque<DevBuf<double>> rounds;
        for (int round = 1;; ++round) {
            std::vector<int> act;
            for (int g = 0; g < G; ++g)
                if (need[(size_t)g] >= round && !fixed[(size_t)g] && cur[(size_t)g].n > 0) act.push_back(g);
            if (act.empty()) break;
            std::vector<SegDesc> segs(act.size());
            long long tot = 0;
            for (size_t k = 0; k < act.size(); ++k) {
                segs[k].pt_base = tot;
                segs[k].n = cur[(size_t)act[k]].n;
                tot += segs[k].n;
            }
            rounds.emplace_back();
            DevBuf<double>& src = rounds.back();
            src.alloc((size_t)tot * 3);
            for (size_t k = 0; k < act.size(); ++k)
                HIP_TRY(hipMemcpyAsync(src.p + (size_t)segs[k].pt_base * 3, cur[(size_t)act[k]].p, (size_t)segs[k].n * 24, hipMemcpyDeviceToDevice, s));
            ops.bounds(src.p, segs);
            rounds.emplace_back();
            DevBuf<double>& dst = rounds.back();
            dst.alloc((size_t)tot * 3);
            std::vector<int> out_n;
            ops.voxel_down_sample(src.p, segs, voxel, dst.p, out_n);
            std::vector<EvrCmp> cmp(act.size());
            std::vector<int> differs(act.size(), 0);
            long long o = 0;
            int maxn = 0;
            for (size_t k = 0; k < act.size(); ++k) {
                cmp[k] = EvrCmp{segs[k].pt_base, o, out_n[k] == segs[k].n ? segs[k].n : 0, 0};
                maxn = std::max(maxn, cmp[k].n);
                o += out_n[k];
            }
            DevBuf<EvrCmp> dc;
            DevBuf<int> dd;
            dc.alloc(cmp.size());
            dd.alloc(cmp.size());
            HIP_TRY(hipMemcpyAsync(dc.p, cmp.data(), cmp.size() * sizeof(EvrCmp), hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemsetAsync(dd.p, 0, cmp.size() * 4, s));
            const unsigned gx = std::max(1u, std::min(cdiv((size_t)std::max(maxn, 1) * 3, 256), 1024u));
            for (size_t k0 = 0; k0 < cmp.size(); k0 += 32768) {
                hipLaunchKernelGGL(k_evr_same, dim3(gx, (unsigned)std::min<size_t>(32768, cmp.size() - k0)), dim3(256), 0, s, (const double*)src.p,
                                   (const double*)dst.p, (const EvrCmp*)dc.p + k0, dd.p + k0);
                HMSG_CHECK_LAUNCH();
            }
            HIP_TRY(hipMemcpyAsync(differs.data(), dd.p, cmp.size() * 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            for (size_t k = 0; k < act.size(); ++k) {
                const int g = act[k];
                cur[(size_t)g] = EvrVersion{dst.p + (size_t)cmp[k].b0 * 3, out_n[k]};
                ver[(size_t)g].push_back(cur[(size_t)g]);
                if (out_n[k] == segs[k].n && !differs[k]) fixed[(size_t)g] = 1;      // the same bits: every later version is this one
            }
            src.release();
        }
        std::map<std::pair<int, int>, int> bidx;          // (g, stored version) -> cloud of set B
        std::vector<EvrVersion> bclouds;
        auto version = [&](int g, int v) {
            const int nst = (int)ver[(size_t)g].size();
            const int k = std::min(v, nst);                // (beyond the stored ones: the fixed point; none stored: an empty room)
            auto it = bidx.find({g, k});
            if (it != bidx.end()) return it->second;
            bclouds.push_back(k > 0 ? ver[(size_t)g][(size_t)k - 1] : EvrVersion{nullptr, 0});
            return bidx[{g, k}] = (int)bclouds.size() - 1;
        };
        std::vector<int32_t> pr1(NC * 2), pr2(NC * 2);
        for (size_t k = 0; k < NC; ++k) {
            pr1[k * 2] = pr2[k * 2] = (int32_t)k;
            pr1[k * 2 + 1] = version(cells[k].g, cells[k].j);
            pr2[k * 2 + 1] = version(cells[k].g, visits[(size_t)cells[k].g] + cells[k].j);
        }
        const size_t NB = bclouds.size();
        std::vector<long long> offB(NB + 1, 0);
        for (size_t b = 0; b < NB; ++b) offB[b + 1] = offB[b] + bclouds[b].n;
        DevBuf<double> B;
        B.alloc((size_t)offB[NB] * 3);
        for (size_t b = 0; b < NB; ++b)
            if (bclouds[b].n)
                HIP_TRY(hipMemcpyAsync(B.p + (size_t)offB[b] * 3, bclouds[b].p, (size_t)bclouds[b].n * 24, hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
        // ---- the counts: loop 1 in find_overlapping_ratio_faiss's float32 form, loop 2 in find_intersection_share's float64 form
        std::vector<uint32_t> c1(NC * 2, 0u), c2(NC * 2, 0u);
        const int mode = h->cfg.overlap_distance_form == HMSG_OVERLAP_FAISS_BLAS ? EV_BLAS : EV_DIRECT;
        static_assert(sizeof(long long) == sizeof(int64_t), "offsets");
        if (assoc_out)
            ev_cloud_set_overlaps(h, mode, (int32_t)NC, A.p, (const int64_t*)offA.data(), (int32_t)NB, B.p, (const int64_t*)offB.data(), (int64_t)NC,
                                  pr1.data(), radius, c1.data());
        if (over_pred_out || over_gt_out)
            ev_cloud_set_overlaps(h, EV_KD, (int32_t)NC, A.p, (const int64_t*)offA.data(), (int32_t)NB, B.p, (const int64_t*)offB.data(), (int64_t)NC,
                                  pr2.data(), radius, c2.data());
        for (size_t k = 0; k < NC; ++k) {
            const size_t cell = (size_t)cells[k].p * (size_t)G + (size_t)cells[k].g;
            const double na = (double)(offA[k + 1] - offA[k]);
            const double nb1 = (double)bclouds[(size_t)pr1[k * 2 + 1]].n, nb2 = (double)bclouds[(size_t)pr2[k * 2 + 1]].n;
            assoc[cell] = (na == 0 || nb1 == 0) ? 0.0 : std::max((double)c1[k * 2] / na, (double)c1[k * 2 + 1] / nb1);
            // find_intersection_share(map, obj) = (points of map with a point of obj inside the bound) / len(obj): it can exceed 1
            over_pred[cell] = (na == 0 || nb2 == 0) ? 0.0 : std::min((double)c2[k * 2 + 1] / na, 1.0);      // map = gt, obj = pred
            over_gt[cell] = (na == 0 || nb2 == 0) ? 0.0 : std::min((double)c2[k * 2] / nb2, 1.0);            // map = pred, obj = gt
        }
    }
    if (assoc_out) write_out(assoc_out, assoc.data(), PG * 8);
    if (over_pred_out) write_out(over_pred_out, over_pred.data(), PG * 8);
    if (over_gt_out) write_out(over_gt_out, over_gt.data(), PG * 8);
    if (n_gated) *n_gated = (int64_t)NC;
}

}  // namespace

extern "C" int hmsg_eval_rooms(hmsg_t* h, int32_t P, const double* pred_pts, const int64_t* pred_off, const double* pred_zero_level,
                               const double* pred_height, int32_t G, const double* gt_pts, const int64_t* gt_off, const double* gt_min_h,
                               const double* gt_max_h, const double* gt_mean_h, int32_t F, const double* floor_lower, const double* floor_upper,
                               double voxel, double radius, double* assoc, double* over_pred, double* over_gt, int64_t* n_gated) {
    if (!h) return HMSG_ERR_INVALID;
    return hmsg_boundary(h, [&] {
        ev_rooms(h, P, pred_pts, pred_off, pred_zero_level, pred_height, G, gt_pts, gt_off, gt_min_h, gt_max_h, gt_mean_h, F, floor_lower, floor_upper,
                 voxel, radius, assoc, over_pred, over_gt, n_gated);
    });
}

// ================================================================================ object_semantics_eval_tp_auc (:557-589): the ranks
// hmsg_eval_semantic_ranks.  One workgroup per assigned pair: the embedding in float32, normalised as torchmetrics'
// pairwise_cosine_similarity normalises it (x / ||x||, element by element), then a wave per class: the text row's norm, the dot
// product of the two normalised rows.  Every class runs the same lane-strided loops and the same butterfly, so rows of the same
// bits give similarities of the same bits wherever they stand in the table.  The order of the similarities is numpy's sort order
// (evs_key: NaN above every number, -0 equal to +0), ties broken by the class index as a stable ascending argsort read from its end
// breaks them.
namespace {

__device__ __forceinline__ unsigned evs_key(float v) {
    if (v != v) return 0xFFFFFFFFu;
    if (v == 0.0f) v = 0.0f;
    const unsigned u = __float_as_uint(v);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}

__global__ void __launch_bounds__(256) k_evs_ranks(const void* __restrict__ emb, int emb_f64, int D, const float* __restrict__ text, int C,
                                                   const int* __restrict__ class_name, const int* __restrict__ target, unsigned* __restrict__ keys,
                                                   int* __restrict__ rank) {
    HIP_DYNAMIC_SHARED(float, xn)                        // [D]
    __shared__ float red[4];
    __shared__ int acc, best;
    const int i = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float ss = 0.0f;
    for (int d = tid; d < D; d += 256) {
        const float x = emb_f64 ? (float)((const double*)emb)[(size_t)i * D + d] : ((const float*)emb)[(size_t)i * D + d];
        xn[d] = x;
        ss = __fadd_rn(ss, __fmul_rn(x, x));
    }
    ss = wave_sum_f32(ss);
    if (lane == 0) red[wave] = ss;
    if (tid == 0) best = C;
    __syncthreads();
    const float nrm = __fsqrt_rn(__fadd_rn(__fadd_rn(red[0], red[1]), __fadd_rn(red[2], red[3])));
    for (int d = tid; d < D; d += 256) xn[d] = __fdiv_rn(xn[d], nrm);
    __syncthreads();
    unsigned* kp = keys + (size_t)i * C;
    for (int c = wave; c < C; c += 4) {
        const float* t = text + (size_t)c * D;
        float ts = 0.0f;
        for (int d = lane; d < D; d += 64) ts = __fadd_rn(ts, __fmul_rn(t[d], t[d]));
        const float tn = __fsqrt_rn(wave_sum_f32(ts));
        float dot = 0.0f;
        for (int d = lane; d < D; d += 64) dot = __fadd_rn(dot, __fmul_rn(xn[d], __fdiv_rn(t[d], tn)));
        dot = wave_sum_f32(dot);
        if (lane == 0) kp[c] = evs_key(dot);
    }
    __threadfence();
    __syncthreads();
    const int tgt = target[i];
    if (tgt >= 0)
        for (int t = 0; t < C; ++t) {
            if (class_name[t] != tgt) continue;          // (the same for every lane of the workgroup)
            const unsigned kt = kp[t];
            int cnt = 0;
            for (int c = tid; c < C; c += 256) {
                const unsigned kc = kp[c];
                cnt += (kc > kt || (kc == kt && c > t)) ? 1 : 0;
            }
            cnt = wave_sum_i32(cnt);
            if (tid == 0) acc = 0;
            __syncthreads();
            if (lane == 0) atomicAdd(&acc, cnt);
            __syncthreads();
            if (tid == 0) best = min(best, acc);
            __syncthreads();
        }
    if (tid == 0) rank[i] = best;
}

void ev_semantic_ranks(hmsg_ctx* h, int32_t n, const void* emb, int32_t emb_is_f64, int32_t D, int32_t C, const float* text,
                       const int32_t* class_name_id, const int32_t* target_name_id, int32_t* rank) {
    hipStream_t s = h->stream;
    HMSG_REQUIRE(n >= 0 && D > 0 && C > 0, HMSG_ERR_INVALID, "hmsg_eval_semantic_ranks: bad shape");
    HMSG_REQUIRE(D <= 8192, HMSG_ERR_UNSUPPORTED, "hmsg_eval_semantic_ranks: embeddings of more than 8192 components");
    HMSG_REQUIRE(text && class_name_id && (n == 0 || (emb && target_name_id && rank)), HMSG_ERR_INVALID, "hmsg_eval_semantic_ranks: null argument");
    if (n == 0) return;
    DevBuf<float> uf, ut;
    DevBuf<double> ud;
    DevBuf<int32_t> uc, ug, own_rank;
    DevBuf<unsigned> keys;
    const void* de = emb_is_f64 ? (const void*)stage_in(ud, (const double*)emb, (size_t)n * D, s, Up::direct)
                                : (const void*)stage_in(uf, (const float*)emb, (size_t)n * D, s, Up::direct);
    const float* dt = stage_in(ut, text, (size_t)C * D, s, Up::direct);
    const int32_t* dc = stage_in(uc, class_name_id, (size_t)C, s, Up::direct);
    const int32_t* dg = stage_in(ug, target_name_id, (size_t)n, s, Up::direct);
    int32_t* dr = stage_out(own_rank, rank, (size_t)n);
    keys.alloc((size_t)n * C);
    {
        ProfScope ps(h->prof, s, "k_evs_ranks", (double)n * ((double)C * D * 4 + (double)D * 8));
        hipLaunchKernelGGL(k_evs_ranks, dim3((unsigned)n), dim3(256), (size_t)D * 4, s, de, (int)(emb_is_f64 != 0), (int)D, dt, (int)C, (const int*)dc,
                           (const int*)dg, keys.p, (int*)dr);
        HMSG_CHECK_LAUNCH();
    }
    unstage_out(rank, dr, (size_t)n, s);
    HIP_TRY(hipStreamSynchronize(s));
}

void evm_check_pairs(const char* who, const double* M, int32_t P, int32_t G, const int32_t* row, const int32_t* col, int32_t n) {
    HMSG_REQUIRE(P >= 0 && G >= 0 && n >= 0 && (M || (size_t)P * G == 0) && (n == 0 || (row && col)), HMSG_ERR_INVALID,
                 std::string(who) + ": bad shape or null argument");
    for (int32_t k = 0; k < n; ++k)
        HMSG_REQUIRE(row[k] >= 0 && row[k] < P && col[k] >= 0 && col[k] < G, HMSG_ERR_INVALID, std::string(who) + ": a pair outside the matrix");
}
hmsg_eval_counts evm_export(const eval_metrics::Counts& c) {
    hmsg_eval_counts o;
    o.tp = c.tp, o.tn = 0, o.fp = c.fp, o.fn = c.fn;
    o.acc = c.acc, o.prec = c.prec, o.recall = c.recall;
    return o;
}

}  // namespace

extern "C" int hmsg_eval_semantic_ranks(hmsg_t* h, int32_t n, const void* emb, int32_t emb_is_f64, int32_t D, int32_t C, const float* text,
                                        const int32_t* class_name_id, const int32_t* target_name_id, int32_t* rank) {
    if (!h) return HMSG_ERR_INVALID;
    return hmsg_boundary(h, [&] { ev_semantic_ranks(h, n, emb, emb_is_f64, D, C, text, class_name_id, target_name_id, rank); });
}

// ---- the host metrics (hmsg_eval_metrics_host.h) behind the C ABI; host arrays
extern "C" int hmsg_eval_floors(const double* gt_lower, const double* gt_upper, int32_t Fg, const double* pred_vertices, int32_t Fp,
                                hmsg_eval_counts* out) {
    return hmsg_boundary("hmsg_eval_floors", -1, [&] {
        HMSG_REQUIRE(out && Fg >= 0 && Fp >= 0 && (Fg == 0 || (gt_lower && gt_upper)) && (Fp == 0 || pred_vertices), HMSG_ERR_INVALID, "null argument");
        eval_metrics::Counts c;
        HMSG_REQUIRE(eval_metrics::floor_metrics(gt_lower, gt_upper, Fg, pred_vertices, Fp, &c), HMSG_ERR_INVALID,
                     "no floors, or " + std::to_string(Fg) + " ground-truth floors against " + std::to_string(Fp) + " predicted (the reference raises there)");
        *out = evm_export(c);
    });
}

extern "C" int hmsg_eval_metrics_from_matrix(const double* M, int32_t P, int32_t G, const int32_t* row_ind, const int32_t* col_ind, int32_t n,
                                             int32_t which_index, double* ap, double* acc, double* prec, double* recall) {
    return hmsg_boundary("hmsg_eval_metrics_from_matrix", -1, [&] {
        evm_check_pairs("hmsg_eval_metrics_from_matrix", M, P, G, row_ind, col_ind, n);
        HMSG_REQUIRE(which_index >= 0 && which_index < eval_metrics::N_THRESH, HMSG_ERR_INVALID, "which_index outside 0 .. 10");
        const eval_metrics::Sweep s = eval_metrics::threshold_sweep(M, row_ind, col_ind, n, P, G);
        if (ap) *ap = s.ap;
        if (acc) *acc = s.acc[which_index];
        if (prec) *prec = s.prec[which_index];
        if (recall) *recall = s.rec_sorted[which_index];
    });
}

extern "C" int hmsg_eval_counts_at(const double* M, int32_t P, int32_t G, const int32_t* row_ind, const int32_t* col_ind, int32_t n, double threshold,
                                   hmsg_eval_counts* out) {
    return hmsg_boundary("hmsg_eval_counts_at", -1, [&] {
        evm_check_pairs("hmsg_eval_counts_at", M, P, G, row_ind, col_ind, n);
        HMSG_REQUIRE(out, HMSG_ERR_INVALID, "null argument");
        *out = evm_export(eval_metrics::counts_at(M, G, row_ind, col_ind, n, P, G, threshold));
    });
}

extern "C" int hmsg_eval_hydra_means(const double* over_pred, const double* over_gt, int32_t P, int32_t G, double* hydra_prec, double* hydra_recall) {
    return hmsg_boundary("hmsg_eval_hydra_means", -1, [&] {
        HMSG_REQUIRE(P > 0 && G > 0 && over_pred && over_gt && hydra_prec && hydra_recall, HMSG_ERR_INVALID, "bad shape or null argument");
        eval_metrics::hydra_means(over_pred, over_gt, P, G, hydra_prec, hydra_recall);
    });
}

extern "C" int hmsg_eval_top_k(const int32_t* rank, int32_t n, int32_t C, const int32_t* top_k, int32_t n_top_k, double* top_k_acc, double* top_k_auc) {
    return hmsg_boundary("hmsg_eval_top_k", -1, [&] {
        HMSG_REQUIRE(n > 0 && C > 0 && rank && n_top_k >= 0 && (n_top_k == 0 || (top_k && top_k_acc)), HMSG_ERR_INVALID, "bad shape or null argument");
        for (int32_t k = 0; k < n_top_k; ++k) top_k_acc[k] = eval_metrics::top_k_acc(rank, n, top_k[k]);
        if (top_k_auc) *top_k_auc = eval_metrics::top_k_auc(rank, n, C);
    });
}

// test hook (include/hmsg_test.h): hmsg_pair_overlaps (hmsg_objmerge.hip), the exhaustive route, on the same arguments
extern "C" int hmsg_test_pair_overlaps(hmsg_t* h, int32_t n, const double* points, const int64_t* off, int64_t n_pairs, const int32_t* pairs,
                                       double radius, uint32_t* counts) {
    if (!h || n < 0 || n_pairs < 0 || !off || (n_pairs > 0 && (!pairs || !counts || !points))) return HMSG_ERR_INVALID;
    return hmsg_boundary(h, [&] {
        HMSG_REQUIRE(n_pairs < (1ll << 30), HMSG_ERR_UNSUPPORTED, "hmsg_test_pair_overlaps: too many pairs");
        std::vector<long long> start((size_t)n);
        std::vector<int> count((size_t)n), pa((size_t)n_pairs), pb((size_t)n_pairs);
        for (int i = 0; i < n; ++i) {
            HMSG_REQUIRE(off[i + 1] >= off[i] && off[i] >= 0, HMSG_ERR_INVALID, "hmsg_test_pair_overlaps: bad offsets");
            start[(size_t)i] = off[i];
            count[(size_t)i] = (int)(off[i + 1] - off[i]);
        }
        for (int64_t p = 0; p < n_pairs; ++p) {
            pa[(size_t)p] = pairs[p * 2], pb[(size_t)p] = pairs[p * 2 + 1];
            HMSG_REQUIRE(pa[(size_t)p] >= 0 && pa[(size_t)p] < n && pb[(size_t)p] >= 0 && pb[(size_t)p] < n, HMSG_ERR_INVALID,
                         "hmsg_test_pair_overlaps: a pair names a cloud that does not exist");
        }
        std::vector<double> ov((size_t)n_pairs);
        hmsg_pair_overlaps(h, points, start.data(), count.data(), (int)n_pairs, pa.data(), pb.data(), radius, ov.data(), counts);
    });
}
