// A12: text-query -> node retrieval over a resident node-embedding table.
//
// Reference: Graph.query_hmsg_object (fsr_vln/memory/hmsg/graph/graph.py:3056-3162), and the plain
// similarity GEMVs of query_floor (:2231-2252) / query_hmsg_room (:3204-3272).
//
//   sim = T[C, D] . E[N', D]^T  (float32 text x float64 embeddings -> float64, graph.py:3127)
//   plain top-k by sim[qid] (descending); with negative prompts: objects whose arg-max class (first max)
//   is the query class, ordered by descending score; if there is none, the plain top-k (graph.py:3133-3151).
//   Exact score ties (bit-equal scores: duplicate embeddings) are broken by candidate position = room order, then
//   node order.  That is what np.argsort(-score) of the negative-prompt path gives for them; the plain path's
//   np.argsort(sim)[::-1] has no defined order for equal keys (numpy's default sort is not stable: for three
//   duplicates it returned 5, 0, 2 in tests/test_emu_parity.py::test_query_exact_score_ties), so only the SET of tied
//   nodes and their scores can be compared there.
//
// MI355X design: the table stays in HBM as float64; all Q x C text rows are scored against ALL nodes by
// one f64-MFMA GEMM (v_mfma_f64_16x16x4_f64), then one workgroup per query walks its candidate rooms
// (CSR room -> nodes) and keeps an exact top-k.
#include "hmsg_boundary.h"
#include "hmsg_query_rules.h"

#include <algorithm>
#include <chrono>

__global__ void k_f32_to_f64(const float* __restrict__ a, double* __restrict__ b, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) b[i] = (double)a[i];
}

// S[M][N] = A[M][D] . B[N][D]^T, one wave per 16x16 tile.
// v_mfma_f64_16x16x4_f64: lane l feeds A[i = l&15][k = l>>4], B[k = l>>4][j = l&15];
// result reg r of lane l is C[row = (l>>4) + 4r][col = l&15].
__global__ void __launch_bounds__(256) k_gemm_f64(const double* __restrict__ A, const double* __restrict__ B, int M, long long N,
                                                  int D, double* __restrict__ S) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long tn = (N + 15) / 16;
    long long tile = (long long)blockIdx.x * 4 + wv;
    const long long ntiles = (long long)((M + 15) / 16) * tn;
    const bool active = tile < ntiles;
    if (!active) tile = ntiles - 1;
    const int m0 = (int)(tile / tn) * 16;
    const long long n0 = (tile % tn) * 16;
    const int ar = m0 + (lane & 15);
    const long long br = n0 + (lane & 15);
    const double* ap = A + (size_t)(ar < M ? ar : M - 1) * D;
    const double* bp = B + (size_t)(br < N ? br : N - 1) * D;
    const f64x4 acc = gemm_f64_tile16(ap, ar < M, bp, br < N, D);
    if (!active) return;
    const long long col = n0 + (lane & 15);
    for (int r = 0; r < 4; ++r) {
        int row = m0 + (lane >> 4) + 4 * r;
        if (row < M && col < N) S[(size_t)row * N + col] = acc[r];
    }
}

// Tiled version for the batched query path: a 256-thread workgroup owns a 128x128 tile of S, the four waves a
// 2x2 arrangement of 64x64 quadrants = 4x4 accumulators of 16x16 (64 result registers per lane).  Per 16-wide k
// step the workgroup stages a 128x16 panel of A and of B in LDS (k-major, one 64-byte global load per thread and
// matrix, double-buffered: the loads of step t+1 are in flight while the 64 MFMAs of step t run), and every wave
// reads 4 + 4 fragments for 16 MFMAs.  128x128x16 multiply-adds per 32 KB staged = 16 FLOP per byte of L2 traffic
// (the one-wave-per-tile kernel above moves 1 byte per FLOP and has no reuse at all).
#define GT 128
#define GK 16
#define GPAD 2
__global__ void __launch_bounds__(256) k_gemm_f64_tiled(const double* __restrict__ A, const double* __restrict__ B, int M,
                                                        long long N, int D, double* __restrict__ S) {
    __shared__ double sa[2][GK][GT + GPAD];
    __shared__ double sb[2][GK][GT + GPAD];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wr = wv >> 1, wc = wv & 1;
    const long long tn = (N + GT - 1) / GT;
    const int m0 = (int)(blockIdx.x / tn) * GT;
    const long long n0 = (long long)(blockIdx.x % tn) * GT;
    // staging: thread t loads 8 consecutive k of row t>>1 (64 bytes) of each matrix
    const int lrow = tid >> 1, lk = (tid & 1) * 8;
    const int ar = m0 + lrow < M ? m0 + lrow : M - 1;
    const long long br = n0 + lrow < N ? n0 + lrow : N - 1;
    const double* ap = A + (size_t)ar * D;
    const double* bp = B + (size_t)br * D;
    f64x4 acc[4][4];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
    double ra[8], rb[8];
    auto load = [&](int k0) {
        for (int u = 0; u < 8; ++u) {
            const int k = k0 + lk + u;
            ra[u] = k < D ? ap[k] : 0.0;
            rb[u] = k < D ? bp[k] : 0.0;
        }
    };
    auto stage = [&](int buf) {
        for (int u = 0; u < 8; ++u) {
            sa[buf][lk + u][lrow] = ra[u];
            sb[buf][lk + u][lrow] = rb[u];
        }
    };
    load(0);
    stage(0);
    __syncthreads();
    const int nk = (D + GK - 1) / GK;
    const int kq = lane >> 4, li = lane & 15;
    for (int t = 0; t < nk; ++t) {
        const int buf = t & 1;
        if (t + 1 < nk) load((t + 1) * GK);
        for (int k = 0; k < GK; k += 4) {
            double fa[4], fb[4];
            for (int i = 0; i < 4; ++i) fa[i] = sa[buf][k + kq][wr * 64 + i * 16 + li];
            for (int j = 0; j < 4; ++j) fb[j] = sb[buf][k + kq][wc * 64 + j * 16 + li];
            for (int i = 0; i < 4; ++i)
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        if (t + 1 < nk) stage(buf ^ 1);
        __syncthreads();
    }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            const long long col = n0 + wc * 64 + j * 16 + li;
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + wr * 64 + i * 16 + kq + 4 * r;
                if (row < M && col < N) S[(size_t)row * N + col] = acc[i][j][r];
            }
        }
}

// One workgroup per query: the exact top k (hmsg_query_rules.h) of the nodes of the query's rooms, in room order then node order.
__global__ void __launch_bounds__(256) k_query_topk(const double* __restrict__ S, long long N, int C, const int* __restrict__ qid,
                                                    const int* __restrict__ q_room_off, const int* __restrict__ q_rooms,
                                                    const int* __restrict__ room_off, const int* __restrict__ room_nodes,
                                                    int n_rooms, int k, int use_neg, int* __restrict__ out_idx,
                                                    int* __restrict__ out_room, double* __restrict__ out_score) {
    __shared__ double sh_s[128];
    __shared__ long long sh_k[128];
    __shared__ int sh_any;
    const int q = blockIdx.x, tid = threadIdx.x;
    const int myq = qid[q];
    const double* Sq = S + (size_t)q * C * N;
    const int* rq = q_rooms + q_room_off[q];
    const int nq = q_room_off[q + 1] - q_room_off[q];
    // this thread's nodes of the query's rooms: f(key, node)
    auto each_node = [&](auto&& f) {
        for (int j = 0; j < nq; ++j) {
            const int r = rq[j];
            if (r < 0 || r >= n_rooms) continue;
            const int b = room_off[r], e = room_off[r + 1];
            for (int t = b + tid; t < e; t += 256) f(qkey(j, t - b), room_nodes[t]);
        }
    };
    if (tid == 0) sh_any = 0;
    __syncthreads();
    // pass 0: does any candidate have arg-max class == query class?
    if (use_neg) {
        int any = 0;
        each_node([&](long long, int node) { any |= argmax_class_is(Sq, N, C, node, myq) ? 1 : 0; });
        if (any) sh_any = 1;
    }
    __syncthreads();
    const bool filtered = use_neg && sh_any;
    pick_top_k<256>(
        k, sh_s, sh_k,
        [&](auto&& offer) {
            each_node([&](long long key, int node) {
                if (!filtered || argmax_class_is(Sq, N, C, node, myq)) offer(Sq[(size_t)myq * N + node], key);
            });
        },
        [&](int round, double s, long long key, bool) {
            if (tid != 0) return;
            const size_t o = (size_t)q * k + round;
            const int r = key != QKEY_NONE ? rq[qkey_j(key)] : -1;
            out_idx[o] = r >= 0 ? room_nodes[room_off[r] + qkey_place(key)] : -1;
            out_room[o] = r;
            out_score[o] = r >= 0 ? s : 0.0;
        });
}

// the room level of one index, as room_select sees it for query q
struct IndexRooms {
    const double *S_room, *S_view;       // this query's rows
    const int *view_off, *keys, *list;   // list: the floor's rooms, or NULL for all rooms in order
    int L;
    bool bad_floor;
    __device__ int room_at(int i) const { return list ? list[i] : i; }
    __device__ double name_sim(int i) const { return S_room[room_at(i)]; }
    __device__ double view_max(int i) const {
        const int r = room_at(i);
        double mx = -1e308;
        for (int v = view_off[r]; v < view_off[r + 1]; ++v) mx = fmax(mx, S_view[v]);
        return mx;
    }
    __device__ bool has_views(int i) const { return view_off[room_at(i) + 1] != view_off[room_at(i)]; }
    __device__ int room_key(int r) const { return keys[r]; }
};
// The room selection (hmsg_query_rules.h) over the index's own tables, one workgroup per query.
__global__ void __launch_bounds__(256) k_room_select(int n_rooms, int n_floors, const double* __restrict__ S_room,
                                                     const double* __restrict__ S_view, long long n_views,
                                                     const int* __restrict__ view_off, const int* __restrict__ room_key,
                                                     const int* __restrict__ floor_room_off, const int* __restrict__ floor_rooms,
                                                     const int* __restrict__ floor_id, const int* __restrict__ mode, int max_sel,
                                                     int* __restrict__ sel, int* __restrict__ nsel, int* __restrict__ q_rooms,
                                                     int* __restrict__ err) {
    const int q = blockIdx.x, f = floor_id[q];
    IndexRooms src;
    src.S_room = S_room + (size_t)q * n_rooms;
    src.S_view = S_view + (size_t)q * n_views;
    src.view_off = view_off;
    src.keys = room_key;
    src.bad_floor = f >= n_floors;
    src.list = f < 0 || src.bad_floor ? nullptr : floor_rooms + floor_room_off[f];
    src.L = f < 0 ? n_rooms : (src.bad_floor ? 0 : floor_room_off[f + 1] - floor_room_off[f]);
    room_select(src, mode[q], max_sel, sel + (size_t)q * max_sel, nsel + q, q_rooms + (size_t)q * max_sel, err + q);
}
__global__ void k_fill_offsets(int* off, int n, int stride) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) off[i] = i * stride;
}

namespace {
// S[M][N] = A[M][D] . B[N][D]^T  (B = the node table unless given)
void gemm(hmsg_index* ix, const double* A, int M, double* S, const double* B = nullptr, long long N = -1) {
    if (!B) {
        B = ix->E.p;
        N = ix->N;
    }
    if (M >= 64 && N >= 64) {                // (the tiled kernel: timed when profiling is on)
        ProfScope ps(ix->prof, ix->stream, "k_gemm_f64", 2.0 * (double)M * (double)N * (double)ix->D);
        hmsg_gemm_f64(A, M, B, N, ix->D, S, ix->stream);
        return;
    }
    hmsg_gemm_f64(A, M, B, N, ix->D, S, ix->stream);
}
}  // namespace

void hmsg_gemm_f64(const double* A, int M, const double* B, long long N, int D, double* S, hipStream_t s) {
    if (M <= 0 || N <= 0) return;
    if (M >= 64 && N >= 64) {
        const long long tiles = (long long)((M + GT - 1) / GT) * ((N + GT - 1) / GT);
        hipLaunchKernelGGL(k_gemm_f64_tiled, dim3((unsigned)tiles), dim3(256), 0, s, A, B, M, N, D, S);
    } else {
        const long long tiles = (long long)((M + 15) / 16) * ((N + 15) / 16);
        hipLaunchKernelGGL(k_gemm_f64, dim3(cdiv((size_t)tiles, 4)), dim3(256), 0, s, A, B, M, N, D, S);
    }
    HMSG_CHECK_LAUNCH();
}

hmsg_index* hmsg_index_create_rooms_only(int device, int D) {
    hmsg_index* ix = new hmsg_index();
    ix->device = device;
    ix->D = D;
    try {
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipStreamCreateWithFlags(&ix->stream, hipStreamNonBlocking));
        ix->room_off.alloc(1);
        const int zero = 0;
        HIP_TRY(hipMemcpy(ix->room_off.p, &zero, 4, hipMemcpyHostToDevice));
    } catch (...) {
        hmsg_index_destroy(ix);
        throw;
    }
    return ix;
}

QueryScan hmsg_query_scan(int Q, const int* room_mode, const int* floor_id) {
    QueryScan sc;
    for (int q = 0; q < Q; ++q) {
        sc.in_range = sc.in_range && room_mode[q] >= 0 && room_mode[q] <= 3 && floor_id[q] >= -1;
        sc.need_label |= room_mode[q] == 1;
        sc.need_view |= room_mode[q] >= 2;
        sc.max_floor = std::max(sc.max_floor, floor_id[q]);
    }
    return sc;
}
std::string hmsg_query_precondition(const char* who, const QueryScan& sc, int n_floors, bool have_room_text, bool have_room_names) {
    const std::string w = std::string(who) + ": ";
    if (!sc.in_range || (n_floors >= 0 && sc.max_floor >= n_floors)) return w + "bad floor id / room mode";
    if ((sc.need_label || sc.need_view) && !have_room_text) return w + "room text rows missing";
    if (sc.need_label && !have_room_names) return w + "label mode without room name embeddings";
    return "";
}
void hmsg_text_rows_to_f64(hipStream_t s, const float* src, size_t n, DevBuf<float>& tmp, DevBuf<double>& dst) {
    dst.ensure(n);
    src = stage_in(tmp, src, n, s, Up::bounce, true);
    hipLaunchKernelGGL(k_f32_to_f64, dim3(cdiv(n, 256)), dim3(256), 0, s, src, dst.p, n);
    HMSG_CHECK_LAUNCH();
}
bool hmsg_query_pack_words(int* h_words, int Q, const int* floor_id, const int* room_mode, const int* qid) {
    memcpy(h_words, floor_id, (size_t)Q * 4);
    memcpy(h_words + Q, room_mode, (size_t)Q * 4);
    const bool qid_dev = hmsg_is_device_ptr(qid);
    if (!qid_dev) memcpy(h_words + 2 * (size_t)Q, qid, (size_t)Q * 4);
    return qid_dev;
}
void QueryOut::give(const char* who, hipStream_t s, const char* d, const char* h, double* out_score, int* out_sel, int* out_nsel, int* out_idx,
                    int* out_room) const {
    bool any_dev = false;
    auto one = [&](void* dst, size_t off, size_t n) {
        if (hmsg_is_device_ptr(dst)) {
            HIP_TRY(hipMemcpyAsync(dst, d + off, n, hipMemcpyDeviceToDevice, s));
            any_dev = true;
        } else {
            memcpy(dst, h + off, n);
        }
    };
    one(out_score, 0, (size_t)Q * k * 8);
    one(out_sel, o_sel, (size_t)Q * max_rooms * 4);
    one(out_nsel, o_nsel, (size_t)Q * 4);
    one(out_idx, o_idx, (size_t)Q * k * 4);
    one(out_room, o_room, (size_t)Q * k * 4);
    if (any_dev) HIP_TRY(hipStreamSynchronize(s));
    const int* herr = (const int*)(h + o_err);
    for (int q = 0; q < Q; ++q)
        HMSG_REQUIRE(!herr[q], HMSG_ERR_INVALID,
                     std::string(who) + ": a query's room stage failed like the reference would (a room without view embeddings, or a "
                                        "view-mode room number that is no position of the floor's room list)");
}

extern "C" {

int hmsg_index_create(int32_t device_id, int32_t dim, int64_t n, const void* emb, int32_t emb_is_f64, const int32_t* room_of_node,
                      hmsg_index_t** out) {
    if (!out) return HMSG_ERR_INVALID;
    *out = nullptr;
    if (dim <= 0 || n <= 0 || !emb || !room_of_node) return HMSG_ERR_INVALID;
    hmsg_index* ix = nullptr;
    const int rc = hmsg_boundary("hmsg_index_create", device_id, [&] {
        ix = new hmsg_index();
        ix->device = device_id;
        ix->D = dim;
        ix->N = n;
        HIP_TRY(hipStreamCreateWithFlags(&ix->stream, hipStreamNonBlocking));
        ix->E.alloc((size_t)n * dim);
        const size_t cnt = (size_t)n * dim;
        if (emb_is_f64) {
            copy_in(ix->E.p, emb, cnt * 8, ix->stream, Up::bounce);
        } else {
            DevBuf<float> tmp;               // (a device table is widened straight from the caller's memory)
            const float* e32 = stage_in(tmp, (const float*)emb, cnt, ix->stream, Up::bounce);
            hipLaunchKernelGGL(k_f32_to_f64, dim3(cdiv(cnt, 256)), dim3(256), 0, ix->stream, e32, ix->E.p, cnt);
            HMSG_CHECK_LAUNCH();
            HIP_TRY(hipStreamSynchronize(ix->stream));
        }
        std::vector<int> rooms((size_t)n);
        read_in(rooms.data(), room_of_node, (size_t)n * 4);
        int nr = 0;
        for (int r : rooms) {
            HMSG_REQUIRE(r >= 0, HMSG_ERR_INVALID, "negative room id");
            nr = std::max(nr, r + 1);
        }
        ix->n_rooms = nr;
        std::vector<int> off(nr + 1, 0), nodes((size_t)n);
        for (int r : rooms) off[r + 1]++;
        for (int r = 0; r < nr; ++r) off[r + 1] += off[r];
        std::vector<int> cur(off.begin(), off.end() - 1);
        for (long long i = 0; i < n; ++i) nodes[cur[rooms[i]]++] = (int)i;
        ix->room_of.alloc((size_t)n);
        ix->room_off.alloc(nr + 1);
        ix->room_nodes.alloc((size_t)n);
        HIP_TRY(hipMemcpyAsync(ix->room_of.p, rooms.data(), (size_t)n * 4, hipMemcpyHostToDevice, ix->stream));
        HIP_TRY(hipMemcpyAsync(ix->room_off.p, off.data(), (size_t)(nr + 1) * 4, hipMemcpyHostToDevice, ix->stream));
        HIP_TRY(hipMemcpyAsync(ix->room_nodes.p, nodes.data(), (size_t)n * 4, hipMemcpyHostToDevice, ix->stream));
        HIP_TRY(hipStreamSynchronize(ix->stream));
    });
    if (rc != HMSG_OK) {
        delete ix;
        return rc;
    }
    *out = ix;
    return HMSG_OK;
}

void hmsg_index_destroy(hmsg_index_t* ix) {
    if (!ix) return;
    (void)hipSetDevice(ix->device);
    if (ix->stream) {
        (void)hipStreamSynchronize(ix->stream);
        (void)hipStreamDestroy(ix->stream);
    }
    ix->prof.clear();
    delete ix;
}

const char* hmsg_index_last_error(const hmsg_index_t* ix) { return ix ? ix->err.c_str() : "null index"; }

int hmsg_index_set_profiling(hmsg_index_t* ix, int32_t on) {
    if (!ix) return HMSG_ERR_INVALID;
    ix->prof.enabled = on != 0;
    return HMSG_OK;
}
// launches, total milliseconds and total FLOP of the similarity GEMM since the index was created
int hmsg_index_profile(hmsg_index_t* ix, int64_t* launches, double* total_ms, double* total_flop) {
    if (!ix || !launches || !total_ms || !total_flop) return HMSG_ERR_INVALID;
    (void)hipStreamSynchronize(ix->stream);
    *launches = 0;
    *total_ms = *total_flop = 0.0;
    for (auto& e : ix->prof.ev) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, e.a, e.b) != hipSuccess) continue;
        ++*launches;
        *total_ms += t;
        *total_flop += e.work;
    }
    return HMSG_OK;
}

int hmsg_query_objects(hmsg_index_t* ix, int32_t Q, int32_t C, const float* T, const int32_t* qid, const int32_t* room_off,
                       const int32_t* rooms, int32_t k, int32_t use_negatives, int32_t* out_idx, int32_t* out_room,
                       double* out_score) {
    if (!ix) return HMSG_ERR_INVALID;
    return hmsg_boundary(ix, [&] {
        HMSG_REQUIRE(Q >= 0 && C >= 1 && T && qid && room_off && k >= 1 && out_idx && out_room && out_score, HMSG_ERR_INVALID,
                     "hmsg_query_objects: bad argument");
        if (Q == 0) return;
        const size_t nT = (size_t)Q * C * ix->D;
        hmsg_text_rows_to_f64(ix->stream, T, nT, ix->Tf, ix->T64);
        ix->S.ensure((size_t)Q * C * ix->N);
        gemm(ix, ix->T64.p, Q * C, ix->S.p);
        std::vector<int> hoff(Q + 1);
        read_in(hoff.data(), room_off, (size_t)(Q + 1) * 4);
        const int nr = hoff[Q];
        HMSG_REQUIRE(nr == 0 || rooms, HMSG_ERR_INVALID, "rooms list missing");
        ix->d_qid.ensure(Q);
        ix->d_roff.ensure(Q + 1);
        ix->d_rooms.ensure(std::max(nr, 1));
        ix->d_oidx.ensure((size_t)Q * k);
        ix->d_oroom.ensure((size_t)Q * k);
        ix->d_oscore.ensure((size_t)Q * k);
        copy_in(ix->d_qid.p, qid, (size_t)Q * 4, ix->stream, Up::direct);
        HIP_TRY(hipMemcpyAsync(ix->d_roff.p, hoff.data(), (size_t)(Q + 1) * 4, hipMemcpyHostToDevice, ix->stream));
        copy_in(ix->d_rooms.p, rooms, (size_t)nr * 4, ix->stream, Up::direct);
        hipLaunchKernelGGL(k_query_topk, dim3(Q), dim3(256), 0, ix->stream, (const double*)ix->S.p, ix->N, C, (const int*)ix->d_qid.p,
                           (const int*)ix->d_roff.p, (const int*)ix->d_rooms.p, (const int*)ix->room_off.p,
                           (const int*)ix->room_nodes.p, ix->n_rooms, k, use_negatives, ix->d_oidx.p, ix->d_oroom.p, ix->d_oscore.p);
        HMSG_CHECK_LAUNCH();
        HIP_TRY(hipMemcpyAsync(out_idx, ix->d_oidx.p, (size_t)Q * k * 4, hipMemcpyDeviceToHost, ix->stream));
        HIP_TRY(hipMemcpyAsync(out_room, ix->d_oroom.p, (size_t)Q * k * 4, hipMemcpyDeviceToHost, ix->stream));
        HIP_TRY(hipMemcpyAsync(out_score, ix->d_oscore.p, (size_t)Q * k * 8, hipMemcpyDeviceToHost, ix->stream));
        HIP_TRY(hipStreamSynchronize(ix->stream));
    });
}

int hmsg_index_set_hierarchy(hmsg_index_t* ix, int32_t n_rooms, int32_t n_floors, const int32_t* floor_room_off, const int32_t* floor_rooms,
                             const double* room_name_emb, const int64_t* view_off, const double* view_emb, const int32_t* room_key) {
    if (!ix) return HMSG_ERR_INVALID;
    return hmsg_boundary(ix, [&] {
        const int R = n_rooms;                   // (rooms without objects included: >= the largest room id of a node + 1)
        HMSG_REQUIRE(R >= ix->n_rooms && n_floors >= 0 && (n_floors == 0 || (floor_room_off && floor_rooms)) && view_off && room_key,
                     HMSG_ERR_INVALID, "hmsg_index_set_hierarchy: bad argument");
        ix->h_rooms = R;
        for (int f = 0; f < n_floors; ++f)
            for (int j = floor_room_off[f]; j < floor_room_off[f + 1]; ++j)
                HMSG_REQUIRE(floor_rooms[j] >= 0 && floor_rooms[j] < R, HMSG_ERR_INVALID, "hmsg_index_set_hierarchy: room id out of range");
        const long long NV = view_off[R];
        HMSG_REQUIRE(NV >= 0 && NV < (1ll << 31) && (NV == 0 || view_emb), HMSG_ERR_INVALID, "hmsg_index_set_hierarchy: bad view table");
        ix->n_floors = n_floors;
        ix->n_views = NV;
        std::vector<int> voff((size_t)R + 1);
        for (int r = 0; r <= R; ++r) voff[(size_t)r] = (int)view_off[r];
        ix->view_off.alloc((size_t)R + 1);
        ix->room_key.alloc((size_t)std::max(R, 1));
        ix->floor_room_off.alloc((size_t)n_floors + 1);
        const int nfr = n_floors ? floor_room_off[n_floors] : 0;
        ix->floor_rooms.alloc((size_t)std::max(nfr, 1));
        HIP_TRY(hipMemcpyAsync(ix->view_off.p, voff.data(), ((size_t)R + 1) * 4, hipMemcpyHostToDevice, ix->stream));
        HIP_TRY(hipMemcpyAsync(ix->room_key.p, room_key, (size_t)R * 4, hipMemcpyHostToDevice, ix->stream));
        std::vector<int> zero(1, 0);
        HIP_TRY(hipMemcpyAsync(ix->floor_room_off.p, n_floors ? floor_room_off : zero.data(), ((size_t)n_floors + 1) * 4, hipMemcpyHostToDevice, ix->stream));
        if (nfr) HIP_TRY(hipMemcpyAsync(ix->floor_rooms.p, floor_rooms, (size_t)nfr * 4, hipMemcpyHostToDevice, ix->stream));
        if (room_name_emb) {
            ix->room_name_emb.alloc((size_t)std::max(R, 1) * ix->D);
            copy_in(ix->room_name_emb.p, room_name_emb, (size_t)R * ix->D * 8, ix->stream, Up::bounce);
        } else {
            ix->room_name_emb.release();
        }
        ix->view_emb.alloc((size_t)std::max<long long>(NV, 1) * ix->D);
        copy_in(ix->view_emb.p, view_emb, (size_t)NV * ix->D * 8, ix->stream, Up::bounce);
        HIP_TRY(hipStreamSynchronize(ix->stream));
        ix->have_hier = true;
    });
}

int hmsg_query_hier(hmsg_index_t* ix, int32_t Q, int32_t C, const float* T_obj, const int32_t* qid, const float* T_room,
                    const int32_t* floor_id, const int32_t* room_mode, int32_t k, int32_t use_negatives, int32_t max_rooms,
                    int32_t* out_sel, int32_t* out_nsel, int32_t* out_idx, int32_t* out_room, double* out_score) {
    if (!ix) return HMSG_ERR_INVALID;
    return hmsg_boundary(ix, [&] {
        HMSG_REQUIRE(ix->have_hier, HMSG_ERR_INVALID, "hmsg_query_hier: hmsg_index_set_hierarchy first");
        HMSG_REQUIRE(Q >= 0 && C >= 1 && T_obj && qid && floor_id && room_mode && k >= 1 && max_rooms >= 1 && out_sel && out_nsel && out_idx &&
                         out_room && out_score,
                     HMSG_ERR_INVALID, "hmsg_query_hier: bad argument");
        if (Q == 0) return;
        const int R = ix->h_rooms;
        // HMSG_DEBUG_TIMING: where a call spends its time (each lap drains the stream first)
        static const bool dbg = getenv("HMSG_DEBUG_TIMING") != nullptr;
        auto t_prev = std::chrono::steady_clock::now();
        auto lap = [&](const char* what) {
            if (!dbg) return;
            (void)hipStreamSynchronize(ix->stream);
            const auto t = std::chrono::steady_clock::now();
            fprintf(stderr, "[hmsg query_hier] %-22s %.3f ms\n", what, std::chrono::duration<double, std::milli>(t - t_prev).count());
            t_prev = t;
        };
        const QueryScan sc = hmsg_query_scan(Q, room_mode, floor_id);
        const bool need_label = sc.need_label, need_view = sc.need_view;
        const std::string why = hmsg_query_precondition("hmsg_query_hier", sc, ix->n_floors, T_room != nullptr, ix->room_name_emb.p != nullptr);
        HMSG_REQUIRE(why.empty(), HMSG_ERR_INVALID, why);
        // room stage: similarities of the room text with the room names / the view embeddings (float64 MFMA GEMM)
        ix->S_room.ensure((size_t)Q * std::max(R, 1));
        ix->S_view.ensure((size_t)Q * std::max<long long>(ix->n_views, 1));
        if (need_label || need_view) {
            hmsg_text_rows_to_f64(ix->stream, T_room, (size_t)Q * ix->D, ix->Tr, ix->Tr64);
            if (need_label) gemm(ix, ix->Tr64.p, Q, ix->S_room.p, ix->room_name_emb.p, R);
            if (need_view && ix->n_views) gemm(ix, ix->Tr64.p, Q, ix->S_view.p, ix->view_emb.p, ix->n_views);
        }
        lap("room text + room GEMM");
        // per-query words: one packed upload from pinned memory
        ix->h_qin.ensure((size_t)Q * 3 + 4);
        ix->d_qin.ensure((size_t)Q * 3 + 4);
        const bool qid_dev = hmsg_query_pack_words(ix->h_qin.p, Q, floor_id, room_mode, qid);
        upload_pinned(ix->d_qin.p, ix->h_qin.p, (((size_t)Q * 3 + 3) / 4) * 16, ix->stream);
        int* const d_floor = ix->d_qin.p;
        int* const d_mode = ix->d_qin.p + Q;
        int* const d_qid = ix->d_qin.p + 2 * (size_t)Q;
        if (qid_dev) HIP_TRY(hipMemcpyAsync(d_qid, qid, (size_t)Q * 4, hipMemcpyDeviceToDevice, ix->stream));
        const QueryOut out(Q, k, max_rooms);
        ix->d_qout.ensure(out.bytes);
        ix->h_qout.ensure(out.bytes);
        char* const d_out = ix->d_qout.p;
        ix->d_rooms.ensure((size_t)Q * max_rooms);
        ix->d_roff.ensure((size_t)Q + 1);
        hipLaunchKernelGGL(k_room_select, dim3(Q), dim3(256), 0, ix->stream, R, ix->n_floors, (const double*)ix->S_room.p,
                           (const double*)ix->S_view.p, ix->n_views, (const int*)ix->view_off.p, (const int*)ix->room_key.p,
                           (const int*)ix->floor_room_off.p, (const int*)ix->floor_rooms.p, (const int*)d_floor,
                           (const int*)d_mode, max_rooms, out.sel(d_out), out.nsel(d_out), ix->d_rooms.p, out.err(d_out));
        hipLaunchKernelGGL(k_fill_offsets, dim3(cdiv((size_t)Q + 1, 256)), dim3(256), 0, ix->stream, ix->d_roff.p, Q, max_rooms);
        HMSG_CHECK_LAUNCH();
        lap("room select");
        // object stage on the rooms the room stage picked, in that order
        hmsg_text_rows_to_f64(ix->stream, T_obj, (size_t)Q * C * ix->D, ix->Tf, ix->T64);
        lap("object text upload");
        ix->S.ensure((size_t)Q * C * ix->N);
        lap("S alloc");
        gemm(ix, ix->T64.p, Q * C, ix->S.p);
        lap("object GEMM");
        hipLaunchKernelGGL(k_query_topk, dim3(Q), dim3(256), 0, ix->stream, (const double*)ix->S.p, ix->N, C, (const int*)d_qid,
                           (const int*)ix->d_roff.p, (const int*)ix->d_rooms.p, (const int*)ix->room_off.p,
                           (const int*)ix->room_nodes.p, ix->n_rooms, k, use_negatives, out.idx(d_out), out.room(d_out), out.score(d_out));
        HMSG_CHECK_LAUNCH();
        lap("top-k");
        HIP_TRY(hipMemcpyAsync(ix->h_qout.p, d_out, out.bytes, hipMemcpyDeviceToHost, ix->stream));
        HIP_TRY(hipStreamSynchronize(ix->stream));
        out.give("hmsg_query_hier", ix->stream, d_out, ix->h_qout.p, out_score, out_sel, out_nsel, out_idx, out_room);
        lap("read-back");
    });
}

int hmsg_similarity(hmsg_index_t* ix, int32_t Q, const float* T, double* S) {
    if (!ix) return HMSG_ERR_INVALID;
    return hmsg_boundary(ix, [&] {
        HMSG_REQUIRE(Q >= 0 && T && S, HMSG_ERR_INVALID, "hmsg_similarity: bad argument");
        if (Q == 0) return;
        hmsg_text_rows_to_f64(ix->stream, T, (size_t)Q * ix->D, ix->Tf, ix->T64);
        ix->S.ensure((size_t)Q * ix->N);
        gemm(ix, ix->T64.p, Q, ix->S.p);
        HIP_TRY(hipMemcpyAsync(S, ix->S.p, (size_t)Q * ix->N * 8, hipMemcpyDeviceToHost, ix->stream));
        HIP_TRY(hipStreamSynchronize(ix->stream));
    });
}

}  // extern "C"
