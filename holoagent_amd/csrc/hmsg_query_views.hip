// The view level of the slow path: what Graph.query_room_obj_slow_reasoning (fsr_vln/memory/hmsg/graph/graph.py:2578-3054) computes
// between its VLM calls, batched over Q queries.
//
//   a. goal views (:2864-2897): the object text against the CLIP embedding of every sampled image of every room of the list
//      (rows in rooms-list order, within a room in sample_images order), np.argmax and the top 24.
//      Order here: descending score, exact ties (bit-equal scores) by ascending candidate position.  Row 0 is np.argmax(sims) (first
//      maximum); the rest is np.argsort(sims)[-k:][::-1] wherever scores differ -- numpy's order of bit-equal keys is undefined
//      (its default sort is not stable: hmsg_query.hip's header has a measured case), so only the set of tied rows compares there.
//   b. re-match in a view (:2962-2986): the text against the embeddings of view.object_ids' objects in that order, np.argmax (first
//      maximum).  A view without objects gives -1 (the reference skips it, :2974).
//   c. the two distances it reports: visualize_pcd_on_image's avg_distance (utils/graph_utils.py:49-70: mean camera z of the points
//      with z > 0) and check_object_in_view(..., return_depth=True) (utils/graph_utils.py:95-157; graph.py:3011-3022).
//
// MI355X design.  (a) one float64 MFMA GEMM of all Q text rows against the resident table (hmsg_gemm_f64), then one workgroup per
// query walks the image rows of its rooms and keeps the exact top k (pick_top_k of hmsg_query_rules.h).  (b) one workgroup per
// query; a wave scores 16 of the view's objects at a time with the GEMM's own 16x16 tile chain on the gathered rows
// (gemm_f64_tile16: the k order of hmsg_similarity, so a score has hmsg_similarity's bits), the best (score, position) goes through a
// wave reduction and LDS.  (c) two stages: a workgroup sums a slice of at most VD_SLICE points of one cloud (thread-strided, wave
// tree, the four waves in order), then one wave per pair adds the slices' partial sums (lane-strided, wave tree) -- fixed orders and
// no floating-point atomics, so a result does not change from run to run.  All three are bound by launch latency at the sizes a
// query application has.
#include "hmsg_query_views.h"

#include "hmsg_boundary.h"
#include "hmsg_query_rules.h"
#include "hmsg_view_project.h"

#include <algorithm>
#include <cmath>

// ------------------------------------------------------------------------------------------------ a. goal views
// One workgroup per query: the exact top kk (<= k) of the image rows of the query's rooms; entries kk .. k are padded.
__global__ void __launch_bounds__(256) k_goal_views_topk(const double* __restrict__ S, long long NI, const int* __restrict__ floor_id,
                                                         int n_rooms, const int* __restrict__ floor_room_off, const int* __restrict__ floor_rooms,
                                                         const int* __restrict__ img_off, const long long* __restrict__ img_id, int k, int kk,
                                                         long long* __restrict__ out_img, int* __restrict__ out_room, double* __restrict__ out_score,
                                                         int* __restrict__ out_n) {
    __shared__ double sh_s[128];
    __shared__ long long sh_k[128];
    const int q = blockIdx.x, tid = threadIdx.x, f = floor_id[q];
    const double* Sq = S + (size_t)q * NI;
    const int* list = f < 0 ? nullptr : floor_rooms + floor_room_off[f];
    const int L = f < 0 ? n_rooms : floor_room_off[f + 1] - floor_room_off[f];
    for (int i = kk + tid; i < k; i += 256) {
        out_img[(size_t)q * k + i] = -1;
        out_room[(size_t)q * k + i] = -1;
        out_score[(size_t)q * k + i] = 0.0;
    }
    int found = 0;
    pick_top_k<256>(
        kk, sh_s, sh_k,
        [&](auto&& offer) {
            for (int j = 0; j < L; ++j) {
                const int r = list ? list[j] : j;
                const int b = img_off[r], e = img_off[r + 1];
                for (int t = b + tid; t < e; t += 256) offer(Sq[t], qkey(j, t - b));
            }
        },
        [&](int round, double s, long long key, bool) {
            if (tid != 0) return;
            const size_t o = (size_t)q * k + round;
            const int r = key != QKEY_NONE ? (list ? list[qkey_j(key)] : qkey_j(key)) : -1;
            out_img[o] = r >= 0 ? img_id[img_off[r] + qkey_place(key)] : -1;
            out_room[o] = r;
            out_score[o] = r >= 0 ? s : 0.0;
            found += r >= 0 ? 1 : 0;
        });
    if (tid == 0) out_n[q] = found;
}

struct hmsg_goal_table {
    int device = 0, D = 0, R = 0, n_floors = 0;
    long long NI = 0;
    hipStream_t stream = nullptr;
    DevBuf<double> E;                // [NI][D]
    DevBuf<int> img_off, floor_room_off, floor_rooms;
    DevBuf<long long> img_id;
    // scratch
    DevBuf<float> Tf, E32;
    DevBuf<double> T64, S, d_score;
    DevBuf<int> d_floor, d_room, d_n;
    DevBuf<long long> d_img;
};

hmsg_goal_table* hmsg_goal_table_create(int device, int D, int n_rooms, const std::vector<int>& img_off, const std::vector<float>& clip,
                                        const std::vector<long long>& img_id, const std::vector<int>& floor_room_off, const std::vector<int>& floor_rooms) {
    HMSG_REQUIRE(D > 0 && n_rooms >= 0 && (int)img_off.size() == n_rooms + 1 && !floor_room_off.empty(), HMSG_ERR_INVALID, "goal view table: bad argument");
    const long long NI = img_off[(size_t)n_rooms];
    HMSG_REQUIRE((long long)img_id.size() == NI && clip.size() == (size_t)NI * (size_t)D, HMSG_ERR_INVALID, "goal view table: rows and ids differ in number");
    hmsg_goal_table* t = new hmsg_goal_table();
    try {
        HIP_TRY(hipSetDevice(device));
        t->device = device;
        t->D = D;
        t->R = n_rooms;
        t->n_floors = (int)floor_room_off.size() - 1;
        t->NI = NI;
        HIP_TRY(hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking));
        hipStream_t s = t->stream;
        if (!NI) t->E.alloc(1);
        t->img_off.alloc(img_off.size());
        t->img_id.alloc((size_t)std::max<long long>(NI, 1));
        t->floor_room_off.alloc(floor_room_off.size());
        t->floor_rooms.alloc(std::max<size_t>(floor_rooms.size(), 1));
        HIP_TRY(hipMemcpyAsync(t->img_off.p, img_off.data(), img_off.size() * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(t->floor_room_off.p, floor_room_off.data(), floor_room_off.size() * 4, hipMemcpyHostToDevice, s));
        if (!floor_rooms.empty()) HIP_TRY(hipMemcpyAsync(t->floor_rooms.p, floor_rooms.data(), floor_rooms.size() * 4, hipMemcpyHostToDevice, s));
        if (NI) {
            const size_t cnt = (size_t)NI * D;
            HIP_TRY(hipMemcpyAsync(t->img_id.p, img_id.data(), (size_t)NI * 8, hipMemcpyHostToDevice, s));
            t->E.alloc(cnt);                                   // (exactly: the table stays for the graph's life)
            hmsg_text_rows_to_f64(s, clip.data(), cnt, t->E32, t->E);
        }
        HIP_TRY(hipStreamSynchronize(s));
        t->E32.release();
    } catch (...) {
        hmsg_goal_table_free(t);
        throw;
    }
    return t;
}

void hmsg_goal_table_free(hmsg_goal_table* t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    if (t->stream) {
        (void)hipStreamSynchronize(t->stream);
        (void)hipStreamDestroy(t->stream);
    }
    delete t;
}

void hmsg_goal_table_topk(hmsg_goal_table* t, int Q, const float* T, const int* floor_id, int k, long long* out_img, int* out_room, double* out_score,
                          int* out_n) {
    HMSG_REQUIRE(Q >= 0 && k >= 1 && (Q == 0 || (T && floor_id && out_img && out_room && out_score && out_n)), HMSG_ERR_INVALID,
                 "hmsg_graph_goal_views: bad argument");
    if (Q == 0) return;
    for (int q = 0; q < Q; ++q)
        HMSG_REQUIRE(floor_id[q] >= -1 && floor_id[q] < t->n_floors, HMSG_ERR_INVALID, "hmsg_graph_goal_views: floor id out of range");
    HIP_TRY(hipSetDevice(t->device));
    hipStream_t s = t->stream;
    const size_t nk = (size_t)Q * (size_t)k;
    t->d_floor.ensure((size_t)Q);
    t->d_img.ensure(nk);
    t->d_room.ensure(nk);
    t->d_score.ensure(nk);
    t->d_n.ensure((size_t)Q);
    HIP_TRY(hipMemcpyAsync(t->d_floor.p, floor_id, (size_t)Q * 4, hipMemcpyHostToDevice, s));
    const int kk = (int)std::min<long long>(k, t->NI);
    if (t->NI) {
        hmsg_text_rows_to_f64(s, T, (size_t)Q * t->D, t->Tf, t->T64);
        t->S.ensure((size_t)Q * (size_t)t->NI);
        hmsg_gemm_f64(t->T64.p, Q, t->E.p, t->NI, t->D, t->S.p, s);
    } else {
        t->S.ensure(1);
    }
    hipLaunchKernelGGL(k_goal_views_topk, dim3((unsigned)Q), dim3(256), 0, s, (const double*)t->S.p, t->NI, (const int*)t->d_floor.p, t->R,
                       (const int*)t->floor_room_off.p, (const int*)t->floor_rooms.p, (const int*)t->img_off.p, (const long long*)t->img_id.p, k, kk,
                       t->d_img.p, t->d_room.p, t->d_score.p, t->d_n.p);
    HMSG_CHECK_LAUNCH();
    copy_out(out_img, t->d_img.p, nk * 8, s);
    copy_out(out_room, t->d_room.p, nk * 4, s);
    copy_out(out_score, t->d_score.p, nk * 8, s);
    copy_out(out_n, t->d_n.p, (size_t)Q * 4, s);
    HIP_TRY(hipStreamSynchronize(s));
}

// ------------------------------------------------------------------------------------------------ b. re-match in a view
// One workgroup (4 waves) per query.  The view's nodes come 16 to a wave pass: lane l scores position 16 * group + (l & 15) -- the
// text row is every row of the A tile, so row 0 of the result (register 0 of lanes 0 .. 15) holds the 16 scores.
__global__ void __launch_bounds__(256) k_rematch_views(const double* __restrict__ T64, const double* __restrict__ E, int D, const int* __restrict__ view,
                                                       const long long* __restrict__ vo_off, const int* __restrict__ vo_nodes,
                                                       int* __restrict__ out_node, double* __restrict__ out_score) {
    __shared__ double s_s[4];
    __shared__ long long s_k[4];
    const int q = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15;
    const long long b = vo_off[view[q]], n = vo_off[view[q] + 1] - b;
    const double* tq = T64 + (size_t)q * D;
    double bs = -INFINITY;
    long long bk = QKEY_NONE;
    const long long groups = (n + 15) / 16;
    for (long long g = wv; g < groups; g += 4) {                    // (wave-uniform: every lane takes part in the MFMA chain)
        const long long pos = g * 16 + li;
        const bool ok = pos < n;
        const int node = vo_nodes[b + (ok ? pos : n - 1)];
        const f64x4 acc = gemm_f64_tile16(tq, true, E + (size_t)node * D, ok, D);
        if (lane < 16 && ok && better(acc[0], pos, bs, bk)) {
            bs = acc[0];
            bk = pos;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {                              // the wave's best (score, position)
        const double os = __shfl_xor(bs, o);
        const long long ok = __shfl_xor(bk, o);
        if (better(os, ok, bs, bk)) {
            bs = os;
            bk = ok;
        }
    }
    if (lane == 0) {
        s_s[wv] = bs;
        s_k[wv] = bk;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w)
            if (better(s_s[w], s_k[w], bs, bk)) {
                bs = s_s[w];
                bk = s_k[w];
            }
        out_node[q] = bk != QKEY_NONE ? vo_nodes[b + bk] : -1;
        out_score[q] = bk != QKEY_NONE ? bs : 0.0;
    }
}

extern "C" int hmsg_index_set_views(hmsg_index_t* ix, int64_t n_views, const int64_t* view_obj_off, const int32_t* view_objs) {
    if (!ix) return HMSG_ERR_INVALID;
    return hmsg_boundary(ix, [&] {
        HMSG_REQUIRE(n_views >= 0 && view_obj_off && view_obj_off[0] == 0, HMSG_ERR_INVALID, "hmsg_index_set_views: bad argument");
        for (int64_t v = 0; v < n_views; ++v)
            HMSG_REQUIRE(view_obj_off[v + 1] >= view_obj_off[v], HMSG_ERR_INVALID, "hmsg_index_set_views: offsets must not decrease");
        const int64_t total = view_obj_off[n_views];
        HMSG_REQUIRE(total == 0 || view_objs, HMSG_ERR_INVALID, "hmsg_index_set_views: object list missing");
        for (int64_t i = 0; i < total; ++i)
            HMSG_REQUIRE(view_objs[i] >= 0 && view_objs[i] < ix->N, HMSG_ERR_INVALID, "hmsg_index_set_views: object index out of range");
        ix->n_obj_views = -1;
        ix->h_vo_off.assign(view_obj_off, view_obj_off + n_views + 1);
        ix->vo_off.alloc((size_t)n_views + 1);
        ix->vo_nodes.alloc((size_t)std::max<int64_t>(total, 1));
        HIP_TRY(hipMemcpyAsync(ix->vo_off.p, view_obj_off, ((size_t)n_views + 1) * 8, hipMemcpyHostToDevice, ix->stream));
        if (total) HIP_TRY(hipMemcpyAsync(ix->vo_nodes.p, view_objs, (size_t)total * 4, hipMemcpyHostToDevice, ix->stream));
        HIP_TRY(hipStreamSynchronize(ix->stream));
        ix->n_obj_views = n_views;
    });
}

extern "C" int hmsg_rematch_in_views(hmsg_index_t* ix, int32_t Q, const float* T, const int32_t* view, int32_t* out_node, double* out_score) {
    if (!ix) return HMSG_ERR_INVALID;
    return hmsg_boundary(ix, [&] {
        HMSG_REQUIRE(ix->n_obj_views >= 0, HMSG_ERR_INVALID, "hmsg_rematch_in_views: hmsg_index_set_views first");
        HMSG_REQUIRE(Q >= 0 && (Q == 0 || (T && view && out_node && out_score)), HMSG_ERR_INVALID, "hmsg_rematch_in_views: bad argument");
        if (Q == 0) return;
        std::vector<int> hv((size_t)Q);
        read_in(hv.data(), view, (size_t)Q * 4);
        for (int q = 0; q < Q; ++q)
            HMSG_REQUIRE(hv[(size_t)q] >= 0 && hv[(size_t)q] < ix->n_obj_views, HMSG_ERR_INVALID, "hmsg_rematch_in_views: view index out of range");
        hipStream_t s = ix->stream;
        hmsg_text_rows_to_f64(s, T, (size_t)Q * ix->D, ix->Tf, ix->T64);
        ix->d_view.ensure((size_t)Q);
        ix->d_vnode.ensure((size_t)Q);
        ix->d_vscore.ensure((size_t)Q);
        HIP_TRY(hipMemcpyAsync(ix->d_view.p, hv.data(), (size_t)Q * 4, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_rematch_views, dim3((unsigned)Q), dim3(256), 0, s, (const double*)ix->T64.p, (const double*)ix->E.p, ix->D,
                           (const int*)ix->d_view.p, (const long long*)ix->vo_off.p, (const int*)ix->vo_nodes.p, ix->d_vnode.p, ix->d_vscore.p);
        HMSG_CHECK_LAUNCH();
        copy_out(out_node, ix->d_vnode.p, (size_t)Q * 4, s);
        copy_out(out_score, ix->d_vscore.p, (size_t)Q * 8, s);
        HIP_TRY(hipStreamSynchronize(s));          // (hv, a pageable source, is done with by now as well)
    });
}

// ------------------------------------------------------------------------------------------------ c. cloud-in-view distances
#define VD_SLICE 2048                 // points of one cloud a workgroup sums: 8 per thread
struct ViewSlice {
    long long p0;      // first point
    int n;             // <= VD_SLICE
    int pair;
};
struct ViewPart {
    double z_front, z_in;
    int n_front, n_in;
};
// stage 1: one workgroup per slice
__global__ void __launch_bounds__(256) k_view_depths_part(const double* __restrict__ pts, const ViewSlice* __restrict__ slices,
                                                          const double* __restrict__ pose_inv, const int* __restrict__ wh, const double* __restrict__ Kmat,
                                                          ViewPart* __restrict__ parts) {
    __shared__ double s_z[4][2];
    __shared__ int s_c[4][2];
    const ViewSlice sl = slices[blockIdx.x];
    const ViewCam cam = view_cam_load(pose_inv + (size_t)sl.pair * 16, Kmat, wh + (size_t)sl.pair * 2);
    int n_front = 0, n_in = 0;
    double zf = 0.0, zi = 0.0;
    for (int k = threadIdx.x; k < sl.n; k += 256) {
        double cz;
        const int where = view_point(cam, pts + (size_t)(sl.p0 + k) * 3, &cz);
        if (where == VIEW_POINT_BEHIND) continue;
        ++n_front;
        zf = __dadd_rn(zf, cz);
        if (where == VIEW_POINT_INSIDE) {
            ++n_in;
            zi = __dadd_rn(zi, cz);
        }
    }
    n_front = wave_sum_i32(n_front);
    n_in = wave_sum_i32(n_in);
    for (int o = 32; o > 0; o >>= 1) {
        zf = __dadd_rn(zf, __shfl_xor(zf, o));
        zi = __dadd_rn(zi, __shfl_xor(zi, o));
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_z[w][0] = zf;
        s_z[w][1] = zi;
        s_c[w][0] = n_front;
        s_c[w][1] = n_in;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        ViewPart p;
        p.z_front = __dadd_rn(__dadd_rn(s_z[0][0], s_z[1][0]), __dadd_rn(s_z[2][0], s_z[3][0]));
        p.z_in = __dadd_rn(__dadd_rn(s_z[0][1], s_z[1][1]), __dadd_rn(s_z[2][1], s_z[3][1]));
        p.n_front = (s_c[0][0] + s_c[1][0]) + (s_c[2][0] + s_c[3][0]);
        p.n_in = (s_c[0][1] + s_c[1][1]) + (s_c[2][1] + s_c[3][1]);
        parts[blockIdx.x] = p;
    }
}
// stage 2: one wave per pair adds its slices (slice_off [n_pairs + 1]) in a fixed order; n_total [pair]: all the cloud's points
__global__ void __launch_bounds__(64) k_view_depths_final(const ViewPart* __restrict__ parts, const long long* __restrict__ slice_off,
                                                          const long long* __restrict__ n_total, double min_ratio, double max_depth,
                                                          double* __restrict__ avg_z_front, unsigned char* __restrict__ visible,
                                                          double* __restrict__ mean_depth) {
    const long long p = blockIdx.x;
    const int lane = threadIdx.x;
    double zf = 0.0, zi = 0.0;
    long long nf = 0, ni = 0;
    for (long long i = slice_off[p] + lane; i < slice_off[p + 1]; i += 64) {
        zf = __dadd_rn(zf, parts[i].z_front);
        zi = __dadd_rn(zi, parts[i].z_in);
        nf += parts[i].n_front;
        ni += parts[i].n_in;
    }
    for (int o = 32; o > 0; o >>= 1) {
        zf = __dadd_rn(zf, __shfl_xor(zf, o));
        zi = __dadd_rn(zi, __shfl_xor(zi, o));
        nf += __shfl_xor(nf, o);
        ni += __shfl_xor(ni, o);
    }
    if (lane != 0) return;
    const double inf = 1e308 * 10.0;
    const long long n = n_total[p];
    unsigned char vis = 0;
    double md = inf;
    if (n > 0 && nf > 0 && ni > 0 && !((double)ni / (double)n < min_ratio)) {
        md = __ddiv_rn(zi, (double)ni);
        vis = md > max_depth ? 0 : 1;
    }
    avg_z_front[p] = nf > 0 ? __ddiv_rn(zf, (double)nf) : inf - inf;          // (NaN: the reference returns None)
    visible[p] = vis;
    mean_depth[p] = md;
}

void hmsg_view_depths(hipStream_t s, const double* d_pts, long long n_pairs, const std::vector<long long>& seg_off, const std::vector<CloudSeg>& segs,
                      const double* pose_inv, const int* wh, const double* K, double min_visible_ratio, double max_depth, double* avg_z_front,
                      unsigned char* visible, double* mean_depth) {
    HMSG_REQUIRE(n_pairs >= 0 && n_pairs < (1ll << 31) && (long long)seg_off.size() == n_pairs + 1, HMSG_ERR_INVALID, "view depths: bad argument");
    if (n_pairs == 0) return;
    HMSG_REQUIRE(pose_inv && wh && K, HMSG_ERR_INVALID, "view depths: pose_inv, wh and K are needed");
    std::vector<ViewSlice> slices;
    std::vector<long long> slice_off((size_t)n_pairs + 1, 0), n_total((size_t)n_pairs, 0);
    for (long long p = 0; p < n_pairs; ++p) {
        for (long long j = seg_off[(size_t)p]; j < seg_off[(size_t)p + 1]; ++j) {
            const CloudSeg& sg = segs[(size_t)j];
            n_total[(size_t)p] += sg.n;
            for (long long o = 0; o < sg.n; o += VD_SLICE) slices.push_back(ViewSlice{sg.p0 + o, (int)std::min<long long>(VD_SLICE, sg.n - o), (int)p});
        }
        slice_off[(size_t)p + 1] = (long long)slices.size();
    }
    HMSG_REQUIRE(slices.size() < ((size_t)1 << 31), HMSG_ERR_UNSUPPORTED, "view depths: too many points in one call");
    HMSG_REQUIRE(slices.empty() || d_pts, HMSG_ERR_INVALID, "view depths: no points");
    // every table in ONE packed upload (slices | slice_off | n_total | pose_inv | K | wh, all 8-byte aligned) and every result in ONE
    // packed read-back (avg | mean depth | visible): a call is two kernels and two copies whatever the number of pairs
    const size_t P = (size_t)n_pairs, NS = slices.size();
    const size_t o_soff = NS * sizeof(ViewSlice), o_ntot = o_soff + (P + 1) * 8, o_pose = o_ntot + P * 8, o_K = o_pose + P * 128, o_wh = o_K + 72,
                 in_bytes = o_wh + P * 8;
    std::vector<unsigned char> h_in(in_bytes);
    if (NS) memcpy(h_in.data(), slices.data(), o_soff);
    memcpy(h_in.data() + o_soff, slice_off.data(), (P + 1) * 8);
    memcpy(h_in.data() + o_ntot, n_total.data(), P * 8);
    memcpy(h_in.data() + o_pose, pose_inv, P * 128);
    memcpy(h_in.data() + o_K, K, 72);
    memcpy(h_in.data() + o_wh, wh, P * 8);
    const size_t o_md = P * 8, o_vis = 2 * P * 8, out_bytes = o_vis + P;
    DevBuf<unsigned char> d_in, d_out;
    DevBuf<ViewPart> d_parts;
    d_in.alloc(in_bytes);
    d_out.alloc(out_bytes);
    d_parts.alloc(NS);
    h2d_bounce(d_in.p, h_in.data(), in_bytes, s);
    const double* d_pose = (const double*)(d_in.p + o_pose);
    const double* d_K = (const double*)(d_in.p + o_K);
    const int* d_wh = (const int*)(d_in.p + o_wh);
    if (NS)
        hipLaunchKernelGGL(k_view_depths_part, dim3((unsigned)NS), dim3(256), 0, s, d_pts, (const ViewSlice*)d_in.p, d_pose, d_wh, d_K, d_parts.p);
    hipLaunchKernelGGL(k_view_depths_final, dim3((unsigned)n_pairs), dim3(64), 0, s, (const ViewPart*)d_parts.p, (const long long*)(d_in.p + o_soff),
                       (const long long*)(d_in.p + o_ntot), min_visible_ratio, max_depth, (double*)d_out.p, d_out.p + o_vis, (double*)(d_out.p + o_md));
    HMSG_CHECK_LAUNCH();
    std::vector<unsigned char> h_out(out_bytes);
    HIP_TRY(hipMemcpyAsync(h_out.data(), d_out.p, out_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (avg_z_front) memcpy(avg_z_front, h_out.data(), P * 8);
    if (mean_depth) memcpy(mean_depth, h_out.data() + o_md, P * 8);
    if (visible) memcpy(visible, h_out.data() + o_vis, P);
}

extern "C" int hmsg_points_view_depths(int32_t device_id, int64_t n_pairs, const int64_t* pts_off, const double* pts, const double* pose_inv,
                                       const int32_t* wh, const double* K, double min_visible_ratio, double max_depth, double* avg_z_front,
                                       uint8_t* visible, double* mean_depth) {
    return hmsg_boundary("hmsg_points_view_depths", -1, [&] {
        HMSG_REQUIRE(n_pairs >= 0 && (n_pairs == 0 || (pts_off && pose_inv && wh && K)), HMSG_ERR_INVALID, "hmsg_points_view_depths: bad argument");
        if (n_pairs == 0) return;
        HIP_TRY(hipSetDevice(device_id));
        std::vector<long long> seg_off((size_t)n_pairs + 1);
        std::vector<CloudSeg> segs((size_t)n_pairs);
        HMSG_REQUIRE(pts_off[0] == 0, HMSG_ERR_INVALID, "hmsg_points_view_depths: pts_off[0] must be 0");
        for (int64_t p = 0; p < n_pairs; ++p) {
            HMSG_REQUIRE(pts_off[p + 1] >= pts_off[p], HMSG_ERR_INVALID, "hmsg_points_view_depths: offsets must not decrease");
            seg_off[(size_t)p] = p;
            segs[(size_t)p] = CloudSeg{pts_off[p], pts_off[p + 1] - pts_off[p]};
        }
        seg_off[(size_t)n_pairs] = n_pairs;
        const size_t total = (size_t)pts_off[n_pairs];
        HMSG_REQUIRE(total == 0 || pts, HMSG_ERR_INVALID, "hmsg_points_view_depths: no points");
        ScopedStream s(hipStreamNonBlocking);
        DevBuf<double> d_pts;
        const double* dp = total ? stage_in(d_pts, pts, total * 3, s, Up::bounce) : pts;
        hmsg_view_depths(s, dp, n_pairs, seg_off, segs, pose_inv, wh, K, min_visible_ratio, max_depth, avg_z_front, visible, mean_depth);
    });
}
