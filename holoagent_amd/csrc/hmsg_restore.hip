// hmsg_restore_stage (include/hmsg.h): a map, an instance pool and the pooled features from stage artefacts back into a handle,
// which is afterwards where hmsg_pool_instances leaves one as far as the graph level can tell.  The points go up once and are
// not read back; what the host needs of them -- the box of every instance, the map's extent, "every coordinate finite" -- comes
// from one pass over each array (k_stage_bounds).
#include "hmsg_boundary.h"
#include "hmsg_stage_files.h"

#include <cmath>

namespace {

// A wave takes chunks of BD_CHUNK consecutive points, lane l the points l, l + 64, ... of the chunk: the work is split by POINTS,
// so a pool of instances of 1 to 10^5 points balances by itself and the launch does not depend on the number of instances.
//   * a chunk inside ONE instance (nearly all of them once instances are larger than a chunk): running min / max in registers,
//     one wave reduction, six 64-bit atomics from lane 0 on the order-preserving keys of enc_f64 (hmsg_common.h; there is no
//     native float64 atomic min).  A 10^5-point instance sends ~100 waves to its six words.
//   * a chunk that crosses instance ends: every lane looks its point's instance up between the chunk's first and last one and
//     keeps a running box of its own, flushed with atomics when the instance changes (a lane's points are 64 apart, so that is
//     once per instance the chunk meets, at most).
// box: [n_seg][6] keys, preset to {~0, ~0, ~0, 0, 0, 0}; *bad |= 1 when a coordinate is NaN or +-Inf.
constexpr int BD_CHUNK = 1024;

// the segment of point p: the largest k in [lo, hi] with off[k] <= p (empty segments share their start with the next one and lose)
__device__ __forceinline__ long long bd_seg_of(const long long* __restrict__ off, long long p, long long lo, long long hi) {
    while (lo < hi) {
        const long long mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= p) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
__device__ __forceinline__ bool bd_finite(double v) {
    return ((unsigned long long)__double_as_longlong(v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}
// running box of a lane as enc_f64 keys: the keys are a total order (-0.0 below +0.0), so the result does not depend on the
// order the points are met in
struct BdBox {
    unsigned long long mn[3], mx[3];
    __device__ __forceinline__ void clear() {
        for (int a = 0; a < 3; ++a) mn[a] = ~0ull, mx[a] = 0ull;
    }
    __device__ __forceinline__ bool add(const double* __restrict__ p) {          // false: a coordinate is not finite
        bool ok = true;
        for (int a = 0; a < 3; ++a) {
            const double v = p[a];
            ok &= bd_finite(v);
            const unsigned long long k = enc_f64(v);
            mn[a] = k < mn[a] ? k : mn[a];
            mx[a] = k > mx[a] ? k : mx[a];
        }
        return ok;
    }
    __device__ __forceinline__ void flush(unsigned long long* __restrict__ box, long long k) const {
        for (int a = 0; a < 3; ++a) {
            atomicMin(&box[(size_t)k * 6 + a], mn[a]);
            atomicMax(&box[(size_t)k * 6 + 3 + a], mx[a]);
        }
    }
};
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t = __shfl_xor(v, o);
        v = t < v ? t : v;
    }
    return v;
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t = __shfl_xor(v, o);
        v = t > v ? t : v;
    }
    return v;
}

__global__ void k_stage_bounds_init(unsigned long long* __restrict__ box, long long n_seg, unsigned* __restrict__ bad) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_seg * 6) box[i] = (i % 6) < 3 ? ~0ull : 0ull;
    if (i == 0) *bad = 0u;
}

__global__ void k_stage_bounds(const double* __restrict__ pts, long long P, const long long* __restrict__ off, long long n_seg,
                               unsigned long long* __restrict__ box, unsigned* __restrict__ bad) {
    const int lane = threadIdx.x & 63;
    const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    const long long nchunks = (P + BD_CHUNK - 1) / BD_CHUNK;
    bool nonfinite = false;
    for (long long c = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6; c < nchunks; c += nwaves) {       // (c is wave-uniform)
        const long long p0 = c * BD_CHUNK, p1 = p0 + BD_CHUNK < P ? p0 + BD_CHUNK : P;
        const long long k0 = bd_seg_of(off, p0, 0, n_seg - 1), k1 = bd_seg_of(off, p1 - 1, k0, n_seg - 1);
        BdBox b;
        b.clear();
        if (k0 == k1) {
            for (long long p = p0 + lane; p < p1; p += 64) nonfinite |= !b.add(pts + (size_t)p * 3);
            for (int a = 0; a < 3; ++a) {
                b.mn[a] = wave_min_u64(b.mn[a]);
                b.mx[a] = wave_max_u64(b.mx[a]);
            }
            if (lane == 0) b.flush(box, k0);         // (a chunk is never empty: the keys are those of real points)
        } else {
            long long cur = -1;
            for (long long p = p0 + lane; p < p1; p += 64) {
                const long long k = bd_seg_of(off, p, k0, k1);
                if (k != cur) {
                    if (cur >= 0) b.flush(box, cur);
                    cur = k;
                    b.clear();
                }
                nonfinite |= !b.add(pts + (size_t)p * 3);
            }
            if (cur >= 0) b.flush(box, cur);
        }
    }
    if (__any(nonfinite) && lane == 0) atomicOr(bad, 1u);
}

// the pass over P points in n_seg segments (off: device, n_seg + 1 entries); box / bad: device, any contents
void stage_bounds(const double* pts, long long P, const long long* off, long long n_seg, unsigned long long* box, unsigned* bad, hipStream_t s) {
    hipLaunchKernelGGL(k_stage_bounds_init, dim3(cdiv((size_t)std::max<long long>(n_seg * 6, 1), 256)), dim3(256), 0, s, box, n_seg, bad);
    HMSG_CHECK_LAUNCH();
    if (P <= 0 || n_seg <= 0) return;
    const size_t nchunks = (size_t)((P + BD_CHUNK - 1) / BD_CHUNK);
    hipLaunchKernelGGL(k_stage_bounds, dim3((unsigned)std::min<size_t>(cdiv(nchunks, 4), 2048)), dim3(256), 0, s, pts, P, off, n_seg, box, bad);
    HMSG_CHECK_LAUNCH();
}

}  // namespace

extern "C" int hmsg_restore_stage(hmsg_t* h, int64_t V, const double* map_xyz, const double* map_rgb, const float* map_feats, int64_t n_inst,
                                  const int64_t* inst_off, const double* inst_xyz, const float* inst_feats, const double* K) {
    if (!h) return HMSG_ERR_INVALID;
    return hmsg_boundary(h, [&] {
        HMSG_REQUIRE(!h->restored, HMSG_ERR_INVALID, "hmsg_restore_stage: the handle was restored already (hmsg_reset first)");
        HMSG_REQUIRE(h->n_frames == 0 && h->n_offered == 0 && !h->map_ready && !h->merged && !h->tree_partial && !h->fold_pipe, HMSG_ERR_INVALID,
                     "hmsg_restore_stage: the handle holds frames or a map (hmsg_reset first)");
        hmsg_graph_early_abort(h);
        ++h->inst_epoch;
        HMSG_REQUIRE(V >= 1 && V <= 0x7fffffffll && map_xyz && n_inst >= 0 && n_inst <= 0x7fffffffll && inst_off && K, HMSG_ERR_INVALID,
                     "hmsg_restore_stage: bad argument (a map of 1 .. 2^31 - 1 points, inst_off and K are needed)");
        // ---- the offsets: checked on the host before anything is sized by them
        std::vector<long long> off((size_t)n_inst + 3);
        {
            std::vector<int64_t> o((size_t)n_inst + 1);
            read_in(o.data(), inst_off, o.size() * 8);
            std::string msg;
            HMSG_REQUIRE(stage_check_offsets(o.data(), n_inst, &msg) == STAGE_OK, HMSG_ERR_INVALID, "hmsg_restore_stage: " + msg);
            for (size_t i = 0; i < o.size(); ++i) off[i] = (long long)o[i];
            for (int64_t i = 0; i < n_inst; ++i)
                HMSG_REQUIRE(o[(size_t)i + 1] - o[(size_t)i] <= 0x7fffffffll, HMSG_ERR_UNSUPPORTED, "hmsg_restore_stage: an instance of 2^31 points or more");
        }
        const long long P = off[(size_t)n_inst];
        HMSG_REQUIRE((P == 0 || inst_xyz) && (n_inst == 0 || inst_feats), HMSG_ERR_INVALID, "hmsg_restore_stage: instance points / features missing");
        off[(size_t)n_inst + 1] = 0;               // (the map as one segment, behind the instances' offsets)
        off[(size_t)n_inst + 2] = V;
        double Kh[9];
        read_in(Kh, K, sizeof(Kh));
        const size_t D = (size_t)h->cfg.feat_dim;
        hipStream_t s = h->stream;
        DbgLaps laps("restore", s);
        // ---- everything goes into buffers of this call; the handle changes only when the arrays have passed
        DevBuf<double> pts, cols, ipts;
        DevBuf<float> feats, ifeats;
        DevBuf<long long> d_off;
        DevBuf<unsigned long long> d_box;          // [n_inst][6] | [6] the map | one word: the not-finite flag
        pts.alloc((size_t)V * 3);
        cols.alloc((size_t)V * 3);
        ipts.alloc((size_t)std::max<long long>(P, 1) * 3);
        ifeats.alloc((size_t)std::max<int64_t>(n_inst, 1) * D);
        d_off.alloc(off.size());
        d_box.alloc((size_t)n_inst * 6 + 6 + 1);
        copy_in(pts.p, map_xyz, (size_t)V * 24, s, Up::bounce);
        if (map_rgb) copy_in(cols.p, map_rgb, (size_t)V * 24, s, Up::bounce);
        else cols.zero(s);
        if (map_feats) {
            feats.alloc((size_t)V * D);
            copy_in(feats.p, map_feats, (size_t)V * D * 4, s, Up::bounce);
        }
        copy_in(ipts.p, inst_xyz, (size_t)P * 24, s, Up::bounce);
        copy_in(ifeats.p, inst_feats, (size_t)n_inst * D * 4, s, Up::bounce);
        upload(d_off.p, off.data(), off.size() * 8, s, Up::bounce);
        laps.lap("arrays up");
        unsigned long long* const map_box = d_box.p + (size_t)n_inst * 6;
        unsigned* const bad_inst = (unsigned*)(map_box + 6);
        unsigned* const bad_map = bad_inst + 1;
        {
            ProfScope ps(h->prof, s, "k_stage_bounds", (double)(P + V) * 24.0);
            stage_bounds(ipts.p, P, d_off.p, n_inst, d_box.p, bad_inst, s);
            stage_bounds(pts.p, V, d_off.p + (size_t)n_inst + 1, 1, map_box, bad_map, s);
        }
        std::vector<unsigned long long> hb((size_t)n_inst * 6 + 6 + 1);
        HIP_TRY(hipMemcpyAsync(hb.data(), d_box.p, hb.size() * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        laps.lap("bounds pass");
        const unsigned long long flags = hb.back();
        HMSG_REQUIRE((unsigned)(flags >> 32) == 0u, HMSG_ERR_INVALID, "hmsg_restore_stage: a map coordinate is not finite");
        HMSG_REQUIRE((unsigned)flags == 0u, HMSG_ERR_INVALID, "hmsg_restore_stage: an instance coordinate is not finite");
        // ---- commit
        double mn[3], mx[3];
        for (int a = 0; a < 3; ++a) {
            mn[a] = dec_f64(hb[(size_t)n_inst * 6 + a]);
            mx[a] = dec_f64(hb[(size_t)n_inst * 6 + 3 + a]);
        }
        // the grid covers the cloud's extent at the handle's voxel size, laid out as hmsg_finalize_map lays it out -- extent only: a
        // restored cloud need not have one point per cell, and there is no bitmap / rank / candidate list behind it
        GridGeom g;
        g.vs = h->cfg.voxel_size;
        g.ox = mn[0] - g.vs * 0.5;
        g.oy = mn[1] - g.vs * 0.5;
        g.oz = mn[2] - g.vs * 0.5;
        const double ex[3] = {std::floor((mx[0] - g.ox) / g.vs), std::floor((mx[1] - g.oy) / g.vs), std::floor((mx[2] - g.oz) / g.vs)};
        HMSG_REQUIRE(ex[0] < 1e9 && ex[1] < 1e9 && ex[2] < 1e9, HMSG_ERR_UNSUPPORTED, "hmsg_restore_stage: the map's extent is too large for the voxel size");
        g.nx = (int)ex[0] + 2;
        g.ny = (int)ex[1] + 2;
        g.nz = (int)ex[2] + 2;
        g.nzp = (g.nz + 63) / 64 * 64;
        g.nwords = (long long)g.nx * g.ny * (g.nzp / 64);
        h->grid = g;
        h->V = h->V0 = (long long)V;
        h->pts.swap(pts);
        h->cols.swap(cols);
        h->feats_final = map_feats != nullptr;
        if (map_feats) h->feats.swap(feats);
        h->have_cand = false;
        memcpy(h->K, Kh, sizeof(Kh));
        h->have_K = true;
        h->cam = CamK{Kh[0], Kh[4], Kh[2], Kh[5]};
        h->inst.pts.swap(ipts);
        h->inst.off.assign(off.begin(), off.begin() + (long)n_inst + 1);
        h->inst.total = P;
        h->inst.box.assign((size_t)n_inst * 6, 0.0);           // (an empty instance: six zeros, as after a denoise that emptied it)
        for (int64_t k = 0; k < n_inst; ++k)
            if (off[(size_t)k + 1] > off[(size_t)k])
                for (int a = 0; a < 6; ++a) h->inst.box[(size_t)k * 6 + a] = dec_f64(hb[(size_t)k * 6 + a]);
        h->inst_feats.swap(ifeats);
        h->masks3d.off.clear();
        h->masks3d.total = 0;
        h->nodes.clear();
        h->node_label.clear();
        h->room_n = 0;
        h->room_total = 0;
        h->inst_denoised = false;
        hmsg_kd_start(h);                          // host copy of the cloud + the restated cKDTree on its side thread, as hmsg_finalize_map
        h->map_ready = h->merged = h->pooled = h->restored = true;
        laps.lap("commit + cKDTree start");
    });
}
