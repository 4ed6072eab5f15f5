// A frame's masks as SAM's uncompressed run-length records -> the resident per-pixel membership bitsets, without a dense
// mask in between (include/hmsg.h: hmsg_add_frame_features_rle, hmsg_rle_to_bitsets, hmsg_rle_to_masks).
//
// Reference: segment_anything/utils/amg.py mask_to_rle_pytorch / rle_to_mask (the record SamAutomaticMaskGenerator keeps
// internally and returns with output_mode="uncompressed_rle"); the dense hand-over it replaces is k_bitset (hmsg_fuse.hip).
//
// MI355X design notes
//  * A record runs down the COLUMNS of the image (position t = x * H + y), the bitsets are row-major: the decode is a
//    transposition.  A workgroup owns 16 columns x TY rows of one frame as u64 words in LDS ([TY][16][NW], 8 KB: TY = 64 at
//    NW = 1, 16 at NW = 4), ORs the masks' one-runs into it with LDS atomics and then writes the tile row by row: every output
//    word is stored exactly once, 16 * NW consecutive words (whole 128-byte lines) per tile row, and a pixel no mask covers
//    gets its zero from the same store -- no memset of the bitsets, no global atomic.
//  * A thread takes (mask, column) pairs of the tile, 16 consecutive lanes the columns of one mask: they search the same
//    array of run starts (binary search for the run that holds the column's first row in the tile), then walk the runs to
//    the tile's last row.  Most pairs end after the search -- a SAM mask touches few columns -- so a pair costs log2(runs)
//    dependent cached loads, and the kernel's time is that chain times the pairs a thread takes in turn: hence the narrow
//    tile (M = 32: two pairs per thread, 320 workgroups at 640x480).  The first version, 64 columns x 64 rows, had eight pairs
//    per thread and 80 workgroups and took 29 us a frame at either size (profiles/rle_masks_first_tile_64x64.json).  A one-run ORs
//    one word per covered row, consecutive lanes into consecutive 8 * NW-byte words.
//  * Nothing the caller hands over can move a store: a position is clamped to the column's rows inside the tile before it
//    becomes an LDS index, the tile's store is guarded by H and W, and the run starts themselves are clamped to H * W.
#include "hmsg_boundary.h"
#include "hmsg_rle.h"

#include <climits>

#define RLE_TILE_X 16
#define RLE_TILE_WORDS 1024           /* u64 words of a tile: 8 KB of LDS */
#define RLE_SCAN_PER_LANE 4

// ------------------------------------------------------------------------------------------ K_rle_scan
// Segmented exclusive prefix sum: a wave per mask, 64 x 4 counts per step (a lane adds its four, the wave scans the lane sums).
// starts[j] = sum of the mask's counts before j (clamped to HW), totals[t] = the mask's sum (64-bit: u32 counts of a malformed record may add up past 2^32), and
// *first_bad = the smallest mask index whose record is empty or does not sum to HW.
__global__ void k_rle_scan(const unsigned* __restrict__ counts, const long long* __restrict__ run_off, long long cnt_base,
                           int t_first, int n_masks, unsigned HW, unsigned* __restrict__ starts,
                           unsigned long long* __restrict__ totals, int* __restrict__ first_bad) {
    const int lane = threadIdx.x & 63;
    const int t = t_first + (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    if (t >= t_first + n_masks) return;
    const long long a = run_off[t] - cnt_base, b = run_off[t + 1] - cnt_base;
    unsigned long long carry = 0;
    for (long long j0 = a; j0 < b; j0 += 64 * RLE_SCAN_PER_LANE) {
        const long long j = j0 + (long long)lane * RLE_SCAN_PER_LANE;
        unsigned long long c[RLE_SCAN_PER_LANE], incl = 0;
#pragma unroll
        for (int q = 0; q < RLE_SCAN_PER_LANE; ++q) {
            c[q] = j + q < b ? (unsigned long long)counts[j + q] : 0ull;
            incl += c[q];
        }
        const unsigned long long own = incl;
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long up = __shfl_up(incl, (unsigned)d);
            if (lane >= d) incl += up;
        }
        unsigned long long run = carry + incl - own;              // sum of everything before this lane's first count
#pragma unroll
        for (int q = 0; q < RLE_SCAN_PER_LANE; ++q) {
            if (j + q < b) starts[j + q] = (unsigned)min(run, (unsigned long long)HW);
            run += c[q];
        }
        carry += __shfl(incl, 63);
    }
    if (lane == 0) {
        totals[t] = carry;
        if (a >= b || carry != (unsigned long long)HW) atomicMin(first_bad, t);
    }
}

// ------------------------------------------------------------------------------------------ K_rle_bitset
// grid (ceil(W / 16), ceil(H / TY), frames); TY * 16 * NW <= RLE_TILE_WORDS.  mask_off[f]: first mask of frame f, nmask[f]
// how many it has (rows >= nmask[f] of the hand-over are padding: nothing is read for them).
__global__ __launch_bounds__(256) void k_rle_bitset(const unsigned* __restrict__ starts, const long long* __restrict__ run_off,
                                                    long long cnt_base, const int* __restrict__ mask_off,
                                                    const int* __restrict__ nmask, int M, int H, int W, int NW, int TY,
                                                    unsigned long long* __restrict__ bits) {
    __shared__ unsigned long long tile[RLE_TILE_WORDS];
    const int f = blockIdx.z, x0 = blockIdx.x * RLE_TILE_X, y0 = blockIdx.y * TY;
    const int rows = min(TY, H - y0), roww = RLE_TILE_X * NW;
    const unsigned HW = (unsigned)H * (unsigned)W;
    for (int j = threadIdx.x; j < rows * roww; j += blockDim.x) tile[j] = 0ull;
    __syncthreads();
    const int nm = min(nmask[f], M), m0 = mask_off[f];
    for (int p = threadIdx.x; p < nm * RLE_TILE_X; p += blockDim.x) {
        const int i = p / RLE_TILE_X, xl = p % RLE_TILE_X, x = x0 + xl;
        const long long a = run_off[m0 + i] - cnt_base, k = run_off[m0 + i + 1] - run_off[m0 + i];
        if (x >= W || k <= 0) continue;
        const unsigned* S = starts + a;
        const unsigned t0 = (unsigned)x * (unsigned)H + (unsigned)y0, t1 = t0 + (unsigned)rows;
        long long lo = 0, hi = k;                       // the last run that starts at or before t0 (S[0] = 0)
        while (hi - lo > 1) {
            const long long mid = (lo + hi) >> 1;
            if (S[mid] <= t0) lo = mid;
            else hi = mid;
        }
        unsigned long long* col = tile + (size_t)xl * NW + (i >> 6);
        const unsigned long long bit = 1ull << (i & 63);
        unsigned s = S[lo];
        for (long long r = lo; r < k; ++r) {
            const unsigned e = r + 1 < k ? S[r + 1] : HW;
            if (r & 1) {
                const unsigned b0 = max(s, t0), b1 = min(e, t1);
                for (unsigned t = b0; t < b1; ++t) atomicOr(col + (size_t)(t - t0) * roww, bit);
            }
            if (e >= t1) break;
            s = e;
        }
    }
    __syncthreads();
    unsigned long long* o = bits + (size_t)f * HW * NW;
    for (int j = threadIdx.x; j < rows * roww; j += blockDim.x) {
        const int row = j / roww, rem = j - row * roww;
        if (x0 + rem / NW < W) o[((size_t)(y0 + row) * W + x0) * NW + rem] = tile[j];
    }
}

// ------------------------------------------------------------------------------------------ K_rle_masks
// bitsets u64 [HW][NW] -> dense masks u8 [M][HW] (0/1): what the crop kernels read.  Off the hot path.
__global__ void k_rle_masks(const unsigned long long* __restrict__ bits, int M, size_t HW, int NW, unsigned char* __restrict__ out) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)M * HW) return;
    const int i = (int)(idx / HW);
    const size_t p = idx - (size_t)i * HW;
    out[idx] = (unsigned char)((bits[p * NW + (i >> 6)] >> (i & 63)) & 1ull);
}

namespace {
// counts of a chunk the staging buffer takes (256 MB); HMSG_DEBUG_RLE_CHUNK_COUNTS: a small value, so that a test reaches the
// several-chunks path with a scene of a few frames
long long chunk_budget() {
    const char* e = getenv("HMSG_DEBUG_RLE_CHUNK_COUNTS");
    const long long x = e ? atoll(e) : 0;
    return x > 0 ? x : (long long)64 << 20;
}

// the run starts of chunk c into r.starts (and the masks' totals, and the flag)
void load_chunk(hmsg_rle_handover& r, int c, hipStream_t s, Prof* prof) {
    if (r.resident == c) return;
    const int t0 = r.mask_off[(size_t)r.chunk_first[(size_t)c]], t1 = r.mask_off[(size_t)r.chunk_first[(size_t)c + 1]];
    const long long base = r.run_off[(size_t)t0], cnt = r.run_off[(size_t)t1] - base;
    r.resident = -1;
    const uint32_t* d_counts = r.counts + base;
    if (!r.counts_dev && cnt > 0) {
        r.st_counts.ensure((size_t)cnt);
        HIP_TRY(hipMemcpyAsync(r.st_counts.p, r.counts + base, (size_t)cnt * 4, hipMemcpyHostToDevice, s));
        d_counts = r.st_counts.p;
    }
    r.starts.ensure((size_t)std::max<long long>(cnt, 1));
    if (t1 > t0) {
        ProfScope ps(prof, s, "k_rle_scan", 8.0 * (double)cnt);
        hipLaunchKernelGGL(k_rle_scan, dim3(cdiv((size_t)(t1 - t0), 4)), dim3(256), 0, s, d_counts, (const long long*)r.d_run_off.p,
                           base, t0, t1 - t0, (unsigned)((size_t)r.H * r.W), r.starts.p, r.totals.p, r.d_bad.p);
    }
    HMSG_CHECK_LAUNCH();
    r.resident = c;
}
}  // namespace

void hmsg_rle_begin(hmsg_rle_handover& r, int H, int W, int n, const int* nm, const uint32_t* counts, const int64_t* run_off,
                    int max_chunk_frames, hipStream_t s, Prof* prof) {
    HMSG_REQUIRE(H > 0 && W > 0 && (long long)H * W <= INT_MAX, HMSG_ERR_INVALID, "run-length masks: H * W must be in [1, 2^31)");
    r.H = H;
    r.W = W;
    r.n = n;
    r.counts = counts;
    r.mask_off.assign((size_t)n + 1, 0);
    for (int f = 0; f < n; ++f) {
        HMSG_REQUIRE((long long)r.mask_off[(size_t)f] + nm[f] <= INT_MAX, HMSG_ERR_INVALID, "run-length masks: too many masks in one hand-over");
        r.mask_off[(size_t)f + 1] = r.mask_off[(size_t)f] + nm[f];
    }
    const int T = r.mask_off[(size_t)n];
    HMSG_REQUIRE(run_off && (counts || T == 0), HMSG_ERR_INVALID, "run-length masks: null counts / run_off");
    r.run_off.resize((size_t)T + 1);
    read_in(r.run_off.data(), run_off, ((size_t)T + 1) * 8);
    HMSG_REQUIRE(r.run_off[0] == 0, HMSG_ERR_INVALID, "run-length masks: run_off[0] must be 0 (mask 0)");
    for (int t = 0; t < T; ++t) {
        HMSG_REQUIRE(r.run_off[(size_t)t + 1] >= r.run_off[(size_t)t], HMSG_ERR_INVALID,
                     "run-length masks: run_off decreases at mask " + std::to_string(t));
        HMSG_REQUIRE(r.run_off[(size_t)t + 1] > r.run_off[(size_t)t], HMSG_ERR_INVALID,
                     "run-length masks: mask " + std::to_string(t) + " has no counts");
    }
    r.counts_dev = T > 0 && hmsg_is_device_ptr(counts);
    // chunks of whole frames: counts within the staging budget (a frame above it is a chunk of its own), frames within the caller's
    const long long budget = chunk_budget();
    const int max_fr = std::max(1, std::min(max_chunk_frames, 32768));
    r.chunk_first.assign(1, 0);
    for (int f = 0, c0 = 0; f < n; ++f) {
        const long long upto = r.run_off[(size_t)r.mask_off[(size_t)f + 1]] - r.run_off[(size_t)r.mask_off[(size_t)c0]];
        if (f > c0 && (f - c0 >= max_fr || (!r.counts_dev && upto > budget))) {
            r.chunk_first.push_back(f);
            c0 = f;
        }
    }
    r.chunk_first.push_back(n);
    r.d_run_off.alloc((size_t)T + 1);
    r.d_mask_off.alloc((size_t)n + 1);
    r.d_nmask.alloc((size_t)std::max(n, 1));
    r.totals.alloc((size_t)std::max(T, 1));
    r.d_bad.alloc(1);
    const int none = INT_MAX;
    HIP_TRY(hipMemcpyAsync(r.d_run_off.p, r.run_off.data(), ((size_t)T + 1) * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(r.d_mask_off.p, r.mask_off.data(), ((size_t)n + 1) * 4, hipMemcpyHostToDevice, s));
    if (n) HIP_TRY(hipMemcpyAsync(r.d_nmask.p, nm, (size_t)n * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(r.d_bad.p, &none, 4, hipMemcpyHostToDevice, s));
    r.resident = -1;
    for (int c = 0; c < r.chunks(); ++c) load_chunk(r, c, s, prof);
    int bad = none;
    HIP_TRY(hipMemcpyAsync(&bad, r.d_bad.p, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));                  // (also: nm, `none` and the host tables are free again)
    if (bad != none) {
        unsigned long long tot = 0;
        HIP_TRY(hipMemcpy(&tot, r.totals.p + bad, 8, hipMemcpyDeviceToHost));
        int f = 0;
        while (f + 1 < n && r.mask_off[(size_t)f + 1] <= bad) ++f;
        throw hmsg_error{HMSG_ERR_INVALID, "run-length masks: the counts of mask " + std::to_string(bad) + " (frame " + std::to_string(f) +
                                               " of the hand-over, its mask " + std::to_string(bad - r.mask_off[(size_t)f]) + ") sum to " +
                                               std::to_string(tot) + ", not H * W = " + std::to_string((long long)H * W)};
    }
}

void hmsg_rle_decode(hmsg_rle_handover& r, int c, int M, int NW, unsigned long long* bits, hipStream_t s, Prof* prof) {
    load_chunk(r, c, s, prof);
    const int f0 = r.chunk_first[(size_t)c], nc = r.chunk_first[(size_t)c + 1] - f0;
    if (nc <= 0) return;
    const int TY = std::max(1, std::min(RLE_TILE_WORDS / (RLE_TILE_X * NW), r.H));
    const long long base = r.run_off[(size_t)r.mask_off[(size_t)f0]];
    {
        ProfScope ps(prof, s, "k_rle_bitset", 4.0 * (double)(r.run_off[(size_t)r.mask_off[(size_t)f0 + nc]] - base) + (double)nc * r.H * r.W * 8.0 * NW);
        hipLaunchKernelGGL(k_rle_bitset, dim3(cdiv((size_t)r.W, RLE_TILE_X), cdiv((size_t)r.H, (size_t)TY), (unsigned)nc), dim3(256), 0, s,
                           (const unsigned*)r.starts.p, (const long long*)r.d_run_off.p, base, (const int*)r.d_mask_off.p + f0,
                           (const int*)r.d_nmask.p + f0, M, r.H, r.W, NW, TY, bits);
    }
    HMSG_CHECK_LAUNCH();
}

// ------------------------------------------------------------------------------------------ the two calls without a handle
namespace {
void rle_one_frame(int H, int W, int M, const uint32_t* counts, const int64_t* run_off, uint64_t* out_bits, uint8_t* out_masks) {
    HMSG_REQUIRE(M >= 0 && M <= 256, HMSG_ERR_INVALID, "M out of range (<= 256)");
    const int NW = (std::max(M, 1) + 63) / 64;
    const size_t HW = (size_t)H * W;
    ScopedStream s(hipStreamNonBlocking);
    hmsg_rle_handover r;
    hmsg_rle_begin(r, H, W, 1, &M, counts, run_off, 1, s, nullptr);
    DevBuf<unsigned long long> d_bits;
    DevBuf<unsigned char> d_masks;
    unsigned long long* p_bits = (unsigned long long*)out_bits;
    if (!out_bits || !hmsg_is_device_ptr(out_bits)) {
        d_bits.alloc(HW * NW);
        p_bits = d_bits.p;
    }
    hmsg_rle_decode(r, 0, M, NW, p_bits, s, nullptr);
    if (out_bits && p_bits != (unsigned long long*)out_bits) HIP_TRY(hipMemcpyAsync(out_bits, p_bits, HW * NW * 8, hipMemcpyDeviceToHost, s));
    if (out_masks && M > 0) {
        unsigned char* p_masks = stage_out(d_masks, out_masks, (size_t)M * HW);
        hipLaunchKernelGGL(k_rle_masks, dim3(cdiv((size_t)M * HW, 256)), dim3(256), 0, s, (const unsigned long long*)p_bits, M, HW, NW, p_masks);
        HMSG_CHECK_LAUNCH();
        unstage_out(out_masks, p_masks, (size_t)M * HW, s);
    }
    HIP_TRY(hipStreamSynchronize(s));
}
}  // namespace

extern "C" int hmsg_rle_to_bitsets(int32_t device_id, int32_t H, int32_t W, int32_t M, const uint32_t* counts, const int64_t* run_off,
                                   uint64_t* out_bits) {
    if (!out_bits) return HMSG_ERR_INVALID;
    return hmsg_boundary("hmsg_rle_to_bitsets", device_id, [&] { rle_one_frame(H, W, M, counts, run_off, out_bits, nullptr); });
}

extern "C" int hmsg_rle_to_masks(int32_t device_id, int32_t H, int32_t W, int32_t M, const uint32_t* counts, const int64_t* run_off,
                                 uint8_t* out_masks) {
    if (!out_masks && M > 0) return HMSG_ERR_INVALID;
    return hmsg_boundary("hmsg_rle_to_masks", device_id, [&] { rle_one_frame(H, W, M, counts, run_off, nullptr, out_masks); });
}
