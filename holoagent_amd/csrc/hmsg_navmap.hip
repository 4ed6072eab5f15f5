// The image half of a floor's navigation graph on the device (include/hmsg.h: hmsg_nav_grid, hmsg_nav_floor_maps and their
// hmsg_graph_* forms): a storey's cloud -> obstacle map, floor region, pose discs, free map, its main region, that region's
// boundary cells in row-major order, and the top-down colour image.  No point of the storey goes to the host.
//
// Reference: graph/navigation_graph.py NavigationGraph.__init__ (:57-65), create_occupancy_grid (:221-240), get_poses_region
// (:348-377, the pose selection and the disc are hmsg_nav_host.h), get_main_free_map (:400-422), get_largest_region (:316-322),
// get_top_down_rgb_map (:458-481) and the boundary step of get_voronoi_graph (:511-521).  Every output is integer work (the
// obstacle map is a whole number of sixteenths), so every output is exact and independent of the order the points arrive in.
//
// MI355X design notes
//  * The cloud is read twice: k_nav_bounds (min / max, reduced over the wave by shuffles and over the workgroup through LDS, one
//    64-bit atomicMin / atomicMax per workgroup and axis on an order-preserving code of the float64; a grid-stride loop of at most
//    512 workgroups) and k_nav_points, which makes both occupancy maps and the top-down keys in one pass.  An occupancy cell is a byte that every point of the cell stores the same 1 to: a plain store, no atomic (cells
//    are hit a few dozen times each; a read-modify-write would serialise them at the L2 for nothing).  The top-down winner of a
//    cell is one 64-bit atomicMax of (height cell + 1) << 32 | ~index: the greatest height cell wins, of equal ones the lowest
//    index, whatever the arrival order.  A storey of a built graph is selected by the slab test inside both kernels: the
//    points keep their map order, which is all the tie rule needs, and nothing is compacted.
//  * The images are small (a few hundred thousand cells) beside the cloud: a thread per cell, bytes in and out, separable
//    dilation, the 3 x 3 blur as an integer sum of sixteenths.  All of them are bound by launch latency, not by bandwidth.
//  * Labelling is hmsg_sam_post.hip's label equivalence (k_spcc_*, through hmsg_cc8_components) on the one free map: the same
//    code, not a copy.  Area counts sit at each component's root; a root's key (area << 32 | root + 1) orders components by area
//    and, among equal areas, by label (labels follow the roots' raster order), so the two largest are two atomicMax passes.
//  * The boundary list is an ordered compaction: a ballot per wave counts, one wave scans the waves' counts, the same ballot
//    writes each cell at its rank.  An atomic append would give Qhull another input order and so another vertex numbering.
//  * The median: a thread per cell holds the 3 x 3 neighbourhood's 27 bytes in registers and ranks each of them once against all
//    27; the three outputs (each takes its own and its neighbouring channels, the channel axis reflected like the other two)
//    are weighted sums of the same per-channel ranks.
#include "hmsg_boundary.h"
#include "hmsg_nav_host.h"

#include <cfloat>
#include <climits>

#define NAV_T 256
#define NAV_MAX_CELLS (1ll << 28)

// an order-preserving code of a float64 (u64 compare == double compare)
__host__ __device__ static inline unsigned long long nav_ord(double v) {
    long long b;
    memcpy(&b, &v, 8);
    return b < 0 ? ~(unsigned long long)b : ((unsigned long long)b | 0x8000000000000000ull);
}
static inline double nav_unord(unsigned long long k) {
    const unsigned long long b = (k & 0x8000000000000000ull) ? (k & 0x7fffffffffffffffull) : ~k;
    double v;
    memcpy(&v, &b, 8);
    return v;
}

// ------------------------------------------------------------------------------------------ the cloud
// mm[0..2] = min codes, mm[3..5] = max codes of the points with y_lo <= y <= y_hi; cnt[0] = how many there are, cnt[1] = points
// of the whole cloud with a coordinate that is not finite (fmin / fmax and the slab test would pass a NaN over in silence)
__global__ __launch_bounds__(NAV_T) void k_nav_bounds(const double* __restrict__ xyz, long long n, double y_lo, double y_hi,
                                                      unsigned long long* __restrict__ mm, unsigned long long* __restrict__ cnt) {
    double lo[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, hi[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
    unsigned long long c = 0, bad = 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const double p[3] = {xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2]};
        const double y = p[1];
        if (!(p[0] - p[0] == 0.0 && p[1] - p[1] == 0.0 && p[2] - p[2] == 0.0)) {       // (v - v is NaN for a NaN and for an infinity)
            ++bad;
            continue;
        }
        if (!(y >= y_lo && y <= y_hi)) continue;
        ++c;
#pragma unroll
        for (int a = 0; a < 3; ++a) lo[a] = fmin(lo[a], p[a]), hi[a] = fmax(hi[a], p[a]);
    }
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) lo[a] = fmin(lo[a], __shfl_xor(lo[a], o)), hi[a] = fmax(hi[a], __shfl_xor(hi[a], o));
        c += __shfl_xor(c, o);
        bad += __shfl_xor(bad, o);
    }
    // the workgroup's four waves meet in LDS: seven atomics a workgroup on the seven shared words, not seven a wave
    __shared__ double s_lo[NAV_T / 64][3], s_hi[NAV_T / 64][3];
    __shared__ unsigned long long s_c[NAV_T / 64], s_bad[NAV_T / 64];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) s_lo[wave][a] = lo[a], s_hi[wave][a] = hi[a];
        s_c[wave] = c, s_bad[wave] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < NAV_T / 64; ++w) {
#pragma unroll
            for (int a = 0; a < 3; ++a) lo[a] = fmin(lo[a], s_lo[w][a]), hi[a] = fmax(hi[a], s_hi[w][a]);
            c += s_c[w], bad += s_bad[w];
        }
        if (c) {
#pragma unroll
            for (int a = 0; a < 3; ++a) atomicMin(&mm[a], nav_ord(lo[a])), atomicMax(&mm[3 + a], nav_ord(hi[a]));
            atomicAdd(cnt, c);
        }
        if (bad) atomicAdd(cnt + 1, bad);
    }
}

// one pass: obstacle cells (band_lo < y < band_hi), region cells (y < region_hi) and, with keys, the top-down winner of each
// region cell.  The cell of a coordinate is floor((v - min) / cell) in float64: subtract, then divide.
__global__ __launch_bounds__(NAV_T) void k_nav_points(const double* __restrict__ xyz, long long n, double y_lo, double y_hi, double min_x,
                                                      double min_y, double min_z, double cell, double band_lo, double band_hi,
                                                      double region_hi, int H, int W, unsigned char* __restrict__ obst,
                                                      unsigned char* __restrict__ reg, unsigned long long* __restrict__ keys) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double y = xyz[i * 3 + 1];
    if (!(y >= y_lo && y <= y_hi)) return;
    const double fx = floor((xyz[i * 3] - min_x) / cell), fz = floor((xyz[i * 3 + 2] - min_z) / cell);
    if (!(fx >= 0.0 && fx < (double)W && fz >= 0.0 && fz < (double)H)) return;          // (never for a cloud inside its own bounds)
    const size_t c = (size_t)(int)fz * W + (int)fx;
    if (y > band_lo && y < band_hi) obst[c] = 1;
    if (y < region_hi) {
        reg[c] = 1;
        if (keys) {
            const double fh = floor((y - min_y) / cell);
            const unsigned long long hc = fh >= 0.0 && fh < 2147483646.0 ? (unsigned long long)fh : 0ull;
            const unsigned long long key = ((hc + 1ull) << 32) | (unsigned long long)(~(unsigned)i);
            if (keys[c] < key) atomicMax(&keys[c], key);        // (a key only grows: a cell already above this one needs no atomic)
        }
    }
}

// ------------------------------------------------------------------------------------------ occupancy images
// cv2.dilate with a d x d box, one axis at a time: offsets -(d / 2) .. d - 1 - d / 2, the window clipped at the border
__global__ __launch_bounds__(NAV_T) void k_nav_dilate(const unsigned char* __restrict__ in, int H, int W, int d, int along_rows,
                                                      unsigned char* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= H * W) return;
    const int r = i / W, c = i - r * W;
    unsigned char v = 0;
    for (int k = -(d / 2); k <= d - 1 - d / 2; ++k) {
        const int rr = along_rows ? r + k : r, cc = along_rows ? c : c + k;
        if (rr >= 0 && rr < H && cc >= 0 && cc < W) v |= in[(size_t)rr * W + cc];
    }
    out[i] = v ? 1 : 0;
}
// cv2.GaussianBlur(float32, (3, 3), 0): (1, 2, 1) x (1, 2, 1) / 16, the border reflected without repeating the edge; a sum of at
// most 16 ones is exact in any order.  blur == 0: the image as it is.  map (optional) = the float32 image, bin = image > 0.
__device__ __forceinline__ int nav_reflect101(int i, int n) { return n == 1 ? 0 : (i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i)); }
__global__ __launch_bounds__(NAV_T) void k_nav_blur(const unsigned char* __restrict__ in, int H, int W, int blur, float* __restrict__ map,
                                                    unsigned char* __restrict__ bin) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= H * W) return;
    const int r = i / W, c = i - r * W;
    int s = 0;
    if (blur) {
        for (int dr = -1; dr <= 1; ++dr)
            for (int dc = -1; dc <= 1; ++dc)
                s += (2 - abs(dr)) * (2 - abs(dc)) * (int)in[(size_t)nav_reflect101(r + dr, H) * W + nav_reflect101(c + dc, W)];
    } else {
        s = 16 * (int)in[i];
    }
    if (map) map[i] = (float)s / 16.0f;
    bin[i] = s > 0 ? 1 : 0;
}
// grid (poses), cells int32 [poses][2] (x, z); half: the disc's half-width per |row offset|, r + 1 entries
__global__ __launch_bounds__(NAV_T) void k_nav_discs(const int* __restrict__ cells, const int* __restrict__ half, int r, int H, int W,
                                                     unsigned char* __restrict__ poses_map) {
    const long long cx = cells[blockIdx.x * 2], cy = cells[blockIdx.x * 2 + 1];
    const int side = 2 * r + 1;
    for (int t = threadIdx.x; t < side * side; t += blockDim.x) {
        const int dy = t / side - r, dx = t % side - r;
        if (abs(dx) > half[abs(dy)]) continue;
        const long long y = cy + dy, x = cx + dx;
        if (y >= 0 && y < H && x >= 0 && x < W) poses_map[(size_t)y * W + (size_t)x] = 1;
    }
}
// free = (region or disc) and obstacle_map == 0
__global__ __launch_bounds__(NAV_T) void k_nav_free(const unsigned char* __restrict__ reg, const unsigned char* __restrict__ poses,
                                                    const unsigned char* __restrict__ obst, int HW, unsigned char* __restrict__ free_map) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= HW) return;
    free_map[i] = ((reg[i] | poses[i]) && !obst[i]) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------ the height map (N10, H1 to H3)
// one pass: a point below top_hi takes part; its cell is k_nav_points', its height q = floor((y - zero) / unit) clamped to
// [0, 65535]; raw[cell] = the greatest q (an integer maximum: any order gives it), known[cell] = 1 (every point stores the same)
__global__ __launch_bounds__(NAV_T) void k_nav_height_points(const double* __restrict__ xyz, long long n, double y_lo, double y_hi, double min_x,
                                                             double min_z, double cell, double zero, double unit, double top_hi, int H, int W,
                                                             int* __restrict__ raw, unsigned char* __restrict__ known) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double y = xyz[i * 3 + 1];
    if (!(y >= y_lo && y <= y_hi) || !(y < top_hi)) return;
    const double fx = floor((xyz[i * 3] - min_x) / cell), fz = floor((xyz[i * 3 + 2] - min_z) / cell);
    if (!(fx >= 0.0 && fx < (double)W && fz >= 0.0 && fz < (double)H)) return;          // (never for a cloud inside its own bounds)
    const size_t c = (size_t)(int)fz * W + (int)fx;
    const double fq = floor((y - zero) / unit);
    const int q = fq >= 65535.0 ? 65535 : (fq > 0.0 ? (int)fq : 0);
    known[c] = 1;
    if (raw[c] < q) atomicMax(&raw[c], q);                      // (a cell only grows: one already at this height needs no atomic)
}
// the maximum over a d x d box (d odd), one axis at a time, the window clipped at the border; out16: the last pass narrows
__global__ __launch_bounds__(NAV_T) void k_nav_height_max(const int* __restrict__ in, int H, int W, int d, int along_rows, int* __restrict__ out,
                                                          unsigned short* __restrict__ out16) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= H * W) return;
    const int r = i / W, c = i - r * W;
    int v = 0;
    for (int k = -(d / 2); k <= d / 2; ++k) {
        const int rr = along_rows ? r + k : r, cc = along_rows ? c : c + k;
        if (rr >= 0 && rr < H && cc >= 0 && cc < W) v = max(v, in[(size_t)rr * W + cc]);
    }
    if (out16) out16[i] = (unsigned short)v;
    else out[i] = v;
}

// ------------------------------------------------------------------------------------------ the main region
// st[0] = components, st[1] = free cells, st[2] = the greatest key (area << 32 | root + 1)
__global__ __launch_bounds__(NAV_T) void k_nav_roots(int HW, const int* __restrict__ lab, const int* __restrict__ cnt,
                                                     unsigned long long* __restrict__ st) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool root = i < HW && lab[i] == i;
    const unsigned long long area = root ? (unsigned long long)(unsigned)cnt[i] : 0ull;
    unsigned long long n = root ? 1ull : 0ull, sum = area, best = root ? ((area << 32) | (unsigned long long)(i + 1)) : 0ull;
    for (int o = 32; o > 0; o >>= 1) {
        n += __shfl_xor(n, o);
        sum += __shfl_xor(sum, o);
        const unsigned long long b = __shfl_xor(best, o);
        best = b > best ? b : best;
    }
    if ((threadIdx.x & 63) == 0 && n) {
        atomicAdd(&st[0], n);
        atomicAdd(&st[1], sum);
        atomicMax(&st[2], best);
    }
}
// st[3] = the greatest key below st[2]
__global__ __launch_bounds__(NAV_T) void k_nav_second(int HW, const int* __restrict__ lab, const int* __restrict__ cnt,
                                                      unsigned long long* __restrict__ st) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long first = st[2];
    const bool root = i < HW && lab[i] == i;
    unsigned long long best = root ? (((unsigned long long)(unsigned)cnt[i] << 32) | (unsigned long long)(i + 1)) : 0ull;
    if (best == first) best = 0ull;
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long b = __shfl_xor(best, o);
        best = b > best ? b : best;
    }
    if ((threadIdx.x & 63) == 0 && best) atomicMax(&st[3], best);
}
// main = (label == the chosen one): root >= 0: the component of that root; root < 0: the background.  rank: roots in front of
// `root` (its label is rank + 1)
__global__ __launch_bounds__(NAV_T) void k_nav_main(int HW, const int* __restrict__ lab, const unsigned char* __restrict__ free_map, int root,
                                                    unsigned char* __restrict__ main_map, unsigned long long* __restrict__ rank) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = i < HW;
    const int l = in ? lab[i] : -1;
    const unsigned long long before = __ballot(in && l == i && i < root);
    if ((threadIdx.x & 63) == 0 && before) atomicAdd(rank, (unsigned long long)__popcll(before));
    if (in) main_map[i] = root < 0 ? (free_map[i] ? 0 : 1) : (l == root ? 1 : 0);
}

// ------------------------------------------------------------------------------------------ the boundary, in row-major order
// main minus its erosion by the 4-neighbour cross, outside counting as 0
__device__ __forceinline__ bool nav_is_boundary(const unsigned char* __restrict__ m, int i, int H, int W) {
    if (!m[i]) return false;
    const int r = i / W, c = i - r * W;
    return !(r > 0 && m[i - W] && r < H - 1 && m[i + W] && c > 0 && m[i - 1] && c < W - 1 && m[i + 1]);
}
__global__ __launch_bounds__(NAV_T) void k_nav_bcount(const unsigned char* __restrict__ m, int H, int W, int* __restrict__ wave_cnt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long b = __ballot(i < H * W && nav_is_boundary(m, i, H, W));
    if ((threadIdx.x & 63) == 0) wave_cnt[i >> 6] = __popcll(b);
}
// one wave: wave_off = exclusive scan of wave_cnt [nw], *total = the sum
__global__ __launch_bounds__(64) void k_nav_bscan(int nw, const int* __restrict__ wave_cnt, long long* __restrict__ wave_off,
                                                  long long* __restrict__ total) {
    const int lane = threadIdx.x;
    long long carry = 0;
    for (int w0 = 0; w0 < nw; w0 += 64) {
        const int w = w0 + lane;
        const long long n = w < nw ? wave_cnt[w] : 0;
        long long incl = n;
        for (int d = 1; d < 64; d <<= 1) {
            const long long up = __shfl_up(incl, (unsigned)d);
            if (lane >= d) incl += up;
        }
        if (w < nw) wave_off[w] = carry + incl - n;
        carry += __shfl(incl, 63);
    }
    if (lane == 0) *total = carry;
}
__global__ __launch_bounds__(NAV_T) void k_nav_bwrite(const unsigned char* __restrict__ m, int H, int W, const long long* __restrict__ wave_off,
                                                      int* __restrict__ rc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
    const bool is = i < H * W && nav_is_boundary(m, i, H, W);
    const unsigned long long b = __ballot(is);
    if (!is) return;
    const long long at = wave_off[i >> 6] + __popcll(b & ((1ull << lane) - 1ull));
    rc[at * 2] = i / W;
    rc[at * 2 + 1] = i % W;
}

// ------------------------------------------------------------------------------------------ the top-down image
// the winner's colour, uint8(c * 255) truncated; an empty cell is 0
__global__ __launch_bounds__(NAV_T) void k_nav_colour(const unsigned long long* __restrict__ keys, const double* __restrict__ rgb, int HW,
                                                      unsigned char* __restrict__ img) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= HW) return;
    const unsigned long long k = keys[i];
    unsigned char v[3] = {0, 0, 0};
    if (k) {
        const size_t p = (size_t)(~(unsigned)(k & 0xffffffffull));
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double c = rgb[p * 3 + a] * 255.0;
            v[a] = (unsigned char)(c >= 0.0 && c < 256.0 ? (int)c : 0);
        }
    }
    img[(size_t)i * 3] = v[0], img[(size_t)i * 3 + 1] = v[1], img[(size_t)i * 3 + 2] = v[2];
}
// scipy.ndimage.median_filter(size=3) of the (H, W, 3) array, mode reflect (the edge repeated) on all three axes, channels reversed.
// Output channel ch takes the 27 values of the 3 x 3 cells in channels ch - 1 .. ch + 1 with the channel axis reflected: channel
// 0 counts twice for output 0, channel 2 twice for output 2.  The 27 bytes of the neighbourhood stay in registers; each of them in
// turn (read again through the cache: no dynamic register index) is ranked against all 27 once, per channel, and the three
// weighted ranks say for which outputs it is the 14th smallest.  A value that an output's multiset does not hold has no rank there.
__global__ __launch_bounds__(NAV_T) void k_nav_median(const unsigned char* __restrict__ img, int H, int W, unsigned char* __restrict__ bgr) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= H * W) return;
    const int r = i / W, c = i - r * W;
    int px[9][3];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int rr = min(max(r + k / 3 - 1, 0), H - 1), cc = min(max(c + k % 3 - 1, 0), W - 1);
        const unsigned char* p = img + ((size_t)rr * W + cc) * 3;
        px[k][0] = p[0], px[k][1] = p[1], px[k][2] = p[2];
    }
    int med[3] = {0, 0, 0};
#pragma unroll 1
    for (int a = 0; a < 27; ++a) {
        const int ka = a / 3;
        const int rr = min(max(r + ka / 3 - 1, 0), H - 1), cc = min(max(c + ka % 3 - 1, 0), W - 1);
        const int v = img[((size_t)rr * W + cc) * 3 + (a - ka * 3)];
        int lt[3] = {0, 0, 0}, le[3] = {0, 0, 0};
#pragma unroll
        for (int k = 0; k < 9; ++k)
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) lt[ch] += px[k][ch] < v ? 1 : 0, le[ch] += px[k][ch] <= v ? 1 : 0;
        if (2 * lt[0] + lt[1] <= 13 && 13 < 2 * le[0] + le[1]) med[0] = v;
        if (lt[0] + lt[1] + lt[2] <= 13 && 13 < le[0] + le[1] + le[2]) med[1] = v;
        if (lt[1] + 2 * lt[2] <= 13 && 13 < le[1] + 2 * le[2]) med[2] = v;
    }
    bgr[(size_t)i * 3 + 2] = (unsigned char)med[0], bgr[(size_t)i * 3 + 1] = (unsigned char)med[1], bgr[(size_t)i * 3] = (unsigned char)med[2];
}

// ------------------------------------------------------------------------------------------ the calls
namespace {
thread_local int g_nav_last_rounds = 0;       // what hmsg_test_nav_last reports: the labelling rounds of this thread's last call

struct NavGrid {
    double mn[3], mx[3];
    int W, H;             // grid[0] = columns (x), grid[1] = rows (z)
    long long n_in;       // points inside the slab
};

void nav_check_params(const hmsg_nav_params& p, const char* fn) {
    const std::string f = fn;
    HMSG_REQUIRE(std::isfinite(p.cell_size) && p.cell_size > 0.0, HMSG_ERR_INVALID, f + ": cell_size must be positive");
    HMSG_REQUIRE(std::isfinite(p.obstacle_lo) && std::isfinite(p.obstacle_hi) && std::isfinite(p.region_max) && std::isfinite(p.pose_radius) &&
                     std::isfinite(p.pose_eps) && p.pose_radius >= 0.0 && p.pose_eps >= 0.0,
                 HMSG_ERR_INVALID, f + ": a parameter is not finite or negative");
    HMSG_REQUIRE(p.dilation >= 0 && p.dilation <= 63, HMSG_ERR_INVALID, f + ": dilation must be in [0, 63]");
    HMSG_REQUIRE(p.blur == 0 || p.blur == 3, HMSG_ERR_UNSUPPORTED, f + ": blur must be 3 (the reference) or 0 (none)");
    HMSG_REQUIRE(p.pose_min_samples >= 1, HMSG_ERR_INVALID, f + ": pose_min_samples < 1");
    HMSG_REQUIRE(p.region_rule == 0 || p.region_rule == 1, HMSG_ERR_INVALID, f + ": region_rule must be 0 or 1");
    HMSG_REQUIRE(p.pose_radius / p.cell_size < 4096.0, HMSG_ERR_INVALID, f + ": pose_radius is more than 4096 cells");
}

// bounds and grid of the points of d_xyz with y_lo <= y <= y_hi
NavGrid nav_grid(hipStream_t s, const double* d_xyz, long long n, double y_lo, double y_hi, double cell, const char* fn) {
    const std::string f = fn;
    DevBuf<unsigned long long> mm;
    mm.alloc(8);
    unsigned long long init[8] = {~0ull, ~0ull, ~0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    HIP_TRY(hipMemcpyAsync(mm.p, init, sizeof(init), hipMemcpyHostToDevice, s));
    if (n) {
        const unsigned blocks = (unsigned)std::min<size_t>(cdiv((size_t)n, NAV_T), 512);       // (a grid-stride loop: two workgroups a CU)
        hipLaunchKernelGGL(k_nav_bounds, dim3(blocks), dim3(NAV_T), 0, s, d_xyz, n, y_lo, y_hi, mm.p, mm.p + 6);
        HMSG_CHECK_LAUNCH();
    }
    unsigned long long got[8];
    HIP_TRY(hipMemcpyAsync(got, mm.p, sizeof(got), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    NavGrid g{};
    g.n_in = (long long)got[6];
    HMSG_REQUIRE(got[7] == 0, HMSG_ERR_INVALID, f + ": " + std::to_string(got[7]) + " points have a coordinate that is not finite");
    HMSG_REQUIRE(g.n_in > 0, HMSG_ERR_INVALID, f + ": the storey has no points");
    int grid[3];
    for (int a = 0; a < 3; ++a) {
        g.mn[a] = nav_unord(got[a]), g.mx[a] = nav_unord(got[3 + a]);
        HMSG_REQUIRE(std::isfinite(g.mn[a]) && std::isfinite(g.mx[a]), HMSG_ERR_INVALID, f + ": a coordinate is not finite");
        const double cells = std::ceil((g.mx[a] - g.mn[a]) / cell + 1.0);
        HMSG_REQUIRE(cells < (double)NAV_MAX_CELLS, HMSG_ERR_UNSUPPORTED, f + ": the grid has more than 2^28 cells along an axis");
        grid[a] = (int)cells;
    }
    g.W = grid[0], g.H = grid[2];
    HMSG_REQUIRE((long long)g.W * g.H < NAV_MAX_CELLS, HMSG_ERR_UNSUPPORTED, f + ": the grid has 2^28 cells or more");
    return g;
}

void nav_put_grid(const NavGrid& g, double* pcd_min, double* pcd_max, int32_t* grid) {
    for (int a = 0; a < 3; ++a) {
        if (pcd_min) pcd_min[a] = g.mn[a];
        if (pcd_max) pcd_max[a] = g.mx[a];
    }
    if (grid) grid[0] = g.W, grid[1] = g.H;
}
}  // namespace

// the stage on device points (hmsg_common.h); d_rgb may be null.  poses: host or device memory.
void hmsg_nav_maps_device(const char* fn, const hmsg_nav_params& prm, const double* d_xyz, const double* d_rgb, long long n, double y_lo,
                          double y_hi, double zero_level, int n_poses, const double* poses, hmsg_nav_maps* out) {
    const std::string f = fn;
    nav_check_params(prm, fn);
    HMSG_REQUIRE(n >= 0 && n < (1ll << 32) && n_poses >= 0 && std::isfinite(zero_level), HMSG_ERR_INVALID,
                 f + ": 0 <= n < 2^32, n_poses >= 0 and a finite zero_level");
    HMSG_REQUIRE(!out->boundary_rc || out->boundary_capacity >= 0, HMSG_ERR_INVALID, f + ": boundary_capacity < 0");
    out->n_boundary = 0, out->n_regions = 0, out->main_label = -1, out->main_area = 0;
    ScopedStream s(hipStreamNonBlocking);
    const NavGrid g = nav_grid(s, d_xyz, n, y_lo, y_hi, prm.cell_size, fn);
    nav_put_grid(g, out->pcd_min, out->pcd_max, out->grid);
    const int H = g.H, W = g.W, HW = H * W;
    const dim3 gi(cdiv((size_t)HW, NAV_T)), b(NAV_T);

    // ---- the poses that mark free space: chosen on the host (a few thousand heights), drawn on the device
    HMSG_REQUIRE(n_poses > 0 && poses, HMSG_ERR_INVALID, f + ": no pose on the floor");
    std::vector<double> P((size_t)n_poses * 16), heights((size_t)n_poses);
    read_in(P.data(), poses, P.size() * 8);
    for (int i = 0; i < n_poses; ++i) {
        heights[(size_t)i] = P[(size_t)i * 16 + 7];
        HMSG_REQUIRE(std::isfinite(heights[(size_t)i]), HMSG_ERR_INVALID, f + ": the height of pose " + std::to_string(i) + " is not finite");
    }
    const std::vector<int32_t> keep = nav_host::select_poses(heights.data(), heights.size(), prm.pose_eps, prm.pose_min_samples);
    HMSG_REQUIRE(!keep.empty(), HMSG_ERR_INVALID, f + ": no pose is left near the major pose height");
    std::vector<int32_t> cells(keep.size() * 2);
    for (size_t k = 0; k < keep.size(); ++k) {
        cells[k * 2] = nav_host::trunc_i32((P[(size_t)keep[k] * 16 + 3] - g.mn[0]) / prm.cell_size);
        cells[k * 2 + 1] = nav_host::trunc_i32((P[(size_t)keep[k] * 16 + 11] - g.mn[2]) / prm.cell_size);
    }
    const int radius = (int)(prm.pose_radius / prm.cell_size);
    const std::vector<int32_t> half = nav_host::circle_half_widths(radius);

    // ---- one pass over the cloud
    DevBuf<unsigned char> obst0, reg0, tmp, dil, obst_bin, own_region, own_poses, own_free, own_main, img, own_bgr;
    DevBuf<float> own_map;
    DevBuf<unsigned long long> keys;
    obst0.alloc((size_t)HW), reg0.alloc((size_t)HW), tmp.alloc((size_t)HW), dil.alloc((size_t)HW), obst_bin.alloc((size_t)HW);
    obst0.zero(s), reg0.zero(s);
    const bool want_td = d_rgb && out->top_down_bgr;
    if (want_td) keys.alloc((size_t)HW), keys.zero(s);
    const double band_lo = zero_level + prm.obstacle_lo, band_hi = zero_level + prm.obstacle_hi, region_hi = zero_level + prm.region_max;
    hipLaunchKernelGGL(k_nav_points, dim3(cdiv((size_t)n, NAV_T)), b, 0, s, d_xyz, n, y_lo, y_hi, g.mn[0], g.mn[1], g.mn[2], prm.cell_size, band_lo,
                       band_hi, region_hi, H, W, obst0.p, reg0.p, want_td ? keys.p : (unsigned long long*)nullptr);
    HMSG_CHECK_LAUNCH();

    // ---- create_occupancy_grid of both, the discs, the free map
    float* p_map = stage_out(own_map, out->obstacle_map, (size_t)HW);
    unsigned char* p_region = stage_out(own_region, out->region_map, (size_t)HW);
    unsigned char* p_poses = stage_out(own_poses, out->poses_map, (size_t)HW);
    unsigned char* p_free = stage_out(own_free, out->free_map, (size_t)HW);
    unsigned char* p_main = stage_out(own_main, out->main_free_map, (size_t)HW);
    if (!p_region) own_region.alloc((size_t)HW), p_region = own_region.p;
    if (!p_poses) own_poses.alloc((size_t)HW), p_poses = own_poses.p;
    if (!p_free) own_free.alloc((size_t)HW), p_free = own_free.p;
    if (!p_main) own_main.alloc((size_t)HW), p_main = own_main.p;
    auto occupancy = [&](const unsigned char* cells_in, float* map, unsigned char* bin) {
        const unsigned char* d = cells_in;
        if (prm.dilation > 0) {
            hipLaunchKernelGGL(k_nav_dilate, gi, b, 0, s, cells_in, H, W, prm.dilation, 0, tmp.p);
            hipLaunchKernelGGL(k_nav_dilate, gi, b, 0, s, (const unsigned char*)tmp.p, H, W, prm.dilation, 1, dil.p);
            d = dil.p;
        }
        hipLaunchKernelGGL(k_nav_blur, gi, b, 0, s, d, H, W, prm.blur, map, bin);
    };
    occupancy(obst0.p, p_map, obst_bin.p);
    occupancy(reg0.p, nullptr, p_region);
    DevBuf<int> d_cells, d_half;
    d_cells.alloc(cells.size()), d_half.alloc(half.size());
    HIP_TRY(hipMemcpyAsync(d_cells.p, cells.data(), cells.size() * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_half.p, half.data(), half.size() * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(p_poses, 0, (size_t)HW, s));
    hipLaunchKernelGGL(k_nav_discs, dim3((unsigned)keep.size()), b, 0, s, (const int*)d_cells.p, (const int*)d_half.p, radius, H, W, p_poses);
    hipLaunchKernelGGL(k_nav_free, gi, b, 0, s, (const unsigned char*)p_region, (const unsigned char*)p_poses, (const unsigned char*)obst_bin.p, HW,
                       p_free);
    HMSG_CHECK_LAUNCH();

    // ---- get_largest_region
    DevBuf<int> lab, cnt;
    DevBuf<unsigned long long> st;
    lab.alloc((size_t)HW), cnt.alloc((size_t)HW), st.alloc(5);
    st.zero(s);
    g_nav_last_rounds = hmsg_cc8_components(s, p_free, 1, H, W, 1, lab.p, cnt.p);
    hipLaunchKernelGGL(k_nav_roots, gi, b, 0, s, HW, (const int*)lab.p, (const int*)cnt.p, st.p);
    hipLaunchKernelGGL(k_nav_second, gi, b, 0, s, HW, (const int*)lab.p, (const int*)cnt.p, st.p);
    HMSG_CHECK_LAUNCH();
    unsigned long long h_st[4];
    HIP_TRY(hipMemcpyAsync(h_st, st.p, sizeof(h_st), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    out->n_regions = (int32_t)h_st[0] + 1;                  // the background is a label
    HMSG_REQUIRE(h_st[0] >= 1, HMSG_ERR_INVALID, f + ": no free cell (the labelling has fewer than two labels)");
    const unsigned long long bg_key = ((unsigned long long)HW - h_st[1]) << 32;      // label 0: the smallest label of its area
    unsigned long long chosen;
    if (prm.region_rule == 1) {
        chosen = h_st[2];
    } else {                                                // the second in descending order of (area, label), the background counted
        unsigned long long top[3] = {h_st[2], h_st[3], bg_key};
        std::sort(top, top + 3, [](unsigned long long a, unsigned long long c) { return a > c; });
        chosen = h_st[0] >= 2 ? top[1] : std::min(h_st[2], bg_key);
    }
    const int root = (chosen & 0xffffffffull) ? (int)(chosen & 0xffffffffull) - 1 : -1;
    out->main_area = (int64_t)(chosen >> 32);
    hipLaunchKernelGGL(k_nav_main, gi, b, 0, s, HW, (const int*)lab.p, (const unsigned char*)p_free, root, p_main, st.p + 4);
    HMSG_CHECK_LAUNCH();

    // ---- the boundary list
    const int nw = (int)cdiv((size_t)HW, 64);
    DevBuf<int> wave_cnt;
    DevBuf<long long> wave_off;
    wave_cnt.alloc((size_t)gi.x * (NAV_T / 64)), wave_off.alloc((size_t)nw + 1);
    hipLaunchKernelGGL(k_nav_bcount, gi, b, 0, s, (const unsigned char*)p_main, H, W, wave_cnt.p);
    hipLaunchKernelGGL(k_nav_bscan, dim3(1), dim3(64), 0, s, nw, (const int*)wave_cnt.p, wave_off.p, wave_off.p + nw);
    HMSG_CHECK_LAUNCH();
    long long total = 0;
    unsigned long long rank = 0;
    HIP_TRY(hipMemcpyAsync(&total, wave_off.p + nw, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&rank, st.p + 4, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    out->n_boundary = total;
    out->main_label = root < 0 ? 0 : (int32_t)rank + 1;
    const bool list_too_short = out->boundary_rc && total > out->boundary_capacity;      // (reported when the maps are out)
    DevBuf<int> own_rc;
    if (out->boundary_rc && total && !list_too_short) {
        int* p_rc = stage_out(own_rc, out->boundary_rc, (size_t)total * 2);
        hipLaunchKernelGGL(k_nav_bwrite, gi, b, 0, s, (const unsigned char*)p_main, H, W, (const long long*)wave_off.p, p_rc);
        HMSG_CHECK_LAUNCH();
        unstage_out(out->boundary_rc, p_rc, (size_t)total * 2, s);
    }

    // ---- the top-down image
    if (want_td) {
        img.alloc((size_t)HW * 3);
        unsigned char* p_bgr = stage_out(own_bgr, out->top_down_bgr, (size_t)HW * 3);
        hipLaunchKernelGGL(k_nav_colour, gi, b, 0, s, (const unsigned long long*)keys.p, d_rgb, HW, img.p);
        hipLaunchKernelGGL(k_nav_median, gi, b, 0, s, (const unsigned char*)img.p, H, W, p_bgr);
        HMSG_CHECK_LAUNCH();
        unstage_out(out->top_down_bgr, p_bgr, (size_t)HW * 3, s);
    }
    if (out->obstacle_map) unstage_out(out->obstacle_map, p_map, (size_t)HW, s);
    if (out->region_map) unstage_out(out->region_map, p_region, (size_t)HW, s);
    if (out->poses_map) unstage_out(out->poses_map, p_poses, (size_t)HW, s);
    if (out->free_map) unstage_out(out->free_map, p_free, (size_t)HW, s);
    if (out->main_free_map) unstage_out(out->main_free_map, p_main, (size_t)HW, s);
    HIP_TRY(hipStreamSynchronize(s));
    if (list_too_short)
        throw hmsg_error{HMSG_ERR_INVALID, f + ": " + std::to_string(total) + " boundary cells, boundary_rc holds " +
                                               std::to_string((long long)out->boundary_capacity) + " (n_boundary says what is needed)"};
}

void hmsg_nav_grid_device(const char* fn, double cell_size, const double* d_xyz, long long n, double y_lo, double y_hi, double* pcd_min,
                          double* pcd_max, int32_t* grid) {
    HMSG_REQUIRE(std::isfinite(cell_size) && cell_size > 0.0 && n >= 0, HMSG_ERR_INVALID, std::string(fn) + ": cell_size must be positive, n >= 0");
    ScopedStream s(hipStreamNonBlocking);
    nav_put_grid(nav_grid(s, d_xyz, n, y_lo, y_hi, cell_size, fn), pcd_min, pcd_max, grid);
}

// N10, H1 to H3: the bounds come from nav_grid (k_nav_bounds), so the map lies cell for cell on hmsg_nav_maps_device's
void hmsg_nav_height_device(const char* fn, const hmsg_height_params& prm, const double* d_xyz, long long n, double y_lo, double y_hi,
                            double zero_level, uint16_t* top, uint8_t* known, double* pcd_min, double* pcd_max, int32_t* grid) {
    const std::string f = fn;
    HMSG_REQUIRE(std::isfinite(prm.cell_size) && prm.cell_size > 0.0, HMSG_ERR_INVALID, f + ": cell_size must be positive");
    HMSG_REQUIRE(std::isfinite(prm.height_unit) && prm.height_unit > 0.0, HMSG_ERR_INVALID, f + ": height_unit must be positive");
    HMSG_REQUIRE(std::isfinite(prm.top_max) && prm.top_max > 0.0, HMSG_ERR_INVALID, f + ": top_max must be positive");
    HMSG_REQUIRE(prm.dilation >= 0 && prm.dilation <= 63, HMSG_ERR_INVALID, f + ": dilation must be in [0, 63]");
    HMSG_REQUIRE(prm.dilation == 0 || (prm.dilation & 1), HMSG_ERR_UNSUPPORTED, f + ": an even dilation has no centre cell");
    HMSG_REQUIRE(n >= 0 && n < (1ll << 32) && std::isfinite(zero_level), HMSG_ERR_INVALID, f + ": 0 <= n < 2^32 and a finite zero_level");
    ScopedStream s(hipStreamNonBlocking);
    const NavGrid g = nav_grid(s, d_xyz, n, y_lo, y_hi, prm.cell_size, fn);
    nav_put_grid(g, pcd_min, pcd_max, grid);
    const int H = g.H, W = g.W, HW = H * W;
    const dim3 gi(cdiv((size_t)HW, NAV_T)), b(NAV_T);
    DevBuf<int> raw, tmp;
    DevBuf<unsigned short> own_top;
    DevBuf<unsigned char> own_known;
    raw.alloc((size_t)HW), raw.zero(s);
    unsigned short* p_top = stage_out(own_top, (unsigned short*)top, (size_t)HW);
    unsigned char* p_known = stage_out(own_known, known, (size_t)HW);
    if (!p_known) own_known.alloc((size_t)HW), p_known = own_known.p;
    HIP_TRY(hipMemsetAsync(p_known, 0, (size_t)HW, s));
    hipLaunchKernelGGL(k_nav_height_points, dim3(cdiv((size_t)n, NAV_T)), b, 0, s, d_xyz, n, y_lo, y_hi, g.mn[0], g.mn[2], prm.cell_size, zero_level,
                       prm.height_unit, zero_level + prm.top_max, H, W, raw.p, p_known);
    const int d = prm.dilation > 1 ? prm.dilation : 1;
    if (d > 1) {
        tmp.alloc((size_t)HW);
        hipLaunchKernelGGL(k_nav_height_max, gi, b, 0, s, (const int*)raw.p, H, W, d, 0, tmp.p, (unsigned short*)nullptr);
        hipLaunchKernelGGL(k_nav_height_max, gi, b, 0, s, (const int*)tmp.p, H, W, d, 1, (int*)nullptr, p_top);
    } else {
        hipLaunchKernelGGL(k_nav_height_max, gi, b, 0, s, (const int*)raw.p, H, W, 1, 0, (int*)nullptr, p_top);
    }
    HMSG_CHECK_LAUNCH();
    unstage_out((unsigned short*)top, (const unsigned short*)p_top, (size_t)HW, s);
    if (known) unstage_out(known, (const unsigned char*)p_known, (size_t)HW, s);
    HIP_TRY(hipStreamSynchronize(s));
}

extern "C" void hmsg_height_default_params(hmsg_height_params* p) {
    if (!p) return;
    p->cell_size = 0.03;
    p->height_unit = 0.01;
    p->top_max = 2.5;
    p->dilation = 5;
    p->reserved_ = 0;
}

extern "C" int hmsg_nav_height_map(int32_t device_id, const hmsg_height_params* prm, int64_t n, const double* xyz, double zero_level,
                                   uint16_t* top, uint8_t* known, double* pcd_min, double* pcd_max, int32_t* grid) {
    if (!prm || !xyz || !top) return HMSG_ERR_INVALID;
    return hmsg_boundary("hmsg_nav_height_map", device_id, [&] {
        HMSG_REQUIRE(n >= 0, HMSG_ERR_INVALID, "hmsg_nav_height_map: n < 0");
        ScopedStream s(hipStreamNonBlocking);
        DevBuf<double> own_xyz;
        const double* d_xyz = stage_in(own_xyz, xyz, (size_t)n * 3, s, Up::bounce);
        HIP_TRY(hipStreamSynchronize(s));
        hmsg_nav_height_device("hmsg_nav_height_map", *prm, d_xyz, n, -INFINITY, INFINITY, zero_level, top, known, pcd_min, pcd_max, grid);
    });
}

extern "C" void hmsg_nav_default_params(hmsg_nav_params* p) {
    if (!p) return;
    p->cell_size = 0.03;
    p->obstacle_lo = 1.4;
    p->obstacle_hi = 2.5;
    p->region_max = 1.5;
    p->pose_radius = 0.5;
    p->pose_eps = 0.1;
    p->dilation = 5;
    p->blur = 3;
    p->pose_min_samples = 5;
    p->region_rule = 0;
}

extern "C" int hmsg_nav_grid(int32_t device_id, double cell_size, int64_t n, const double* xyz, double* pcd_min, double* pcd_max, int32_t* grid) {
    if (!xyz || !grid) return HMSG_ERR_INVALID;
    return hmsg_boundary("hmsg_nav_grid", device_id, [&] {
        ScopedStream s(hipStreamNonBlocking);
        DevBuf<double> own;
        const double* d_xyz = stage_in(own, xyz, (size_t)std::max<int64_t>(n, 0) * 3, s, Up::bounce);
        HIP_TRY(hipStreamSynchronize(s));
        hmsg_nav_grid_device("hmsg_nav_grid", cell_size, d_xyz, n, -INFINITY, INFINITY, pcd_min, pcd_max, grid);
    });
}

extern "C" int hmsg_nav_floor_maps(int32_t device_id, const hmsg_nav_params* prm, int64_t n, const double* xyz, const double* rgb,
                                   double zero_level, int32_t n_poses, const double* poses, hmsg_nav_maps* out) {
    if (!prm || !xyz || !out) return HMSG_ERR_INVALID;
    return hmsg_boundary("hmsg_nav_floor_maps", device_id, [&] {
        HMSG_REQUIRE(n >= 0, HMSG_ERR_INVALID, "hmsg_nav_floor_maps: n < 0");
        ScopedStream s(hipStreamNonBlocking);
        DevBuf<double> own_xyz, own_rgb;
        const double* d_xyz = stage_in(own_xyz, xyz, (size_t)n * 3, s, Up::bounce);
        const double* d_rgb = rgb && out->top_down_bgr ? stage_in(own_rgb, rgb, (size_t)n * 3, s, Up::bounce) : nullptr;
        HIP_TRY(hipStreamSynchronize(s));
        hmsg_nav_maps_device("hmsg_nav_floor_maps", *prm, d_xyz, d_rgb, n, -INFINITY, INFINITY, zero_level, n_poses, poses, out);
    });
}

// ---- the same stage on a slab of a scene's map (the Python Graph holds a scene, not a graph handle)
static void nav_scene_ready(hmsg_ctx* h, double y_lo, double y_hi, const char* fn) {
    HMSG_REQUIRE(h->map_ready, HMSG_ERR_INVALID, std::string(fn) + ": map not finalised");
    HMSG_REQUIRE(y_lo <= y_hi, HMSG_ERR_INVALID, std::string(fn) + ": y_lo <= y_hi (NaN is refused)");
    HIP_TRY(hipStreamSynchronize(h->stream));
}
extern "C" int hmsg_map_nav_grid(hmsg_t* hc, double y_lo, double y_hi, double cell_size, double* pcd_min, double* pcd_max, int32_t* grid) {
    hmsg_ctx* h = hc;
    if (!h || !grid) return HMSG_ERR_INVALID;
    return hmsg_boundary(h, [&] {
        nav_scene_ready(h, y_lo, y_hi, "hmsg_map_nav_grid");
        hmsg_nav_grid_device("hmsg_map_nav_grid", cell_size, (const double*)h->pts.p, (long long)h->V, y_lo, y_hi, pcd_min, pcd_max, grid);
    });
}
extern "C" int hmsg_map_nav_floor_maps(hmsg_t* hc, double y_lo, double y_hi, double zero_level, const hmsg_nav_params* prm, int32_t n_poses,
                                       const double* poses, hmsg_nav_maps* out) {
    hmsg_ctx* h = hc;
    if (!h || !prm || !out) return HMSG_ERR_INVALID;
    return hmsg_boundary(h, [&] {
        nav_scene_ready(h, y_lo, y_hi, "hmsg_map_nav_floor_maps");
        hmsg_nav_maps_device("hmsg_map_nav_floor_maps", *prm, (const double*)h->pts.p, (const double*)h->cols.p, (long long)h->V, y_lo, y_hi,
                             zero_level, n_poses, poses, out);
    });
}

extern "C" int hmsg_map_nav_height_map(hmsg_t* hc, double y_lo, double y_hi, double zero_level, const hmsg_height_params* prm, uint16_t* top,
                                       uint8_t* known, double* pcd_min, double* pcd_max, int32_t* grid) {
    hmsg_ctx* h = hc;
    if (!h || !prm || !top) return HMSG_ERR_INVALID;
    return hmsg_boundary(h, [&] {
        nav_scene_ready(h, y_lo, y_hi, "hmsg_map_nav_height_map");
        hmsg_nav_height_device("hmsg_map_nav_height_map", *prm, (const double*)h->pts.p, (long long)h->V, y_lo, y_hi, zero_level, top, known,
                               pcd_min, pcd_max, grid);
    });
}

extern "C" int hmsg_test_nav_last(int32_t* label_rounds) {
    if (label_rounds) *label_rounds = g_nav_last_rounds;
    return HMSG_OK;
}
