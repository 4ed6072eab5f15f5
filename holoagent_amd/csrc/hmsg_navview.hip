// Viewpoints on a floor's free map (include/hmsg.h, N8: hmsg_nav_viewpoints, hmsg_nav_view_route): for a goal cell, the passable,
// reached cells within a band of distances from which the goal is in sight on the obstacle map, and the best of them to stand on.
// N7's snap (R4) takes the nearest passable cell whatever lies between it and the goal; with a clearance that cell can be on the
// other side of a wall.  The reference has no such stage (its goal pose is an object's centre, goal_pose_publisher.py:260-271; the
// slow path looks for the object again on arrival), so the rules V1 to V5 are this library's own and stand in the header.  All of
// it is integer work with one right answer.
//
// MI355X design notes
//  * k_navv_view: a workgroup of 256 threads (four waves) per goal.  r_max2 <= 255^2 (V5) bounds the window round the goal to
//    511 x 511 cells; the workgroup packs the window's blocking bytes, clipped to the image, into LDS bits: a wave reads 64
//    consecutive bytes of a row (one coalesced load), __ballot makes them one 64-bit word.  511 rows x 17 words (16 of bits, one of
//    padding: an odd stride, so threads on neighbouring rows of one column do not meet on a bank) = 34 KB, one workgroup's whole
//    sight map; a line walk never touches global memory.
//  * A thread takes the window's cells in row-major order, 256 apart.  A cell is dropped by the d2 band, the passable byte and
//    the field before anything is walked; the walk is V1 with an error term (no division), leaves at the first blocking bit, and
//    reads only cells inside the bounding box of its two endpoints, both of which are inside the window.  Lanes of a wave hold
//    neighbouring cells, so their lines have nearly the same length and the same first steps.
//  * The key of V4 is (field value, d2, index) or (d2, field value, index): 31 + 17 + 28 bits, more than a 64-bit word, so there
//    is no packed atomic minimum.  A thread keeps its least triple, the triples meet by wave shuffles and then through LDS, as
//    k_navr_snap's pairs do; n_visible is summed the same way.  No global atomics.  The index is the global row-major one, whose
//    order on the window's cells is the window's own.
//  * visible (where asked for) is written whole by the goal's workgroup with plain byte stores from consecutive lanes: the
//    window's cells by the thread that judged them, every other cell 0.
//  * k_navv_view_h (N10: hmsg_nav_viewpoints_h, hmsg_nav_view_route_h) is the same body with heights (S1 to S5).  A 511 x 511
//    window of u16 heights is 522 KB; what fits LDS is two bitmaps, because for one goal the ray stays within [min(eye, goal_h),
//    max(eye, goal_h)]: "tall" cells (T >= the upper end) always block, cells that are not "not low" (T < the lower end) never
//    do, and only a cell between the two has its height read from the map (at most some 700 KB, resident in L2).  With eye ==
//    goal_h, or a map of 0 and 65535, no such read happens and the walk is k_navv_view's.  Two bitmaps at stride 17 are 69.5 KB:
//    the device's LDS limit per workgroup (hipDeviceAttributeMaxSharedMemoryPerBlock, read once) decides between that and
//    stride 16 (65.4 KB with the reduction's words, rows of one column two to a bank).
#include "hmsg_navroute_dev.h"

#include <climits>
#include <map>
#include <mutex>

#define NAVV_T 256
#define NAVV_RMAX 255                    // V5: sqrt of the largest r_max2
#define NAVV_SIDE (2 * NAVV_RMAX + 1)
#define NAVV_LD 17                       // LDS row stride of the bitmap in words (16 hold 512 bits; odd: see above)
#define NAVV_MAX_CELLS (1ll << 28)
#define NAVV_NONE HMSG_NAV_UNREACHED

template <int LD>
__device__ static inline unsigned navv_bit(const unsigned* __restrict__ s_b, int r, int c) { return (s_b[r * LD + (c >> 5)] >> (c & 31)) & 1u; }

// V1 between the window cells a and b, a the smaller (row, col) pair: is the sight clear?  The minor coordinate is m0 +
// floor((2 i dm + n) / (2 n)), kept as a quotient q and a remainder e in [0, 2 n).  blocks(r, c, w0, wn, m) says whether the cell
// stands in the way of a ray that is at (h0 * w0 + hn * wn) / m there (w0 + wn == m): V2 has no heights and ignores the weights,
// S2 compares its height with them.  The weights of a line cell i are (n - i, i, n), those of the two cells a diagonal step
// i - 1 -> i squeezes between (2 n - 2 i + 1, 2 i - 1, 2 n).
template <class F>
__device__ static inline bool navv_walk(int ar, int ac, int br, int bc, F blocks) {
    const int dr = br - ar, dc = bc - ac, adc = dc < 0 ? -dc : dc, n = dr > adc ? dr : adc;
    const bool by_row = dr >= adc;
    const int dm = by_row ? dc : dr, step = dc < 0 ? -1 : 1;
    int e = n, q = 0, pr = ar, pc = ac;
    for (int i = 1; i <= n; ++i) {
        e += 2 * dm;
        if (e >= 2 * n) e -= 2 * n, ++q;
        else if (e < 0) e += 2 * n, --q;
        const int r = by_row ? ar + i : ar + q, c = by_row ? ac + q : ac + step * i;
        if (r != pr && c != pc && blocks(pr, c, 2 * n - 2 * i + 1, 2 * i - 1, 2 * n) && blocks(r, pc, 2 * n - 2 * i + 1, 2 * i - 1, 2 * n))
            return false;                                                                          // a diagonal step between two blocking cells
        if (i < n && blocks(r, c, n - i, i, n)) return false;                                      // (the endpoints never block)
        pr = r, pc = c;
    }
    return true;
}

// (a, b, i) < (oa, ob, oi)
__device__ static inline bool navv_less(int a, int b, int i, int oa, int ob, int oi) {
    return a < oa || (a == oa && (b < ob || (b == ob && i < oi)));
}

// One workgroup per goal, for V3 (HEIGHTS false: blk is the blocking image) and for S3 (HEIGHTS true: top is the height map).
// R: floor(sqrt(r_max2)), the window's half side.  field may be nullptr (every cell's value is 0); view_d2, view_dist, n_visible
// and visible may be nullptr; goal_r2 may be nullptr (no footprint).
// S2 on two bitmaps: for one goal the ray's height lies in [lo, hi] = [min(eye, goal_h), max(eye, goal_h)] all the way, so a
// cell with T >= hi ("tall") blocks wherever the ray is and a cell with T < lo (not "not low") never does; only a cell between
// the two has its height read from the map, and the footprint applied to it again (T is not stored anywhere).
template <int LD, bool HEIGHTS>
__device__ __forceinline__ void navv_body(int rows, int cols, const unsigned char* __restrict__ blk, const unsigned short* __restrict__ top,
                                          const unsigned char* __restrict__ pass, const int* __restrict__ field, long long r_min2,
                                          long long r_max2, int R, int prefer, int eye, long long n, const int* __restrict__ goal_rc,
                                          const int* __restrict__ goal_h, const long long* __restrict__ goal_r2, int* __restrict__ view_rc,
                                          long long* __restrict__ view_d2, int* __restrict__ view_dist, int* __restrict__ n_visible,
                                          unsigned char* __restrict__ visible) {
    __shared__ unsigned s_b[(HEIGHTS ? 2 : 1) * NAVV_SIDE * LD];        // HEIGHTS: "tall", then "not low"
    __shared__ int s_ka[NAVV_T / 64], s_kb[NAVV_T / 64], s_ki[NAVV_T / 64], s_cnt[NAVV_T / 64];
    const unsigned* s_nl = s_b + (HEIGHTS ? NAVV_SIDE * LD : 0);
    const int HW = rows * cols, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (long long t = blockIdx.x; t < n; t += gridDim.x) {
        const int gr = goal_rc[t * 2], gc = goal_rc[t * 2 + 1];
        unsigned char* __restrict__ vis = visible ? visible + (size_t)t * HW : nullptr;
        const bool inside = gr >= 0 && gr < rows && gc >= 0 && gc < cols;               // (the same for the whole workgroup)
        int wr0 = 0, wc0 = 0, wh = 0, ww = 0;
        int ka = INT_MAX, kb = INT_MAX, ki = INT_MAX, cnt = 0;
        if (inside) {
            wr0 = max(gr - R, 0), wc0 = max(gc - R, 0);
            wh = min(gr + R, rows - 1) - wr0 + 1, ww = min(gc + R, cols - 1) - wc0 + 1;
            const int glr = gr - wr0, glc = gc - wc0;
            int gh = 0, lo = 0, hi = 0;
            long long fp2 = -1;
            if (HEIGHTS) {
                gh = min(max(goal_h[t], 0), 65535);
                lo = min(eye, gh), hi = max(eye, gh);
                if (goal_r2) fp2 = goal_r2[t];
            }
            // T of S2 for a window cell: 0 inside the goal's footprint, else the map's height
            auto T_of = [&](int lr, int lc) -> int {
                const int dr = lr - glr, dc = lc - glc;
                if ((long long)(dr * dr + dc * dc) <= fp2) return 0;
                return (int)top[(size_t)(wr0 + lr) * cols + wc0 + lc];
            };
            // the window's bytes as bits: a wave takes 64 columns of a row at a time (at most 8 such chunks a row)
            const int chunks = (ww + 63) >> 6;
            for (int k = wave; k < wh * chunks; k += NAVV_T / 64) {
                const int lr = k / chunks, ch = k - lr * chunks, lc = ch * 64 + lane;
                if (HEIGHTS) {
                    const int T = lc < ww ? T_of(lr, lc) : -1;
                    const unsigned long long m = __ballot(T >= hi), ml = __ballot(T >= lo);
                    if (lane < 2) s_b[lr * LD + ch * 2 + lane] = (unsigned)(m >> (32 * lane));
                    else if (lane < 4) s_b[NAVV_SIDE * LD + lr * LD + ch * 2 + lane - 2] = (unsigned)(ml >> (32 * (lane - 2)));
                } else {
                    const unsigned long long m = __ballot(lc < ww && blk[(size_t)(wr0 + lr) * cols + wc0 + lc] != 0);
                    if (lane < 2) s_b[lr * LD + ch * 2 + lane] = (unsigned)(m >> (32 * lane));
                }
            }
            __syncthreads();
            for (int i = tid; i < wh * ww; i += NAVV_T) {               // (ascending per thread)
                const int lr = i / ww, lc = i - lr * ww;
                const int gi = (wr0 + lr) * cols + wc0 + lc;
                const int dr = lr - glr, dc = lc - glc, d2 = dr * dr + dc * dc;          // at most 2 * 255^2
                bool ok = false;
                int fv = 0;
                if (d2 >= r_min2 && d2 <= r_max2 && pass[gi]) {
                    if (field) fv = field[gi];
                    if (fv != NAVV_NONE) {
                        // V1's line starts at the smaller (row, col) pair; S1: each end keeps its height
                        const bool goal_first = glr < lr || (glr == lr && glc < lc);
                        const int ar = goal_first ? glr : lr, ac = goal_first ? glc : lc, br = goal_first ? lr : glr, bc = goal_first ? lc : glc;
                        if (HEIGHTS) {
                            const int h0 = goal_first ? gh : eye, hn = goal_first ? eye : gh;
                            ok = navv_walk(ar, ac, br, bc, [&](int r, int c, int w0, int wn, int m) -> bool {
                                if (!navv_bit<LD>(s_nl, r, c)) return false;
                                if (navv_bit<LD>(s_b, r, c)) return true;
                                return T_of(r, c) * m >= h0 * w0 + hn * wn;              // (at most 65535 * 510)
                            });
                        } else {
                            ok = navv_walk(ar, ac, br, bc, [&](int r, int c, int, int, int) -> bool { return navv_bit<LD>(s_b, r, c) != 0; });
                        }
                    }
                }
                if (vis) vis[gi] = ok ? 1 : 0;
                if (!ok) continue;
                ++cnt;
                const int a = prefer ? d2 : fv, b = prefer ? fv : d2;
                if (navv_less(a, b, gi, ka, kb, ki)) ka = a, kb = b, ki = gi;
            }
        }
        if (vis) {
            for (int i = tid; i < HW; i += NAVV_T) {                    // every cell outside the window
                const int r = i / cols, c = i - r * cols;
                if (!(r >= wr0 && r < wr0 + wh && c >= wc0 && c < wc0 + ww)) vis[i] = 0;
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const int oa = __shfl_xor(ka, o), ob = __shfl_xor(kb, o), oi = __shfl_xor(ki, o);
            cnt += __shfl_xor(cnt, o);
            if (navv_less(oa, ob, oi, ka, kb, ki)) ka = oa, kb = ob, ki = oi;
        }
        if (lane == 0) s_ka[wave] = ka, s_kb[wave] = kb, s_ki[wave] = ki, s_cnt[wave] = cnt;
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < NAVV_T / 64; ++w) {
                cnt += s_cnt[w];
                if (navv_less(s_ka[w], s_kb[w], s_ki[w], ka, kb, ki)) ka = s_ka[w], kb = s_kb[w], ki = s_ki[w];
            }
            const bool none = ki == INT_MAX;
            view_rc[t * 2] = none ? -1 : ki / cols;
            view_rc[t * 2 + 1] = none ? -1 : ki % cols;
            if (view_d2) view_d2[t] = none ? -1 : (prefer ? ka : kb);
            if (view_dist) view_dist[t] = none ? NAVV_NONE : (prefer ? kb : ka);
            if (n_visible) n_visible[t] = cnt;
        }
        __syncthreads();                                                // (the bitmaps and the partial keys are the next goal's too)
    }
}

__global__ __launch_bounds__(NAVV_T) void k_navv_view(int rows, int cols, const unsigned char* __restrict__ blk, const unsigned char* __restrict__ pass,
                                                      const int* __restrict__ field, long long r_min2, long long r_max2, int R, int prefer, long long n,
                                                      const int* __restrict__ goal_rc, int* __restrict__ view_rc, long long* __restrict__ view_d2,
                                                      int* __restrict__ view_dist, int* __restrict__ n_visible, unsigned char* __restrict__ visible) {
    navv_body<NAVV_LD, false>(rows, cols, blk, nullptr, pass, field, r_min2, r_max2, R, prefer, 0, n, goal_rc, nullptr, nullptr, view_rc, view_d2,
                              view_dist, n_visible, visible);
}
// LD = NAVV_LD (17, two bitmaps of 34 748 B) where a workgroup may have that much LDS, else 16 (2 x 32 704 B, under 64 KB)
template <int LD>
__global__ __launch_bounds__(NAVV_T) void k_navv_view_h(int rows, int cols, const unsigned short* __restrict__ top,
                                                        const unsigned char* __restrict__ pass, const int* __restrict__ field, long long r_min2,
                                                        long long r_max2, int R, int prefer, int eye, long long n, const int* __restrict__ goal_rc,
                                                        const int* __restrict__ goal_h, const long long* __restrict__ goal_r2,
                                                        int* __restrict__ view_rc, long long* __restrict__ view_d2, int* __restrict__ view_dist,
                                                        int* __restrict__ n_visible, unsigned char* __restrict__ visible) {
    navv_body<LD, true>(rows, cols, nullptr, top, pass, field, r_min2, r_max2, R, prefer, eye, n, goal_rc, goal_h, goal_r2, view_rc, view_d2,
                        view_dist, n_visible, visible);
}

// ------------------------------------------------------------------------------------------ the calls
namespace {
void navv_check(int32_t rows, int32_t cols, const hmsg_view_params& p, const char* fn) {
    const std::string f = fn;
    HMSG_REQUIRE(rows >= 1 && cols >= 1, HMSG_ERR_INVALID, f + ": rows and cols must be at least 1");
    HMSG_REQUIRE(p.r_min2 >= 0, HMSG_ERR_INVALID, f + ": r_min2 < 0");
    HMSG_REQUIRE(p.r_max2 >= p.r_min2, HMSG_ERR_INVALID, f + ": r_max2 < r_min2");
    HMSG_REQUIRE(p.prefer == 0 || p.prefer == 1, HMSG_ERR_INVALID, f + ": prefer is neither 0 (least walk) nor 1 (closest look)");
    HMSG_REQUIRE(p.r_max2 <= (long long)NAVV_RMAX * NAVV_RMAX, HMSG_ERR_UNSUPPORTED, f + ": r_max2 above 255^2 (the window no longer fits LDS)");
    HMSG_REQUIRE((long long)rows * cols < NAVV_MAX_CELLS, HMSG_ERR_UNSUPPORTED, f + ": the image has 2^28 cells or more");
}

// all device memory; d_field, d_d2, d_dist, d_nvis and d_visible may be nullptr
void navv_view_dev(hipStream_t s, int rows, int cols, const unsigned char* d_blk, const unsigned char* d_pass, const int* d_field,
                   const hmsg_view_params& p, long long n, const int* d_goal, int* d_cell, long long* d_d2, int* d_dist, int* d_nvis,
                   unsigned char* d_visible) {
    if (n <= 0) return;
    int R = 0;
    while ((long long)(R + 1) * (R + 1) <= p.r_max2) ++R;               // floor(sqrt(r_max2)) <= 255
    hipLaunchKernelGGL(k_navv_view, dim3((unsigned)std::min<long long>(n, 1 << 20)), dim3(NAVV_T), 0, s, rows, cols, d_blk, d_pass, d_field,
                       (long long)p.r_min2, (long long)p.r_max2, R, (int)p.prefer, n, d_goal, d_cell, d_d2, d_dist, d_nvis, d_visible);
    HMSG_CHECK_LAUNCH();
}

// The LDS row stride of k_navv_view_h: 17 needs 2 x 34 748 B of bitmaps plus the reduction's 64 B, more than the 64 KB a
// workgroup has on older parts; the device's own limit decides, read once per device (never a launch that is tried).
constexpr size_t NAVV_H_LDS17 = 2ull * NAVV_SIDE * NAVV_LD * 4 + 4 * (NAVV_T / 64) * 4 + 64;       // (69 568 B as compiled, alignment included)
int g_navv_force_ld = 0;                      // hmsg_test_nav_sight_layout: 16 or 17, 0 = by the device
int navv_h_lds_limit() {
#ifdef HMSG_EMU_BUILD
    return 1 << 30;                           // (the simulator's LDS is host memory)
#else
    static std::mutex mu;
    static std::map<int, int> seen;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    auto it = seen.find(dev);
    if (it != seen.end()) return it->second;
    int v = 0;
    HIP_TRY(hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
    seen[dev] = v;
    return v;
#endif
}
int navv_h_ld() {
    const bool fits = (size_t)navv_h_lds_limit() >= NAVV_H_LDS17;
    if (g_navv_force_ld == 16 || (g_navv_force_ld == NAVV_LD && fits)) return g_navv_force_ld;
    return fits ? NAVV_LD : 16;
}

void navv_check_h(int eye, const char* fn) {
    HMSG_REQUIRE(eye >= 0 && eye <= 65535, HMSG_ERR_INVALID, std::string(fn) + ": eye outside [0, 65535]");
}
// goal_r2 (host or device, may be null) on the device, refused when an entry is below -1; own keeps the upload alive
const long long* navv_stage_r2(DevBuf<long long>& own, const int64_t* goal_r2, size_t n, hipStream_t s, const char* fn) {
    if (!goal_r2 || !n) return nullptr;
    std::vector<long long> h(n);
    read_in(h.data(), goal_r2, n * 8);
    for (size_t k = 0; k < n; ++k)
        HMSG_REQUIRE(h[k] >= -1, HMSG_ERR_INVALID, std::string(fn) + ": goal_r2[" + std::to_string(k) + "] < -1");
    return stage_in(own, (const long long*)goal_r2, n, s, Up::bounce);
}

// all device memory; d_field, d_r2, d_d2, d_dist, d_nvis and d_visible may be nullptr
void navv_view_h_dev(hipStream_t s, int rows, int cols, const unsigned short* d_top, const unsigned char* d_pass, const int* d_field,
                     const hmsg_view_params& p, int eye, long long n, const int* d_goal, const int* d_gh, const long long* d_r2, int* d_cell,
                     long long* d_d2, int* d_dist, int* d_nvis, unsigned char* d_visible) {
    if (n <= 0) return;
    int R = 0;
    while ((long long)(R + 1) * (R + 1) <= p.r_max2) ++R;               // floor(sqrt(r_max2)) <= 255
    const dim3 grid((unsigned)std::min<long long>(n, 1 << 20)), block(NAVV_T);
    if (navv_h_ld() == NAVV_LD)
        hipLaunchKernelGGL(k_navv_view_h<NAVV_LD>, grid, block, 0, s, rows, cols, d_top, d_pass, d_field, (long long)p.r_min2, (long long)p.r_max2, R,
                           (int)p.prefer, eye, n, d_goal, d_gh, d_r2, d_cell, d_d2, d_dist, d_nvis, d_visible);
    else
        hipLaunchKernelGGL(k_navv_view_h<16>, grid, block, 0, s, rows, cols, d_top, d_pass, d_field, (long long)p.r_min2, (long long)p.r_max2, R,
                           (int)p.prefer, eye, n, d_goal, d_gh, d_r2, d_cell, d_d2, d_dist, d_nvis, d_visible);
    HMSG_CHECK_LAUNCH();
}
}  // namespace

// test hook (include/hmsg_test.h): force_ld 16 or 17 forces k_navv_view_h's LDS row stride (17 only where it fits), 0 leaves it
// to the device; *ld_in_use and *lds_limit (either may be NULL) report what runs and the device's limit per workgroup
extern "C" int hmsg_test_nav_sight_layout(int32_t device_id, int32_t force_ld, int32_t* ld_in_use, int32_t* lds_limit) {
    if (force_ld != 0 && force_ld != 16 && force_ld != NAVV_LD) return HMSG_ERR_INVALID;
    return hmsg_boundary("hmsg_test_nav_sight_layout", device_id, [&] {
        g_navv_force_ld = force_ld;
        if (ld_in_use) *ld_in_use = navv_h_ld();
        if (lds_limit) *lds_limit = navv_h_lds_limit();
    });
}

extern "C" void hmsg_view_default_params(hmsg_view_params* p) {
    if (!p) return;
    p->r_min2 = 0;
    p->r_max2 = 100 * 100;
    p->prefer = 0;
    p->reserved_ = 0;
}

extern "C" int hmsg_nav_viewpoints(int32_t device_id, int32_t rows, int32_t cols, const uint8_t* blocking, const uint8_t* passable,
                                   const int32_t* field, const hmsg_view_params* prm, int64_t n_goals, const int32_t* goal_rc, int32_t* view_rc,
                                   int64_t* view_d2, int32_t* view_dist, int32_t* n_visible, uint8_t* visible) {
    if (!blocking || !passable || !prm || (n_goals > 0 && (!goal_rc || !view_rc))) return HMSG_ERR_INVALID;
    return hmsg_boundary("hmsg_nav_viewpoints", device_id, [&] {
        navv_check(rows, cols, *prm, "hmsg_nav_viewpoints");
        HMSG_REQUIRE(n_goals >= 0, HMSG_ERR_INVALID, "hmsg_nav_viewpoints: n_goals < 0");
        if (n_goals == 0) return;
        ScopedStream s(hipStreamNonBlocking);
        const size_t HW = (size_t)rows * cols, n = (size_t)n_goals;
        DevBuf<unsigned char> own_blk, own_pass, own_vis;
        DevBuf<int> own_field, own_goal, own_cell, own_dist, own_nvis;
        DevBuf<long long> own_d2;
        const unsigned char* d_blk = stage_in(own_blk, blocking, HW, s, Up::bounce);
        const unsigned char* d_pass = stage_in(own_pass, passable, HW, s, Up::bounce);
        const int* d_field = field ? stage_in(own_field, field, HW, s, Up::bounce) : nullptr;
        const int* d_goal = stage_in(own_goal, goal_rc, n * 2, s, Up::bounce);
        int* d_cell = stage_out(own_cell, view_rc, n * 2);
        long long* d_d2 = stage_out(own_d2, (long long*)view_d2, n);
        int* d_dist = stage_out(own_dist, view_dist, n);
        int* d_nvis = stage_out(own_nvis, n_visible, n);
        unsigned char* d_vis = stage_out(own_vis, visible, n * HW);
        navv_view_dev(s, rows, cols, d_blk, d_pass, d_field, *prm, n_goals, d_goal, d_cell, d_d2, d_dist, d_nvis, d_vis);
        unstage_out(view_rc, d_cell, n * 2, s);
        if (view_d2) unstage_out((long long*)view_d2, (const long long*)d_d2, n, s);
        if (view_dist) unstage_out(view_dist, d_dist, n, s);
        if (n_visible) unstage_out(n_visible, d_nvis, n, s);
        if (visible) unstage_out(visible, d_vis, n * HW, s);
        HIP_TRY(hipStreamSynchronize(s));
    });
}

// hmsg_nav_route with its goal snap (R4) replaced by V4 on the start's field, and only that
extern "C" int hmsg_nav_view_route(int32_t device_id, int32_t rows, int32_t cols, const uint8_t* main_free_map, const uint8_t* blocking,
                                   const hmsg_route_params* route_prm, const hmsg_view_params* view_prm, const int32_t* start_rc, int64_t n_goals,
                                   const int32_t* goal_rc, hmsg_nav_routes* out, int32_t* n_visible) {
    if (!main_free_map || !blocking || !route_prm || !view_prm || !start_rc || !out || (n_goals > 0 && !goal_rc)) return HMSG_ERR_INVALID;
    return hmsg_boundary("hmsg_nav_view_route", device_id, [&] {
        navv_check(rows, cols, *view_prm, "hmsg_nav_view_route");
        DevBuf<unsigned char> own_blk;
        DevBuf<int> own_nvis;
        navr_route_run("hmsg_nav_view_route", rows, cols, main_free_map, route_prm, start_rc, n_goals, goal_rc, out,
                       [&](hipStream_t s, const unsigned char* d_pass, const int* d_field, const int* d_goal, int* d_cell, long long* d_d2) {
                           if (n_goals <= 0) return;
                           const size_t HW = (size_t)rows * cols, n = (size_t)n_goals;
                           const unsigned char* d_blk = stage_in(own_blk, blocking, HW, s, Up::bounce);
                           int* d_nvis = stage_out(own_nvis, n_visible, n);
                           navv_view_dev(s, rows, cols, d_blk, d_pass, d_field, *view_prm, n_goals, d_goal, d_cell, d_d2, nullptr, d_nvis, nullptr);
                           if (n_visible) unstage_out(n_visible, d_nvis, n, s);
                       });
    });
}

// ------------------------------------------------------------------------------------------ N10: sight with heights (S1 to S5)
extern "C" int hmsg_nav_viewpoints_h(int32_t device_id, int32_t rows, int32_t cols, const uint16_t* top, const uint8_t* passable,
                                     const int32_t* field, const hmsg_view_params* prm, int32_t eye, int64_t n_goals, const int32_t* goal_rc,
                                     const int32_t* goal_h, const int64_t* goal_r2, int32_t* view_rc, int64_t* view_d2, int32_t* view_dist,
                                     int32_t* n_visible, uint8_t* visible) {
    if (!top || !passable || !prm || (n_goals > 0 && (!goal_rc || !goal_h || !view_rc))) return HMSG_ERR_INVALID;
    return hmsg_boundary("hmsg_nav_viewpoints_h", device_id, [&] {
        navv_check(rows, cols, *prm, "hmsg_nav_viewpoints_h");
        navv_check_h(eye, "hmsg_nav_viewpoints_h");
        HMSG_REQUIRE(n_goals >= 0, HMSG_ERR_INVALID, "hmsg_nav_viewpoints_h: n_goals < 0");
        if (n_goals == 0) return;
        ScopedStream s(hipStreamNonBlocking);
        const size_t HW = (size_t)rows * cols, n = (size_t)n_goals;
        DevBuf<unsigned short> own_top;
        DevBuf<unsigned char> own_pass, own_vis;
        DevBuf<int> own_field, own_goal, own_gh, own_cell, own_dist, own_nvis;
        DevBuf<long long> own_d2, own_r2;
        const long long* d_r2 = navv_stage_r2(own_r2, goal_r2, n, s, "hmsg_nav_viewpoints_h");
        const unsigned short* d_top = stage_in(own_top, (const unsigned short*)top, HW, s, Up::bounce);
        const unsigned char* d_pass = stage_in(own_pass, passable, HW, s, Up::bounce);
        const int* d_field = field ? stage_in(own_field, field, HW, s, Up::bounce) : nullptr;
        const int* d_goal = stage_in(own_goal, goal_rc, n * 2, s, Up::bounce);
        const int* d_gh = stage_in(own_gh, goal_h, n, s, Up::bounce);
        int* d_cell = stage_out(own_cell, view_rc, n * 2);
        long long* d_d2 = stage_out(own_d2, (long long*)view_d2, n);
        int* d_dist = stage_out(own_dist, view_dist, n);
        int* d_nvis = stage_out(own_nvis, n_visible, n);
        unsigned char* d_vis = stage_out(own_vis, visible, n * HW);
        navv_view_h_dev(s, rows, cols, d_top, d_pass, d_field, *prm, eye, n_goals, d_goal, d_gh, d_r2, d_cell, d_d2, d_dist, d_nvis, d_vis);
        unstage_out(view_rc, d_cell, n * 2, s);
        if (view_d2) unstage_out((long long*)view_d2, (const long long*)d_d2, n, s);
        if (view_dist) unstage_out(view_dist, d_dist, n, s);
        if (n_visible) unstage_out(n_visible, d_nvis, n, s);
        if (visible) unstage_out(visible, d_vis, n * HW, s);
        HIP_TRY(hipStreamSynchronize(s));
    });
}

// hmsg_nav_view_route with S3 in V3's place, and only that: the same navr_route_run
extern "C" int hmsg_nav_view_route_h(int32_t device_id, int32_t rows, int32_t cols, const uint8_t* main_free_map, const uint16_t* top,
                                     const hmsg_route_params* route_prm, const hmsg_view_params* view_prm, int32_t eye, const int32_t* start_rc,
                                     int64_t n_goals, const int32_t* goal_rc, const int32_t* goal_h, const int64_t* goal_r2, hmsg_nav_routes* out,
                                     int32_t* n_visible) {
    if (!main_free_map || !top || !route_prm || !view_prm || !start_rc || !out || (n_goals > 0 && (!goal_rc || !goal_h))) return HMSG_ERR_INVALID;
    return hmsg_boundary("hmsg_nav_view_route_h", device_id, [&] {
        navv_check(rows, cols, *view_prm, "hmsg_nav_view_route_h");
        navv_check_h(eye, "hmsg_nav_view_route_h");
        DevBuf<unsigned short> own_top;
        DevBuf<int> own_nvis, own_gh;
        DevBuf<long long> own_r2;
        navr_route_run("hmsg_nav_view_route_h", rows, cols, main_free_map, route_prm, start_rc, n_goals, goal_rc, out,
                       [&](hipStream_t s, const unsigned char* d_pass, const int* d_field, const int* d_goal, int* d_cell, long long* d_d2) {
                           if (n_goals <= 0) return;
                           const size_t HW = (size_t)rows * cols, n = (size_t)n_goals;
                           const long long* d_r2 = navv_stage_r2(own_r2, goal_r2, n, s, "hmsg_nav_view_route_h");
                           const unsigned short* d_top = stage_in(own_top, (const unsigned short*)top, HW, s, Up::bounce);
                           const int* d_gh = stage_in(own_gh, goal_h, n, s, Up::bounce);
                           int* d_nvis = stage_out(own_nvis, n_visible, n);
                           navv_view_h_dev(s, rows, cols, d_top, d_pass, d_field, *view_prm, eye, n_goals, d_goal, d_gh, d_r2, d_cell, d_d2, nullptr, d_nvis,
                                           nullptr);
                           if (n_visible) unstage_out(n_visible, d_nvis, n, s);
                       });
    });
}
