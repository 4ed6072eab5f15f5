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
#include "hmsg_navroute_dev.h"

#include <climits>

#define NAVV_T 256
#define NAVV_RMAX 255                    // V5: sqrt of the largest r_max2
#define NAVV_SIDE (2 * NAVV_RMAX + 1)
#define NAVV_LD 17                       // LDS row stride of the bitmap in words (16 hold 512 bits; odd: see above)
#define NAVV_MAX_CELLS (1ll << 28)
#define NAVV_NONE HMSG_NAV_UNREACHED

__device__ static inline unsigned navv_bit(const unsigned* __restrict__ s_b, int r, int c) { return (s_b[r * NAVV_LD + (c >> 5)] >> (c & 31)) & 1u; }

// V2 on the window's bitmap: is the sight between the window cells a and b clear?  V1's line starts at the smaller (row, col)
// pair; the minor coordinate is m0 + floor((2 i dm + n) / (2 n)), kept as a quotient q and a remainder e in [0, 2 n).
__device__ static bool navv_clear(const unsigned* __restrict__ s_b, int ar, int ac, int br, int bc) {
    if (br < ar || (br == ar && bc < ac)) {
        const int tr = ar, tc = ac;
        ar = br, ac = bc, br = tr, bc = tc;
    }
    const int dr = br - ar, dc = bc - ac, adc = dc < 0 ? -dc : dc, n = dr > adc ? dr : adc;
    const bool by_row = dr >= adc;
    const int dm = by_row ? dc : dr, step = dc < 0 ? -1 : 1;
    int e = n, q = 0, pr = ar, pc = ac;
    for (int i = 1; i <= n; ++i) {
        e += 2 * dm;
        if (e >= 2 * n) e -= 2 * n, ++q;
        else if (e < 0) e += 2 * n, --q;
        const int r = by_row ? ar + i : ar + q, c = by_row ? ac + q : ac + step * i;
        if (r != pr && c != pc && navv_bit(s_b, pr, c) && navv_bit(s_b, r, pc)) return false;     // a diagonal step between two blocking cells
        if (i < n && navv_bit(s_b, r, c)) return false;                                            // (the endpoints never block)
        pr = r, pc = c;
    }
    return true;
}

// (a, b, i) < (oa, ob, oi)
__device__ static inline bool navv_less(int a, int b, int i, int oa, int ob, int oi) {
    return a < oa || (a == oa && (b < ob || (b == ob && i < oi)));
}

// R: floor(sqrt(r_max2)), the window's half side.  field may be nullptr (every cell's value is 0); view_d2, view_dist, n_visible
// and visible may be nullptr.
__global__ __launch_bounds__(NAVV_T) void k_navv_view(int rows, int cols, const unsigned char* __restrict__ blk, const unsigned char* __restrict__ pass,
                                                      const int* __restrict__ field, long long r_min2, long long r_max2, int R, int prefer, long long n,
                                                      const int* __restrict__ goal_rc, int* __restrict__ view_rc, long long* __restrict__ view_d2,
                                                      int* __restrict__ view_dist, int* __restrict__ n_visible, unsigned char* __restrict__ visible) {
    __shared__ unsigned s_b[NAVV_SIDE * NAVV_LD];
    __shared__ int s_ka[NAVV_T / 64], s_kb[NAVV_T / 64], s_ki[NAVV_T / 64], s_cnt[NAVV_T / 64];
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
            // the window's blocking bytes as bits: a wave takes 64 columns of a row at a time (at most 8 such chunks a row)
            const int chunks = (ww + 63) >> 6;
            for (int k = wave; k < wh * chunks; k += NAVV_T / 64) {
                const int lr = k / chunks, ch = k - lr * chunks, lc = ch * 64 + lane;
                const unsigned long long m = __ballot(lc < ww && blk[(size_t)(wr0 + lr) * cols + wc0 + lc] != 0);
                if (lane < 2) s_b[lr * NAVV_LD + ch * 2 + lane] = (unsigned)(m >> (32 * lane));
            }
            __syncthreads();
            const int glr = gr - wr0, glc = gc - wc0;
            for (int i = tid; i < wh * ww; i += NAVV_T) {               // (ascending per thread)
                const int lr = i / ww, lc = i - lr * ww;
                const int gi = (wr0 + lr) * cols + wc0 + lc;
                const int dr = lr - glr, dc = lc - glc, d2 = dr * dr + dc * dc;          // at most 2 * 255^2
                bool ok = false;
                int fv = 0;
                if (d2 >= r_min2 && d2 <= r_max2 && pass[gi]) {
                    if (field) fv = field[gi];
                    ok = fv != NAVV_NONE && navv_clear(s_b, lr, lc, glr, glc);
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
        __syncthreads();                                                // (the bitmap and the partial keys are the next goal's too)
    }
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
}  // namespace

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
