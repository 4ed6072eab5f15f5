// Routes on a floor's free map (include/hmsg.h, N7: hmsg_nav_clearance, hmsg_nav_distance_fields, hmsg_nav_snap_cells,
// hmsg_nav_paths, hmsg_nav_route): exact integer distance fields of the 8-neighbour grid graph, the clearance of a mask, the
// nearest candidate cell of a target and the cells of the way, all on the device beside the maps of hmsg_navmap.hip.  The reference
// has no such stage (navigation_graph.py:23,36 imports skfmm, defines compute_sdf and never calls it): the rules R1 to R5 are
// this library's own and stand in the header.  Every output is integer work with one right answer.
//
// MI355X design notes
//  * Field (k_navr_relax): the image is cut into 64 x 64 tiles.  A workgroup of 256 threads holds one tile plus a one-cell halo
//    in LDS (66 x 66 int32 at a row stride of 67 words and the passable bytes: 22 KB, seven workgroups a CU) and relaxes it by
//    R1 until nothing in it changes.  A thread owns 16 consecutive cells of a row and sweeps them left to right, then right to
//    left, so a value travels 16 cells along a row per sweep; with the odd stride the 64 lanes of a wave (16 rows x 4 segments)
//    hit 64 different banks at every step of the sweep.  A tile that changed writes its interior back and stamps its eight
//    neighbours "active in the next round"; a launch is one round over all tiles of all fields (the third grid dimension), and a
//    tile that is not stamped leaves after one load.  int32 minimum is monotone and idempotent: a tile that reads a neighbour's
//    cell while the neighbour is writing it sees the old or the new value, both upper bounds, and is stamped for the next round
//    by that neighbour; the fixed point is the answer whatever the order.  No float anywhere, no atomics on the field.
//  * There is no cap on rounds.  The host enqueues a batch of rounds (4, 8, 16, then 32 at a time), each with a counter of its
//    own, and reads the counters back once per batch: the loop ends when the last round of a batch changed no tile.  Rounds
//    after the fixed point cost one load of a stamp per tile.
//  * Clearance is the same kernel with every cell of the image passable and the corner rule off, started from 0 outside the
//    mask and from R3's closed form for "outside the image" inside it.
//  * Snap (k_navr_snap): a workgroup per target scans all cells; a thread keeps the least (d2, index) pair of its cells, the
//    pairs meet by wave shuffles and through LDS.  d2 can reach 2^57 (target indices clamped to +-2^20, an image side below
//    2^28), so (d2, index) does not fit one 64-bit word and is compared as a pair.
//  * Paths (k_navr_walk): a lane per goal, two passes over the same walk: count, one wave's ordered scan of the counts, write
//    from the back.  The walk is a dependent chain of global loads; it stays here because the field does.
#include "hmsg_navroute_dev.h"

#include <climits>

#define NAVR_MAX_CELLS (1ll << 28)
#define NAVR_CLAMP (1ll << 20)
#define NAVR_NONE HMSG_NAV_UNREACHED

// R1's order: N, S, W, E, NW, NE, SW, SE
__device__ static const int NAVR_DR[8] = {-1, 1, 0, 0, -1, -1, 1, 1};
__device__ static const int NAVR_DC[8] = {0, 0, -1, 1, -1, 1, -1, 1};

// ------------------------------------------------------------------------------------------ fields
__global__ __launch_bounds__(NAVR_T) void k_navr_fill(int* __restrict__ p, long long n, int v) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}
// grid (sources, fields): a source on a passable cell of the image is 0 and stamps its tile and the eight round it for round 1
// (the neighbours too: a tile stamps them only when it CHANGES, and a tile whose only news is its source does not)
__global__ __launch_bounds__(NAVR_T) void k_navr_sources(int rows, int cols, const unsigned char* __restrict__ pass, const long long* __restrict__ src_off,
                                                         const int* __restrict__ src_rc, int* __restrict__ field, int* __restrict__ act, int ntx,
                                                         int nty) {
    const int f = blockIdx.y;
    const long long k = src_off[f] + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= src_off[f + 1]) return;
    const int r = src_rc[k * 2], c = src_rc[k * 2 + 1];
    if (r < 0 || r >= rows || c < 0 || c >= cols) return;
    const size_t i = (size_t)r * cols + c;
    if (!pass[i]) return;
    field[(size_t)f * rows * cols + i] = 0;
    const int ty = r / NAVR_TILE, tx = c / NAVR_TILE;
    for (int y = max(ty - 1, 0); y <= min(ty + 1, nty - 1); ++y)
        for (int x = max(tx - 1, 0); x <= min(tx + 1, ntx - 1); ++x) act[((size_t)f * nty + y) * ntx + x] = 1;
}
// R3's start: 0 outside the mask, the straight walk to the nearest cell outside the image inside it
__global__ __launch_bounds__(NAVR_T) void k_navr_clear_init(int rows, int cols, const unsigned char* __restrict__ mask, int w_straight,
                                                            int* __restrict__ clr) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * cols) return;
    const int r = i / cols, c = i - r * cols;
    clr[i] = mask[i] ? w_straight * (1 + min(min(r, rows - 1 - r), min(c, cols - 1 - c))) : 0;
}

// One round: grid (tile columns, tile rows, fields).  pass == nullptr: every cell of the image is passable.  CORNER: R1's rule for
// diagonal moves.  A tile runs when its stamp is this round's (or already the next one's); changed counts the tiles that changed.
template <bool CORNER>
__global__ __launch_bounds__(NAVR_T) void k_navr_relax(int rows, int cols, const unsigned char* __restrict__ pass, int w_straight, int w_diag,
                                                       int* __restrict__ field, int* __restrict__ act, int round, unsigned* __restrict__ changed) {
    __shared__ int s_f[NAVR_SIDE * NAVR_LD];
    __shared__ unsigned char s_p[NAVR_SIDE * NAVR_PLD];
    __shared__ int s_chg[3];
    __shared__ int s_run;
    const int tid = threadIdx.x, ntx = gridDim.x, nty = gridDim.y, ntiles = ntx * nty;
    const int tx = blockIdx.x, ty = blockIdx.y;
    int* __restrict__ fld = field + (size_t)blockIdx.z * rows * cols;
    int* __restrict__ a = act + (size_t)blockIdx.z * ntiles;
    if (tid == 0) s_run = a[ty * ntx + tx] >= round ? 1 : 0, s_chg[0] = 0;
    __syncthreads();
    if (!s_run) return;
    const int r0 = ty * NAVR_TILE - 1, c0 = tx * NAVR_TILE - 1;
    for (int i = tid; i < NAVR_SIDE * NAVR_SIDE; i += NAVR_T) {
        const int lr = i / NAVR_SIDE, lc = i - lr * NAVR_SIDE, r = r0 + lr, c = c0 + lc;
        const bool in = r >= 0 && r < rows && c >= 0 && c < cols;
        const bool p = in && (pass ? pass[(size_t)r * cols + c] != 0 : true);
        s_p[lr * NAVR_PLD + lc] = p ? 1 : 0;
        s_f[lr * NAVR_LD + lc] = p ? fld[(size_t)r * cols + c] : NAVR_NONE;
    }
    __syncthreads();
    // a thread's 16 cells: local row 1 + tid / 4, local columns 1 + 16 * (tid % 4) ...
    const int lr = 1 + (tid >> 2), lc0 = 1 + ((tid & 3) << 4);
    bool any = false;
    for (int it = 0;; ++it) {
        if (tid == 0) s_chg[(it + 1) % 3] = 0;          // (read last in iteration it - 2, written next in it + 1: one barrier each between)
        bool chg = false;
        for (int k = 0; k < 32; ++k) {
            const int lc = lc0 + (k < 16 ? k : 31 - k);
            if (!s_p[lr * NAVR_PLD + lc]) continue;
            const int cur = s_f[lr * NAVR_LD + lc];
            int best = cur;
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                const int dr = d < 4 ? (d == 0 ? -1 : (d == 1 ? 1 : 0)) : (d < 6 ? -1 : 1);
                const int dc = d < 4 ? (d == 2 ? -1 : (d == 3 ? 1 : 0)) : ((d & 1) ? 1 : -1);
                if (CORNER && d >= 4 && !(s_p[(lr + dr) * NAVR_PLD + lc] && s_p[lr * NAVR_PLD + lc + dc])) continue;
                const int v = s_f[(lr + dr) * NAVR_LD + lc + dc];
                const int w = d < 4 ? w_straight : w_diag;
                if (v != NAVR_NONE && v + w < best) best = v + w;
            }
            if (best < cur) s_f[lr * NAVR_LD + lc] = best, chg = true;
        }
        if (chg) s_chg[it % 3] = 1;
        __syncthreads();
        if (!s_chg[it % 3]) break;
        any = true;
    }
    if (!any) return;
    for (int k = 0; k < 16; ++k) {
        const int lc = lc0 + k, r = r0 + lr, c = c0 + lc;
        if (s_p[lr * NAVR_PLD + lc]) fld[(size_t)r * cols + c] = s_f[lr * NAVR_LD + lc];     // (s_p: inside the image)
    }
    if (tid < 8) {
        const int ny = ty + NAVR_DR[tid], nx = tx + NAVR_DC[tid];
        if (ny >= 0 && ny < nty && nx >= 0 && nx < ntx) a[ny * ntx + nx] = round + 1;
    } else if (tid == 8) {
        atomicAdd(changed, 1u);
    }
}
// grid (cells, fields): n_reached[f] += finite cells
__global__ __launch_bounds__(NAVR_T) void k_navr_count(const int* __restrict__ field, int HW, unsigned long long* __restrict__ n_reached) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long b = __ballot(i < HW && field[(size_t)blockIdx.y * HW + i] != NAVR_NONE);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&n_reached[blockIdx.y], (unsigned long long)__popcll(b));
}
// passable = mask where clearance >= min_clearance
__global__ __launch_bounds__(NAVR_T) void k_navr_threshold(const unsigned char* __restrict__ mask, const int* __restrict__ clr, int min_clearance, int HW,
                                                           unsigned char* __restrict__ pass) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < HW) pass[i] = (mask[i] && clr[i] >= min_clearance) ? 1 : 0;
}
__global__ __launch_bounds__(NAVR_T) void k_navr_binary(const unsigned char* __restrict__ mask, int HW, unsigned char* __restrict__ pass) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < HW) pass[i] = mask[i] ? 1 : 0;
}
// dist[k] = field at cell k, unreached for the cell (-1, -1)
__global__ __launch_bounds__(NAVR_T) void k_navr_gather(const int* __restrict__ field, int cols, long long n, const int* __restrict__ cell_rc,
                                                        int* __restrict__ dist) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int r = cell_rc[k * 2], c = cell_rc[k * 2 + 1];
    dist[k] = r < 0 ? NAVR_NONE : field[(size_t)r * cols + c];
}

// ------------------------------------------------------------------------------------------ snap (R4)
__global__ __launch_bounds__(NAVR_T) void k_navr_snap(int rows, int cols, const unsigned char* __restrict__ pass, const int* __restrict__ field,
                                                      long long n, const int* __restrict__ target_rc, int* __restrict__ snapped_rc,
                                                      long long* __restrict__ d2_out) {
    __shared__ long long s_d[NAVR_T / 64];
    __shared__ int s_i[NAVR_T / 64];
    const int HW = rows * cols, tid = threadIdx.x;
    for (long long t = blockIdx.x; t < n; t += gridDim.x) {
        const long long tr = min(max((long long)target_rc[t * 2], -NAVR_CLAMP), NAVR_CLAMP);
        const long long tc = min(max((long long)target_rc[t * 2 + 1], -NAVR_CLAMP), NAVR_CLAMP);
        long long bd = LLONG_MAX;
        int bi = INT_MAX;
        for (int i = tid; i < HW; i += NAVR_T) {               // (ascending per thread: a strict < keeps the smaller index)
            if (!pass[i] || (field && field[i] == NAVR_NONE)) continue;
            const int r = i / cols, c = i - r * cols;
            const long long dr = r - tr, dc = c - tc, d = dr * dr + dc * dc;
            if (d < bd) bd = d, bi = i;
        }
        for (int o = 32; o > 0; o >>= 1) {
            const long long od = __shfl_xor(bd, o);
            const int oi = __shfl_xor(bi, o);
            if (od < bd || (od == bd && oi < bi)) bd = od, bi = oi;
        }
        if ((tid & 63) == 0) s_d[tid >> 6] = bd, s_i[tid >> 6] = bi;
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < NAVR_T / 64; ++w)
                if (s_d[w] < bd || (s_d[w] == bd && s_i[w] < bi)) bd = s_d[w], bi = s_i[w];
            const bool none = bi == INT_MAX;
            snapped_rc[t * 2] = none ? -1 : bi / cols;
            snapped_rc[t * 2 + 1] = none ? -1 : bi % cols;
            if (d2_out) d2_out[t] = none ? -1 : bd;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------ paths (R5)
// WRITE false: cnt[g] = cells of goal g's path (0: no path).  WRITE true: the cells, from the back, at off[g] .. off[g + 1].
// Every step lowers the value by at least 1, so no cell comes twice and the walk ends whatever the field holds; a walk that finds
// no neighbour to step to (a field that is no fixed point of R2) has no path.
template <bool WRITE>
__global__ __launch_bounds__(NAVR_T) void k_navr_walk(int rows, int cols, const unsigned char* __restrict__ pass, const int* __restrict__ field,
                                                      int w_straight, int w_diag, long long n, const int* __restrict__ goal_rc,
                                                      long long* __restrict__ cnt, const long long* __restrict__ off, int* __restrict__ path_rc) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    int r = goal_rc[g * 2], c = goal_rc[g * 2 + 1];
    long long count = 0, at = 0, first = 0;
    if (WRITE) {
        first = off[g], at = off[g + 1];
        if (at == first) return;
    }
    if (r >= 0 && r < rows && c >= 0 && c < cols && pass[(size_t)r * cols + c] && field[(size_t)r * cols + c] != NAVR_NONE) {
        long long v = field[(size_t)r * cols + c];
        count = 1;
        if (WRITE) --at, path_rc[at * 2] = r, path_rc[at * 2 + 1] = c;
        while (v != 0) {
            int d = 0;
            for (; d < 8; ++d) {
                const int nr = r + NAVR_DR[d], nc = c + NAVR_DC[d];
                if (nr < 0 || nr >= rows || nc < 0 || nc >= cols || !pass[(size_t)nr * cols + nc]) continue;
                if (d >= 4 && !(pass[(size_t)nr * cols + c] && pass[(size_t)r * cols + nc])) continue;
                const int fv = field[(size_t)nr * cols + nc];
                if (fv == NAVR_NONE || (long long)fv + (d < 4 ? w_straight : w_diag) != v) continue;
                r = nr, c = nc, v = fv;
                break;
            }
            if (d == 8 || (WRITE && at == first)) {
                count = 0;
                break;
            }
            ++count;
            if (WRITE) --at, path_rc[at * 2] = r, path_rc[at * 2 + 1] = c;
        }
    }
    if (!WRITE) cnt[g] = count;
}
// one wave: off = exclusive scan of cnt [n], off[n] = the sum
__global__ __launch_bounds__(64) void k_navr_scan(long long n, const long long* __restrict__ cnt, long long* __restrict__ off) {
    const int lane = threadIdx.x;
    long long carry = 0;
    for (long long w0 = 0; w0 < n; w0 += 64) {
        const long long w = w0 + lane;
        const long long v = w < n ? cnt[w] : 0;
        long long incl = v;
        for (int d = 1; d < 64; d <<= 1) {
            const long long up = __shfl_up(incl, (unsigned)d);
            if (lane >= d) incl += up;
        }
        if (w < n) off[w] = carry + incl - v;
        carry += __shfl(incl, 63);
    }
    if (lane == 0) off[n] = carry;
}

// ------------------------------------------------------------------------------------------ the calls
namespace {
thread_local int g_navr_rounds = 0, g_navr_trips = 0;       // what hmsg_test_nav_route_last reports
}  // namespace

void navr_last_reset() { g_navr_rounds = g_navr_trips = 0; }
void navr_last_get(int* rounds, int* trips) { *rounds = g_navr_rounds, *trips = g_navr_trips; }
void navr_check(int32_t rows, int32_t cols, const hmsg_route_params& p, const char* fn) {
    const std::string f = fn;
    HMSG_REQUIRE(rows >= 1 && cols >= 1, HMSG_ERR_INVALID, f + ": rows and cols must be at least 1");
    HMSG_REQUIRE(p.w_straight >= 1 && p.w_diag >= p.w_straight, HMSG_ERR_INVALID, f + ": 1 <= w_straight <= w_diag");
    HMSG_REQUIRE(p.min_clearance >= 0, HMSG_ERR_INVALID, f + ": min_clearance < 0");
    const long long HW = (long long)rows * cols;
    HMSG_REQUIRE(HW < NAVR_MAX_CELLS, HMSG_ERR_UNSUPPORTED, f + ": the image has 2^28 cells or more");
    HMSG_REQUIRE(HW * p.w_diag < (1ll << 31), HMSG_ERR_UNSUPPORTED, f + ": rows * cols * w_diag reaches 2^31");
}
namespace {
void navr_check_shape(int32_t rows, int32_t cols, const char* fn) {
    hmsg_route_params p;
    hmsg_route_default_params(&p);
    p.w_straight = p.w_diag = 1;
    navr_check(rows, cols, p, fn);
}

}  // namespace
// one round over all tiles of nf fields (hmsg_navroute_dev.h)
void navr_relax_round(hipStream_t s, int rows, int cols, const unsigned char* d_pass, const hmsg_route_params& p, bool corner, int nf, int* d_field,
                      int* d_act, int round, unsigned* d_changed) {
    const dim3 grid(cdiv((size_t)cols, NAVR_TILE), cdiv((size_t)rows, NAVR_TILE), (unsigned)nf);
    if (corner)
        hipLaunchKernelGGL(k_navr_relax<true>, grid, dim3(NAVR_T), 0, s, rows, cols, d_pass, p.w_straight, p.w_diag, d_field, d_act, round, d_changed);
    else
        hipLaunchKernelGGL(k_navr_relax<false>, grid, dim3(NAVR_T), 0, s, rows, cols, d_pass, p.w_straight, p.w_diag, d_field, d_act, round, d_changed);
}
// rounds in growing batches until the last round of a batch changed nothing (hmsg_navroute_dev.h)
void navr_rounds(hipStream_t s, const navr_round_fn& enqueue) {
    constexpr int MAXB = 32;
    DevBuf<unsigned> chg;
    chg.alloc(MAXB);
    unsigned h[MAXB];
    int round = 1, batch = 4;
    for (;;) {
        HIP_TRY(hipMemsetAsync(chg.p, 0, sizeof(unsigned) * (size_t)batch, s));
        for (int b = 0; b < batch; ++b) enqueue(round + b, chg.p + b);
        HMSG_CHECK_LAUNCH();
        HIP_TRY(hipMemcpyAsync(h, chg.p, sizeof(unsigned) * (size_t)batch, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        ++g_navr_trips;
        for (int b = 0; b < batch && h[b]; ++b) ++g_navr_rounds;
        if (!h[batch - 1]) return;
        round += batch;
        batch = std::min(batch * 2, MAXB);
    }
}
// rounds until no tile is stamped; act: i32 [nf][tiles], stamped 1 where a tile starts
void navr_relax(hipStream_t s, int rows, int cols, const unsigned char* d_pass, const hmsg_route_params& p, bool corner, int nf, int* d_field,
                int* d_act) {
    navr_rounds(s, [&](int round, unsigned* d_changed) { navr_relax_round(s, rows, cols, d_pass, p, corner, nf, d_field, d_act, round, d_changed); });
}

void navr_fill_dev(hipStream_t s, int* d_p, long long n, int v) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_navr_fill, dim3(cdiv((size_t)n, NAVR_T)), dim3(NAVR_T), 0, s, d_p, n, v);
}
void navr_scan_dev(hipStream_t s, long long n, const long long* d_cnt, long long* d_off) {
    hipLaunchKernelGGL(k_navr_scan, dim3(1), dim3(64), 0, s, n, d_cnt, d_off);
}
// d_fields i32 [nf][rows][cols] from the sources src_rc[src_off[f] .. src_off[f + 1]) (device memory, cells outside the image skipped)
void navr_fields_dev(hipStream_t s, int rows, int cols, const unsigned char* d_pass, const hmsg_route_params& p, long long nf_all,
                     const long long* d_src_off, const int* d_src_rc, long long max_sources, int* d_fields, unsigned long long* d_n_reached) {
    const int HW = rows * cols, ntx = (int)cdiv((size_t)cols, NAVR_TILE), ntiles = ntx * (int)cdiv((size_t)rows, NAVR_TILE);
    DevBuf<int> act;
    for (long long f0 = 0; f0 < nf_all; f0 += 32768) {                   // (a grid's second and third dimension end at 65535)
        const int nf = (int)std::min<long long>(32768, nf_all - f0);
        int* fld = d_fields + (size_t)f0 * HW;
        act.alloc((size_t)nf * ntiles);
        act.zero(s);
        const long long cells = (long long)nf * HW;
        hipLaunchKernelGGL(k_navr_fill, dim3(cdiv((size_t)cells, NAVR_T)), dim3(NAVR_T), 0, s, fld, cells, (int)NAVR_NONE);
        if (max_sources > 0)
            hipLaunchKernelGGL(k_navr_sources, dim3(cdiv((size_t)max_sources, NAVR_T), (unsigned)nf), dim3(NAVR_T), 0, s, rows, cols, d_pass,
                               d_src_off + f0, d_src_rc, fld, act.p, ntx, ntiles / ntx);
        HMSG_CHECK_LAUNCH();
        navr_relax(s, rows, cols, d_pass, p, true, nf, fld, act.p);
        if (d_n_reached) {
            HIP_TRY(hipMemsetAsync(d_n_reached + f0, 0, sizeof(unsigned long long) * (size_t)nf, s));
            hipLaunchKernelGGL(k_navr_count, dim3(cdiv((size_t)HW, NAVR_T), (unsigned)nf), dim3(NAVR_T), 0, s, (const int*)fld, HW, d_n_reached + f0);
            HMSG_CHECK_LAUNCH();
        }
    }
}
namespace {

void navr_clearance_dev(hipStream_t s, int rows, int cols, const unsigned char* d_mask, const hmsg_route_params& p, int* d_clr) {
    const int HW = rows * cols, ntiles = (int)(cdiv((size_t)cols, NAVR_TILE) * cdiv((size_t)rows, NAVR_TILE));
    DevBuf<int> act;
    act.alloc((size_t)ntiles);
    hipLaunchKernelGGL(k_navr_clear_init, dim3(cdiv((size_t)HW, NAVR_T)), dim3(NAVR_T), 0, s, rows, cols, d_mask, p.w_straight, d_clr);
    hipLaunchKernelGGL(k_navr_fill, dim3(cdiv((size_t)ntiles, NAVR_T)), dim3(NAVR_T), 0, s, act.p, (long long)ntiles, 1);
    HMSG_CHECK_LAUNCH();
    navr_relax(s, rows, cols, nullptr, p, false, 1, d_clr, act.p);
}

}  // namespace
// hmsg_nav_route's first step: d_pass = the mask where its clearance reaches min_clearance (0: the mask's cells as 1 / 0)
void navr_passable_dev(hipStream_t s, int rows, int cols, const unsigned char* d_mask, const hmsg_route_params& p, unsigned char* d_pass) {
    const size_t HW = (size_t)rows * cols;
    const dim3 gi(cdiv(HW, NAVR_T)), b(NAVR_T);
    if (p.min_clearance > 0) {
        DevBuf<int> clr;
        clr.alloc(HW);
        navr_clearance_dev(s, rows, cols, d_mask, p, clr.p);
        hipLaunchKernelGGL(k_navr_threshold, gi, b, 0, s, d_mask, (const int*)clr.p, p.min_clearance, (int)HW, d_pass);
    } else {
        hipLaunchKernelGGL(k_navr_binary, gi, b, 0, s, d_mask, (int)HW, d_pass);
    }
    HMSG_CHECK_LAUNCH();
}
void navr_snap_dev(hipStream_t s, int rows, int cols, const unsigned char* d_pass, const int* d_field, long long n, const int* d_target,
                   int* d_snapped, long long* d_d2) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_navr_snap, dim3((unsigned)std::min<long long>(n, 1 << 20)), dim3(NAVR_T), 0, s, rows, cols, d_pass, d_field, n, d_target,
                       d_snapped, d_d2);
    HMSG_CHECK_LAUNCH();
}
namespace {

// path_off (device, [n + 1]) and the total; the list into path_rc (caller memory, host or device) when it is wanted and fits.
// Returns the total; *too_short says that a wanted list was not written.
long long navr_paths_dev(hipStream_t s, int rows, int cols, const unsigned char* d_pass, const hmsg_route_params& p, const int* d_field,
                         long long n, const int* d_goal, long long* d_off, int32_t* path_rc, long long capacity, bool* too_short) {
    DevBuf<long long> cnt;
    cnt.alloc((size_t)std::max<long long>(n, 1));
    const dim3 grid(cdiv((size_t)std::max<long long>(n, 1), NAVR_T));
    if (n > 0)
        hipLaunchKernelGGL(k_navr_walk<false>, grid, dim3(NAVR_T), 0, s, rows, cols, d_pass, d_field, p.w_straight, p.w_diag, n, d_goal, cnt.p,
                           (const long long*)nullptr, (int*)nullptr);
    hipLaunchKernelGGL(k_navr_scan, dim3(1), dim3(64), 0, s, n, (const long long*)cnt.p, d_off);
    HMSG_CHECK_LAUNCH();
    long long total = 0;
    HIP_TRY(hipMemcpyAsync(&total, d_off + n, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *too_short = path_rc && total > capacity;
    if (path_rc && total && !*too_short) {
        DevBuf<int> own;
        int* p_rc = stage_out(own, path_rc, (size_t)total * 2);
        hipLaunchKernelGGL(k_navr_walk<true>, grid, dim3(NAVR_T), 0, s, rows, cols, d_pass, d_field, p.w_straight, p.w_diag, n, d_goal,
                           (long long*)nullptr, (const long long*)d_off, p_rc);
        HMSG_CHECK_LAUNCH();
        unstage_out(path_rc, p_rc, (size_t)total * 2, s);
        HIP_TRY(hipStreamSynchronize(s));
    }
    return total;
}

}  // namespace
[[noreturn]] void navr_throw_short(const char* fn, long long total, long long capacity) {
    throw hmsg_error{HMSG_ERR_INVALID, std::string(fn) + ": " + std::to_string(total) + " path cells, path_rc holds " + std::to_string(capacity) +
                                           " (the count says what is needed)"};
}

extern "C" void hmsg_route_default_params(hmsg_route_params* p) {
    if (!p) return;
    p->w_straight = 5;
    p->w_diag = 7;
    p->min_clearance = 0;
    p->reserved_ = 0;
}

extern "C" int hmsg_nav_clearance(int32_t device_id, int32_t rows, int32_t cols, const uint8_t* mask, const hmsg_route_params* prm,
                                  int32_t* clearance) {
    if (!mask || !prm || !clearance) return HMSG_ERR_INVALID;
    return hmsg_boundary("hmsg_nav_clearance", device_id, [&] {
        navr_check(rows, cols, *prm, "hmsg_nav_clearance");
        g_navr_rounds = g_navr_trips = 0;
        ScopedStream s(hipStreamNonBlocking);
        const size_t HW = (size_t)rows * cols;
        DevBuf<unsigned char> own_mask;
        DevBuf<int> own_clr;
        const unsigned char* d_mask = stage_in(own_mask, mask, HW, s, Up::bounce);
        int* d_clr = stage_out(own_clr, clearance, HW);
        navr_clearance_dev(s, rows, cols, d_mask, *prm, d_clr);
        unstage_out(clearance, d_clr, HW, s);
        HIP_TRY(hipStreamSynchronize(s));
    });
}

extern "C" int hmsg_nav_distance_fields(int32_t device_id, int32_t rows, int32_t cols, const uint8_t* passable, const hmsg_route_params* prm,
                                        int32_t n_fields, const int64_t* src_off, const int32_t* src_rc, int32_t* fields, int64_t* n_reached) {
    if (!passable || !prm || !src_off || !fields) return HMSG_ERR_INVALID;
    return hmsg_boundary("hmsg_nav_distance_fields", device_id, [&] {
        const std::string f = "hmsg_nav_distance_fields";
        navr_check(rows, cols, *prm, f.c_str());
        HMSG_REQUIRE(n_fields >= 0, HMSG_ERR_INVALID, f + ": n_fields < 0");
        g_navr_rounds = g_navr_trips = 0;
        if (n_fields == 0) return;
        // the offsets and the cells are read on the host: both are checked before anything runs
        std::vector<long long> off((size_t)n_fields + 1);
        read_in(off.data(), src_off, off.size() * 8);
        long long most = 0;
        HMSG_REQUIRE(off[0] >= 0, HMSG_ERR_INVALID, f + ": src_off[0] < 0");
        for (int32_t k = 0; k < n_fields; ++k) {
            HMSG_REQUIRE(off[(size_t)k + 1] >= off[(size_t)k], HMSG_ERR_INVALID, f + ": src_off decreases at field " + std::to_string(k));
            most = std::max(most, off[(size_t)k + 1] - off[(size_t)k]);
        }
        const long long total = off[(size_t)n_fields];
        HMSG_REQUIRE(total == off[0] || src_rc, HMSG_ERR_INVALID, f + ": src_rc is null");
        std::vector<int32_t> rc((size_t)total * 2);
        if (total) read_in(rc.data(), src_rc, rc.size() * 4);
        for (long long k = off[0]; k < total; ++k)
            HMSG_REQUIRE(rc[(size_t)k * 2] >= 0 && rc[(size_t)k * 2] < rows && rc[(size_t)k * 2 + 1] >= 0 && rc[(size_t)k * 2 + 1] < cols,
                         HMSG_ERR_INVALID, f + ": source " + std::to_string(k) + " lies outside the image");
        ScopedStream s(hipStreamNonBlocking);
        const size_t HW = (size_t)rows * cols;
        DevBuf<unsigned char> own_pass;
        DevBuf<long long> d_off;
        DevBuf<int> d_rc, own_fields;
        DevBuf<unsigned long long> d_cnt;
        const unsigned char* d_pass = stage_in(own_pass, passable, HW, s, Up::bounce);
        d_off.alloc(off.size()), d_rc.alloc(rc.size());
        HIP_TRY(hipMemcpyAsync(d_off.p, off.data(), off.size() * 8, hipMemcpyHostToDevice, s));
        if (total) upload(d_rc.p, rc.data(), rc.size() * 4, s, Up::bounce);
        int* d_fields = stage_out(own_fields, fields, HW * (size_t)n_fields);
        if (n_reached) d_cnt.alloc((size_t)n_fields);
        navr_fields_dev(s, rows, cols, d_pass, *prm, n_fields, d_off.p, d_rc.p, most, d_fields, n_reached ? d_cnt.p : nullptr);
        unstage_out(fields, d_fields, HW * (size_t)n_fields, s);
        if (n_reached) copy_out(n_reached, d_cnt.p, (size_t)n_fields * 8, s);
        HIP_TRY(hipStreamSynchronize(s));
    });
}

extern "C" int hmsg_nav_snap_cells(int32_t device_id, int32_t rows, int32_t cols, const uint8_t* passable, const int32_t* field, int64_t n,
                                   const int32_t* target_rc, int32_t* snapped_rc, int64_t* d2) {
    if (!passable || (n > 0 && (!target_rc || !snapped_rc))) return HMSG_ERR_INVALID;
    return hmsg_boundary("hmsg_nav_snap_cells", device_id, [&] {
        navr_check_shape(rows, cols, "hmsg_nav_snap_cells");
        HMSG_REQUIRE(n >= 0, HMSG_ERR_INVALID, "hmsg_nav_snap_cells: n < 0");
        if (n == 0) return;
        ScopedStream s(hipStreamNonBlocking);
        const size_t HW = (size_t)rows * cols;
        DevBuf<unsigned char> own_pass;
        DevBuf<int> own_field, own_t, own_s;
        DevBuf<long long> own_d;
        const unsigned char* d_pass = stage_in(own_pass, passable, HW, s, Up::bounce);
        const int* d_field = field ? stage_in(own_field, field, HW, s, Up::bounce) : nullptr;
        const int* d_t = stage_in(own_t, target_rc, (size_t)n * 2, s, Up::bounce);
        int* d_s = stage_out(own_s, snapped_rc, (size_t)n * 2);
        long long* d_d = stage_out(own_d, (long long*)d2, (size_t)n);
        navr_snap_dev(s, rows, cols, d_pass, d_field, n, d_t, d_s, d_d);
        unstage_out(snapped_rc, d_s, (size_t)n * 2, s);
        if (d2) unstage_out((long long*)d2, (const long long*)d_d, (size_t)n, s);
        HIP_TRY(hipStreamSynchronize(s));
    });
}

extern "C" int hmsg_nav_paths(int32_t device_id, int32_t rows, int32_t cols, const uint8_t* passable, const hmsg_route_params* prm,
                              const int32_t* field, int64_t n_goals, const int32_t* goal_rc, int64_t* path_off, int32_t* path_rc, int64_t capacity,
                              int64_t* n_needed) {
    if (!passable || !prm || !field || !n_needed || (n_goals > 0 && !goal_rc)) return HMSG_ERR_INVALID;
    return hmsg_boundary("hmsg_nav_paths", device_id, [&] {
        navr_check(rows, cols, *prm, "hmsg_nav_paths");
        HMSG_REQUIRE(n_goals >= 0 && (!path_rc || capacity >= 0), HMSG_ERR_INVALID, "hmsg_nav_paths: n_goals < 0 or capacity < 0");
        *n_needed = 0;
        ScopedStream s(hipStreamNonBlocking);
        const size_t HW = (size_t)rows * cols;
        DevBuf<unsigned char> own_pass;
        DevBuf<int> own_field, own_g;
        DevBuf<long long> d_off;
        const unsigned char* d_pass = stage_in(own_pass, passable, HW, s, Up::bounce);
        const int* d_field = stage_in(own_field, field, HW, s, Up::bounce);
        const int* d_g = n_goals ? stage_in(own_g, goal_rc, (size_t)n_goals * 2, s, Up::bounce) : nullptr;
        d_off.alloc((size_t)n_goals + 1);
        bool too_short = false;
        const long long total = navr_paths_dev(s, rows, cols, d_pass, *prm, d_field, n_goals, d_g, d_off.p, path_rc, capacity, &too_short);
        *n_needed = total;
        if (path_off) copy_out(path_off, d_off.p, ((size_t)n_goals + 1) * 8, s);
        HIP_TRY(hipStreamSynchronize(s));
        if (too_short) navr_throw_short("hmsg_nav_paths", total, capacity);
    });
}

// the composition, and only that: clearance -> passable, snap the start, one field, the goals' cells among the reached (R4 for
// hmsg_nav_route, V4 for hmsg_nav_view_route: `snap` is the one step in which the two differ), paths
void navr_route_run(const char* fn, int32_t rows, int32_t cols, const uint8_t* main_free_map, const hmsg_route_params* prm, const int32_t* start_rc,
                    int64_t n_goals, const int32_t* goal_rc, hmsg_nav_routes* out, const navr_goal_snap& snap) {
    navr_check(rows, cols, *prm, fn);
    HMSG_REQUIRE(n_goals >= 0 && (!out->path_rc || out->path_capacity >= 0), HMSG_ERR_INVALID, std::string(fn) + ": n_goals < 0 or path_capacity < 0");
    out->n_path_cells = 0, out->start_d2 = -1, out->start_cell[0] = out->start_cell[1] = -1;
    g_navr_rounds = g_navr_trips = 0;
    ScopedStream s(hipStreamNonBlocking);
    const size_t HW = (size_t)rows * cols, n = (size_t)n_goals;
    const dim3 b(NAVR_T);
    DevBuf<unsigned char> own_mask, own_pass;
    DevBuf<int> own_field, own_start, own_goal, own_cell, own_dist, start;
    DevBuf<long long> own_d2, d_off, src_off, start_d2;
    const unsigned char* d_mask = stage_in(own_mask, main_free_map, HW, s, Up::bounce);
    const int* d_start = stage_in(own_start, start_rc, 2, s, Up::direct);
    const int* d_goal = n ? stage_in(own_goal, goal_rc, n * 2, s, Up::bounce) : nullptr;
    // 1. passable
    unsigned char* d_pass = stage_out(own_pass, out->passable, HW);
    if (!d_pass) own_pass.alloc(HW), d_pass = own_pass.p;
    navr_passable_dev(s, rows, cols, d_mask, *prm, d_pass);
    // 2. the start, 3. its field
    start.alloc(2), start_d2.alloc(1), src_off.alloc(2);
    navr_snap_dev(s, rows, cols, d_pass, nullptr, 1, d_start, start.p, start_d2.p);
    const long long h_off[2] = {0, 1};
    HIP_TRY(hipMemcpyAsync(src_off.p, h_off, sizeof(h_off), hipMemcpyHostToDevice, s));
    int* d_field = stage_out(own_field, out->field, HW);
    if (!d_field) own_field.alloc(HW), d_field = own_field.p;
    navr_fields_dev(s, rows, cols, d_pass, *prm, 1, src_off.p, start.p, 1, d_field, nullptr);
    // 4. the goals among the reached cells, their distances
    int* d_cell = stage_out(own_cell, out->goal_cell, n * 2);
    if (!d_cell) own_cell.alloc(n * 2), d_cell = own_cell.p;
    long long* d_d2 = stage_out(own_d2, (long long*)out->goal_d2, n);
    int* d_dist = stage_out(own_dist, out->goal_dist, n);
    snap(s, d_pass, d_field, d_goal, d_cell, d_d2);
    if (d_dist && n) {
        hipLaunchKernelGGL(k_navr_gather, dim3(cdiv(n, NAVR_T)), b, 0, s, (const int*)d_field, cols, (long long)n, (const int*)d_cell, d_dist);
        HMSG_CHECK_LAUNCH();
    }
    // 5. the paths
    d_off.alloc(n + 1);
    bool too_short = false;
    const long long total = navr_paths_dev(s, rows, cols, d_pass, *prm, d_field, n_goals, d_cell, d_off.p, out->path_rc, out->path_capacity,
                                           &too_short);
    out->n_path_cells = total;
    if (out->path_off) copy_out(out->path_off, d_off.p, (n + 1) * 8, s);
    if (out->passable) unstage_out(out->passable, d_pass, HW, s);
    if (out->field) unstage_out(out->field, d_field, HW, s);
    if (out->goal_cell) unstage_out(out->goal_cell, d_cell, n * 2, s);
    if (out->goal_d2) unstage_out((long long*)out->goal_d2, (const long long*)d_d2, n, s);
    if (out->goal_dist) unstage_out(out->goal_dist, d_dist, n, s);
    long long h_d2 = -1;
    HIP_TRY(hipMemcpyAsync(out->start_cell, start.p, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&h_d2, start_d2.p, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    out->start_d2 = h_d2;
    if (too_short) navr_throw_short(fn, total, out->path_capacity);
}

extern "C" int hmsg_nav_route(int32_t device_id, int32_t rows, int32_t cols, const uint8_t* main_free_map, const hmsg_route_params* prm,
                              const int32_t* start_rc, int64_t n_goals, const int32_t* goal_rc, hmsg_nav_routes* out) {
    if (!main_free_map || !prm || !start_rc || !out || (n_goals > 0 && !goal_rc)) return HMSG_ERR_INVALID;
    return hmsg_boundary("hmsg_nav_route", device_id, [&] {
        navr_route_run("hmsg_nav_route", rows, cols, main_free_map, prm, start_rc, n_goals, goal_rc, out,
                       [&](hipStream_t s, const unsigned char* d_pass, const int* d_field, const int* d_goal, int* d_cell, long long* d_d2) {
                           navr_snap_dev(s, rows, cols, d_pass, d_field, n_goals, d_goal, d_cell, d_d2);
                       });
    });
}

extern "C" int hmsg_test_nav_route_last(int32_t* rounds, int32_t* round_trips) {
    if (rounds) *rounds = g_navr_rounds;
    if (round_trips) *round_trips = g_navr_trips;
    return HMSG_OK;
}
