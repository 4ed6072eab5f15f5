// Rooms on a floor's free map (include/hmsg.h, N11: hmsg_nav_room_labels, hmsg_nav_doors, hmsg_nav_path_rooms,
// hmsg_nav_room_doors): every reached cell of the passable map gets the room whose seeds are nearest by the walk (G1, G2), the
// cells where two rooms touch are gathered into doors (D1 to D4), and a way is cut into legs by room (L1).  The reference has no
// counterpart (its graph has no room-room edge, its navigation graph knows no rooms): the rules are this library's and stand in
// the header.  Every output is integer work with one right answer.
//
// MI355X design notes
//  * Field: `dist` is N7's relaxation from the union of the seeds, navr_fields_dev as it is.
//  * Labels (k_navg_relax): a second tile kernel on k_navr_relax's plan -- 64 x 64 tiles with a one-cell halo, 256 threads, a
//    thread sweeping its 16 cells of a row left to right and back, stamps for the next round, navr_rounds' growing batches, no cap
//    on rounds.  LDS holds the tile's dist (read-only), its labels (both 66 x 66 int32 at the odd row stride 67) and the passable
//    bytes: 39.9 KB, four workgroups a CU.  A cell takes the least label over its legal tight predecessors (dist[n] + w ==
//    dist[c]), G2's second form.  Minimum is monotone and idempotent and a label only ever falls towards the answer, so the field's
//    race argument holds: a halo cell read while its owner writes it is the old or the new value, both upper bounds, and the owner
//    stamps this tile for the next round.  The packed (dist, room) 64-bit relaxation was not taken: it doubles the bytes of the
//    field kernel's LDS tile and of every load of the hot loop, would be a second copy of k_navr_relax with another word type, and
//    the 32-bit field is wanted as an output anyway.
//  * Seeds: the host has read and checked them, and hands the device one room index per seed; atomicMin on the label image gives
//    a cell seeded by several rooms the least of them.  This is the only atomic on the image, before the first round.
//  * Threshold (k_navd_threshold): one pass writes `other`, a flag and the cell's own index as its parent in the forest.
//  * Doors: the flagged cells are compacted in row-major order (one exclusive scan of the flags), joined by atomicMin hooking
//    between 8-neighbours of equal pair (k_navd_hook: the larger root is hung under the smaller, so a component's root is its least
//    row-major index whatever the order), flattened (k_navd_flatten) and their roots listed.  The host orders the doors -- dozens --
//    by D4; the cells are brought into (door, row-major) order by one stable radix sort of the compacted list by door number, whose
//    segment starts are door_off.  Three read-backs in all, none of which grows with a door's length.
//  * Legs (k_navg_legs): a lane per path, two passes over the same cells (count, one wave's scan, write), as k_navr_walk.
#include "hmsg_navroute_dev.h"

#include <algorithm>
#include <climits>
#include <vector>

#define NAVG_NONE INT_MAX                // "no label yet" while the labels settle; -1 in what the caller sees
#define NAVG_MAX_ADJ_ROOMS 4096

// ------------------------------------------------------------------------------------------ labels (G1, G2)
// a seed on a passable cell: the least room that seeds it; its tile and the eight round it start in round 1
__global__ __launch_bounds__(NAVR_T) void k_navg_seeds(int rows, int cols, const unsigned char* __restrict__ pass, long long n,
                                                       const int* __restrict__ seed_rc, const int* __restrict__ seed_room, int* label,
                                                       int* __restrict__ act, int ntx, int nty) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int r = seed_rc[k * 2], c = seed_rc[k * 2 + 1];
    if (r < 0 || r >= rows || c < 0 || c >= cols) return;
    const size_t i = (size_t)r * cols + c;
    if (!pass[i]) return;
    atomicMin(&label[i], seed_room[k]);
    const int ty = r / NAVR_TILE, tx = c / NAVR_TILE;
    for (int y = max(ty - 1, 0); y <= min(ty + 1, nty - 1); ++y)
        for (int x = max(tx - 1, 0); x <= min(tx + 1, ntx - 1); ++x) act[(size_t)y * ntx + x] = 1;
}

// One round: grid (tile columns, tile rows).  A tile runs when its stamp is this round's (or already the next one's); `changed`
// counts the tiles that changed.  dist is the settled field and is only read.
__global__ __launch_bounds__(NAVR_T) void k_navg_relax(int rows, int cols, const unsigned char* __restrict__ pass, int w_straight, int w_diag,
                                                       const int* __restrict__ dist, int* __restrict__ label, int* __restrict__ act, int round,
                                                       unsigned* __restrict__ changed) {
    __shared__ int s_d[NAVR_SIDE * NAVR_LD];
    __shared__ int s_l[NAVR_SIDE * NAVR_LD];
    __shared__ unsigned char s_p[NAVR_SIDE * NAVR_PLD];
    __shared__ int s_chg[3];
    __shared__ int s_run;
    const int tid = threadIdx.x, ntx = gridDim.x, nty = gridDim.y;
    const int tx = blockIdx.x, ty = blockIdx.y;
    if (tid == 0) s_run = act[ty * ntx + tx] >= round ? 1 : 0, s_chg[0] = 0;
    __syncthreads();
    if (!s_run) return;
    const int r0 = ty * NAVR_TILE - 1, c0 = tx * NAVR_TILE - 1;
    for (int i = tid; i < NAVR_SIDE * NAVR_SIDE; i += NAVR_T) {
        const int lr = i / NAVR_SIDE, lc = i - lr * NAVR_SIDE, r = r0 + lr, c = c0 + lc;
        const bool in = r >= 0 && r < rows && c >= 0 && c < cols;
        const bool p = in && pass[(size_t)r * cols + c] != 0;
        s_p[lr * NAVR_PLD + lc] = p ? 1 : 0;
        s_d[lr * NAVR_LD + lc] = p ? dist[(size_t)r * cols + c] : HMSG_NAV_UNREACHED;
        s_l[lr * NAVR_LD + lc] = p ? label[(size_t)r * cols + c] : NAVG_NONE;
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
            const int here = s_d[lr * NAVR_LD + lc];
            if (!s_p[lr * NAVR_PLD + lc] || here == HMSG_NAV_UNREACHED) continue;
            const int cur = s_l[lr * NAVR_LD + lc];
            int best = cur;
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                const int dr = d < 4 ? (d == 0 ? -1 : (d == 1 ? 1 : 0)) : (d < 6 ? -1 : 1);
                const int dc = d < 4 ? (d == 2 ? -1 : (d == 3 ? 1 : 0)) : ((d & 1) ? 1 : -1);
                if (d >= 4 && !(s_p[(lr + dr) * NAVR_PLD + lc] && s_p[lr * NAVR_PLD + lc + dc])) continue;
                const int v = s_d[(lr + dr) * NAVR_LD + lc + dc];           // (unreached where the neighbour is not passable)
                const int w = d < 4 ? w_straight : w_diag;
                if (v != HMSG_NAV_UNREACHED && v + w == here) best = min(best, s_l[(lr + dr) * NAVR_LD + lc + dc]);
            }
            if (best < cur) s_l[lr * NAVR_LD + lc] = best, chg = true;
        }
        if (chg) s_chg[it % 3] = 1;
        __syncthreads();
        if (!s_chg[it % 3]) break;
        any = true;
    }
    if (!any) return;
    for (int k = 0; k < 16; ++k) {
        const int lc = lc0 + k, r = r0 + lr, c = c0 + lc;
        if (s_p[lr * NAVR_PLD + lc]) label[(size_t)r * cols + c] = s_l[lr * NAVR_LD + lc];     // (s_p: inside the image)
    }
    if (tid < 8) {
        const int dr = tid < 4 ? (tid == 0 ? -1 : (tid == 1 ? 1 : 0)) : (tid < 6 ? -1 : 1);
        const int dc = tid < 4 ? (tid == 2 ? -1 : (tid == 3 ? 1 : 0)) : ((tid & 1) ? 1 : -1);
        const int ny = ty + dr, nx = tx + dc;
        if (ny >= 0 && ny < nty && nx >= 0 && nx < ntx) act[ny * ntx + nx] = round + 1;
    } else if (tid == 8) {
        atomicAdd(changed, 1u);
    }
}
// "no label" becomes -1; n_cells[r] += the cells of label r (one add per wave and label in it)
__global__ __launch_bounds__(NAVR_T) void k_navg_finish(int HW, int* __restrict__ label, unsigned long long* __restrict__ n_cells) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
    int l = -1;
    if (i < HW) {
        l = label[i];
        if (l == NAVG_NONE) label[i] = l = -1;
    }
    if (!n_cells) return;
    unsigned long long todo = __ballot(l >= 0);
    while (todo) {
        const int lead = __ffsll(todo) - 1;
        const int ll = __shfl(l, lead);
        const unsigned long long same = __ballot(l == ll) & todo;
        if (lane == lead) atomicAdd(&n_cells[ll], (unsigned long long)__popcll(same));
        todo &= ~same;
    }
}

// ------------------------------------------------------------------------------------------ threshold cells (D1, D2)
// other[i], flag[i] = 1 for a threshold cell, parent[i] = i for one and -1 else; *bad = 1 when a label lies outside [-1, n_rooms)
__global__ __launch_bounds__(NAVR_T) void k_navd_threshold(int rows, int cols, const unsigned char* __restrict__ pass, const int* __restrict__ label,
                                                           int n_rooms, int* __restrict__ other, unsigned* __restrict__ flag, int* __restrict__ parent,
                                                           int* __restrict__ bad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * cols) return;
    const int r = i / cols, c = i - r * cols, la = label[i];
    if (la < -1 || la >= n_rooms) *bad = 1;
    int o = INT_MAX;
    if (la >= 0 && pass[i]) {
#pragma unroll
        for (int d = 0; d < 8; ++d) {
            const int dr = d < 4 ? (d == 0 ? -1 : (d == 1 ? 1 : 0)) : (d < 6 ? -1 : 1);
            const int dc = d < 4 ? (d == 2 ? -1 : (d == 3 ? 1 : 0)) : ((d & 1) ? 1 : -1);
            const int nr = r + dr, nc = c + dc;
            if (nr < 0 || nr >= rows || nc < 0 || nc >= cols || !pass[(size_t)nr * cols + nc]) continue;
            if (d >= 4 && !(pass[(size_t)nr * cols + c] && pass[(size_t)r * cols + nc])) continue;
            const int lb = label[(size_t)nr * cols + nc];
            if (lb >= 0 && lb != la && lb < o) o = lb;
        }
    }
    const bool t = o != INT_MAX;
    other[i] = t ? o : -1;
    flag[i] = t ? 1u : 0u;
    parent[i] = t ? i : -1;
}
// the flagged cells in row-major order: pos = the exclusive scan of flag
__global__ __launch_bounds__(NAVR_T) void k_navd_compact(int HW, const unsigned* __restrict__ pos, const int* __restrict__ other, int* __restrict__ cell) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < HW && other[i] >= 0) cell[pos[i]] = i;
}

// ------------------------------------------------------------------------------------------ doors (D3, D4)
__device__ static inline int navd_find(int* parent, int x) {
    for (;;) {
        const int p = __atomic_load_n(&parent[x], __ATOMIC_RELAXED);
        if (p == x) return x;
        x = p;
    }
}
// the larger root goes under the smaller; a root that somebody else hung meanwhile is retried from where it hangs now
__device__ static inline void navd_unite(int* parent, int a, int b) {
    for (;;) {
        a = navd_find(parent, a), b = navd_find(parent, b);
        if (a == b) return;
        if (a > b) {
            const int t = a;
            a = b, b = t;
        }
        const int old = atomicMin(&parent[b], a);
        if (old == b) return;
        b = old;
    }
}
// a lane per threshold cell: joins it with the neighbours E, SW, S, SE of the same pair (the other four are those cells' own work)
__global__ __launch_bounds__(NAVR_T) void k_navd_hook(int rows, int cols, int n, const int* __restrict__ cell, const int* __restrict__ label,
                                                      const int* __restrict__ other, int* parent) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int i = cell[k], r = i / cols, c = i - r * cols;
    const int la = label[i], oa = other[i], lo = min(la, oa), hi = max(la, oa);
    const int DR[4] = {0, 1, 1, 1}, DC[4] = {1, -1, 0, 1};
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const int nr = r + DR[d], nc = c + DC[d];
        if (nr >= rows || nc < 0 || nc >= cols) continue;
        const int j = nr * cols + nc, ob = other[j];
        if (ob < 0) continue;
        const int lb = label[j];
        if (min(lb, ob) == lo && max(lb, ob) == hi) navd_unite(parent, i, j);
    }
}
// every threshold cell points at its root; the roots are listed (in no order) with their pair
__global__ __launch_bounds__(NAVR_T) void k_navd_flatten(int n, const int* __restrict__ cell, int* parent) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) parent[cell[k]] = navd_find(parent, cell[k]);
}
__global__ __launch_bounds__(NAVR_T) void k_navd_roots(int n, const int* __restrict__ cell, const int* __restrict__ parent, const int* __restrict__ label,
                                                       const int* __restrict__ other, unsigned* __restrict__ n_doors, int* __restrict__ root_pq) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int i = cell[k];
    if (parent[i] != i) return;
    const unsigned at = atomicAdd(n_doors, 1u);             // (at most n roots: root_pq holds 3 * n)
    root_pq[at * 3] = i, root_pq[at * 3 + 1] = min(label[i], other[i]), root_pq[at * 3 + 2] = max(label[i], other[i]);
}
// slot[root of door k] = k, the doors in D4's order
__global__ __launch_bounds__(NAVR_T) void k_navd_slots(int n_doors, const int* __restrict__ root, int* __restrict__ slot) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n_doors) slot[root[k]] = k;
}
__global__ __launch_bounds__(NAVR_T) void k_navd_keys(int n, const int* __restrict__ cell, const int* __restrict__ parent, const int* __restrict__ slot,
                                                      unsigned* __restrict__ key, unsigned long long* __restrict__ val) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) key[k] = (unsigned)slot[parent[cell[k]]], val[k] = (unsigned long long)cell[k];
}
__global__ __launch_bounds__(NAVR_T) void k_navd_emit(int n, int cols, const unsigned long long* __restrict__ val, int* __restrict__ door_rc) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int i = (int)val[k];
    door_rc[k * 2] = i / cols, door_rc[k * 2 + 1] = i - (i / cols) * cols;
}

// ------------------------------------------------------------------------------------------ legs (L1)
// WRITE false: cnt[p] = the legs of path p.  WRITE true: leg_room and leg_first at leg_off[p] ...
template <bool WRITE>
__global__ __launch_bounds__(NAVR_T) void k_navg_legs(int rows, int cols, const int* __restrict__ label, long long n, const long long* __restrict__ path_off,
                                                      const int* __restrict__ path_rc, long long* __restrict__ cnt, const long long* __restrict__ leg_off,
                                                      int* __restrict__ leg_room, long long* __restrict__ leg_first) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const long long a = path_off[p], b = path_off[p + 1];
    long long legs = 0, at = WRITE ? leg_off[p] : 0;
    int last = 0;
    for (long long k = a; k < b; ++k) {
        const int r = path_rc[k * 2], c = path_rc[k * 2 + 1];
        const int l = (r >= 0 && r < rows && c >= 0 && c < cols) ? label[(size_t)r * cols + c] : -1;
        if (k == a || l != last) {
            if (WRITE) leg_room[at] = l, leg_first[at] = k - a, ++at;
            ++legs;
        }
        last = l;
    }
    if (!WRITE) cnt[p] = legs;
}

// ------------------------------------------------------------------------------------------ the calls
namespace {
thread_local int g_navg_rounds = 0, g_navg_trips = 0;       // what hmsg_test_nav_rooms_last reports

// the seeds as the host read them: checked, with a room index per seed
struct NavgSeeds {
    long long first = 0, total = 0;                 // seed_off[0], seed_off[n_rooms]
    std::vector<int32_t> rc, room;                  // [total][2], [total]
};
void navg_read_seeds(const std::string& f, int32_t rows, int32_t cols, int32_t n_rooms, const int64_t* seed_off, const int32_t* seed_rc, NavgSeeds& sd) {
    HMSG_REQUIRE(n_rooms >= 0, HMSG_ERR_INVALID, f + ": n_rooms < 0");
    std::vector<long long> off((size_t)n_rooms + 1);
    read_in(off.data(), seed_off, off.size() * 8);
    HMSG_REQUIRE(off[0] >= 0, HMSG_ERR_INVALID, f + ": seed_off[0] < 0");
    for (int32_t k = 0; k < n_rooms; ++k)
        HMSG_REQUIRE(off[(size_t)k + 1] >= off[(size_t)k], HMSG_ERR_INVALID, f + ": seed_off decreases at room " + std::to_string(k));
    sd.first = off[0], sd.total = off[(size_t)n_rooms];
    HMSG_REQUIRE(sd.total == sd.first || seed_rc, HMSG_ERR_INVALID, f + ": seed_rc is null");
    sd.rc.assign((size_t)sd.total * 2, 0), sd.room.assign((size_t)sd.total, 0);
    if (sd.total) read_in(sd.rc.data(), seed_rc, sd.rc.size() * 4);
    for (int32_t r = 0; r < n_rooms; ++r)
        for (long long k = off[(size_t)r]; k < off[(size_t)r + 1]; ++k) {
            HMSG_REQUIRE(sd.rc[(size_t)k * 2] >= 0 && sd.rc[(size_t)k * 2] < rows && sd.rc[(size_t)k * 2 + 1] >= 0 && sd.rc[(size_t)k * 2 + 1] < cols,
                         HMSG_ERR_INVALID, f + ": seed " + std::to_string(k) + " lies outside the image");
            sd.room[(size_t)k] = r;
        }
}

// G1, G2 on device buffers: d_label i32 [rows][cols]; d_dist i32 [rows][cols] or nullptr; d_n_cells u64 [n_rooms] or nullptr
void navg_labels_dev(hipStream_t s, int rows, int cols, const unsigned char* d_pass, const hmsg_route_params& p, int n_rooms, const NavgSeeds& sd,
                     int* d_label, int* d_dist, unsigned long long* d_n_cells) {
    const size_t HW = (size_t)rows * cols;
    const int ntx = (int)cdiv((size_t)cols, NAVR_TILE), nty = (int)cdiv((size_t)rows, NAVR_TILE);
    DevBuf<int> own_dist, d_rc, d_room, act;
    DevBuf<long long> d_off;
    if (!d_dist) own_dist.alloc(HW), d_dist = own_dist.p;
    d_rc.alloc(sd.rc.size()), d_room.alloc(sd.room.size()), d_off.alloc(2);
    const long long n_seeds = sd.total - sd.first, h_off[2] = {sd.first, sd.total};
    HIP_TRY(hipMemcpyAsync(d_off.p, h_off, sizeof(h_off), hipMemcpyHostToDevice, s));
    if (sd.total) {
        upload(d_rc.p, sd.rc.data(), sd.rc.size() * 4, s, Up::bounce);
        upload(d_room.p, sd.room.data(), sd.room.size() * 4, s, Up::bounce);
    }
    // G1: the field of the union of the seeds
    navr_fields_dev(s, rows, cols, d_pass, p, 1, d_off.p, d_rc.p, n_seeds, d_dist, nullptr);
    // G2: the least room over the tight predecessors
    act.alloc((size_t)ntx * nty);
    act.zero(s);
    navr_fill_dev(s, d_label, (long long)HW, NAVG_NONE);
    if (n_seeds > 0)
        hipLaunchKernelGGL(k_navg_seeds, dim3(cdiv((size_t)n_seeds, NAVR_T)), dim3(NAVR_T), 0, s, rows, cols, d_pass, n_seeds,
                           (const int*)d_rc.p + sd.first * 2, (const int*)d_room.p + sd.first, d_label, act.p, ntx, nty);
    HMSG_CHECK_LAUNCH();
    const dim3 grid((unsigned)ntx, (unsigned)nty);
    const int* dist = d_dist;
    navr_rounds(s, [&](int round, unsigned* d_changed) {
        hipLaunchKernelGGL(k_navg_relax, grid, dim3(NAVR_T), 0, s, rows, cols, d_pass, p.w_straight, p.w_diag, dist, d_label, act.p, round, d_changed);
    });
    if (d_n_cells && n_rooms) HIP_TRY(hipMemsetAsync(d_n_cells, 0, sizeof(unsigned long long) * (size_t)n_rooms, s));
    hipLaunchKernelGGL(k_navg_finish, dim3(cdiv(HW, NAVR_T)), dim3(NAVR_T), 0, s, (int)HW, d_label, n_rooms ? d_n_cells : nullptr);
    HMSG_CHECK_LAUNCH();
}

struct NavdShort {
    bool doors = false, cells = false;
};
// D1 to D4 on the device images d_pass and d_label; the table's own arrays are the caller's (host or device).  Ends synchronised.
NavdShort navd_doors_dev(hipStream_t s, const std::string& f, int rows, int cols, const unsigned char* d_pass, const int* d_label, int n_rooms,
                         hmsg_nav_door_table* out) {
    const size_t HW = (size_t)rows * cols;
    const dim3 gi(cdiv(HW, NAVR_T)), b(NAVR_T);
    NavdShort too_short;
    DevBuf<int> own_other, parent, bad, cell, root_pq, d_root, slot, own_rc;
    DevBuf<unsigned> flag, scan_tmp, n_roots, d_seg;
    int* d_other = stage_out(own_other, out->other, HW);
    if (!d_other) own_other.alloc(HW), d_other = own_other.p;
    flag.alloc(HW), parent.alloc(HW), bad.alloc(1);
    bad.zero(s);
    hipLaunchKernelGGL(k_navd_threshold, gi, b, 0, s, rows, cols, d_pass, d_label, n_rooms, d_other, flag.p, parent.p, bad.p);
    HMSG_CHECK_LAUNCH();
    unsigned long long n_thr = 0;
    hmsg_scan_u32(flag.p, flag.p, HW, s, scan_tmp, &n_thr);                 // (read-back 1: the threshold cells, and the labels' check)
    int h_bad = 0;
    HIP_TRY(hipMemcpyAsync(&h_bad, bad.p, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    HMSG_REQUIRE(!h_bad, HMSG_ERR_INVALID, f + ": a label lies outside [-1, n_rooms)");
    if (out->other) unstage_out(out->other, d_other, HW, s);
    const int n = (int)n_thr;
    std::vector<int32_t> pq;                                                // the doors in D4's order: root, p, q
    std::vector<long long> off(1, 0);
    unsigned n_doors = 0;
    SortBufs sb;
    if (n > 0) {
        const dim3 gn(cdiv((size_t)n, NAVR_T));
        cell.alloc((size_t)n), root_pq.alloc((size_t)n * 3), n_roots.alloc(1);
        n_roots.zero(s);
        hipLaunchKernelGGL(k_navd_compact, gi, b, 0, s, (int)HW, (const unsigned*)flag.p, (const int*)d_other, cell.p);
        hipLaunchKernelGGL(k_navd_hook, gn, b, 0, s, rows, cols, n, (const int*)cell.p, d_label, (const int*)d_other, parent.p);
        hipLaunchKernelGGL(k_navd_flatten, gn, b, 0, s, n, (const int*)cell.p, parent.p);
        hipLaunchKernelGGL(k_navd_roots, gn, b, 0, s, n, (const int*)cell.p, (const int*)parent.p, d_label, (const int*)d_other, n_roots.p, root_pq.p);
        HMSG_CHECK_LAUNCH();
        HIP_TRY(hipMemcpyAsync(&n_doors, n_roots.p, 4, hipMemcpyDeviceToHost, s));          // (read-back 2: the doors)
        HIP_TRY(hipStreamSynchronize(s));
        std::vector<int32_t> raw((size_t)n_doors * 3);
        HIP_TRY(hipMemcpyAsync(raw.data(), root_pq.p, raw.size() * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        std::vector<int> order(n_doors);
        for (unsigned k = 0; k < n_doors; ++k) order[k] = (int)k;
        std::sort(order.begin(), order.end(), [&](int x, int y) {
            const int32_t *a = &raw[(size_t)x * 3], *c = &raw[(size_t)y * 3];
            return a[1] != c[1] ? a[1] < c[1] : (a[2] != c[2] ? a[2] < c[2] : a[0] < c[0]);
        });
        pq.resize(raw.size());
        std::vector<int32_t> roots(n_doors);
        for (unsigned k = 0; k < n_doors; ++k) {
            for (int j = 0; j < 3; ++j) pq[(size_t)k * 3 + j] = raw[(size_t)order[k] * 3 + j];
            roots[k] = pq[(size_t)k * 3];
        }
        // the cells by (door, row-major index): a stable sort of the row-major list by door
        d_root.alloc(n_doors), slot.alloc(HW), d_seg.alloc((size_t)n_doors + 1);
        HIP_TRY(hipMemcpyAsync(d_root.p, roots.data(), (size_t)n_doors * 4, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_navd_slots, dim3(cdiv((size_t)n_doors, NAVR_T)), b, 0, s, (int)n_doors, (const int*)d_root.p, slot.p);
        sb.keys.alloc((size_t)n), sb.vals.alloc((size_t)n);
        hipLaunchKernelGGL(k_navd_keys, gn, b, 0, s, n, (const int*)cell.p, (const int*)parent.p, (const int*)slot.p, sb.keys.p, sb.vals.p);
        HMSG_CHECK_LAUNCH();
        hmsg_sort_pairs(sb, (size_t)n, bits_for(n_doors), s);
        hmsg_sort_segment_starts(sb.res_keys, (size_t)n, d_seg.p, n_doors, s);
        std::vector<unsigned> seg((size_t)n_doors + 1);
        HIP_TRY(hipMemcpyAsync(seg.data(), d_seg.p, seg.size() * 4, hipMemcpyDeviceToHost, s));         // (read-back 3: door_off)
        HIP_TRY(hipStreamSynchronize(s));
        off.assign(seg.begin(), seg.end());
    }
    out->n_doors = n_doors, out->n_door_cells = n;
    too_short.doors = (out->door_pair || out->door_off) && (long long)n_doors > out->door_capacity;
    too_short.cells = out->door_rc && (long long)n > out->cell_capacity;
    if (!too_short.doors) {
        if (out->door_off) write_out(out->door_off, off.data(), off.size() * 8);
        if (out->door_pair && n_doors) {
            std::vector<int32_t> pair((size_t)n_doors * 2);
            for (unsigned k = 0; k < n_doors; ++k) pair[(size_t)k * 2] = pq[(size_t)k * 3 + 1], pair[(size_t)k * 2 + 1] = pq[(size_t)k * 3 + 2];
            write_out(out->door_pair, pair.data(), pair.size() * 4);
        }
    }
    if (out->door_rc && n > 0 && !too_short.cells) {
        int* d_rc = stage_out(own_rc, out->door_rc, (size_t)n * 2);
        hipLaunchKernelGGL(k_navd_emit, dim3(cdiv((size_t)n, NAVR_T)), b, 0, s, n, cols, (const unsigned long long*)sb.res_vals, d_rc);
        HMSG_CHECK_LAUNCH();
        unstage_out(out->door_rc, d_rc, (size_t)n * 2, s);
    }
    if (out->adjacency && n_rooms) {
        std::vector<int32_t> adj((size_t)n_rooms * n_rooms, 0);
        for (unsigned k = 0; k < n_doors; ++k) {
            const size_t p = (size_t)pq[(size_t)k * 3 + 1], q = (size_t)pq[(size_t)k * 3 + 2];
            ++adj[p * n_rooms + q], ++adj[q * n_rooms + p];
        }
        write_out(out->adjacency, adj.data(), adj.size() * 4);
    }
    HIP_TRY(hipStreamSynchronize(s));
    return too_short;
}
void navd_check_table(const std::string& f, int32_t n_rooms, const hmsg_nav_door_table* out) {
    HMSG_REQUIRE(n_rooms >= 0, HMSG_ERR_INVALID, f + ": n_rooms < 0");
    HMSG_REQUIRE(out->door_capacity >= 0 && out->cell_capacity >= 0, HMSG_ERR_INVALID, f + ": door_capacity < 0 or cell_capacity < 0");
    HMSG_REQUIRE(!out->adjacency || n_rooms <= NAVG_MAX_ADJ_ROOMS, HMSG_ERR_UNSUPPORTED, f + ": adjacency with more than 4096 rooms");
}
[[noreturn]] void navd_throw_short(const std::string& f, const NavdShort& t, const hmsg_nav_door_table* out) {
    if (t.doors)
        throw hmsg_error{HMSG_ERR_INVALID, f + ": " + std::to_string(out->n_doors) + " doors, the table holds " + std::to_string(out->door_capacity) +
                                               " (the counts say what is needed)"};
    throw hmsg_error{HMSG_ERR_INVALID, f + ": " + std::to_string(out->n_door_cells) + " door cells, door_rc holds " + std::to_string(out->cell_capacity) +
                                           " (the counts say what is needed)"};
}
void navg_last_take() { navr_last_get(&g_navg_rounds, &g_navg_trips); }

}  // namespace

extern "C" int hmsg_nav_room_labels(int32_t device_id, int32_t rows, int32_t cols, const uint8_t* passable, const hmsg_route_params* prm,
                                    int32_t n_rooms, const int64_t* seed_off, const int32_t* seed_rc, int32_t* label, int32_t* dist,
                                    int64_t* n_cells) {
    if (!passable || !prm || !seed_off || !label) return HMSG_ERR_INVALID;
    return hmsg_boundary("hmsg_nav_room_labels", device_id, [&] {
        const std::string f = "hmsg_nav_room_labels";
        navr_check(rows, cols, *prm, f.c_str());
        NavgSeeds sd;
        navg_read_seeds(f, rows, cols, n_rooms, seed_off, seed_rc, sd);
        navr_last_reset();
        g_navg_rounds = g_navg_trips = 0;
        ScopedStream s(hipStreamNonBlocking);
        const size_t HW = (size_t)rows * cols;
        DevBuf<unsigned char> own_pass;
        DevBuf<int> own_label, own_dist;
        DevBuf<unsigned long long> d_cnt;
        const unsigned char* d_pass = stage_in(own_pass, passable, HW, s, Up::bounce);
        int* d_label = stage_out(own_label, label, HW);
        int* d_dist = stage_out(own_dist, dist, HW);
        if (n_cells) d_cnt.alloc((size_t)n_rooms);
        navg_labels_dev(s, rows, cols, d_pass, *prm, n_rooms, sd, d_label, d_dist, n_cells ? d_cnt.p : nullptr);
        unstage_out(label, d_label, HW, s);
        if (dist) unstage_out(dist, d_dist, HW, s);
        if (n_cells && n_rooms) copy_out(n_cells, d_cnt.p, (size_t)n_rooms * 8, s);
        HIP_TRY(hipStreamSynchronize(s));
        navg_last_take();
    });
}

extern "C" int hmsg_nav_doors(int32_t device_id, int32_t rows, int32_t cols, const uint8_t* passable, const int32_t* label, int32_t n_rooms,
                              hmsg_nav_door_table* out) {
    if (!passable || !label || !out) return HMSG_ERR_INVALID;
    return hmsg_boundary("hmsg_nav_doors", device_id, [&] {
        const std::string f = "hmsg_nav_doors";
        hmsg_route_params p;
        hmsg_route_default_params(&p);
        p.w_straight = p.w_diag = 1;                                    // (the shape's limits alone)
        navr_check(rows, cols, p, f.c_str());
        navd_check_table(f, n_rooms, out);
        out->n_doors = out->n_door_cells = 0;
        ScopedStream s(hipStreamNonBlocking);
        const size_t HW = (size_t)rows * cols;
        DevBuf<unsigned char> own_pass;
        DevBuf<int> own_label;
        const unsigned char* d_pass = stage_in(own_pass, passable, HW, s, Up::bounce);
        const int* d_label = stage_in(own_label, label, HW, s, Up::bounce);
        const NavdShort t = navd_doors_dev(s, f, rows, cols, d_pass, d_label, n_rooms, out);
        if (t.doors || t.cells) navd_throw_short(f, t, out);
    });
}

extern "C" int hmsg_nav_path_rooms(int32_t device_id, int32_t rows, int32_t cols, const int32_t* label, int64_t n_paths, const int64_t* path_off,
                                   const int32_t* path_rc, int64_t* leg_off, int32_t* leg_room, int64_t* leg_first, int64_t capacity,
                                   int64_t* n_needed) {
    if (!label || !path_off || !n_needed) return HMSG_ERR_INVALID;
    return hmsg_boundary("hmsg_nav_path_rooms", device_id, [&] {
        const std::string f = "hmsg_nav_path_rooms";
        hmsg_route_params p;
        hmsg_route_default_params(&p);
        p.w_straight = p.w_diag = 1;
        navr_check(rows, cols, p, f.c_str());
        HMSG_REQUIRE(n_paths >= 0 && capacity >= 0, HMSG_ERR_INVALID, f + ": n_paths < 0 or capacity < 0");
        *n_needed = 0;
        const size_t n = (size_t)n_paths, HW = (size_t)rows * cols;
        std::vector<long long> off(n + 1);
        read_in(off.data(), path_off, off.size() * 8);
        HMSG_REQUIRE(off[0] >= 0, HMSG_ERR_INVALID, f + ": path_off[0] < 0");
        for (size_t k = 0; k < n; ++k) HMSG_REQUIRE(off[k + 1] >= off[k], HMSG_ERR_INVALID, f + ": path_off decreases at path " + std::to_string(k));
        HMSG_REQUIRE(off[n] == off[0] || path_rc, HMSG_ERR_INVALID, f + ": path_rc is null");
        ScopedStream s(hipStreamNonBlocking);
        DevBuf<int> own_label, own_rc, own_room;
        DevBuf<long long> d_off, cnt, d_leg_off, own_first;
        const int* d_label = stage_in(own_label, label, HW, s, Up::bounce);
        const int* d_rc = off[n] ? stage_in(own_rc, path_rc, (size_t)off[n] * 2, s, Up::bounce) : nullptr;
        d_off.alloc(n + 1), cnt.alloc(std::max<size_t>(n, 1)), d_leg_off.alloc(n + 1);
        HIP_TRY(hipMemcpyAsync(d_off.p, off.data(), off.size() * 8, hipMemcpyHostToDevice, s));
        const dim3 grid(cdiv(std::max<size_t>(n, 1), NAVR_T)), b(NAVR_T);
        if (n)
            hipLaunchKernelGGL(k_navg_legs<false>, grid, b, 0, s, rows, cols, d_label, (long long)n, (const long long*)d_off.p, d_rc, cnt.p,
                               (const long long*)nullptr, (int*)nullptr, (long long*)nullptr);
        navr_scan_dev(s, (long long)n, cnt.p, d_leg_off.p);
        HMSG_CHECK_LAUNCH();
        long long total = 0;
        HIP_TRY(hipMemcpyAsync(&total, d_leg_off.p + n, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        *n_needed = total;
        if (leg_off) copy_out(leg_off, d_leg_off.p, (n + 1) * 8, s);
        const bool wanted = leg_room || leg_first, too_short = wanted && total > capacity;
        if (wanted && total && !too_short) {
            HMSG_REQUIRE(leg_room && leg_first, HMSG_ERR_INVALID, f + ": leg_room and leg_first come together");
            int* d_room = stage_out(own_room, leg_room, (size_t)total);
            long long* d_first = stage_out(own_first, (long long*)leg_first, (size_t)total);
            hipLaunchKernelGGL(k_navg_legs<true>, grid, b, 0, s, rows, cols, d_label, (long long)n, (const long long*)d_off.p, d_rc, (long long*)nullptr,
                               (const long long*)d_leg_off.p, d_room, d_first);
            HMSG_CHECK_LAUNCH();
            unstage_out(leg_room, d_room, (size_t)total, s);
            unstage_out((long long*)leg_first, (const long long*)d_first, (size_t)total, s);
        }
        HIP_TRY(hipStreamSynchronize(s));
        if (too_short)
            throw hmsg_error{HMSG_ERR_INVALID, f + ": " + std::to_string(total) + " legs, the lists hold " + std::to_string(capacity) +
                                                   " (the count says what is needed)"};
    });
}

// the composition, and only that: clearance -> passable (as hmsg_nav_route), the labels, the doors; nothing leaves the device between
extern "C" int hmsg_nav_room_doors(int32_t device_id, int32_t rows, int32_t cols, const uint8_t* main_free_map, const hmsg_route_params* prm,
                                   int32_t n_rooms, const int64_t* seed_off, const int32_t* seed_rc, int32_t* label, uint8_t* passable,
                                   hmsg_nav_door_table* out) {
    if (!main_free_map || !prm || !seed_off || !label || !out) return HMSG_ERR_INVALID;
    return hmsg_boundary("hmsg_nav_room_doors", device_id, [&] {
        const std::string f = "hmsg_nav_room_doors";
        navr_check(rows, cols, *prm, f.c_str());
        NavgSeeds sd;
        navg_read_seeds(f, rows, cols, n_rooms, seed_off, seed_rc, sd);
        navd_check_table(f, n_rooms, out);
        out->n_doors = out->n_door_cells = 0;
        navr_last_reset();
        g_navg_rounds = g_navg_trips = 0;
        ScopedStream s(hipStreamNonBlocking);
        const size_t HW = (size_t)rows * cols;
        DevBuf<unsigned char> own_mask, own_pass;
        DevBuf<int> own_label;
        const unsigned char* d_mask = stage_in(own_mask, main_free_map, HW, s, Up::bounce);
        unsigned char* d_pass = stage_out(own_pass, passable, HW);
        if (!d_pass) own_pass.alloc(HW), d_pass = own_pass.p;
        int* d_label = stage_out(own_label, label, HW);
        navr_passable_dev(s, rows, cols, d_mask, *prm, d_pass);
        navg_labels_dev(s, rows, cols, d_pass, *prm, n_rooms, sd, d_label, nullptr, nullptr);
        navg_last_take();
        const NavdShort t = navd_doors_dev(s, f, rows, cols, d_pass, d_label, n_rooms, out);
        unstage_out(label, d_label, HW, s);
        if (passable) unstage_out(passable, d_pass, HW, s);
        HIP_TRY(hipStreamSynchronize(s));
        if (t.doors || t.cells) navd_throw_short(f, t, out);
    });
}

extern "C" int hmsg_test_nav_rooms_last(int32_t* rounds, int32_t* round_trips) {
    if (rounds) *rounds = g_navg_rounds;
    if (round_trips) *round_trips = g_navg_trips;
    return HMSG_OK;
}
