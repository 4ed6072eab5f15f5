// Routes across storeys (include/hmsg.h, N9: hmsg_nav_seeded_fields, hmsg_nav_building_fields, hmsg_nav_building_paths,
// hmsg_nav_building_route): exact integer fields over several maps joined at a few cells, the goals' cells and the cells of the way
// through such joins.  The reference has no such stage; the rules B1 to B6 are this library's own and stand in the header.  The
// relaxation is hmsg_navroute.hip's (hmsg_navroute_dev.h: navr_relax_round, navr_relax): nothing of it is restated here.
//
// MI355X design notes
//  * Building field: a ROUND is one relaxation launch per storey (grid z = the starts) and one link launch (k_navb_links: a thread
//    per start, link and direction reads the field at one end and, where it is finite, atomicMin's value + cost into the other
//    end; a link that lowered its far end stamps that tile and the eight round it for the next round and counts as a change).  The
//    launches of a round follow each other on one stream, so the atomics of the link launch never meet the plain stores of a tile's
//    write-back.  Rounds are enqueued in N7's growing batches (4, 8, 16, 32), each round with a change counter of its own that the
//    tiles and the links share; the host reads the counters once per batch and stops when the last round of a batch changed
//    nothing.  No cap on rounds.  int32 minimum is monotone and idempotent, so the fixed point is the answer whatever the order:
//    a way that goes up, across and down again settles in as many rounds as it needs.  No float, and no atomic on a field but the
//    seeds' and the links'.
//  * Seeds (k_navb_seeds): costs go in by atomicMin (duplicate seeds on a cell race otherwise), then N7's relaxation as it is.
//  * n_reached (k_navb_count): a ballot per wave, the waves' counts meet in LDS, ONE atomic per workgroup that found anything.
//  * Paths (k_navb_walk): N7's two passes (count, one wave's scan, write from the back) with (storey, row, col) triples.  The link
//    list is consulted only where no neighbour continues the walk, which a way does once per link it crosses; it is scanned in
//    index order (B5's order is the list's, and a building has a handful of links).
#include "hmsg_navroute_dev.h"

#include <algorithm>
#include <climits>
#include <numeric>

#define NAVB_NONE HMSG_NAV_UNREACHED
#define NAVB_MAX_STOREYS 256
#define NAVB_MAX_LINKS (1 << 20)

struct NavbStorey {                      // a storey as the kernels see it
    int rows, cols, ntx, nty;
    const unsigned char* pass;
    int* field;                          // i32 [starts][rows][cols]
    int* act;                            // i32 [starts][tiles]
};

__device__ static const int NAVB_DR[8] = {-1, 1, 0, 0, -1, -1, 1, 1};      // R1's order
__device__ static const int NAVB_DC[8] = {0, 0, -1, 1, -1, 1, -1, 1};

// the tile of (r, c) and the eight round it run in round v (the neighbours too: a tile stamps them only when it CHANGES)
__device__ static inline void navb_stamp(int* __restrict__ a, int ntx, int nty, int r, int c, int v) {
    const int ty = r / NAVR_TILE, tx = c / NAVR_TILE;
    for (int y = max(ty - 1, 0); y <= min(ty + 1, nty - 1); ++y)
        for (int x = max(tx - 1, 0); x <= min(tx + 1, ntx - 1); ++x) a[y * ntx + x] = v;
}

// grid (seeds, fields)
__global__ __launch_bounds__(NAVR_T) void k_navb_seeds(int rows, int cols, const unsigned char* __restrict__ pass, const long long* __restrict__ off,
                                                       const int* __restrict__ rc, const int* __restrict__ cost, int* __restrict__ field,
                                                       int* __restrict__ act, int ntx, int nty) {
    const int f = blockIdx.y;
    const long long k = off[f] + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= off[f + 1]) return;
    const int r = rc[k * 2], c = rc[k * 2 + 1];
    if (r < 0 || r >= rows || c < 0 || c >= cols || cost[k] < 0) return;
    const size_t i = (size_t)r * cols + c;
    if (!pass[i]) return;
    atomicMin(&field[(size_t)f * rows * cols + i], cost[k]);
    navb_stamp(act + (size_t)f * ntx * nty, ntx, nty, r, c, 1);
}
// a thread per start: start i32 [n][3] (storey, row, col); a start on no passable cell of its image starts nothing
__global__ __launch_bounds__(NAVR_T) void k_navb_starts(const NavbStorey* __restrict__ st, int n_storeys, int n, const int* __restrict__ start) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int l = start[k * 3], r = start[k * 3 + 1], c = start[k * 3 + 2];
    if (l < 0 || l >= n_storeys) return;
    const NavbStorey S = st[l];
    if (r < 0 || r >= S.rows || c < 0 || c >= S.cols || !S.pass[(size_t)r * S.cols + c]) return;
    S.field[((size_t)k * S.rows + r) * S.cols + c] = 0;
    navb_stamp(S.act + (size_t)k * S.ntx * S.nty, S.ntx, S.nty, r, c, 1);
}
// a thread per (start, link, direction); links i32 [n_links][7], checked by the host
__global__ __launch_bounds__(NAVR_T) void k_navb_links(const NavbStorey* __restrict__ st, int n_links, const int* __restrict__ links, int n_starts,
                                                       int round, unsigned* __restrict__ changed) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)n_starts * n_links * 2) return;
    const int dir = (int)(t & 1), k = (int)((t >> 1) % n_links), s = (int)((t >> 1) / n_links);
    const int* L = links + (size_t)k * 7;
    const NavbStorey A = st[L[dir ? 3 : 0]], B = st[L[dir ? 0 : 3]];
    const size_t ia = (size_t)L[dir ? 4 : 1] * A.cols + L[dir ? 5 : 2], ib = (size_t)L[dir ? 1 : 4] * B.cols + L[dir ? 2 : 5];
    if (!A.pass[ia] || !B.pass[ib]) return;                               // (B2: the link does not exist)
    const int v = *(const volatile int*)(A.field + (size_t)s * A.rows * A.cols + ia);
    if (v == NAVB_NONE) return;
    // B6 bounds the field's values, not this sum: a link walked BACK from its far end offers at least twice its cost more than
    // the near end holds, and with a cost near 2^31 that no longer fits.  Such an offer never wins, so it is dropped here.
    const long long sum = (long long)v + L[6];
    if (sum >= (long long)NAVB_NONE) return;
    const int nv = (int)sum;
    if (atomicMin(B.field + (size_t)s * B.rows * B.cols + ib, nv) <= nv) return;
    navb_stamp(B.act + (size_t)s * B.ntx * B.nty, B.ntx, B.nty, L[dir ? 1 : 4], L[dir ? 2 : 5], round + 1);
    atomicAdd(changed, 1u);
}
// grid (cells, fields): out[field * stride] += finite cells; one atomic per workgroup
__global__ __launch_bounds__(NAVR_T) void k_navb_count(const int* __restrict__ field, int HW, unsigned long long* __restrict__ out, int stride) {
    __shared__ int s_n[NAVR_T / 64];
    const int i = blockIdx.x * blockDim.x + threadIdx.x, tid = threadIdx.x;
    const unsigned long long b = __ballot(i < HW && field[(size_t)blockIdx.y * HW + i] != NAVB_NONE);
    if ((tid & 63) == 0) s_n[tid >> 6] = __popcll(b);
    __syncthreads();
    if (tid == 0) {
        int n = 0;
        for (int w = 0; w < NAVR_T / 64; ++w) n += s_n[w];
        if (n) atomicAdd(&out[(size_t)blockIdx.y * stride], (unsigned long long)n);
    }
}
__global__ void k_navb_triple(int storey, const int* __restrict__ rc, int* __restrict__ out3) {
    if (threadIdx.x == 0 && blockIdx.x == 0) out3[0] = storey, out3[1] = rc[0], out3[2] = rc[1];
}
// the goals were snapped storey by storey in sorted order: goal perm[i] has storey[i], the cell cell_p[i] and d2_p[i]
__global__ __launch_bounds__(NAVR_T) void k_navb_goal_out(const NavbStorey* __restrict__ st, long long n, const long long* __restrict__ perm,
                                                          const int* __restrict__ storey, const int* __restrict__ cell_p,
                                                          const long long* __restrict__ d2_p, int* __restrict__ goal_cell,
                                                          long long* __restrict__ goal_d2, int* __restrict__ goal_dist) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long g = perm[i];
    const int l = storey[i], r = cell_p[i * 2], c = cell_p[i * 2 + 1];
    goal_cell[g * 3] = l, goal_cell[g * 3 + 1] = r, goal_cell[g * 3 + 2] = c;
    if (goal_d2) goal_d2[g] = d2_p[i];
    if (goal_dist) goal_dist[g] = r < 0 ? NAVB_NONE : st[l].field[(size_t)r * st[l].cols + c];
}

// B5, a lane per goal.  WRITE false: cnt[g] = cells of goal g's path (0: no path).  WRITE true: the triples, from the back, at
// off[g] .. off[g + 1].  The fields are those of ONE start.
template <bool WRITE>
__global__ __launch_bounds__(NAVR_T) void k_navb_walk(const NavbStorey* __restrict__ st, int n_storeys, int n_links, const int* __restrict__ links,
                                                      int w_straight, int w_diag, long long n, const int* __restrict__ goal,
                                                      long long* __restrict__ cnt, const long long* __restrict__ off, int* __restrict__ path) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    int l = goal[g * 3], r = goal[g * 3 + 1], c = goal[g * 3 + 2];
    long long count = 0, at = 0, first = 0;
    if (WRITE) {
        first = off[g], at = off[g + 1];
        if (at == first) return;
    }
    if (l >= 0 && l < n_storeys && r >= 0 && r < st[l].rows && c >= 0 && c < st[l].cols && st[l].pass[(size_t)r * st[l].cols + c] &&
        st[l].field[(size_t)r * st[l].cols + c] != NAVB_NONE) {
        long long v = st[l].field[(size_t)r * st[l].cols + c];
        count = 1;
        if (WRITE) --at, path[at * 3] = l, path[at * 3 + 1] = r, path[at * 3 + 2] = c;
        while (v != 0) {
            const NavbStorey S = st[l];
            bool stepped = false;
            for (int d = 0; d < 8 && !stepped; ++d) {
                const int nr = r + NAVB_DR[d], nc = c + NAVB_DC[d];
                if (nr < 0 || nr >= S.rows || nc < 0 || nc >= S.cols || !S.pass[(size_t)nr * S.cols + nc]) continue;
                if (d >= 4 && !(S.pass[(size_t)nr * S.cols + c] && S.pass[(size_t)r * S.cols + nc])) continue;
                const int fv = S.field[(size_t)nr * S.cols + nc];
                if (fv == NAVB_NONE || (long long)fv + (d < 4 ? w_straight : w_diag) != v) continue;
                r = nr, c = nc, v = fv, stepped = true;
            }
            for (int k = 0; k < n_links && !stepped; ++k) {
                const int* L = links + (size_t)k * 7;
                for (int dir = 0; dir < 2 && !stepped; ++dir) {          // dir 0: the walk a -> b, here is b
                    const int* H = L + (dir ? 0 : 3);
                    const int* O = L + (dir ? 3 : 0);
                    if (H[0] != l || H[1] != r || H[2] != c) continue;
                    const NavbStorey T = st[O[0]];
                    if (!T.pass[(size_t)O[1] * T.cols + O[2]]) continue;  // (here is passable: the walk stands on it)
                    const int fv = T.field[(size_t)O[1] * T.cols + O[2]];
                    if (fv == NAVB_NONE || (long long)fv + L[6] != v) continue;
                    l = O[0], r = O[1], c = O[2], v = fv, stepped = true;
                }
            }
            if (!stepped || (WRITE && at == first)) {
                count = 0;
                break;
            }
            ++count;
            if (WRITE) --at, path[at * 3] = l, path[at * 3 + 1] = r, path[at * 3 + 2] = c;
        }
    }
    if (!WRITE) cnt[g] = count;
}

namespace {
thread_local int g_navb_rounds = 0, g_navb_trips = 0;       // what hmsg_test_nav_building_last reports

struct Navb {                            // a building, checked: the shapes and the links on the host, the links on the device
    int n_storeys = 0, n_links = 0;
    std::vector<int> rows, cols, ntx, nty;
    std::vector<size_t> HW;
    std::vector<int32_t> links;
    DevBuf<int> d_links;
    int tiles(int l) const { return ntx[(size_t)l] * nty[(size_t)l]; }
};

// B6 for the building; the links are read (host or device memory) and go up once
void navb_check(const std::string& f, Navb& B, int32_t n_storeys, const int32_t* rows, const int32_t* cols, int32_t n_links, const int32_t* links,
                const hmsg_route_params& p, hipStream_t s) {
    HMSG_REQUIRE(n_storeys >= 1 && n_storeys <= NAVB_MAX_STOREYS, HMSG_ERR_INVALID, f + ": 1 <= n_storeys <= 256");
    HMSG_REQUIRE(n_links >= 0 && n_links < NAVB_MAX_LINKS, HMSG_ERR_INVALID, f + ": 0 <= n_links < 2^20");
    HMSG_REQUIRE(n_links == 0 || links, HMSG_ERR_INVALID, f + ": links is null");
    B.n_storeys = n_storeys, B.n_links = n_links;
    long long cells = 0;
    for (int32_t l = 0; l < n_storeys; ++l) {
        navr_check(rows[l], cols[l], p, f.c_str());
        B.rows.push_back(rows[l]), B.cols.push_back(cols[l]);
        B.ntx.push_back((int)cdiv((size_t)cols[l], NAVR_TILE)), B.nty.push_back((int)cdiv((size_t)rows[l], NAVR_TILE));
        B.HW.push_back((size_t)rows[l] * cols[l]);
        cells += (long long)rows[l] * cols[l];
    }
    B.links.resize((size_t)n_links * 7);
    if (n_links) read_in(B.links.data(), links, B.links.size() * 4);
    long long costs = 0;
    for (int32_t k = 0; k < n_links; ++k) {
        const int32_t* L = B.links.data() + (size_t)k * 7;
        const std::string which = f + ": link " + std::to_string(k);
        HMSG_REQUIRE(L[0] >= 0 && L[0] < n_storeys && L[3] >= 0 && L[3] < n_storeys, HMSG_ERR_INVALID, which + " names a storey out of range");
        HMSG_REQUIRE(L[1] >= 0 && L[1] < rows[L[0]] && L[2] >= 0 && L[2] < cols[L[0]] && L[4] >= 0 && L[4] < rows[L[3]] && L[5] >= 0 &&
                         L[5] < cols[L[3]],
                     HMSG_ERR_INVALID, which + " has an endpoint outside its image");
        HMSG_REQUIRE(L[6] >= 1, HMSG_ERR_INVALID, which + " has a cost < 1");
        costs += L[6];
    }
    HMSG_REQUIRE(cells * p.w_diag + costs < (1ll << 31), HMSG_ERR_UNSUPPORTED, f + ": w_diag * cells + the links' costs reaches 2^31");
    B.d_links.alloc(B.links.size());
    if (n_links) upload(B.d_links.p, B.links.data(), B.links.size() * 4, s, Up::direct);
}

void navb_storeys_up(hipStream_t s, const Navb& B, DevBuf<NavbStorey>& d_st, const std::vector<const unsigned char*>& d_pass,
                     const std::vector<int*>& d_field, const std::vector<int*>& d_act, std::vector<NavbStorey>& h_st) {
    h_st.resize((size_t)B.n_storeys);
    for (int l = 0; l < B.n_storeys; ++l)
        h_st[(size_t)l] = NavbStorey{B.rows[(size_t)l], B.cols[(size_t)l], B.ntx[(size_t)l], B.nty[(size_t)l], d_pass[(size_t)l], d_field[(size_t)l],
                                     d_act.empty() ? nullptr : d_act[(size_t)l]};
    HIP_TRY(hipMemcpyAsync(d_st.p, h_st.data(), sizeof(NavbStorey) * h_st.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));                                     // (h_st may change after this)
}

// B3: d_field[l] i32 [n_starts][rows_l][cols_l] for the starts d_start i32 [n_starts][3] (device); d_n_reached u64 [n_starts][n_storeys]
void navb_fields_dev(hipStream_t s, const Navb& B, const hmsg_route_params& p, const std::vector<const unsigned char*>& d_pass, long long n_all,
                     const int* d_start, const std::vector<int*>& d_field, unsigned long long* d_n_reached) {
    constexpr int MAXB = 32;
    const int nl = B.n_storeys;
    DevBuf<unsigned> chg;
    chg.alloc(MAXB);
    DevBuf<NavbStorey> d_st;
    d_st.alloc((size_t)nl);
    std::vector<DevBuf<int>> act((size_t)nl);
    std::vector<NavbStorey> h_st;
    unsigned h[MAXB];
    if (d_n_reached) HIP_TRY(hipMemsetAsync(d_n_reached, 0, sizeof(unsigned long long) * (size_t)n_all * nl, s));
    for (long long f0 = 0; f0 < n_all; f0 += 32768) {                     // (a grid's third dimension ends at 65535)
        const int nf = (int)std::min<long long>(32768, n_all - f0);
        std::vector<int*> fld((size_t)nl), a((size_t)nl);
        for (int l = 0; l < nl; ++l) {
            fld[(size_t)l] = d_field[(size_t)l] + (size_t)f0 * B.HW[(size_t)l];
            act[(size_t)l].alloc((size_t)nf * B.tiles(l));
            act[(size_t)l].zero(s);
            a[(size_t)l] = act[(size_t)l].p;
            navr_fill_dev(s, fld[(size_t)l], (long long)nf * (long long)B.HW[(size_t)l], (int)NAVB_NONE);
        }
        navb_storeys_up(s, B, d_st, d_pass, fld, a, h_st);
        hipLaunchKernelGGL(k_navb_starts, dim3(cdiv((size_t)nf, NAVR_T)), dim3(NAVR_T), 0, s, (const NavbStorey*)d_st.p, nl, nf, d_start + f0 * 3);
        HMSG_CHECK_LAUNCH();
        const long long link_threads = (long long)nf * B.n_links * 2;
        int round = 1, batch = 4;
        for (;;) {
            HIP_TRY(hipMemsetAsync(chg.p, 0, sizeof(unsigned) * (size_t)batch, s));
            for (int b = 0; b < batch; ++b) {
                for (int l = 0; l < nl; ++l)
                    navr_relax_round(s, B.rows[(size_t)l], B.cols[(size_t)l], d_pass[(size_t)l], p, true, nf, fld[(size_t)l], a[(size_t)l], round + b,
                                     chg.p + b);
                if (link_threads)
                    hipLaunchKernelGGL(k_navb_links, dim3(cdiv((size_t)link_threads, NAVR_T)), dim3(NAVR_T), 0, s, (const NavbStorey*)d_st.p,
                                       B.n_links, (const int*)B.d_links.p, nf, round + b, chg.p + b);
            }
            HMSG_CHECK_LAUNCH();
            HIP_TRY(hipMemcpyAsync(h, chg.p, sizeof(unsigned) * (size_t)batch, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            ++g_navb_trips;
            for (int b = 0; b < batch && h[b]; ++b) ++g_navb_rounds;
            if (!h[batch - 1]) break;
            round += batch;
            batch = std::min(batch * 2, MAXB);
        }
        if (d_n_reached)
            for (int l = 0; l < nl; ++l)
                hipLaunchKernelGGL(k_navb_count, dim3(cdiv(B.HW[(size_t)l], NAVR_T), (unsigned)nf), dim3(NAVR_T), 0, s, (const int*)fld[(size_t)l],
                                   (int)B.HW[(size_t)l], d_n_reached + (size_t)f0 * nl + l, nl);
        HMSG_CHECK_LAUNCH();
        HIP_TRY(hipStreamSynchronize(s));                                 // (act is given back before the next chunk takes it)
    }
}

// B5: path_off (device, [n + 1]) and the total; the list into path_src (caller memory, host or device) when it is wanted and fits
long long navb_paths_dev(hipStream_t s, const Navb& B, const NavbStorey* d_st, const hmsg_route_params& p, long long n, const int* d_goal,
                         long long* d_off, int32_t* path_src, long long capacity, bool* too_short) {
    DevBuf<long long> cnt;
    cnt.alloc((size_t)std::max<long long>(n, 1));
    const dim3 grid(cdiv((size_t)std::max<long long>(n, 1), NAVR_T));
    if (n > 0)
        hipLaunchKernelGGL(k_navb_walk<false>, grid, dim3(NAVR_T), 0, s, d_st, B.n_storeys, B.n_links, (const int*)B.d_links.p, p.w_straight, p.w_diag,
                           n, d_goal, cnt.p, (const long long*)nullptr, (int*)nullptr);
    navr_scan_dev(s, n, cnt.p, d_off);
    HMSG_CHECK_LAUNCH();
    long long total = 0;
    HIP_TRY(hipMemcpyAsync(&total, d_off + n, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *too_short = path_src && total > capacity;
    if (path_src && total && !*too_short) {
        DevBuf<int> own;
        int* p_src = stage_out(own, path_src, (size_t)total * 3);
        hipLaunchKernelGGL(k_navb_walk<true>, grid, dim3(NAVR_T), 0, s, d_st, B.n_storeys, B.n_links, (const int*)B.d_links.p, p.w_straight, p.w_diag,
                           n, d_goal, (long long*)nullptr, (const long long*)d_off, p_src);
        HMSG_CHECK_LAUNCH();
        unstage_out(path_src, p_src, (size_t)total * 3, s);
        HIP_TRY(hipStreamSynchronize(s));
    }
    return total;
}

// triples (storey, row, col) read by the host; every storey index must name a storey, and with `cells` every cell lie in its image
std::vector<int32_t> navb_read_triples(const std::string& f, const char* what, const Navb& B, long long n, const int32_t* src, bool cells) {
    std::vector<int32_t> t((size_t)n * 3);
    if (n) read_in(t.data(), src, t.size() * 4);
    for (long long k = 0; k < n; ++k) {
        const int32_t l = t[(size_t)k * 3], r = t[(size_t)k * 3 + 1], c = t[(size_t)k * 3 + 2];
        HMSG_REQUIRE(l >= 0 && l < B.n_storeys, HMSG_ERR_INVALID, f + ": " + what + " " + std::to_string(k) + " names a storey out of range");
        HMSG_REQUIRE(!cells || (r >= 0 && r < B.rows[(size_t)l] && c >= 0 && c < B.cols[(size_t)l]), HMSG_ERR_INVALID,
                     f + ": " + what + " " + std::to_string(k) + " lies outside its image");
    }
    return t;
}
}  // namespace

extern "C" int hmsg_nav_seeded_fields(int32_t device_id, int32_t rows, int32_t cols, const uint8_t* passable, const hmsg_route_params* prm,
                                      int32_t n_fields, const int64_t* seed_off, const int32_t* seed_rc, const int32_t* seed_cost, int32_t* fields,
                                      int64_t* n_reached) {
    if (!passable || !prm || !seed_off || !fields) return HMSG_ERR_INVALID;
    return hmsg_boundary("hmsg_nav_seeded_fields", device_id, [&] {
        const std::string f = "hmsg_nav_seeded_fields";
        navr_check(rows, cols, *prm, f.c_str());
        HMSG_REQUIRE(n_fields >= 0, HMSG_ERR_INVALID, f + ": n_fields < 0");
        navr_last_reset();
        if (n_fields == 0) return;
        std::vector<long long> off((size_t)n_fields + 1);
        read_in(off.data(), seed_off, off.size() * 8);
        long long most = 0;
        HMSG_REQUIRE(off[0] >= 0, HMSG_ERR_INVALID, f + ": seed_off[0] < 0");
        for (int32_t k = 0; k < n_fields; ++k) {
            HMSG_REQUIRE(off[(size_t)k + 1] >= off[(size_t)k], HMSG_ERR_INVALID, f + ": seed_off decreases at field " + std::to_string(k));
            most = std::max(most, off[(size_t)k + 1] - off[(size_t)k]);
        }
        const long long total = off[(size_t)n_fields];
        HMSG_REQUIRE(total == off[0] || (seed_rc && seed_cost), HMSG_ERR_INVALID, f + ": seed_rc or seed_cost is null");
        std::vector<int32_t> rc((size_t)total * 2), cost((size_t)total);
        if (total) read_in(rc.data(), seed_rc, rc.size() * 4), read_in(cost.data(), seed_cost, cost.size() * 4);
        const long long HWll = (long long)rows * cols;
        for (long long k = off[0]; k < total; ++k) {
            HMSG_REQUIRE(rc[(size_t)k * 2] >= 0 && rc[(size_t)k * 2] < rows && rc[(size_t)k * 2 + 1] >= 0 && rc[(size_t)k * 2 + 1] < cols,
                         HMSG_ERR_INVALID, f + ": seed " + std::to_string(k) + " lies outside the image");
            HMSG_REQUIRE(cost[(size_t)k] >= 0, HMSG_ERR_INVALID, f + ": seed " + std::to_string(k) + " has a cost < 0");
            HMSG_REQUIRE((long long)cost[(size_t)k] + HWll * prm->w_diag < (1ll << 31), HMSG_ERR_UNSUPPORTED,
                         f + ": seed cost + rows * cols * w_diag reaches 2^31");
        }
        ScopedStream s(hipStreamNonBlocking);
        const size_t HW = (size_t)rows * cols;
        const int ntx = (int)cdiv((size_t)cols, NAVR_TILE), nty = (int)cdiv((size_t)rows, NAVR_TILE);
        DevBuf<unsigned char> own_pass;
        DevBuf<long long> d_off;
        DevBuf<int> d_rc, d_cost, own_fields, act;
        DevBuf<unsigned long long> d_cnt;
        const unsigned char* d_pass = stage_in(own_pass, passable, HW, s, Up::bounce);
        d_off.alloc(off.size()), d_rc.alloc(rc.size()), d_cost.alloc(cost.size());
        HIP_TRY(hipMemcpyAsync(d_off.p, off.data(), off.size() * 8, hipMemcpyHostToDevice, s));
        if (total) upload(d_rc.p, rc.data(), rc.size() * 4, s, Up::bounce), upload(d_cost.p, cost.data(), cost.size() * 4, s, Up::bounce);
        int* d_fields = stage_out(own_fields, fields, HW * (size_t)n_fields);
        if (n_reached) d_cnt.alloc((size_t)n_fields), d_cnt.zero(s);
        for (long long f0 = 0; f0 < n_fields; f0 += 32768) {
            const int nf = (int)std::min<long long>(32768, n_fields - f0);
            int* fld = d_fields + (size_t)f0 * HW;
            act.alloc((size_t)nf * ntx * nty);
            act.zero(s);
            navr_fill_dev(s, fld, (long long)nf * (long long)HW, (int)NAVB_NONE);
            if (most > 0)
                hipLaunchKernelGGL(k_navb_seeds, dim3(cdiv((size_t)most, NAVR_T), (unsigned)nf), dim3(NAVR_T), 0, s, rows, cols, d_pass,
                                   (const long long*)d_off.p + f0, (const int*)d_rc.p, (const int*)d_cost.p, fld, act.p, ntx, nty);
            HMSG_CHECK_LAUNCH();
            navr_relax(s, rows, cols, d_pass, *prm, true, nf, fld, act.p);
            if (n_reached)
                hipLaunchKernelGGL(k_navb_count, dim3(cdiv(HW, NAVR_T), (unsigned)nf), dim3(NAVR_T), 0, s, (const int*)fld, (int)HW, d_cnt.p + f0, 1);
            HMSG_CHECK_LAUNCH();
        }
        unstage_out(fields, d_fields, HW * (size_t)n_fields, s);
        if (n_reached) copy_out(n_reached, d_cnt.p, (size_t)n_fields * 8, s);
        HIP_TRY(hipStreamSynchronize(s));
    });
}

extern "C" int hmsg_nav_building_fields(int32_t device_id, int32_t n_storeys, const int32_t* rows, const int32_t* cols,
                                        const uint8_t* const* passable, int32_t n_links, const int32_t* links, const hmsg_route_params* prm,
                                        int32_t n_starts, const int32_t* start, int32_t* const* fields, int64_t* n_reached) {
    if (!rows || !cols || !passable || !prm || !fields || (n_starts > 0 && !start)) return HMSG_ERR_INVALID;
    return hmsg_boundary("hmsg_nav_building_fields", device_id, [&] {
        const std::string f = "hmsg_nav_building_fields";
        ScopedStream s(hipStreamNonBlocking);
        Navb B;
        navb_check(f, B, n_storeys, rows, cols, n_links, links, *prm, s);
        HMSG_REQUIRE(n_starts >= 0, HMSG_ERR_INVALID, f + ": n_starts < 0");
        g_navb_rounds = g_navb_trips = 0;
        if (n_starts == 0) return;                                        // (nothing to write: an empty array's pointer may be null)
        for (int l = 0; l < n_storeys; ++l) HMSG_REQUIRE(passable[l] && fields[l], HMSG_ERR_INVALID, f + ": a storey's passable or fields is null");
        const std::vector<int32_t> h_start = navb_read_triples(f, "start", B, n_starts, start, true);
        const size_t nl = (size_t)n_storeys;
        std::vector<DevBuf<unsigned char>> own_pass(nl);
        std::vector<DevBuf<int>> own_fields(nl);
        DevBuf<int> d_start;
        DevBuf<unsigned long long> d_cnt;
        std::vector<const unsigned char*> d_pass(nl);
        std::vector<int*> d_field(nl);
        for (size_t l = 0; l < nl; ++l) {
            d_pass[l] = stage_in(own_pass[l], passable[l], B.HW[l], s, Up::bounce);
            d_field[l] = stage_out(own_fields[l], fields[l], B.HW[l] * (size_t)n_starts);
        }
        d_start.alloc(h_start.size());
        upload(d_start.p, h_start.data(), h_start.size() * 4, s, Up::direct);
        if (n_reached) d_cnt.alloc((size_t)n_starts * nl);
        navb_fields_dev(s, B, *prm, d_pass, n_starts, d_start.p, d_field, n_reached ? d_cnt.p : nullptr);
        for (size_t l = 0; l < nl; ++l) unstage_out(fields[l], d_field[l], B.HW[l] * (size_t)n_starts, s);
        if (n_reached) copy_out(n_reached, d_cnt.p, (size_t)n_starts * nl * 8, s);
        HIP_TRY(hipStreamSynchronize(s));
    });
}

extern "C" int hmsg_nav_building_paths(int32_t device_id, int32_t n_storeys, const int32_t* rows, const int32_t* cols,
                                       const uint8_t* const* passable, int32_t n_links, const int32_t* links, const hmsg_route_params* prm,
                                       const int32_t* const* fields, int64_t n_goals, const int32_t* goals, int64_t* path_off, int32_t* path_src,
                                       int64_t capacity, int64_t* n_needed) {
    if (!rows || !cols || !passable || !prm || !fields || !n_needed || (n_goals > 0 && !goals)) return HMSG_ERR_INVALID;
    return hmsg_boundary("hmsg_nav_building_paths", device_id, [&] {
        const std::string f = "hmsg_nav_building_paths";
        ScopedStream s(hipStreamNonBlocking);
        Navb B;
        navb_check(f, B, n_storeys, rows, cols, n_links, links, *prm, s);
        HMSG_REQUIRE(n_goals >= 0 && (!path_src || capacity >= 0), HMSG_ERR_INVALID, f + ": n_goals < 0 or capacity < 0");
        for (int l = 0; l < n_storeys; ++l) HMSG_REQUIRE(passable[l] && fields[l], HMSG_ERR_INVALID, f + ": a storey's passable or fields is null");
        *n_needed = 0;
        const std::vector<int32_t> h_goal = navb_read_triples(f, "goal", B, n_goals, goals, false);
        const size_t nl = (size_t)n_storeys;
        std::vector<DevBuf<unsigned char>> own_pass(nl);
        std::vector<DevBuf<int>> own_fields(nl);
        DevBuf<int> d_goal;
        DevBuf<long long> d_off;
        DevBuf<NavbStorey> d_st;
        std::vector<const unsigned char*> d_pass(nl);
        std::vector<int*> d_field(nl);
        for (size_t l = 0; l < nl; ++l) {
            d_pass[l] = stage_in(own_pass[l], passable[l], B.HW[l], s, Up::bounce);
            d_field[l] = const_cast<int*>(stage_in(own_fields[l], fields[l], B.HW[l], s, Up::bounce));      // (read only)
        }
        d_st.alloc(nl);
        std::vector<NavbStorey> h_st;
        navb_storeys_up(s, B, d_st, d_pass, d_field, {}, h_st);
        d_goal.alloc(h_goal.size());
        if (n_goals) upload(d_goal.p, h_goal.data(), h_goal.size() * 4, s, Up::bounce);
        d_off.alloc((size_t)n_goals + 1);
        bool too_short = false;
        const long long total = navb_paths_dev(s, B, d_st.p, *prm, n_goals, d_goal.p, d_off.p, path_src, capacity, &too_short);
        *n_needed = total;
        if (path_off) copy_out(path_off, d_off.p, ((size_t)n_goals + 1) * 8, s);
        HIP_TRY(hipStreamSynchronize(s));
        if (too_short) navr_throw_short(f.c_str(), total, capacity);
    });
}

// the composition, and only that: per storey clearance -> passable, the start snapped on its storey, B3 for it, B4 per goal, B5
extern "C" int hmsg_nav_building_route(int32_t device_id, int32_t n_storeys, const int32_t* rows, const int32_t* cols,
                                       const uint8_t* const* main_free_map, int32_t n_links, const int32_t* links, const hmsg_route_params* prm,
                                       const int32_t* start, int64_t n_goals, const int32_t* goals, hmsg_nav_building_routes* out) {
    if (!rows || !cols || !main_free_map || !prm || !start || !out || (n_goals > 0 && !goals)) return HMSG_ERR_INVALID;
    return hmsg_boundary("hmsg_nav_building_route", device_id, [&] {
        const std::string f = "hmsg_nav_building_route";
        ScopedStream s(hipStreamNonBlocking);
        Navb B;
        navb_check(f, B, n_storeys, rows, cols, n_links, links, *prm, s);
        HMSG_REQUIRE(n_goals >= 0 && (!out->path_src || out->path_capacity >= 0), HMSG_ERR_INVALID, f + ": n_goals < 0 or path_capacity < 0");
        for (int l = 0; l < n_storeys; ++l) HMSG_REQUIRE(main_free_map[l], HMSG_ERR_INVALID, f + ": a storey's main_free_map is null");
        out->n_path_cells = 0, out->start_d2 = -1, out->start_cell[0] = out->start_cell[1] = out->start_cell[2] = -1;
        g_navb_rounds = g_navb_trips = 0;
        navr_last_reset();
        const std::vector<int32_t> h_start = navb_read_triples(f, "start", B, 1, start, false);
        const std::vector<int32_t> h_goal = navb_read_triples(f, "goal", B, n_goals, goals, false);
        const size_t nl = (size_t)n_storeys, n = (size_t)n_goals;
        const int ls = h_start[0];
        // 1. passable, storey by storey
        std::vector<DevBuf<unsigned char>> own_mask(nl), own_pass(nl);
        std::vector<DevBuf<int>> own_field(nl);
        std::vector<const unsigned char*> d_pass(nl);
        std::vector<unsigned char*> d_pass_w(nl);
        std::vector<int*> d_field(nl);
        for (size_t l = 0; l < nl; ++l) {
            const unsigned char* d_mask = stage_in(own_mask[l], main_free_map[l], B.HW[l], s, Up::bounce);
            d_pass_w[l] = out->passable ? stage_out(own_pass[l], out->passable[l], B.HW[l]) : nullptr;
            if (!d_pass_w[l]) own_pass[l].alloc(B.HW[l]), d_pass_w[l] = own_pass[l].p;
            navr_passable_dev(s, B.rows[l], B.cols[l], d_mask, *prm, d_pass_w[l]);
            d_pass[l] = d_pass_w[l];
            d_field[l] = out->field ? stage_out(own_field[l], out->field[l], B.HW[l]) : nullptr;
            if (!d_field[l]) own_field[l].alloc(B.HW[l]), d_field[l] = own_field[l].p;
        }
        // 2. the start on its storey, 3. its building field
        DevBuf<int> d_start_rc, d_start_cell, d_start3;
        DevBuf<long long> d_start_d2;
        d_start_rc.alloc(2), d_start_cell.alloc(2), d_start3.alloc(3), d_start_d2.alloc(1);
        upload(d_start_rc.p, h_start.data() + 1, 8, s, Up::direct);
        navr_snap_dev(s, B.rows[(size_t)ls], B.cols[(size_t)ls], d_pass[(size_t)ls], nullptr, 1, d_start_rc.p, d_start_cell.p, d_start_d2.p);
        hipLaunchKernelGGL(k_navb_triple, dim3(1), dim3(64), 0, s, ls, (const int*)d_start_cell.p, d_start3.p);
        HMSG_CHECK_LAUNCH();
        navb_fields_dev(s, B, *prm, d_pass, 1, d_start3.p, d_field, nullptr);
        // 4. the goals among the reached cells of their storeys: sorted by storey, one snap call per storey that has goals
        DevBuf<NavbStorey> d_st;
        d_st.alloc(nl);
        std::vector<NavbStorey> h_st;
        navb_storeys_up(s, B, d_st, d_pass, d_field, {}, h_st);
        std::vector<long long> perm(n);
        std::iota(perm.begin(), perm.end(), 0ll);
        std::stable_sort(perm.begin(), perm.end(), [&](long long a, long long b) { return h_goal[(size_t)a * 3] < h_goal[(size_t)b * 3]; });
        std::vector<int32_t> h_rc(n * 2), h_storey(n);
        for (size_t i = 0; i < n; ++i) {
            const size_t g = (size_t)perm[i];
            h_storey[i] = h_goal[g * 3], h_rc[i * 2] = h_goal[g * 3 + 1], h_rc[i * 2 + 1] = h_goal[g * 3 + 2];
        }
        DevBuf<int> d_rc, d_storey, d_cell_p, own_cell, own_dist;
        DevBuf<long long> d_perm, d_d2_p, own_d2, d_off;
        d_rc.alloc(n * 2), d_storey.alloc(n), d_cell_p.alloc(n * 2), d_perm.alloc(n), d_d2_p.alloc(n);
        if (n) {
            upload(d_rc.p, h_rc.data(), n * 8, s, Up::bounce);
            upload(d_storey.p, h_storey.data(), n * 4, s, Up::bounce);
            upload(d_perm.p, perm.data(), n * 8, s, Up::bounce);
        }
        for (size_t a = 0; a < n;) {
            size_t b = a;
            while (b < n && h_storey[b] == h_storey[a]) ++b;
            const size_t l = (size_t)h_storey[a];
            navr_snap_dev(s, B.rows[l], B.cols[l], d_pass[l], d_field[l], (long long)(b - a), d_rc.p + a * 2, d_cell_p.p + a * 2, d_d2_p.p + a);
            a = b;
        }
        int* d_cell = stage_out(own_cell, out->goal_cell, n * 3);
        if (!d_cell) own_cell.alloc(n * 3), d_cell = own_cell.p;
        long long* d_d2 = stage_out(own_d2, (long long*)out->goal_d2, n);
        int* d_dist = stage_out(own_dist, out->goal_dist, n);
        if (n) {
            hipLaunchKernelGGL(k_navb_goal_out, dim3(cdiv(n, NAVR_T)), dim3(NAVR_T), 0, s, (const NavbStorey*)d_st.p, (long long)n,
                               (const long long*)d_perm.p, (const int*)d_storey.p, (const int*)d_cell_p.p, (const long long*)d_d2_p.p, d_cell, d_d2,
                               d_dist);
            HMSG_CHECK_LAUNCH();
        }
        // 5. the paths
        d_off.alloc(n + 1);
        bool too_short = false;
        const long long total = navb_paths_dev(s, B, d_st.p, *prm, n_goals, d_cell, d_off.p, out->path_src, out->path_capacity, &too_short);
        out->n_path_cells = total;
        if (out->path_off) copy_out(out->path_off, d_off.p, (n + 1) * 8, s);
        for (size_t l = 0; l < nl; ++l) {
            if (out->passable && out->passable[l]) unstage_out(out->passable[l], d_pass_w[l], B.HW[l], s);
            if (out->field && out->field[l]) unstage_out(out->field[l], d_field[l], B.HW[l], s);
        }
        if (out->goal_cell) unstage_out(out->goal_cell, d_cell, n * 3, s);
        if (out->goal_d2) unstage_out((long long*)out->goal_d2, (const long long*)d_d2, n, s);
        if (out->goal_dist) unstage_out(out->goal_dist, d_dist, n, s);
        long long h_d2 = -1;
        int h_cell[2] = {-1, -1};
        HIP_TRY(hipMemcpyAsync(h_cell, d_start_cell.p, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(&h_d2, d_start_d2.p, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        out->start_cell[0] = ls, out->start_cell[1] = h_cell[0], out->start_cell[2] = h_cell[1];
        out->start_d2 = h_d2;
        if (too_short) navr_throw_short(f.c_str(), total, out->path_capacity);
    });
}

extern "C" int hmsg_test_nav_building_last(int32_t* rounds, int32_t* round_trips) {
    if (rounds) *rounds = g_navb_rounds;
    if (round_trips) *round_trips = g_navb_trips;
    return HMSG_OK;
}
