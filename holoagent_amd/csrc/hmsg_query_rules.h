// The rules of the coarse-to-fine query, stated once as device code: the room selection of query_hmsg_room and the exact top-k of
// query_hmsg_object.  hmsg_query.hip (one index) and hmsg_query_sharded.hip (tables that stay sharded) instantiate them over
// their own data, so the two paths agree by construction.
#pragma once
#include "hmsg_common.h"

#include <climits>

// ---- candidate order and the exact top-k ----
// A candidate is (score, key); key = (place in the query's room list, place in the room) is unique per candidate and orders ties
// as "room order, then node order" (hmsg_query.hip's header comment).  QKEY_NONE: no candidate.
#define QKEY_NONE LLONG_MAX
__device__ __forceinline__ long long qkey(int j, int place) { return ((long long)j << 32) | (long long)place; }
__device__ __forceinline__ int qkey_j(long long key) { return (int)(key >> 32); }
__device__ __forceinline__ int qkey_place(long long key) { return (int)(key & 0xffffffffll); }
// (score desc, key asc)
__device__ __forceinline__ bool better(double s1, long long k1, double s2, long long k2) { return s1 > s2 || (s1 == s2 && k1 < k2); }
// strictly after the previous pick (ls, lk) in that order; lk < 0: there is no previous pick
__device__ __forceinline__ bool after_pick(double ls, long long lk, double s, long long key) {
    return lk < 0 || s < ls || (s == ls && key > lk);
}
// whether the arg-max class (first maximum) of `node` over the C rows of Sq [C][N] is myq: the negative prompts' filter
__device__ __forceinline__ bool argmax_class_is(const double* __restrict__ Sq, long long N, int C, int node, int myq) {
    int cls = 0;
    double mx = Sq[node];
    for (int c = 1; c < C; ++c) {
        const double v = Sq[(size_t)c * N + node];
        if (v > mx) {
            mx = v;
            cls = c;
        }
    }
    return cls == myq;
}
// The best (s, key) over the NT threads of the workgroup, through LDS (sh_s, sh_k: NT / 2 entries each), to every thread.  The
// upper half hands its candidates to the lower half, which then halves itself; the order is total, so the result is exact.
template <int NT>
__device__ __forceinline__ void wg_arg_best(double& s, long long& key, double* sh_s, long long* sh_k) {
    const int tid = threadIdx.x;
    if (tid >= NT / 2) {
        sh_s[tid - NT / 2] = s;
        sh_k[tid - NT / 2] = key;
    }
    __syncthreads();
    if (tid < NT / 2) {
        if (better(s, key, sh_s[tid], sh_k[tid])) {
            sh_s[tid] = s;
            sh_k[tid] = key;
        }
    }
    __syncthreads();
    for (int o = NT / 4; o > 0; o >>= 1) {
        if (tid < o && better(sh_s[tid + o], sh_k[tid + o], sh_s[tid], sh_k[tid])) {
            sh_s[tid] = sh_s[tid + o];
            sh_k[tid] = sh_k[tid + o];
        }
        __syncthreads();
    }
    s = sh_s[0];
    key = sh_k[0];
    __syncthreads();
}
// k rounds of "the best candidate strictly after the previous pick": exact and deterministic (k is small).  scan(offer) walks
// this thread's candidates and calls offer(score, key) on each, which says whether the candidate is the thread's best so far;
// emit(round, score, key, mine) receives the workgroup's pick on every thread (key QKEY_NONE: none left; mine: it is this
// thread's candidate).
template <int NT, typename Scan, typename Emit>
__device__ __forceinline__ void pick_top_k(int k, double* sh_s, long long* sh_k, Scan&& scan, Emit&& emit) {
    double ls = 1e308;
    long long lk = -1;
    for (int round = 0; round < k; ++round) {
        double bs = -1e308;
        long long bk = QKEY_NONE;
        scan([&](double sc, long long key) {
            if (!after_pick(ls, lk, sc, key) || !better(sc, key, bs, bk)) return false;
            bs = sc;
            bk = key;
            return true;
        });
        const long long my_key = bk;
        wg_arg_best<NT>(bs, bk, sh_s, sh_k);
        emit(round, bs, bk, bk != QKEY_NONE && bk == my_key);
        ls = bs;                                    // (after "no candidate", (-1e308, QKEY_NONE), nothing follows)
        lk = bk;
    }
}

// ---- room selection ----
// query_hmsg_room (graph.py:3164-3272), one workgroup of 256 threads per query.  rooms_list = self.rooms (floor -1) or floors[f].rooms.
//   mode 1 (label, :3204-3232): similarity of the room text with every room NAME of the list; every room within 1e-3 of
//        the best one, in list order; the numbers returned are positions in rooms_list.
//   mode 2 / 3 (view embeddings, :3247-3272): per room the largest similarity over its view embeddings; rooms sorted by
//        it, descending (Python's sorted: stable, ties keep the list order); the first 5 (mode 2) or 10 (mode 3); the
//        numbers returned are int(room_id.split("_")[-1]) -- which the caller then uses as positions in rooms_list.
//   mode 0: no room stage (every room of the list, in order).
// The selected numbers go to sel[0 .. *nsel); the object stage searches rooms_list[number] in that order
// (query_hmsg_object :3099-3110); a number that is no position of rooms_list raises IndexError there: *err = 1.
// q_rooms [max_sel]: the room ids of those numbers for the object stage, -1 past *nsel.
// Src is the query's view of the room level:
//   int  L                 length of rooms_list (0 for a floor that does not exist)
//   bool bad_floor         the floor id is past the last floor
//   int    room_at(i)      room id of list entry i
//   double name_sim(i)     similarity of the room text with the name of entry i
//   double view_max(i)     largest similarity over the views of entry i (fmax chain from -1e308: -1e308 without views)
//   bool   has_views(i)
//   int    room_key(r)     int(room_id.split("_")[-1]) of room r
#define ROOM_SELECT_CAP 1024                         // rooms of one list the view modes can rank
template <typename Src>
__device__ __forceinline__ void room_select(const Src& src, int m, int max_sel, int* __restrict__ sel, int* __restrict__ nsel,
                                            int* __restrict__ q_rooms, int* __restrict__ err) {
    const int tid = threadIdx.x, L = src.L;
    __shared__ int s_bad;
    __shared__ double s_red[256];
    if (tid == 0) s_bad = src.bad_floor ? 1 : 0;
    __syncthreads();
    if (m == 1) {
        double best = -1e308;
        for (int i = tid; i < L; i += 256) best = fmax(best, src.name_sim(i));
        s_red[tid] = best;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) s_red[tid] = fmax(s_red[tid], s_red[tid + o]);
            __syncthreads();
        }
        best = s_red[0];
        if (tid == 0) {                                         // (a handful of rooms: in list order)
            int n = 0;
            for (int i = 0; i < L && n < max_sel; ++i)
                if (fabs(src.name_sim(i) - best) < 1e-3) sel[n++] = i;
            *nsel = n;
        }
    } else if (m == 2 || m == 3) {
        // per room: max over its views (np.argmax takes the first maximum; only the value matters here)
        __shared__ double s_max[ROOM_SELECT_CAP];
        __shared__ unsigned char s_taken[ROOM_SELECT_CAP];
        const int Lc = min(L, ROOM_SELECT_CAP);
        for (int i = tid; i < Lc; i += 256) {
            s_max[i] = src.view_max(i);
            s_taken[i] = 0;
            if (!src.has_views(i)) s_bad = 1;                   // np.stack([]) raises
        }
        __syncthreads();
        if (tid == 0) {
            if (L > Lc) s_bad = 1;
            // graph.py:3259-3264: `{int(room_id.split("_")[-1]): v for ... in sorted(...)}` -- rooms "0_2" and "1_2" (floor -1 on
            // a multi-storey graph) collapse into ONE key, which keeps the place of its first (best) occurrence; the first
            // 5 / 10 UNIQUE keys are returned (SURVEY hazard 11).
            const int want = m == 2 ? 5 : 10;
            int n = 0;
            for (int taken = 0; taken < Lc && n < want && n < max_sel; ++taken) {   // selection sort of the top few, first index wins ties
                int bi = -1;
                double bv = -1e308;
                for (int i = 0; i < Lc; ++i)
                    if (!s_taken[i] && (bi < 0 || s_max[i] > bv)) {
                        bi = i;
                        bv = s_max[i];
                    }
                s_taken[bi] = 1;
                const int key = src.room_key(src.room_at(bi));
                bool seen = false;
                for (int j = 0; j < n; ++j) seen = seen || sel[j] == key;
                if (!seen) sel[n++] = key;
            }
            *nsel = n;
        }
    } else if (tid == 0) {
        int n = 0;
        for (int i = 0; i < L && n < max_sel; ++i) sel[n++] = i;
        *nsel = n;
    }
    __syncthreads();
    // positions of rooms_list -> room ids for the object stage
    if (tid == 0) {
        const int n = *nsel;
        for (int j = 0; j < max_sel; ++j) {
            int r = -1;
            if (j < n) {
                const int pos = sel[j];
                if (pos < 0 || pos >= L) s_bad = 1;
                else r = src.room_at(pos);
            }
            q_rooms[j] = r;
        }
        *err = s_bad;
    }
}
