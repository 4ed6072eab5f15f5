// The host's half of a sequential merge fold step, in plain C++17 (no HIP headers: tests/host_cpp builds it with g++).
//
//   * box_iou / box_mask / fold_pairs_reference: THE statement of which pairs of a fold step's list go to the overlap test and in
//     which order (merge_3d_masks, graph_utils.py:937-941, with the fold's shortcut: only pairs with a new or changed member).
//   * FoldPlan: the same list, produced in two parts.  While a step's DBSCAN batch runs, the host already knows the next list's
//     order (one output per component), every cloud the step leaves untouched, and the next frame's masks: the pairs among those
//     are enumerated then (plan_ahead), in the time the host would otherwise spin.  Once the results have arrived only the pairs
//     that involve an output of the batch are left (late), and the two parts are merged into exactly the reference's list.
//     The AABBs live in one SoA table that is kept in list order from step to step instead of being refilled from the clouds.
#pragma once

#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

#if defined(__HIPCC__)
#define HMSG_FOLD_HD __host__ __device__
#else
#define HMSG_FOLD_HD
#endif

// AABB IoU of two boxes (graph_utils.py:883-915), the ONE statement of it: the host's pair loops and the pair kernels of the
// hierarchical merge evaluate this function, in float64, without contraction (the library is built with -ffp-contract=off), so a
// pair is a candidate on the device exactly when it is one on the host.  The selections are written out as the comparisons
// std::max / std::min make, not as fmax / fmin.
HMSG_FOLD_HD inline double box_iou(const double* amn, const double* amx, const double* bmn, const double* bmx) {
    // boxes disjoint along an axis: overlap volume 0 -> IoU 0 (or 0/0): never > iou_thresh (>= 0 by contract)
    if (amx[0] <= bmn[0] || bmx[0] <= amn[0] || amx[1] <= bmn[1] || bmx[1] <= amn[1] || amx[2] <= bmn[2] || bmx[2] <= amn[2])
        return 0.0;
    double ov = 1, va = 1, vb = 1;
    for (int k = 0; k < 3; ++k) {
        const double omin = amn[k] < bmn[k] ? bmn[k] : amn[k], omax = bmx[k] < amx[k] ? bmx[k] : amx[k];
        const double d = omax - omin;
        ov *= d < 0.0 ? 0.0 : d;
        va *= amx[k] - amn[k];
        vb *= bmx[k] - bmn[k];
    }
    return ov / (va + vb - ov);   // 0/0 -> NaN -> comparison false, like numpy
}

// cm[j] = box j meets the query box q = {lo0, hi0, lo1, hi1, lo2, hi2} with positive extent on every axis
// (thousands of boxes per fresh cloud per step: compiled for AVX2 when the host has it)
#define HMSG_BOX_MASK_BODY                                                                                          \
    for (int j = 0; j < n; ++j)                                                                                     \
        cm[j] = (unsigned char)!((q[1] <= lo0[j]) | (hi0[j] <= q[0]) | (q[3] <= lo1[j]) | (hi1[j] <= q[2]) |        \
                                 (q[5] <= lo2[j]) | (hi2[j] <= q[4]));
#if !defined(__HIP_DEVICE_COMPILE__) && defined(__x86_64__)
__attribute__((target("avx2"))) inline void box_mask_avx2(int n, const double* lo0, const double* hi0, const double* lo1,
                                                          const double* hi1, const double* lo2, const double* hi2, const double* q,
                                                          unsigned char* cm) {
    HMSG_BOX_MASK_BODY
}
#endif
inline void box_mask(int n, const double* lo0, const double* hi0, const double* lo1, const double* hi1, const double* lo2,
                     const double* hi2, const double* q, unsigned char* cm) {
#if !defined(__HIP_DEVICE_COMPILE__) && defined(__x86_64__)
    static const bool have_avx2 = __builtin_cpu_supports("avx2");
    if (have_avx2) {
        box_mask_avx2(n, lo0, hi0, lo1, hi1, lo2, hi2, q, cm);
        return;
    }
#endif
    HMSG_BOX_MASK_BODY
}

typedef std::vector<std::pair<int, int>> FoldPairList;

// AABBs of a cloud list in SoA form (the reject test -- boxes disjoint on some axis -- is the hot loop), with the number of points
// and the fresh flag of every cloud.  An empty cloud is stored as (+1e300, -1e300): it never pairs.
struct FoldBoxTable {
    std::vector<double> lo[3], hi[3];
    std::vector<unsigned char> fresh;
    std::vector<int> np;
    int n = 0;
    void resize(int m) {
        for (int a = 0; a < 3; ++a) {
            lo[a].resize((size_t)m);
            hi[a].resize((size_t)m);
        }
        fresh.resize((size_t)m);
        np.resize((size_t)m);
        n = m;
    }
    void set(int i, const double* mn, const double* mx, int points, bool fr) {
        for (int a = 0; a < 3; ++a) {
            lo[a][(size_t)i] = points ? mn[a] : 1e300;
            hi[a][(size_t)i] = points ? mx[a] : -1e300;
        }
        np[(size_t)i] = points;
        fresh[(size_t)i] = fr ? 1 : 0;
    }
    void move(int dst, int src) {
        for (int a = 0; a < 3; ++a) {
            lo[a][(size_t)dst] = lo[a][(size_t)src];
            hi[a][(size_t)dst] = hi[a][(size_t)src];
        }
        np[(size_t)dst] = np[(size_t)src];
        fresh[(size_t)dst] = fresh[(size_t)src];
    }
    bool same(int i, const FoldBoxTable& o, int j) const {
        for (int a = 0; a < 3; ++a)
            if (lo[a][(size_t)i] != o.lo[a][(size_t)j] || hi[a][(size_t)i] != o.hi[a][(size_t)j]) return false;
        return np[(size_t)i] == o.np[(size_t)j] && fresh[(size_t)i] == o.fresh[(size_t)j];
    }
    double iou(int i, int j) const {
        const double amn[3] = {lo[0][(size_t)i], lo[1][(size_t)i], lo[2][(size_t)i]}, amx[3] = {hi[0][(size_t)i], hi[1][(size_t)i], hi[2][(size_t)i]};
        const double bmn[3] = {lo[0][(size_t)j], lo[1][(size_t)j], lo[2][(size_t)j]}, bmx[3] = {hi[0][(size_t)j], hi[1][(size_t)j], hi[2][(size_t)j]};
        return box_iou(amn, amx, bmn, bmx);
    }
};

// (buffers of the enumerators, kept between steps)
struct FoldPairScratch {
    std::vector<double> slo[3], shi[3];
    std::vector<unsigned char> cand;
    std::vector<int> sub, from;
};

// The pairs enumerated FROM the clouds from[0 .. nfrom) (ascending, each with points): cloud i's partners are the clouds j != i
// in ascending j whose box has an IoU above the threshold with i's, but for the fresh clouds in front of i (those enumerate the
// pair themselves); a pair is written (lower index, higher index).  from_off (optional): from_off[k] = first pair of from[k],
// from_off[nfrom] = the number of pairs.
// The clouds enumerated from sit in the camera's view while the list holds the whole scene: ONE pass keeps the clouds whose box
// meets the common box of `from`, the per-cloud passes then run over those (a tenth of the list at a 1000-frame scene).
inline void fold_pairs_from(const FoldBoxTable& t, const int* from, int nfrom, double iou_thresh, FoldPairScratch& s, FoldPairList& pairs,
                            std::vector<int>* from_off = nullptr) {
    const int n = t.n;
    if (from_off) from_off->assign((size_t)nfrom + 1, (int)pairs.size());
    if (nfrom == 0) return;
    double u[6] = {1e300, -1e300, 1e300, -1e300, 1e300, -1e300};
    for (int k = 0; k < nfrom; ++k)
        for (int a = 0; a < 3; ++a) {
            u[2 * a] = std::min(u[2 * a], t.lo[a][(size_t)from[k]]);
            u[2 * a + 1] = std::max(u[2 * a + 1], t.hi[a][(size_t)from[k]]);
        }
    s.cand.assign((size_t)n + 8, 0);
    box_mask(n, t.lo[0].data(), t.hi[0].data(), t.lo[1].data(), t.hi[1].data(), t.lo[2].data(), t.hi[2].data(), u, s.cand.data());
    s.sub.clear();
    for (int j = 0; j < n; ++j)
        if (s.cand[(size_t)j]) s.sub.push_back(j);
    const int m = (int)s.sub.size();
    for (int a = 0; a < 3; ++a) {
        s.slo[a].resize((size_t)m);
        s.shi[a].resize((size_t)m);
        for (int q = 0; q < m; ++q) {
            s.slo[a][(size_t)q] = t.lo[a][(size_t)s.sub[(size_t)q]];
            s.shi[a][(size_t)q] = t.hi[a][(size_t)s.sub[(size_t)q]];
        }
    }
    s.cand.assign((size_t)m + 8, 0);
    for (int k = 0; k < nfrom; ++k) {
        const int i = from[k];
        if (from_off) (*from_off)[(size_t)k] = (int)pairs.size();
        // branch-free mask pass (vectorised), then a sparse walk over the few survivors
        unsigned char* cm = s.cand.data();
        const double q[6] = {t.lo[0][(size_t)i], t.hi[0][(size_t)i], t.lo[1][(size_t)i], t.hi[1][(size_t)i], t.lo[2][(size_t)i], t.hi[2][(size_t)i]};
        box_mask(m, s.slo[0].data(), s.shi[0].data(), s.slo[1].data(), s.shi[1].data(), s.slo[2].data(), s.shi[2].data(), q, cm);
        for (int j0 = 0; j0 < m; j0 += 8) {
            unsigned long long w;
            std::memcpy(&w, cm + j0, 8);               // cand is padded to a multiple of 8
            if (!w) continue;
            for (int jq = j0; jq < std::min(j0 + 8, m); ++jq) {
                const int j = s.sub[(size_t)jq];
                if (!cm[jq] || j == i || (t.fresh[(size_t)j] && j < i)) continue;
                if (t.np[(size_t)i] == 0 || t.np[(size_t)j] == 0) continue;   // find_overlapping_ratio_faiss returns 0 for empty clouds
                if (!(t.iou(i, j) > iou_thresh)) continue;
                pairs.emplace_back(std::min(i, j), std::max(i, j));
            }
        }
    }
    if (from_off) (*from_off)[(size_t)nfrom] = (int)pairs.size();
}

// The reference enumerator: every pair of the list with a fresh member, enumerated from the fresh clouds in list order.
inline void fold_pairs_reference(const FoldBoxTable& t, double iou_thresh, FoldPairScratch& s, FoldPairList& pairs) {
    s.from.clear();
    for (int i = 0; i < t.n; ++i)
        if (t.fresh[(size_t)i] && t.np[(size_t)i]) s.from.push_back(i);
    fold_pairs_from(t, s.from.data(), (int)s.from.size(), iou_thresh, s, pairs);
}

// the AABB table of a cloud list (anything with mn[3], mx[3], n, fresh), entries from `first` on
template <class List>
inline void fold_fill_boxes(const List& L, int first, FoldBoxTable& t) {
    t.resize((int)L.size());
    for (int j = first; j < (int)L.size(); ++j) t.set(j, L[(size_t)j].mn, L[(size_t)j].mx, L[(size_t)j].n, L[(size_t)j].fresh);
}

// The cloud list updated where it is, like the table (FoldPlan::advance): a component the step leaves untouched -- one cloud,
// at `src` -- takes its place c <= src in the next list and is from now on neither fresh nor in need of a DBSCAN.
template <class List>
inline void fold_keep_untouched(List& L, size_t c, size_t src) {
    if (src != c) L[c] = L[src];
    L[c].fresh = false;
    L[c].fixed = true;
}

// One fold step after the other:
//     sync / pairs            the list of this step, [what the last step put out | this frame's masks]
//     advance                 the step's components are known: the table becomes the next list's, outputs of the batch pending
//     append + plan_ahead     (when the next frame's masks are known) their pairs among themselves and with the untouched clouds
//     resolve                 the results have arrived: box, points and changed flag of every pending output
// and pairs() of the next step then enumerates only from / against the resolved outputs and merges.
struct FoldPlan {
    FoldBoxTable tab;
    bool synced = false;            // tab describes the list the last step put out (and, ahead == true, the next frame's masks behind it)
    bool ahead = false;             // the masks behind the outputs are in the table and `apairs` holds their pairs
    int n_out = 0;                  // clouds the last step put out
    std::vector<int> pending;       // outputs of the last step's batch (list positions, ascending)
    int n_resolved = 0;
    FoldPairList apairs;            // pairs enumerated from the masks ahead of the results ...
    std::vector<int> aoff;          // ... mask k's at apairs[aoff[k] .. aoff[k + 1])
    FoldPairScratch scratch;
    std::vector<int> unchanged;     // (late: the resolved outputs that came through unchanged and have points)
    double n_ahead_steps = 0, n_late_only_steps = 0;      // (statistics)

    void reset() {
        synced = ahead = false;
        tab.n = 0;
        n_out = 0;
        pending.clear();
        n_resolved = 0;
    }
    // forget the masks taken in ahead (the list they were meant for will not come as planned)
    void drop_ahead() {
        if (!ahead) return;
        ahead = false;
        tab.resize(n_out);
    }
    // The step's components (CSR, in order of their lowest member; seg_of_comp[c] < 0: left untouched): the table becomes the
    // next list's -- component c's output takes place c.  c <= the lowest member of component c, and every member of a later
    // component lies behind it, so the stable compaction runs in place.
    void advance(const int* comp_off, const int* comp_mem, int nc, const int* seg_of_comp) {
        pending.clear();
        n_resolved = 0;
        static const double z[3] = {0, 0, 0};
        for (int c = 0; c < nc; ++c) {
            if (seg_of_comp[c] < 0) {
                const int src = comp_mem[comp_off[c]];
                if (src != c) tab.move(c, src);
                tab.fresh[(size_t)c] = 0;
            } else {
                tab.set(c, z, z, 0, false);         // (pairs with nothing until it is resolved)
                pending.push_back(c);
            }
        }
        tab.resize(nc);
        n_out = nc;
        synced = true;
        ahead = false;
    }
    // a mask of the next frame (fresh, behind the outputs)
    void append(const double* mn, const double* mx, int points) {
        tab.resize(tab.n + 1);
        tab.set(tab.n - 1, mn, mx, points, true);
    }
    // the pairs of the masks appended since advance(), among themselves and with the untouched clouds
    void plan_ahead(double iou_thresh) {
        scratch.from.clear();
        for (int i = n_out; i < tab.n; ++i) scratch.from.push_back(i);
        apairs.clear();
        // (a mask without points enumerates nothing, but keeps its slot in aoff)
        fold_pairs_from(tab, scratch.from.data(), (int)scratch.from.size(), iou_thresh, scratch, apairs, &aoff);
        ahead = true;
    }
    void resolve(int c, const double* mn, const double* mx, int points, bool fr) {
        tab.set(c, mn, mx, points, fr);
        ++n_resolved;
    }
    bool resolved() const { return n_resolved == (int)pending.size(); }
    // The pairs of the step that folds L = [what the last step put out | this frame's masks]: what is left to enumerate once the
    // last step's results are known, merged with what was enumerated ahead; or, when nothing was (first step, the frame was not
    // there then, drop_ahead), the reference enumerator on the kept table with this frame's masks entered behind it.
    template <class List>
    void step_pairs(const List& L, double iou_thresh, FoldPairList& pairs) {
        const int n = (int)L.size();
        if (synced && ahead && tab.n == n && resolved()) {
            pairs_late(iou_thresh, pairs);
            n_ahead_steps += 1;
            return;
        }
        const bool keep = synced && !ahead && resolved() && tab.n <= n;
        fold_fill_boxes(L, keep ? tab.n : 0, tab);
        fold_pairs_reference(tab, iou_thresh, scratch, pairs);
        n_late_only_steps += 1;
    }
    // The step's pair list from the two parts, ahead == true and every pending output resolved:
    //   1. the pairs enumerated from the outputs that changed (fresh), ascending -- they come in front of every mask;
    //   2. mask by mask, its pairs from plan_ahead with the outputs that came through unchanged (not fresh: partners of the mask,
    //      in front of it) merged in by list position.
    void pairs_late(double iou_thresh, FoldPairList& pairs) {
        scratch.from.clear();
        unchanged.clear();
        for (int c : pending) {
            if (tab.np[(size_t)c] == 0) continue;
            (tab.fresh[(size_t)c] ? scratch.from : unchanged).push_back(c);
        }
        fold_pairs_from(tab, scratch.from.data(), (int)scratch.from.size(), iou_thresh, scratch, pairs);
        const int nm = tab.n - n_out;
        if (unchanged.empty()) {
            pairs.insert(pairs.end(), apairs.begin(), apairs.end());
            return;
        }
        for (int k = 0; k < nm; ++k) {
            const int i = n_out + k;
            size_t pa = (size_t)aoff[(size_t)k];
            const size_t pe = (size_t)aoff[(size_t)k + 1];
            if (tab.np[(size_t)i])
                for (int u : unchanged) {
                    if (!(tab.iou(i, u) > iou_thresh)) continue;
                    while (pa < pe && apairs[pa].second == i && apairs[pa].first < u) pairs.push_back(apairs[pa++]);
                    pairs.emplace_back(u, i);
                }
            pairs.insert(pairs.end(), apairs.begin() + (long)pa, apairs.begin() + (long)pe);
        }
    }
};
