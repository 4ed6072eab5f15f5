// The host half of the navigation maps (hmsg_navmap.hip): which poses mark free space, and the disc drawn round each.  No HIP
// in here: tests/host_cpp/nav_host.cpp drives it stand-alone, plain and under the host sanitizers.
//
// Reference: NavigationGraph.get_poses_region (graph/navigation_graph.py:348-377):
//     clusters = DBSCAN(eps=0.1).fit(heights.reshape(-1, 1))            # min_samples = 5, the sample itself counted
//     labels, counts = np.unique(clusters.labels_, return_counts=True)  # noise (-1) is a label like any other
//     major = np.mean(heights[clusters.labels_ == labels[np.argmax(counts)]])
//     keep |h - major| < 0.1, then h < min(kept) + 0.1
//     cell = np.int32((xz - pcd_min[[0, 2]]) / cell_size)               # truncated toward zero
//     cv2.circle(poses_map, cell, int(radius / cell_size), 1, -1)
//
// sklearn's DBSCAN, restated for one dimension:
//   - q is a neighbour of p when (h_p - h_q)^2 <= eps^2 (the tree compares reduced distances);
//   - a core sample has at least min_samples neighbours, itself included;
//   - clusters are numbered in the order of their first core sample; a sample that is no core sample takes the lowest-numbered
//     cluster with a core sample among its neighbours (clusters are grown one after the other, and a labelled sample is never
//     relabelled); everything else is noise, -1.
// On sorted heights a neighbourhood is a contiguous window, so the whole of it is a sort and two sweeps.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <vector>

namespace nav_host {

// numpy's pairwise summation of a contiguous float64 array (numpy/core/src/umath/loops_utils.h.src: DOUBLE_pairwise_sum)
inline double np_sum(const double* a, size_t n) {
    if (n < 8) {
        double r = 0.0;
        for (size_t i = 0; i < n; ++i) r += a[i];
        return r;
    }
    if (n <= 128) {
        double r[8];
        for (int j = 0; j < 8; ++j) r[j] = a[j];
        size_t i = 8;
        for (; i + 8 <= n; i += 8)
            for (int j = 0; j < 8; ++j) r[j] += a[i + (size_t)j];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += a[i];
        return res;
    }
    size_t n2 = n / 2;
    n2 -= n2 % 8;
    return np_sum(a, n2) + np_sum(a + n2, n - n2);
}

inline bool all_finite(const double* h, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(h[i])) return false;
    return true;
}

// DBSCAN(eps, min_samples).fit(h.reshape(-1, 1)).labels_.  sklearn refuses a height that is not finite; here such input (or an
// eps that is) labels everything noise: with a NaN the order below is no order and no sample is its own neighbour.
inline std::vector<int32_t> dbscan_1d(const double* h, size_t n, double eps, int min_samples) {
    std::vector<int32_t> label(n, -1);
    if (!n || !all_finite(h, n) || !std::isfinite(eps) || eps < 0.0) return label;
    std::vector<size_t> order(n);
    std::iota(order.begin(), order.end(), (size_t)0);
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return h[a] < h[b]; });
    const double r2 = eps * eps;
    auto near = [&](size_t a, size_t b) {
        const double d = h[order[a]] - h[order[b]];
        return d * d <= r2;
    };
    // the window [lo[k], hi[k]) of sorted positions that are neighbours of position k
    std::vector<size_t> lo(n), hi(n);
    for (size_t k = 0, l = 0, r = 0; k < n; ++k) {
        while (!near(l, k)) ++l;
        if (r < k + 1) r = k + 1;
        while (r < n && near(r, k)) ++r;
        lo[k] = l, hi[k] = r;
    }
    std::vector<char> core(n);
    for (size_t k = 0; k < n; ++k) core[k] = (long long)(hi[k] - lo[k]) >= (long long)min_samples;
    // components of core samples: consecutive core positions join when they are neighbours (a core sample between two others that
    // are neighbours of each other is a neighbour of both).  comp_min = the component's lowest original index.
    std::vector<int> comp(n, -1);
    std::vector<size_t> comp_min;
    size_t prev = n;
    for (size_t k = 0; k < n; ++k) {
        if (!core[k]) continue;
        if (prev != n && near(prev, k)) {
            comp[k] = comp[prev];
            comp_min[(size_t)comp[k]] = std::min(comp_min[(size_t)comp[k]], order[k]);
        } else {
            comp[k] = (int)comp_min.size();
            comp_min.push_back(order[k]);
        }
        prev = k;
    }
    // numbered by their first core sample
    const size_t C = comp_min.size();
    std::vector<size_t> by_first(C);
    std::iota(by_first.begin(), by_first.end(), (size_t)0);
    std::sort(by_first.begin(), by_first.end(), [&](size_t a, size_t b) { return comp_min[a] < comp_min[b]; });
    std::vector<int32_t> number(C);
    for (size_t i = 0; i < C; ++i) number[by_first[i]] = (int32_t)i;
    // core positions in front of / behind every position, for the border samples
    std::vector<size_t> core_before(n, n), core_after(n, n);
    for (size_t k = 0, last = n; k < n; ++k) {
        if (core[k]) last = k;
        core_before[k] = last;
    }
    for (size_t k = n, last = n; k-- > 0;) {
        if (core[k]) last = k;
        core_after[k] = last;
    }
    for (size_t k = 0; k < n; ++k) {
        if (core[k]) {
            label[order[k]] = number[(size_t)comp[k]];
            continue;
        }
        // a border sample's core neighbours lie in at most two components: the nearest core sample on either side decides
        int32_t best = -1;
        const size_t b = core_before[k], a = core_after[k];
        if (b != n && b >= lo[k]) best = number[(size_t)comp[b]];
        if (a != n && a < hi[k]) {
            const int32_t v = number[(size_t)comp[a]];
            if (best < 0 || v < best) best = v;
        }
        label[order[k]] = best;
    }
    return label;
}

// the poses whose discs are drawn, as indices into h, in order (empty: none is left, which the reference answers by raising)
inline std::vector<int32_t> select_poses(const double* h, size_t n, double eps, int min_samples) {
    std::vector<int32_t> keep;
    if (!n || !all_finite(h, n)) return keep;          // (a height that is not finite: none; hmsg_nav_floor_maps refuses it by name)
    const std::vector<int32_t> label = dbscan_1d(h, n, eps, min_samples);
    // np.unique(return_counts) + argmax: the most frequent label, of equally frequent ones the smallest (noise first)
    int32_t max_label = -1;
    for (int32_t l : label) max_label = std::max(max_label, l);
    std::vector<size_t> count((size_t)max_label + 2, 0);
    for (int32_t l : label) ++count[(size_t)(l + 1)];
    size_t best = 0;
    for (size_t l = 1; l < count.size(); ++l)
        if (count[l] > count[best]) best = l;
    const int32_t major_label = (int32_t)best - 1;
    std::vector<double> sel;
    for (size_t i = 0; i < n; ++i)
        if (label[i] == major_label) sel.push_back(h[i]);
    const double major = np_sum(sel.data(), sel.size()) / (double)sel.size();
    std::vector<int32_t> first;
    for (size_t i = 0; i < n; ++i)
        if (std::fabs(h[i] - major) < eps) first.push_back((int32_t)i);
    if (first.empty()) return keep;
    double mn = h[(size_t)first[0]];
    for (int32_t i : first) mn = std::min(mn, h[(size_t)i]);
    const double limit = mn + eps;
    for (int32_t i : first)
        if (h[(size_t)i] < limit) keep.push_back(i);
    return keep;
}

// np.int32(v) of a float64: truncated toward zero; what does not fit is clamped (numpy leaves it undefined), far outside any grid
inline int32_t trunc_i32(double v) {
    if (!(v > -1073741824.0)) return -1073741824;      // (NaN too)
    if (v > 1073741824.0) return 1073741824;
    return (int32_t)v;
}

// OpenCV's filled circle (imgproc/src/drawing.cpp Circle, fill = true) of radius r as half-widths: row cy + d, |d| <= r, is filled
// over cx - half[|d|] .. cx + half[|d|].  The midpoint walk fills rows cy -/+ dy with half-width dx and rows cy -/+ dx with
// half-width dy; a row filled twice keeps the wider span.
inline std::vector<int32_t> circle_half_widths(int r) {
    std::vector<int32_t> half((size_t)std::max(r, 0) + 1, -1);
    if (r < 0) return half;
    int err = 0, dx = r, dy = 0, plus = 1, minus = 2 * r - 1;
    while (dx >= dy) {
        half[(size_t)dy] = std::max(half[(size_t)dy], (int32_t)dx);
        half[(size_t)dx] = std::max(half[(size_t)dx], (int32_t)dy);
        ++dy;
        err += plus;
        plus += 2;
        if (err > 0) {
            err -= minus;
            --dx;
            minus -= 2;
        }
    }
    return half;
}

}  // namespace nav_host
