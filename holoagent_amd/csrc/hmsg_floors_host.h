// hmsg_segment_floors (include/hmsg.h), the host half: from the height histogram of the re-sampled map to the storeys' slabs --
// Graph.segment_floors_manually (fsr_vln/memory/hmsg/graph/graph.py:645-741) restated.  No HIP in here:
// tests/host_cpp/floors_host.cpp drives this header alone, tests/test_floors_host.py compares it with scipy and numpy.
//
//   gaussian_filter1d_i64   scipy.ndimage.gaussian_filter1d on int64 counts (:645; int64 in -> int64 out, truncated)
//   percentile_linear       np.percentile(.., q), method "linear"
//   find_peaks              scipy.signal.find_peaks(x, distance, height) (:648-651)
//   counts_to_slabs         the three above, the 1-D DBSCAN(eps = 1, min_samples = 1) chaining of the peak heights and the
//                           reference's pick / adjust rules (:680-741)
//
// Two orders are this library's own definitions, because scipy and the reference leave them to numpy's default argsort (introsort
// or an AVX-512 sorting network, depending on the build and the CPU: not stable, so the answer among EQUAL values is not defined),
// and smoothed counts are small truncated integers, so equal peak heights are ordinary:
//   - find_peaks' distance rule walks the peaks from the highest to the lowest and removes the neighbours closer than
//     ceil(distance) of every peak still kept; among peaks of equal height the one at the HIGHER position goes first;
//   - the pick of a chain's highest peak(s), np.argsort(smooth[pk])[-take:], keeps among equal heights the HIGHER positions.
// Both are "a stable ascending sort of the heights, read from its end".  The Python mirror (holoagent_amd/graph.py) states the same.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

namespace floors_host {

// np.sum of a contiguous float64 array (pairwise_sum below its block size of 128: eight running sums)
// (a copy of np_sum_f64 of hmsg_common.h, which pulls in HIP and so cannot be included here: change both together)
inline double np_sum(const double* a, size_t n) {
    if (n < 8) {
        double r = 0.0;
        for (size_t i = 0; i < n; ++i) r += a[i];
        return r;
    }
    double r[8];
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    size_t i = 8;
    for (; i + 8 <= n; i += 8)
        for (int j = 0; j < 8; ++j) r[j] += a[i + (size_t)j];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
}

// scipy.ndimage.gaussian_filter1d(int64 counts, sigma): radius int(4 sigma + 0.5), weights exp(-x^2 / (2 sigma^2)) / sum,
// correlate1d with mode "reflect" (d c b a | a b c d; repeated when the padding is longer than the array), symmetric taps
// paired, result truncated to int64
inline std::vector<long long> gaussian_filter1d_i64(const std::vector<long long>& x, double sigma) {
    const int n = (int)x.size(), r = (int)(4.0 * sigma + 0.5);
    std::vector<double> w((size_t)(2 * r + 1));
    for (int i = -r; i <= r; ++i) w[(size_t)(i + r)] = std::exp(-0.5 / (sigma * sigma) * (double)(i * i));
    const double sum = np_sum(w.data(), w.size());
    for (auto& v : w) v /= sum;
    auto at = [&](int i) {
        if (n == 1) return (double)x[0];
        while (i < 0 || i >= n) i = i < 0 ? -i - 1 : 2 * n - 1 - i;
        return (double)x[(size_t)i];
    };
    std::vector<long long> out((size_t)n);
    for (int i = 0; i < n; ++i) {
        double acc = at(i) * w[(size_t)r];
        for (int j = -r; j < 0; ++j) acc += (at(i + j) + at(i - j)) * w[(size_t)(j + r)];
        out[(size_t)i] = (long long)acc;
    }
    return out;
}

// np.percentile(x, q) (method "linear"); x not empty
inline double percentile_linear(std::vector<long long> x, double q) {
    std::sort(x.begin(), x.end());
    const double quant = q / 100.0;
    // numpy's virtual index of the method: (n - 1) * quantile.  (n * q + (1 - q) - 1, its _compute_virtual_index(alpha = beta = 1),
    // is the same number on paper and a few 1e-14 off in floating point: a height that should be exactly an element of x -- the
    // smoothed counts are integers, and find_peaks keeps a peak AT the height -- would come out a hair above it.)
    const double virt = (double)(x.size() - 1) * quant;
    const double prev = std::floor(virt), gamma = virt - prev;
    const size_t i0 = (size_t)prev, i1 = std::min(i0 + 1, x.size() - 1);
    const double a = (double)x[i0], b = (double)x[i1], d = b - a;
    return gamma >= 0.5 ? b - d * (1.0 - gamma) : a + d * gamma;
}

// positions 0 .. m - 1 in ascending order of key(position), equal keys in ascending position: np.argsort(.., kind="stable")
template <class Key>
inline std::vector<int> stable_argsort(int m, Key key) {
    std::vector<int> order((size_t)m);
    for (int i = 0; i < m; ++i) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return key(a) < key(b); });
    return order;
}

// scipy.signal.find_peaks(x, distance, height): local maxima (plateau midpoints), height filter, then the distance rule by
// descending height -- equal heights: the higher position first (the header comment)
inline std::vector<int> find_peaks(const std::vector<long long>& x, double height, int distance) {
    const int n = (int)x.size();
    std::vector<int> peaks;
    for (int i = 1; i < n - 1; ++i) {
        if (x[(size_t)i - 1] < x[(size_t)i]) {
            int ahead = i + 1;
            while (ahead < n - 1 && x[(size_t)ahead] == x[(size_t)i]) ++ahead;
            if (x[(size_t)ahead] < x[(size_t)i]) {
                peaks.push_back((i + ahead - 1) / 2);
                i = ahead;
            }
        }
    }
    std::vector<int> kept;
    for (int p : peaks)
        if (height <= (double)x[(size_t)p]) kept.push_back(p);
    peaks.swap(kept);
    const int m = (int)peaks.size();
    const std::vector<int> order = stable_argsort(m, [&](int a) { return x[(size_t)peaks[(size_t)a]]; });
    std::vector<char> keep((size_t)m, 1);
    for (int i = m - 1; i >= 0; --i) {
        const int j = order[(size_t)i];
        if (!keep[(size_t)j]) continue;
        for (int k = j - 1; k >= 0 && peaks[(size_t)j] - peaks[(size_t)k] < distance; --k) keep[(size_t)k] = 0;
        for (int k = j + 1; k < m && peaks[(size_t)k] - peaks[(size_t)j] < distance; ++k) keep[(size_t)k] = 0;
    }
    std::vector<int> out;
    for (int i = 0; i < m; ++i)
        if (keep[(size_t)i]) out.push_back(peaks[(size_t)i]);
    return out;
}

struct Slabs {
    std::vector<long long> smooth;      // the filtered counts
    std::vector<int> peaks;             // find_peaks' answer, ascending
    std::vector<double> slabs;          // [n_floors][2]: y_lo, y_hi
};

// counts: np.histogram(y, bins = counts.size()) of heights between ymin and ymax (its edges: linspace(ymin, ymax, bins + 1)).
// counts not empty.
inline Slabs counts_to_slabs(const std::vector<long long>& counts, double ymin, double ymax) {
    Slabs R;
    const int bins = (int)counts.size();
    const double step = (ymax - ymin) / (double)bins;
    auto edge = [&](int j) { return j == bins ? ymax : (double)j * step + ymin; };
    // ---- peaks (:645-651)
    R.smooth = gaussian_filter1d_i64(counts, 2.0);
    const std::vector<long long>& smooth = R.smooth;
    R.peaks = find_peaks(smooth, percentile_linear(smooth, 90.0), (int)std::ceil(0.2 / 0.01));
    const std::vector<int>& peaks = R.peaks;
    const int np_ = (int)peaks.size();
    std::vector<double> locs((size_t)np_);
    for (int i = 0; i < np_; ++i) locs[(size_t)i] = edge(peaks[(size_t)i]);
    // ---- DBSCAN(eps = 1, min_samples = 1) on the peak heights = chains of gaps <= 1; sklearn numbers clusters by first
    // appearance (peaks come in ascending order, so that is the chain order) (:680-683)
    std::vector<int> label((size_t)np_, 0);
    for (int i = 1; i < np_; ++i) label[(size_t)i] = label[(size_t)i - 1] + (locs[(size_t)i] - locs[(size_t)i - 1] > 1.0 ? 1 : 0);
    const int n_lab = np_ ? label[(size_t)np_ - 1] + 1 : 0;
    // ---- per cluster the highest peak (first and last cluster) or the two highest (:690-713)
    std::vector<double> clustered;
    for (int c = 0; c < n_lab; ++c) {
        std::vector<int> pk;
        for (int i = 0; i < np_; ++i)
            if (label[(size_t)i] == c) pk.push_back(peaks[(size_t)i]);
        const int take = (c == 0 || c == n_lab - 1) ? 1 : 2;
        // np.argsort(smooth[pk])[-take:] -- among equal heights the higher positions are kept (numpy's default argsort defines no
        // order among them: the header comment)
        const std::vector<int> ord = stable_argsort((int)pk.size(), [&](int a) { return smooth[(size_t)pk[(size_t)a]]; });
        for (size_t i = pk.size() > (size_t)take ? pk.size() - (size_t)take : 0; i < pk.size(); ++i) clustered.push_back(edge(pk[(size_t)ord[i]]));
    }
    std::sort(clustered.begin(), clustered.end());
    // ---- a 2.5 m gap between picks gets a ceiling 0.2 m under the upper one (:716-727)
    std::vector<double> adj;
    for (size_t i = 0; i + 1 < clustered.size(); ++i) {
        adj.push_back(clustered[i]);
        if (clustered[i + 1] - clustered[i] >= 2.5) adj.push_back(clustered[i + 1] - 0.2);
    }
    if (!clustered.empty()) adj.push_back(clustered.back());
    std::vector<double>& slabs = R.slabs;
    for (size_t i = 0; i + 1 < adj.size(); ++i) {
        slabs.push_back(adj[i]);
        slabs.push_back(adj[i + 1]);
    }
    if (slabs.empty()) {
        slabs.push_back(ymin);
        slabs.push_back(ymax);
    }
    slabs[0] = (slabs[0] + ymin) / 2.0;          // (:735-741)
    slabs[slabs.size() - 1] = ymax;
    return R;
}

}  // namespace floors_host
