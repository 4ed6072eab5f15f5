// The numbers behind the evaluator's matrices (memory/hmsg/eval/hm3dsem_evaluator.py), restated in float64 in the reference's
// operation order: evaluate_floors (:193-263), the threshold sweep of evaluate_rooms / evaluate_objects (:364-383, :467-484),
// np.trapz, the hydra means (:343-356) and object_semantics_eval_tp_auc's accuracies once the ranks are known (:557-589).
// No HIP in here: tests/host_cpp/eval_metrics_host.cpp drives this header alone; hmsg_eval.hip puts the C ABI on top.
//
// What is restated LITERALLY, because it decides bits or values:
//   - np.linspace(0, 1, 11) is i * (1.0 / 10) for i < 10 and 1.0 at the end (0.30000000000000004 at i = 3);
//   - `rec_values.sort()` sorts the recalls ONLY, so np.trapz integrates the precisions in threshold order over the recalls in
//     ascending order, and the room dictionary's "recall@IoU=0.5" is entry 6 of the SORTED list;
//   - np.trapz is (diff(x) * (y[1:] + y[:-1]) / 2.0).sum(), and .sum() of a contiguous float64 array is numpy's pairwise sum:
//     eight running sums below 128 elements, combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), the rest added one by one; a plain
//     loop below 8 elements; halves (the first a multiple of 8) above 128;
//   - np.mean(box, axis=0) adds the eight vertices in order and divides by 8.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace eval_metrics {

enum { N_THRESH = 11 };

// numpy's pairwise summation of a contiguous float64 array (numpy/core/src/umath/loops_utils.h.src: DOUBLE_pairwise_sum)
inline double np_sum(const double* a, size_t n) {
    if (n < 8) {
        double res = 0.0;                     // (no term here is -0.0: x ascends and y >= 0, so the start's sign does not matter)
        for (size_t i = 0; i < n; ++i) res += a[i];
        return res;
    }
    if (n <= 128) {
        double r[8];
        for (int k = 0; k < 8; ++k) r[k] = a[k];
        size_t i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int k = 0; k < 8; ++k) r[k] += a[i + (size_t)k];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += a[i];
        return res;
    }
    size_t n2 = n / 2;
    n2 -= n2 % 8;
    return np_sum(a, n2) + np_sum(a + n2, n - n2);
}

// np.trapz(y, x) of n samples
inline double trapz(const double* y, const double* x, size_t n) {
    if (n < 2) return 0.0;
    std::vector<double> t(n - 1);
    for (size_t i = 0; i + 1 < n; ++i) t[i] = ((x[i + 1] - x[i]) * (y[i + 1] + y[i])) / 2.0;
    return np_sum(t.data(), n - 1);
}

struct Counts {
    int64_t tp = 0, fp = 0, fn = 0;          // tn is 0 throughout the reference
    double acc = 0.0, prec = 0.0, recall = 0.0;
};

// TP = sum(M[row, col] > t); FP = P - TP; FN = G - TP; the three ratios behind their `> 0` guards
inline Counts counts_at(const double* M, int64_t ld, const int32_t* row, const int32_t* col, int64_t n, int64_t P, int64_t G, double t) {
    Counts c;
    for (int64_t k = 0; k < n; ++k) c.tp += M[(int64_t)row[k] * ld + col[k]] > t ? 1 : 0;
    c.fp = P - c.tp;
    c.fn = G - c.tp;
    c.prec = (c.tp + c.fp) > 0 ? (double)c.tp / (double)(c.tp + c.fp) : 0.0;
    c.recall = (c.tp + c.fn) > 0 ? (double)c.tp / (double)(c.tp + c.fn) : 0.0;
    c.acc = (c.tp + c.fp + c.fn) > 0 ? (double)c.tp / (double)(c.tp + c.fp + c.fn) : 0.0;
    return c;
}

inline double linspace01(int i) { return i == N_THRESH - 1 ? 1.0 : (double)i * (1.0 / 10.0); }

struct Sweep {
    double acc[N_THRESH], prec[N_THRESH], rec_sorted[N_THRESH];
    int64_t tp[N_THRESH];
    double ap;
};

// M: [P][G] row-major; (row, col): the n assigned pairs
inline Sweep threshold_sweep(const double* M, const int32_t* row, const int32_t* col, int64_t n, int64_t P, int64_t G) {
    Sweep s;
    for (int i = 0; i < N_THRESH; ++i) {
        const Counts c = counts_at(M, G, row, col, n, P, G, linspace01(i));
        s.tp[i] = c.tp;
        s.acc[i] = c.acc;
        s.prec[i] = c.prec;
        s.rec_sorted[i] = c.recall;
    }
    std::sort(s.rec_sorted, s.rec_sorted + N_THRESH);
    s.ap = trapz(s.prec, s.rec_sorted, N_THRESH);
    return s;
}

// hydra_prec: mean over predicted rooms of the row maxima of over_pred; hydra_recall: mean over ground-truth rooms of the column
// maxima of over_gt (Python float sums starting at 0.0, in order).  P, G > 0.
inline void hydra_means(const double* over_pred, const double* over_gt, int64_t P, int64_t G, double* prec, double* recall) {
    double sp = 0.0, sr = 0.0;
    for (int64_t p = 0; p < P; ++p) {
        double m = over_pred[p * G];
        for (int64_t g = 1; g < G; ++g) m = std::max(m, over_pred[p * G + g]);
        sp += m;
    }
    for (int64_t g = 0; g < G; ++g) {
        double m = over_gt[g];
        for (int64_t p = 1; p < P; ++p) m = std::max(m, over_gt[p * G + g]);
        sr += m;
    }
    *prec = sp / (double)P;
    *recall = sr / (double)G;
}

// flattened, sorted, inner neighbours averaged pairwise: 2 F bounds -> F + 1
inline std::vector<double> storey_bounds(std::vector<double> b) {
    std::sort(b.begin(), b.end());
    std::vector<double> out;
    out.push_back(b.front());
    for (size_t i = 1; i + 1 < b.size(); i += 2) out.push_back((b[i] + b[i + 1]) / 2.0);
    out.push_back(b.back());
    return out;
}

// evaluate_floors.  verts: [Fp][8][3].  false: no floors on a side, or unequal counts (numpy raises in the reference)
inline bool floor_metrics(const double* gt_lower, const double* gt_upper, int64_t Fg, const double* verts, int64_t Fp, Counts* out) {
    if (Fg <= 0 || Fp <= 0 || Fg != Fp) return false;
    std::vector<double> g, p;
    for (int64_t f = 0; f < Fg; ++f) {
        g.push_back(gt_lower[f]);
        g.push_back(gt_upper[f]);
    }
    for (int64_t f = 0; f < Fp; ++f) {
        const double* v = verts + f * 24;
        double sum = v[1], mn = v[1], mx = v[1];
        for (int k = 1; k < 8; ++k) {
            const double y = v[k * 3 + 1];
            sum += y;
            mn = std::min(mn, y);
            mx = std::max(mx, y);
        }
        const double c = sum / 8.0, d = mx - mn;
        p.push_back(c - d / 2.0);
        p.push_back(c + d / 2.0);
    }
    g = storey_bounds(g);
    p = storey_bounds(p);
    Counts c;
    for (size_t i = 0; i < g.size(); ++i) c.tp += std::fabs(g[i] - p[i]) < 0.5 ? 1 : 0;
    c.fp = (int64_t)p.size() - c.tp;
    c.fn = (int64_t)g.size() - c.tp;
    c.prec = (c.tp + c.fp) > 0 ? (double)c.tp / (double)(c.tp + c.fp) : 0.0;
    c.recall = (c.tp + c.fn) > 0 ? (double)c.tp / (double)(c.tp + c.fn) : 0.0;
    c.acc = (c.tp + c.fp + c.fn) > 0 ? (double)c.tp / (double)(c.tp + c.fp + c.fn) : 0.0;
    *out = c;
    return true;
}

// top_k_acc[k] = (pairs with rank < k) / n  (k = 0 never succeeds; n > 0)
inline double top_k_acc(const int32_t* rank, int64_t n, int64_t k) {
    int64_t ok = 0;
    for (int64_t i = 0; i < n; ++i) ok += rank[i] < k ? 1 : 0;
    return (double)ok / (double)n;
}
// np.trapz(acc over k in range(0, C, 10), k / C)
inline double top_k_auc(const int32_t* rank, int64_t n, int64_t C) {
    std::vector<double> acc, x;
    for (int64_t k = 0; k < C; k += 10) {
        acc.push_back(top_k_acc(rank, n, k));
        x.push_back((double)k / (double)C);
    }
    return trapz(acc.data(), x.data(), acc.size());
}

// ---- utils/metric.py from a confusion matrix conf[gt][pred] (L x L, counts): pixel_accuracy (:5-36), mean_accuracy (:39-65),
// per_class_iou (:68-103), mean_iou (:106-140), frequency_weighted_iou (:143-179).  The reference works on float64 masks, so its
// n_ii, t_i, n_ij are float64 counts; `cl` is np.unique of the ground truth (mean_accuracy, pixel_accuracy) or the union with the
// prediction's (the IoUs); a skipped class leaves the 0 its list was made with, and np.sum adds the whole list pairwise.
struct SemsegScores {
    double miou = 0.0, fmiou = 0.0, acc = 0.0, macc = 0.0;
};
inline SemsegScores semseg_metrics(const int64_t* conf, int32_t L, const int32_t* ignore, int32_t n_ignore, double* per_class_iou) {
    std::vector<double> t((size_t)L, 0.0), p((size_t)L, 0.0);      // ground-truth points, predicted points per class
    double m = 0.0;
    for (int32_t g = 0; g < L; ++g)
        for (int32_t q = 0; q < L; ++q) {
            const double v = (double)conf[(size_t)g * L + q];
            t[(size_t)g] += v;
            p[(size_t)q] += v;
            m += v;
        }
    auto ignored = [&](int32_t c) {
        for (int32_t k = 0; k < n_ignore; ++k)
            if (ignore[k] == c) return true;
        return false;
    };
    std::vector<double> acc_terms, iou_terms, fw_terms;
    double sum_nii = 0.0, sum_ti = 0.0, ignored_pts = 0.0;
    int64_t n_gt = 0, n_overlap = 0;
    for (int32_t c = 0; c < L; ++c) {
        const double nii = (double)conf[(size_t)c * L + c], ti = t[(size_t)c], nij = p[(size_t)c];
        const bool in_gt = ti > 0.0, in_union = in_gt || nij > 0.0, ign = ignored(c);
        if (per_class_iou) per_class_iou[c] = !in_union ? std::nan("") : ign ? 0.0 : nii / (ti + nij - nii);
        if (in_gt) {
            ++n_gt;
            if (ign) {
                ++n_overlap;
                acc_terms.push_back(0.0);
            } else {
                sum_nii += nii;
                sum_ti += ti;
                acc_terms.push_back(nii / ti);
            }
        }
        if (in_union) {
            if (ign) ignored_pts += ti;
            const bool skip = ign || ti == 0.0 || nij == 0.0;
            iou_terms.push_back(skip ? 0.0 : nii / (ti + nij - nii));
            fw_terms.push_back(skip ? 0.0 : (ti * nii) / (ti + nij - nii));
        }
    }
    SemsegScores s;
    s.acc = sum_ti == 0.0 ? 0.0 : sum_nii / sum_ti;
    s.macc = np_sum(acc_terms.data(), acc_terms.size()) / (double)(n_gt - n_overlap);
    s.miou = np_sum(iou_terms.data(), iou_terms.size()) / (double)(n_gt - n_overlap);
    s.fmiou = np_sum(fw_terms.data(), fw_terms.size()) / (m - ignored_pts);
    return s;
}

}  // namespace eval_metrics
