// hmsg_lsap (include/hmsg.h): scipy.optimize.linear_sum_assignment restated -- the rectangular shortest-augmenting-path solver
// of D. F. Crouse, "On implementing 2D rectangular assignment algorithms", IEEE Trans. Aerospace and Electronic Systems 52(4),
// 2016, in the form scipy ships it.  No HIP in here: tests/host_cpp/eval_lsap_host.cpp drives this header alone.
//
// The evaluator's association matrices are mostly zeros, so most assignments are ties, and object_semantics_eval_tp_auc
// (hm3dsem_evaluator.py) walks EVERY assigned pair: which of the equally good answers comes back is part of the result.  The
// details that fix it, all kept here:
//   - maximize negates the costs;
//   - more rows than columns: the matrix is transposed first and the answer sorted by row afterwards;
//   - the list of remaining columns starts reversed (nc - 1 ... 0);
//   - scanning it, a column replaces the current minimum when its path cost is lower, or equal and the column is unassigned;
//   - the chosen column is removed by moving the last remaining one into its place.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <numeric>
#include <vector>

enum { LSAP_OK = 0, LSAP_INFEASIBLE = -1, LSAP_INVALID = -2 };

namespace lsap_detail {

// one shortest augmenting path from row i; returns the sink column (-1: none can be reached) and the path's cost
inline int64_t augmenting_path(int64_t nc, const double* cost, const std::vector<double>& u, const std::vector<double>& v,
                               std::vector<int64_t>& path, const std::vector<int64_t>& row4col, std::vector<double>& shortest, int64_t i,
                               std::vector<char>& SR, std::vector<char>& SC, std::vector<int64_t>& remaining, double* p_min) {
    double min_val = 0.0;
    int64_t num_remaining = nc;
    for (int64_t it = 0; it < nc; ++it) remaining[(size_t)it] = nc - it - 1;
    std::fill(SR.begin(), SR.end(), 0);
    std::fill(SC.begin(), SC.end(), 0);
    std::fill(shortest.begin(), shortest.end(), std::numeric_limits<double>::infinity());
    int64_t sink = -1;
    while (sink == -1) {
        int64_t index = -1;
        double lowest = std::numeric_limits<double>::infinity();
        SR[(size_t)i] = 1;
        for (int64_t it = 0; it < num_remaining; ++it) {
            const int64_t j = remaining[(size_t)it];
            const double r = min_val + cost[i * nc + j] - u[(size_t)i] - v[(size_t)j];
            if (r < shortest[(size_t)j]) {
                path[(size_t)j] = i;
                shortest[(size_t)j] = r;
            }
            if (shortest[(size_t)j] < lowest || (shortest[(size_t)j] == lowest && row4col[(size_t)j] == -1)) {
                lowest = shortest[(size_t)j];
                index = it;
            }
        }
        min_val = lowest;
        if (min_val == std::numeric_limits<double>::infinity()) return -1;      // infeasible
        const int64_t j = remaining[(size_t)index];
        if (row4col[(size_t)j] == -1) sink = j;
        else i = row4col[(size_t)j];
        SC[(size_t)j] = 1;
        remaining[(size_t)index] = remaining[(size_t)--num_remaining];
    }
    *p_min = min_val;
    return sink;
}

}  // namespace lsap_detail

// cost: nr x nc, row-major.  row_ind / col_ind: min(nr, nc) entries each, rows ascending.  NaN or -inf entries (after the
// negation of `maximize`): LSAP_INVALID; no complete assignment of finite cost: LSAP_INFEASIBLE -- scipy raises ValueError for both.
inline int lsap_solve(int64_t nr, int64_t nc, const double* input_cost, bool maximize, int64_t* row_ind, int64_t* col_ind) {
    if (nr == 0 || nc == 0) return LSAP_OK;
    const bool transpose = nc < nr;
    std::vector<double> temp;
    if (transpose || maximize) {
        temp.resize((size_t)(nr * nc));
        if (transpose) {
            for (int64_t i = 0; i < nr; ++i)
                for (int64_t j = 0; j < nc; ++j) temp[(size_t)(j * nr + i)] = input_cost[i * nc + j];
            std::swap(nr, nc);
        } else {
            std::copy(input_cost, input_cost + nr * nc, temp.begin());
        }
        if (maximize)
            for (double& c : temp) c = -c;
    }
    const double* cost = temp.empty() ? input_cost : temp.data();
    for (int64_t k = 0; k < nr * nc; ++k)
        if (cost[k] != cost[k] || cost[k] == -std::numeric_limits<double>::infinity()) return LSAP_INVALID;

    std::vector<double> u((size_t)nr, 0.0), v((size_t)nc, 0.0), shortest((size_t)nc);
    std::vector<int64_t> path((size_t)nc, -1), col4row((size_t)nr, -1), row4col((size_t)nc, -1), remaining((size_t)nc);
    std::vector<char> SR((size_t)nr), SC((size_t)nc);
    for (int64_t cur = 0; cur < nr; ++cur) {
        double min_val = 0.0;
        const int64_t sink = lsap_detail::augmenting_path(nc, cost, u, v, path, row4col, shortest, cur, SR, SC, remaining, &min_val);
        if (sink < 0) return LSAP_INFEASIBLE;
        u[(size_t)cur] += min_val;
        for (int64_t i = 0; i < nr; ++i)
            if (SR[(size_t)i] && i != cur) u[(size_t)i] += min_val - shortest[(size_t)col4row[(size_t)i]];
        for (int64_t j = 0; j < nc; ++j)
            if (SC[(size_t)j]) v[(size_t)j] -= min_val - shortest[(size_t)j];
        int64_t j = sink;
        for (;;) {
            const int64_t i = path[(size_t)j];
            row4col[(size_t)j] = i;
            std::swap(col4row[(size_t)i], j);
            if (i == cur) break;
        }
    }
    if (transpose) {
        std::vector<int64_t> order((size_t)nr);
        std::iota(order.begin(), order.end(), (int64_t)0);
        std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return col4row[(size_t)a] < col4row[(size_t)b]; });
        int64_t i = 0;
        for (int64_t w : order) {
            row_ind[i] = col4row[(size_t)w];
            col_ind[i] = w;
            ++i;
        }
    } else {
        for (int64_t i = 0; i < nr; ++i) {
            row_ind[i] = i;
            col_ind[i] = col4row[(size_t)i];
        }
    }
    return LSAP_OK;
}
