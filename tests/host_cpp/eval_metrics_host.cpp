// Stand-alone driver of holoagent_amd/csrc/hmsg_eval_metrics_host.h (the evaluator's metrics: floors, the threshold sweep, np.trapz,
// the hydra means, top-k accuracies from ranks): reads records from stdin, prints what the header makes of each.
// tests/test_eval_metrics_host.py builds it plain and with -fsanitize=address,undefined and compares every float64 with numpy's, bit
// for bit.
//
//   in  (numbers: anything strtod reads, hexadecimal floats included)
//     "M <P> <G> <n>"   P * G matrix entries, then n pairs "row col"
//     "H <P> <G>"       over_pred [P][G], over_gt [P][G]
//     "F <Fg> <Fp>"     lower[Fg], upper[Fg], vertices [Fp][8][3]
//     "K <n> <C> <nk>"  rank[n], k[nk]
//     "T <n>"           y[n], x[n]
//   out (floats as hexadecimal)
//     "M ap acc6 prec6 rec6 | tp0 .. tp10 | tp fp fn acc prec recall"   (the last six: the recount at 0.5)
//     "H hydra_prec hydra_recall"
//     "F tp fp fn acc prec recall"   or "F invalid"
//     "K acc_0 .. acc_nk-1 auc"
//     "T value"
#include "hmsg_eval_metrics_host.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {
bool read_doubles(std::vector<double>& v) {
    for (double& d : v) {
        char word[64];
        if (scanf("%63s", word) != 1) return false;
        d = strtod(word, nullptr);
    }
    return true;
}
bool read_ints(std::vector<int32_t>& v) {
    for (int32_t& d : v) {
        long long x;
        if (scanf("%lld", &x) != 1) return false;
        d = (int32_t)x;
    }
    return true;
}
}  // namespace

int main() {
    namespace E = eval_metrics;
    char tag[8];
    int n_done = 0;
    while (scanf("%7s", tag) == 1) {
        const long long LIM = 1 << 20;
        if (tag[0] == 'M') {
            long long P, G, n;
            if (scanf("%lld %lld %lld", &P, &G, &n) != 3 || P < 0 || G < 0 || n < 0 || P * G > LIM || n > LIM) return 2;
            std::vector<double> M((size_t)(P * G));
            std::vector<int32_t> rc((size_t)n * 2), row((size_t)n), col((size_t)n);
            if (!read_doubles(M) || !read_ints(rc)) return 2;
            for (long long k = 0; k < n; ++k) {
                row[(size_t)k] = rc[(size_t)k * 2], col[(size_t)k] = rc[(size_t)k * 2 + 1];
                if (row[(size_t)k] < 0 || row[(size_t)k] >= P || col[(size_t)k] < 0 || col[(size_t)k] >= G) return 2;
            }
            const E::Sweep s = E::threshold_sweep(M.data(), row.data(), col.data(), n, P, G);
            printf("M %a %a %a %a |", s.ap, s.acc[6], s.prec[6], s.rec_sorted[6]);
            for (int i = 0; i < E::N_THRESH; ++i) printf(" %lld", (long long)s.tp[i]);
            const E::Counts c = E::counts_at(M.data(), G, row.data(), col.data(), n, P, G, 0.5);
            printf(" | %lld %lld %lld %a %a %a\n", (long long)c.tp, (long long)c.fp, (long long)c.fn, c.acc, c.prec, c.recall);
        } else if (tag[0] == 'H') {
            long long P, G;
            if (scanf("%lld %lld", &P, &G) != 2 || P < 1 || G < 1 || P * G > LIM) return 2;
            std::vector<double> a((size_t)(P * G)), b((size_t)(P * G));
            if (!read_doubles(a) || !read_doubles(b)) return 2;
            double pr, re;
            E::hydra_means(a.data(), b.data(), P, G, &pr, &re);
            printf("H %a %a\n", pr, re);
        } else if (tag[0] == 'F') {
            long long Fg, Fp;
            if (scanf("%lld %lld", &Fg, &Fp) != 2 || Fg < 0 || Fp < 0 || Fg > LIM || Fp > LIM) return 2;
            std::vector<double> lo((size_t)Fg), up((size_t)Fg), v((size_t)Fp * 24);
            if (!read_doubles(lo) || !read_doubles(up) || !read_doubles(v)) return 2;
            E::Counts c;
            if (E::floor_metrics(lo.data(), up.data(), Fg, v.data(), Fp, &c))
                printf("F %lld %lld %lld %a %a %a\n", (long long)c.tp, (long long)c.fp, (long long)c.fn, c.acc, c.prec, c.recall);
            else
                printf("F invalid\n");
        } else if (tag[0] == 'K') {
            long long n, C, nk;
            if (scanf("%lld %lld %lld", &n, &C, &nk) != 3 || n < 1 || C < 0 || nk < 0 || n > LIM || C > LIM || nk > LIM) return 2;
            std::vector<int32_t> rank((size_t)n), ks((size_t)nk);
            if (!read_ints(rank) || !read_ints(ks)) return 2;
            printf("K");
            for (int32_t k : ks) printf(" %a", E::top_k_acc(rank.data(), n, k));
            printf(" %a\n", E::top_k_auc(rank.data(), n, C));
        } else if (tag[0] == 'T') {
            long long n;
            if (scanf("%lld", &n) != 1 || n < 0 || n > LIM) return 2;
            std::vector<double> y((size_t)n), x((size_t)n);
            if (!read_doubles(y) || !read_doubles(x)) return 2;
            printf("T %a\n", E::trapz(y.data(), x.data(), (size_t)n));
        } else {
            fprintf(stderr, "bad record tag\n");
            return 2;
        }
        ++n_done;
    }
    return n_done > 0 ? 0 : 2;
}
