// Stand-alone driver of holoagent_amd/csrc/hmsg_lsap_host.h (the assignment behind hmsg_lsap): reads matrices from stdin, prints
// the assignment of each.  tests/test_eval_lsap.py builds it plain and with -fsanitize=address,undefined, feeds it tie-heavy
// rectangular matrices and compares the answers with scipy's, index for index.
//
//   in : "M <nr> <nc> <maximize>" then nr * nc numbers (anything strtod reads: hexadecimal floats, inf, nan), row-major
//   out: "<status> <n> r0 c0 r1 c1 ..." per matrix
#include "hmsg_lsap_host.h"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

int main() {
    char tag[8];
    long long nr, nc;
    int maximize;
    int n_done = 0;
    while (scanf("%7s %lld %lld %d", tag, &nr, &nc, &maximize) == 4) {
        if (tag[0] != 'M' || nr < 0 || nc < 0) {
            fprintf(stderr, "bad header\n");
            return 2;
        }
        std::vector<double> cost((size_t)(nr * nc));
        for (double& c : cost) {
            char word[64];
            if (scanf("%63s", word) != 1) {
                fprintf(stderr, "matrix %d is short\n", n_done);
                return 2;
            }
            c = strtod(word, nullptr);
        }
        const long long n = nr < nc ? nr : nc;
        std::vector<int64_t> row((size_t)n), col((size_t)n);
        const int rc = lsap_solve(nr, nc, cost.data(), maximize != 0, row.data(), col.data());
        printf("%d %lld", rc, rc == LSAP_OK ? n : 0);
        if (rc == LSAP_OK)
            for (long long i = 0; i < n; ++i) printf(" %lld %lld", (long long)row[(size_t)i], (long long)col[(size_t)i]);
        printf("\n");
        ++n_done;
    }
    return n_done > 0 ? 0 : 2;
}
