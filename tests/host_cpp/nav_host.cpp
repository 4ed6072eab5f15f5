// Drives holoagent_amd/csrc/hmsg_nav_host.h stand-alone (tests/test_nav_host.py): no HIP, no Python.
// stdin:  "P <n> <eps hex> <min_samples>" then a line of n heights (hex floats)  ->  "L <labels...>" and "K <kept indices...>"
//         "C <radius>"                                                            ->  "H <half-widths...>"
//         "T <value hex>"                                                         ->  "I <np.int32(value)>"
#include "hmsg_nav_host.h"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

int main() {
    std::string tag;
    while (std::cin >> tag) {
        if (tag == "P") {
            size_t n;
            std::string eps_s;
            int min_samples;
            std::cin >> n >> eps_s >> min_samples;
            const double eps = strtod(eps_s.c_str(), nullptr);
            std::vector<double> h(n);
            for (size_t i = 0; i < n; ++i) {
                std::string s;
                std::cin >> s;
                h[i] = strtod(s.c_str(), nullptr);
            }
            const std::vector<int32_t> label = nav_host::dbscan_1d(h.data(), n, eps, min_samples);
            printf("L");
            for (int32_t l : label) printf(" %d", l);
            printf("\nK");
            for (int32_t k : nav_host::select_poses(h.data(), n, eps, min_samples)) printf(" %d", k);
            printf("\n");
        } else if (tag == "C") {
            int r;
            std::cin >> r;
            printf("H");
            for (int32_t w : nav_host::circle_half_widths(r)) printf(" %d", w);
            printf("\n");
        } else if (tag == "T") {
            std::string s;
            std::cin >> s;
            printf("I %d\n", nav_host::trunc_i32(strtod(s.c_str(), nullptr)));
        } else {
            fprintf(stderr, "unknown record %s\n", tag.c_str());
            return 2;
        }
    }
    return 0;
}
