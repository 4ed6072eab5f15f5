// Stand-alone host program for a sanitizer run of hmsg_kmeans_batch on the kernel simulator build (scripts/kmeans_asan.sh builds
// the simulator's objects with -fsanitize=address and links them with this file; HMSG_DEBUG_EXACT_ALLOC=1 makes every device
// buffer a heap block of exactly its size).  The batched case of tests/test_kmeans_device.py: D = 64, k = 5, sets of 5, 6, 70, 257
// and 600 rows in one call; every set must equal hmsg_kmeans on it bit for bit.  Exit status 0 = equal and no report.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/hmsg.h"

int main() {
    const int D = 64, k = 5, sizes[5] = {5, 6, 70, 257, 600};
    std::vector<int64_t> off(1, 0);
    for (int n : sizes) off.push_back(off.back() + n);
    const int64_t N = off.back();
    std::vector<float> X((size_t)N * D);
    uint64_t state = 88172645463325252ull;
    for (size_t i = 0; i < X.size(); ++i) {                      // xorshift64: rows around 7 directions
        state ^= state << 13, state ^= state >> 7, state ^= state << 17;
        const double u = (double)(state >> 11) / 9007199254740992.0;
        X[i] = (float)(u - 0.5 + 0.4 * std::sin((double)((i / D) % 7) * (double)(i % D)));
    }
    for (int q = 0; q < D; ++q) X[(size_t)(off[3] + 9) * D + q] = X[(size_t)off[3] * D + q];      // one repeated row
    std::vector<int32_t> labels((size_t)N, -7), n_iter(5, -7);
    std::vector<float> centers((size_t)5 * k * D, 7.f), inertia(5, 7.f);
    int rc = hmsg_kmeans_batch(0, 5, off.data(), X.data(), D, k, 5, 100, 0, labels.data(), centers.data(), inertia.data(), n_iter.data());
    if (rc != HMSG_OK) {
        fprintf(stderr, "hmsg_kmeans_batch: %d\n", rc);
        return 1;
    }
    for (int s = 0; s < 5; ++s) {
        const int n = sizes[s];
        std::vector<int32_t> lab((size_t)n);
        std::vector<float> cen((size_t)k * D);
        float in = 0.f;
        int32_t it = 0;
        rc = hmsg_kmeans(X.data() + (size_t)off[s] * D, n, D, k, 5, 100, 0, lab.data(), cen.data(), &in, &it);
        if (rc != HMSG_OK) return 2;
        if (memcmp(lab.data(), labels.data() + off[s], (size_t)n * 4) || memcmp(cen.data(), centers.data() + (size_t)s * k * D, (size_t)k * D * 4) ||
            memcmp(&in, &inertia[s], 4) || it != n_iter[s]) {
            fprintf(stderr, "set %d differs from hmsg_kmeans\n", s);
            return 3;
        }
        printf("set %d: n %d n_iter %d inertia %.9g equal\n", s, n, (int)it, (double)in);
    }
    return 0;
}
