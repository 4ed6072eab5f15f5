// hmsg_rle_to_bitsets / hmsg_rle_to_masks as a stand-alone host program for scripts/rle_asan.sh (kernel simulator build of hmsg_rle.hip under
// AddressSanitizer and UBSan): 300 random frames, a third valid (checked against a plain decode), a third with a wrong sum, a third
// with garbage counts -- the malformed ones must be refused with the output untouched, and no input may move an access out of bounds.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
extern "C" int hmsg_rle_to_bitsets(int32_t, int32_t, int32_t, int32_t, const uint32_t*, const int64_t*, uint64_t*);
extern "C" int hmsg_rle_to_masks(int32_t, int32_t, int32_t, int32_t, const uint32_t*, const int64_t*, uint8_t*);
int main() {
    unsigned seed = 12345;
    auto rnd = [&] { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    int fails = 0;
    for (int it = 0; it < 300; ++it) {
        const int H = 1 + rnd() % 90, W = 1 + rnd() % 150, M = rnd() % 70 + (it % 7 == 0 ? 186 : 0);
        const int NW = ((M > 1 ? M : 1) + 63) / 64;
        std::vector<uint32_t> counts;
        std::vector<int64_t> off(1, 0);
        std::vector<uint8_t> dense((size_t)M * H * W, 0);
        for (int i = 0; i < M; ++i) {
            long left = (long)H * W, pos = 0;
            int r = 0;
            while (left > 0) {
                long c = rnd() % 5 == 0 ? 0 : 1 + rnd() % (rnd() % 3 == 0 ? 400 : 9);
                if (c > left) c = left;
                counts.push_back((uint32_t)c);
                if (r & 1) for (long t = pos; t < pos + c; ++t) dense[(size_t)i * H * W + (t % H) * W + t / H] = 1;
                pos += c; left -= c; ++r;
            }
            off.push_back((int64_t)counts.size());
        }
        const int bad = it % 3;          // 0 valid, 1 a wrong sum, 2 garbage counts (huge)
        std::vector<uint32_t> c2 = counts;
        if (M > 0 && bad == 1) c2[rnd() % c2.size()] += 1 + rnd() % 1000;
        if (M > 0 && bad == 2) for (auto& v : c2) if (rnd() % 4 == 0) v = 0xFFFFFFFFu - rnd() % 3;
        std::vector<uint64_t> bits((size_t)H * W * NW, 0xABABABABABABABABull);
        std::vector<uint8_t> out((size_t)M * H * W + 1, 0xCD);
        const int rc1 = hmsg_rle_to_bitsets(0, H, W, M, c2.data(), off.data(), bits.data());
        const int rc2 = hmsg_rle_to_masks(0, H, W, M, c2.data(), off.data(), out.data());
        if (M == 0 || bad == 0) {
            if (rc1 != 0 || rc2 != 0) { ++fails; printf("valid refused it=%d\n", it); continue; }
            for (size_t p = 0; p < (size_t)H * W; ++p)
                for (int i = 0; i < M; ++i)
                    if (((bits[p * NW + (i >> 6)] >> (i & 63)) & 1) != dense[(size_t)i * H * W + p] || out[(size_t)i * H * W + p] != dense[(size_t)i * H * W + p]) { ++fails; p = (size_t)H * W; break; }
        } else {
            if (rc1 != -1 || rc2 != -1) { ++fails; printf("malformed accepted it=%d bad=%d\n", it, bad); }
            for (auto v : bits) if (v != 0xABABABABABABABABull) { ++fails; break; }
        }
    }
    printf("fails %d\n", fails);
    return fails != 0;
}
