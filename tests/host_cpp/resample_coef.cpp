// The host arithmetic of the CLIP preprocess (holoagent_amd/csrc/hmsg_resample_coef.h) as a stand-alone program: it includes
// nothing but that header, reads requests from standard input and prints the header's integers, which
// tests/test_resample_coef.py compares with the numpy restatement (tests/clip_preprocess_oracle.py).
//   C <in> <out>     -> "C in out ksize" and one line per output index: xmin taps k0 k1 ...
//   W <in> <out> <first> <count>  -> the same for a window of output indices (what a launch uploads)
//   R <H> <W> <S>    -> "R H W S w' h' left top"
//   L                -> "L" and 768 lines: float32 bits and float16 bits of the default ToTensor + Normalize table
//   H <bits>         -> "H f16bits" of the float32 with these bits
#include "hmsg_resample_coef.h"

#include <cstdio>

int main() {
    namespace R = hmsg_resample;
    char op;
    long long n_req = 0;
    while (scanf(" %c", &op) == 1) {
        ++n_req;
        if (op == 'C' || op == 'W') {
            int in, out, first = 0, count;
            if (scanf("%d %d", &in, &out) != 2 || in < 1 || out < 1) return 2;
            count = out;
            if (op == 'W' && (scanf("%d %d", &first, &count) != 2 || first < 0 || count < 0 || first + count > out)) return 2;
            std::vector<int32_t> b, k;
            const int ks = R::coefficients(in, out, first, count, b, k);
            printf("%c %d %d %d\n", op, in, out, ks);
            for (int i = 0; i < count; ++i) {
                printf("%d %d", b[2 * i], b[2 * i + 1]);
                for (int x = 0; x < ks; ++x) printf(" %d", k[(size_t)i * ks + x]);
                printf("\n");
            }
        } else if (op == 'R') {
            int H, W, S, w2, h2;
            if (scanf("%d %d %d", &H, &W, &S) != 3 || H < 1 || W < 1 || S < 1) return 2;
            R::resize_dims(H, W, S, w2, h2);
            printf("R %d %d %d %d %d %d %d\n", H, W, S, w2, h2, R::center_crop_offset(w2, S), R::center_crop_offset(h2, S));
        } else if (op == 'L') {
            const float mean[3] = {0.48145466f, 0.4578275f, 0.40821073f}, stdv[3] = {0.26862954f, 0.26130258f, 0.27577711f};
            float lut[768];
            R::normalize_table(mean, stdv, lut);
            printf("L\n");
            for (int i = 0; i < 768; ++i) {
                uint32_t bits;
                std::memcpy(&bits, &lut[i], 4);
                printf("%u %u\n", bits, (unsigned)R::f32_to_f16_bits(lut[i]));
            }
        } else if (op == 'H') {
            unsigned bits;
            if (scanf("%u", &bits) != 1) return 2;
            float f;
            std::memcpy(&f, &bits, 4);
            printf("H %u\n", (unsigned)R::f32_to_f16_bits(f));
        } else {
            return 2;
        }
    }
    printf("resample_coef ok %lld\n", n_req);
    return 0;
}
