// Stand-alone driver of holoagent_amd/csrc/hmsg_sam_post_host.h (the host decisions of hmsg_sam_postprocess: the filters and both NMS
// passes) for tests/test_sam_post_host.py, which builds it plain and with the host sanitizers.  Nothing but that header is included.
//
// stdin: one request per line block
//   F <N> <iou_thresh> <stab_thresh> <nms_thresh>     then N lines "<iou bits> <n_hi> <n_mid> <n_lo> <x0> <y0> <x1> <y1>"
//       -> "F <rows the IoU filter keeps> | <kept rows after stability + first NMS, in order> | <stability bits of those>"
//   S <K> <nms_thresh>                                then K lines "<changed> <n_mid> <x0> <y0> <x1> <y1>"
//       -> "S <kept positions after the second NMS, in order>"
//   B <HW>                                            -> "B <workgroups per mask of the statistics kernel>"
// Floats travel as the decimal value of their 32 bits.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "hmsg_sam_post_host.h"

static float from_bits(uint32_t b) {
    float f;
    memcpy(&f, &b, 4);
    return f;
}
static uint32_t to_bits(float f) {
    uint32_t b;
    memcpy(&b, &f, 4);
    return b;
}

int main() {
    char kind;
    long n_req = 0;
    while (scanf(" %c", &kind) == 1) {
        ++n_req;
        if (kind == 'F') {
            int N;
            uint32_t b_iou, b_stab, b_nms;
            if (scanf("%d %" SCNu32 " %" SCNu32 " %" SCNu32, &N, &b_iou, &b_stab, &b_nms) != 4 || N < 0) return 2;
            std::vector<float> iou((size_t)N);
            std::vector<SpStats> all((size_t)N);
            for (int i = 0; i < N; ++i) {
                uint32_t b;
                SpStats& s = all[(size_t)i];
                if (scanf("%" SCNu32 " %d %d %d %d %d %d %d", &b, &s.n_hi, &s.n_mid, &s.n_lo, &s.x0, &s.y0, &s.x1, &s.y1) != 8) return 2;
                iou[(size_t)i] = from_bits(b);
            }
            const std::vector<int32_t> rows = sp_iou_filter(N, iou.data(), from_bits(b_iou));
            std::vector<SpStats> st;
            for (int32_t r : rows) st.push_back(all[(size_t)r]);
            const std::vector<int32_t> keep = sp_first_pass(rows, st, iou.data(), from_bits(b_stab), from_bits(b_nms));
            printf("F");
            for (int32_t r : rows) printf(" %d", r);
            printf(" |");
            for (int32_t k : keep) printf(" %d", rows[(size_t)k]);
            printf(" |");
            for (int32_t k : keep) printf(" %" PRIu32, to_bits(sp_stability(st[(size_t)k])));
            printf("\n");
        } else if (kind == 'S') {
            int K;
            uint32_t b_nms;
            if (scanf("%d %" SCNu32, &K, &b_nms) != 2 || K < 0) return 2;
            std::vector<SpStats> st((size_t)K, SP_STATS_INIT);
            std::vector<char> changed((size_t)K);
            for (int k = 0; k < K; ++k) {
                int ch;
                SpStats& s = st[(size_t)k];
                if (scanf("%d %d %d %d %d %d", &ch, &s.n_mid, &s.x0, &s.y0, &s.x1, &s.y1) != 6) return 2;
                changed[(size_t)k] = (char)(ch != 0);
            }
            printf("S");
            for (int32_t k : sp_second_pass(st, changed, from_bits(b_nms))) printf(" %d", k);
            printf("\n");
        } else if (kind == 'B') {
            long long HW;
            if (scanf("%lld", &HW) != 1) return 2;
            printf("B %u\n", sp_stats_blocks(HW));
        } else {
            return 2;
        }
    }
    printf("sam_post_host ok %ld\n", n_req);
    return 0;
}
