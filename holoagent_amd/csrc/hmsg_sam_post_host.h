// The decisions of hmsg_sam_postprocess (include/hmsg.h) that are made on the host from the small statistics table the device
// reads back: the predicted-IoU filter, the stability score, the boxes, both box NMS passes and the launch plan of the
// statistics kernel.  No HIP in here: tests/host_cpp/sam_post_host.cpp drives this header alone.
//
// Reference: segment_anything/automatic_mask_generator.py _process_batch / postprocess_small_regions,
// segment_anything/utils/amg.py calculate_stability_score / batched_mask_to_box / box_xyxy_to_xywh, torchvision.ops.nms (its CPU
// kernel: float32 throughout).  Every float32 operation below is ONE IEEE operation -- compile without FMA contraction.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

// what the statistics kernel leaves per mask: #{v > t + offset}, #{v > t}, #{v > t - offset} and the inclusive extremes of the
// pixels with v > t (x0 > x1 when there is none)
struct SpStats {
    int32_t n_hi, n_mid, n_lo, x0, y0, x1, y1;
};
#define SP_STATS_INIT SpStats{0, 0, 0, 0x7fffffff, 0x7fffffff, -1, -1}

struct SpBox {
    float x0, y0, x1, y1;      // XYXY, inclusive pixel indices (batched_mask_to_box)
};

// Step 1: rows with iou > thresh, in row order; thresh <= 0: every row (automatic_mask_generator.py: `if self.pred_iou_thresh > 0.0`)
inline std::vector<int32_t> sp_iou_filter(int32_t N, const float* iou, float thresh) {
    std::vector<int32_t> keep;
    for (int32_t i = 0; i < N; ++i)
        if (!(thresh > 0.0f) || iou[i] > thresh) keep.push_back(i);
    return keep;
}
// Step 2: calculate_stability_score: int / int is a float32 true division in torch; 0 / 0 = NaN, which fails `>=`
inline float sp_stability(const SpStats& s) { return (float)s.n_hi / (float)s.n_lo; }
inline bool sp_stability_keeps(float score, float thresh) { return !(thresh > 0.0f) || score >= thresh; }
// Step 3: batched_mask_to_box: an empty mask has box [0, 0, 0, 0]
inline SpBox sp_box(const SpStats& s) {
    if (s.n_mid <= 0) return SpBox{0.0f, 0.0f, 0.0f, 0.0f};
    return SpBox{(float)s.x0, (float)s.y0, (float)s.x1, (float)s.y1};
}

// Steps 4 and 5b: torchvision.ops.nms.  Visits boxes by decreasing score -- equal scores by increasing position (a stable sort:
// this library's definition, torch leaves the order among ties open) --, keeps a box that nobody suppressed and lets it suppress
// every later box with inter / (a_i + a_j - inter) > thresh.  Returns the kept positions in visiting order.
inline std::vector<int32_t> sp_nms(const std::vector<SpBox>& box, const std::vector<float>& score, float thresh) {
    const size_t n = box.size();
    std::vector<int32_t> order(n), keep;
    for (size_t i = 0; i < n; ++i) order[i] = (int32_t)i;
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return score[(size_t)a] > score[(size_t)b]; });
    std::vector<float> area(n);
    for (size_t i = 0; i < n; ++i) area[i] = (box[i].x1 - box[i].x0) * (box[i].y1 - box[i].y0);
    std::vector<char> dead(n, 0);
    for (size_t a = 0; a < n; ++a) {
        const size_t i = (size_t)order[a];
        if (dead[i]) continue;
        keep.push_back((int32_t)i);
        for (size_t b = a + 1; b < n; ++b) {
            const size_t j = (size_t)order[b];
            if (dead[j]) continue;
            const float w = std::max(0.0f, std::min(box[i].x1, box[j].x1) - std::max(box[i].x0, box[j].x0));
            const float h = std::max(0.0f, std::min(box[i].y1, box[j].y1) - std::max(box[i].y0, box[j].y0));
            const float inter = w * h;
            const float uni = area[i] + area[j] - inter;
            if (inter / uni > thresh) dead[j] = 1;            // (0 / 0 = NaN: suppresses nothing)
        }
    }
    return keep;
}

// Steps 2 - 4 on the statistics of the rows the IoU filter kept: rows[k] is the row of `logits` that st[k] describes.
// Returns positions k in the order the first NMS leaves them (decreasing predicted IoU).
inline std::vector<int32_t> sp_first_pass(const std::vector<int32_t>& rows, const std::vector<SpStats>& st, const float* iou,
                                          float stability_thresh, float nms_thresh) {
    std::vector<int32_t> pos;
    std::vector<SpBox> box;
    std::vector<float> score;
    for (size_t k = 0; k < rows.size(); ++k) {
        if (!sp_stability_keeps(sp_stability(st[k]), stability_thresh)) continue;
        pos.push_back((int32_t)k);
        box.push_back(sp_box(st[k]));
        score.push_back(iou[rows[k]]);
    }
    std::vector<int32_t> keep = sp_nms(box, score, nms_thresh);
    for (int32_t& v : keep) v = pos[(size_t)v];
    return keep;
}
// Step 5b: postprocess_small_regions' NMS over the re-made boxes: score 1.0 for a mask neither pass changed, else 0.0
inline std::vector<int32_t> sp_second_pass(const std::vector<SpStats>& st_new, const std::vector<char>& changed, float nms_thresh) {
    std::vector<SpBox> box;
    std::vector<float> score;
    for (size_t k = 0; k < st_new.size(); ++k) {
        box.push_back(sp_box(st_new[k]));
        score.push_back(changed[k] ? 0.0f : 1.0f);
    }
    return sp_nms(box, score, nms_thresh);
}

// The statistics kernel's launch plan: 256 threads, SP_STATS_VEC loads of four elements per thread and trip, SP_STATS_TRIPS trips
// per workgroup -- the wave reduction and the atomics behind the last trip cost about as much as one trip --, 1024 workgroups per
// mask at most (grid y = masks: the masks of a frame fill the device many times over either way).
#define SP_STATS_THREADS 256
#define SP_STATS_VEC 4
#define SP_STATS_TRIPS 4
inline unsigned sp_stats_blocks(long long HW) {
    const long long per_block = (long long)SP_STATS_THREADS * SP_STATS_VEC * 4 * SP_STATS_TRIPS;      // elements a workgroup takes
    return (unsigned)std::max<long long>(1, std::min<long long>((HW + per_block - 1) / per_block, 1024));
}
