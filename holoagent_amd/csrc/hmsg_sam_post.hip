// SAM's mask post-processing on the device (include/hmsg.h: hmsg_sam_postprocess): the decoder's logits of one frame -> the
// run-length records of hmsg_add_frame_features_rle, without a mask leaving HBM.
//
// Reference: segment_anything/automatic_mask_generator.py SamAutomaticMaskGenerator._process_batch (everything behind
// predict_torch) and postprocess_small_regions; segment_anything/utils/amg.py calculate_stability_score, batched_mask_to_box,
// mask_to_rle_pytorch, remove_small_regions, box_xyxy_to_xywh; torchvision.ops.nms.  The decisions (filters, both NMS passes)
// are made on the host from a table of seven integers per mask: hmsg_sam_post_host.h.
//
// MI355X design notes
//  * k_sp_stats is the one kernel that reads all of the logits (531 MB a frame at 640x480, 144 x 3 prompts) and is bound by HBM:
//    one pass makes the three counts (stability score, area) and the four box extremes of a mask.  A lane reads 16 bytes at a
//    time, consecutive lanes consecutive 16 bytes; a mask whose first element is not on a 16-byte boundary (H * W no multiple of
//    4) has its first and last elements read one by one by the mask's first workgroup.  One integer division per 16 bytes turns
//    the element index into (x, y).  The seven values are reduced over the wave by shuffles; one lane per wave adds them to
//    the mask's row of the table with atomics (a few dozen per mask).  A row the IoU filter dropped is not read: the grid's y
//    runs over the list of kept rows.  The same kernel over bytes makes the boxes and areas of the masks the small-region pass changed.
//  * Labelling: label equivalence as in hmsg_rooms.hip (lab[p] = smallest pixel index of p's component), here over all
//    surviving masks of the frame in one grid (y = mask), a label being an index inside its own mask (< 2^24).  A pixel starts
//    with the first pixel of its horizontal run inside its wave's 64 pixels.  A round is four scan + flatten pairs and ONE
//    read-back for the whole batch: a "changed" flag per scan, and the labels are final when the round's last scan changed
//    nothing (the two rounds a single flag needs -- one that converges, one that confirms -- become one).  The component sizes are counted at the root
//    with one atomic per run of equal labels inside a wave (a ballot finds the lanes that share the leader's label), not one
//    per pixel: the background of a mask is one component of several hundred thousand pixels.
//  * Run-length coding in three launches: a lane walks one column of one mask (consecutive lanes consecutive columns: every
//    step of the walk reads consecutive bytes) and counts the value changes, the step from the previous column's last pixel
//    included; a wave per mask scans the columns' counts (and carries the position of the last change before every column);
//    the same walk then writes `position - previous position` at the scanned offsets.  The totals go to the host between the
//    scan and the write: a short counts array is refused before anything is written to it.
#include "hmsg_boundary.h"
#include "hmsg_sam_post_host.h"

#include <climits>

#define SP_NONE 0x7fffffff
#define SP_T 256

// ------------------------------------------------------------------------------------------ K_sp_stats
struct SpAcc {
    int n_hi = 0, n_mid = 0, n_lo = 0, x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1;
};
__device__ __forceinline__ void sp_acc(SpAcc& a, float v, int x, int y, float t_hi, float t_mid, float t_lo) {
    a.n_hi += v > t_hi ? 1 : 0;
    a.n_lo += v > t_lo ? 1 : 0;
    if (v > t_mid) {
        a.n_mid += 1;
        a.x0 = min(a.x0, x);
        a.x1 = max(a.x1, x);
        a.y0 = min(a.y0, y);
        a.y1 = max(a.y1, y);
    }
}
// grid (sp_stats_blocks(HW), masks).  T = float: the logits; T = unsigned char: 0/1 masks (thresholds 0.5).  rows (optional):
// the row of `data` that mask k of the grid is.  stats [masks][7], initialised to SP_STATS_INIT.
template <typename T>
__global__ __launch_bounds__(SP_STATS_THREADS) void k_sp_stats(const T* __restrict__ data, const int* __restrict__ rows, int HW, int W,
                                                               float t_hi, float t_mid, float t_lo, int* __restrict__ stats) {
    const int k = blockIdx.y;
    const T* p = data + (size_t)(rows ? rows[k] : k) * (size_t)HW;
    constexpr int VB = (int)sizeof(T) * 4;                                  // bytes of one vector load: four elements
    const int head = min(HW, (int)(((VB - (int)((uintptr_t)p & (uintptr_t)(VB - 1))) & (VB - 1)) / (int)sizeof(T)));
    const int nvec = (HW - head) / 4;
    SpAcc a;
    // a trip of the workgroup takes SP_STATS_VEC * 256 consecutive vectors; a lane's SP_STATS_VEC loads are issued before the first
    // is used (an index past the end reads the last vector again and counts as -inf: no branch between the loads)
    for (int base = blockIdx.x * (SP_STATS_VEC * SP_STATS_THREADS); base < nvec; base += gridDim.x * (SP_STATS_VEC * SP_STATS_THREADS)) {
        float v[SP_STATS_VEC][4];
#pragma unroll
        for (int u = 0; u < SP_STATS_VEC; ++u) {
            const int i = base + u * SP_STATS_THREADS + (int)threadIdx.x, e = head + 4 * min(i, nvec - 1);
            if constexpr (sizeof(T) == 4) {
                const float4 q = *(const float4*)(p + e);
                v[u][0] = q.x, v[u][1] = q.y, v[u][2] = q.z, v[u][3] = q.w;
            } else {
                const unsigned q = *(const unsigned*)(p + e);
                v[u][0] = (float)(q & 255u), v[u][1] = (float)((q >> 8) & 255u), v[u][2] = (float)((q >> 16) & 255u), v[u][3] = (float)(q >> 24);
            }
        }
#pragma unroll
        for (int u = 0; u < SP_STATS_VEC; ++u) {
            const int i = base + u * SP_STATS_THREADS + (int)threadIdx.x, e = head + 4 * i;
            const bool in = i < nvec;
            int y = e / W, x = e - y * W;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                sp_acc(a, in ? v[u][j] : -INFINITY, x, y, t_hi, t_mid, t_lo);
                if (++x == W) x = 0, ++y;
            }
        }
    }
    if (blockIdx.x == 0) {                                                   // the elements in front of and behind the vectors (< 8)
        const int tail0 = head + 4 * nvec, t = threadIdx.x;
        const int e = t < head ? t : tail0 + (t - head);
        if (e < HW && (t < head || e >= tail0)) sp_acc(a, (float)p[e], e % W, e / W, t_hi, t_mid, t_lo);
    }
    for (int o = 32; o > 0; o >>= 1) {
        a.n_hi += __shfl_xor(a.n_hi, o);
        a.n_mid += __shfl_xor(a.n_mid, o);
        a.n_lo += __shfl_xor(a.n_lo, o);
        a.x0 = min(a.x0, __shfl_xor(a.x0, o));
        a.y0 = min(a.y0, __shfl_xor(a.y0, o));
        a.x1 = max(a.x1, __shfl_xor(a.x1, o));
        a.y1 = max(a.y1, __shfl_xor(a.y1, o));
    }
    if ((threadIdx.x & 63) == 0 && (a.n_hi | a.n_mid | a.n_lo)) {
        int* s = stats + (size_t)k * 7;
        if (a.n_hi) atomicAdd(s + 0, a.n_hi);
        if (a.n_lo) atomicAdd(s + 2, a.n_lo);
        if (a.n_mid) {
            atomicAdd(s + 1, a.n_mid);
            atomicMin(s + 3, a.x0);
            atomicMin(s + 4, a.y0);
            atomicMax(s + 5, a.x1);
            atomicMax(s + 6, a.y1);
        }
    }
}

// ------------------------------------------------------------------------------------------ K_sp_threshold
// grid (ceil(HW / SP_T), K): mask k = logits[rows[k]] > t as 0/1 bytes (the out_masks layout)
__global__ __launch_bounds__(SP_T) void k_sp_threshold(const float* __restrict__ logits, const int* __restrict__ rows, int HW, float t,
                                                       unsigned char* __restrict__ masks) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    if (i >= HW) return;
    masks[(size_t)k * HW + i] = logits[(size_t)rows[k] * HW + i] > t ? 1 : 0;
}
// out[j] = masks[sel[j]]
__global__ __launch_bounds__(SP_T) void k_sp_gather(const unsigned char* __restrict__ masks, const int* __restrict__ sel, int HW,
                                                    unsigned char* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
    if (i >= HW) return;
    out[(size_t)j * HW + i] = masks[(size_t)sel[j] * HW + i];
}

// ------------------------------------------------------------------------------------------ batched 8-connected labelling
// All kernels: grid (ceil(HW / SP_T), K), lab / cnt i32 [K][HW].  The pixels of the class ((mask != 0) == fg) are labelled.
// A pixel starts with the index of the first pixel of its horizontal run inside the wave's 64 pixels (a ballot tells every lane
// where its run began), not with its own: the long runs of a mask's background are joined before the first scan.
__global__ __launch_bounds__(SP_T) void k_spcc_init(const unsigned char* __restrict__ masks, int HW, int W, int fg, int* __restrict__ lab,
                                                    int* __restrict__ cnt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
    const size_t g = (size_t)blockIdx.y * HW + min(i, HW - 1);
    const bool in = i < HW && ((masks[g] != 0) ? 1 : 0) == fg;
    const bool left_in = __shfl_up(in ? 1 : 0, 1u) != 0;
    const unsigned long long goes_on = __ballot(in && lane > 0 && left_in && i % W != 0);      // lanes whose left neighbour is of their run
    if (i >= HW) return;
    const unsigned long long starts = ~goes_on & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));  // run starts at or below this lane (bit 0 is set)
    lab[g] = in ? i - (lane - (63 - __clzll(starts))) : SP_NONE;
    cnt[g] = 0;
}
__global__ __launch_bounds__(SP_T) void k_spcc_scan(int H, int W, int* __restrict__ lab_all, int* __restrict__ changed) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= H * W) return;
    int* lab = lab_all + (size_t)blockIdx.y * H * W;
    const int l = lab[i];
    if (l == SP_NONE) return;
    const int r = i / W, c = i - r * W;
    int m = l;
    for (int dr = -1; dr <= 1; ++dr)
        for (int dc = -1; dc <= 1; ++dc) {
            const int rr = r + dr, cc = c + dc;
            if ((!dr && !dc) || rr < 0 || rr >= H || cc < 0 || cc >= W) continue;
            const int q = lab[rr * W + cc];
            if (q < m) m = q;                      // (SP_NONE is the largest int)
        }
    if (m < l) {
        atomicMin(&lab[l], m);                     // hook the old representative as well
        atomicMin(&lab[i], m);
        *changed = 1;
    }
}
__global__ __launch_bounds__(SP_T) void k_spcc_flatten(int HW, int* __restrict__ lab_all) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= HW) return;
    int* lab = lab_all + (size_t)blockIdx.y * HW;
    int l = lab[i];
    if (l == SP_NONE) return;
    for (;;) {
        const int p = lab[l];
        if (p == l) break;
        l = p;
    }
    lab[i] = l;
}
// cnt[root] = pixels of the component: one atomic per group of lanes of a wave with the same label
__global__ __launch_bounds__(SP_T) void k_spcc_count(int HW, const int* __restrict__ lab_all, int* __restrict__ cnt_all) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
    const int l = i < HW ? lab_all[(size_t)blockIdx.y * HW + i] : SP_NONE;
    int* cnt = cnt_all + (size_t)blockIdx.y * HW;
    bool todo = l != SP_NONE;
    for (;;) {
        const unsigned long long open = __ballot(todo);
        if (!open) break;
        const int leader = __ffsll(open) - 1;
        const int ll = __shfl(l, leader);
        const bool same = todo && l == ll;
        const unsigned long long group = __ballot(same);
        if (lane == leader) atomicAdd(&cnt[ll], __popcll(group));
        if (same) todo = false;
    }
}
// holes: a background component of fewer than `area` pixels becomes foreground; flags[k] |= 1 where one exists
__global__ __launch_bounds__(SP_T) void k_spcc_fill(int HW, const int* __restrict__ lab, const int* __restrict__ cnt, int area,
                                                    unsigned char* __restrict__ masks, int* __restrict__ flags) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= HW) return;
    const size_t base = (size_t)blockIdx.y * HW;
    const int l = lab[base + i];
    if (l == SP_NONE || cnt[base + l] >= area) return;
    masks[base + i] = 1;
    flags[blockIdx.y] = 1;
}
// islands, first half: per mask whether a component below / not below `area` exists (flags bit 1 / bit 2) and the largest
// component, among equally large ones the one whose first pixel comes first: best = max of (size << 24 | 0xffffff - root)
__global__ __launch_bounds__(SP_T) void k_spcc_roots(int HW, const int* __restrict__ lab, const int* __restrict__ cnt, int area,
                                                     int* __restrict__ flags, unsigned long long* __restrict__ best) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= HW) return;
    const size_t base = (size_t)blockIdx.y * HW;
    if (lab[base + i] != i) return;
    const int c = cnt[base + i];
    atomicOr(&flags[blockIdx.y], c < area ? 2 : 4);
    atomicMax(&best[blockIdx.y], ((unsigned long long)c << 24) | (unsigned long long)(0xffffff - i));
}
// islands, second half: where a small component exists only the components of at least `area` pixels stay, or the largest
__global__ __launch_bounds__(SP_T) void k_spcc_drop(int HW, const int* __restrict__ lab, const int* __restrict__ cnt, int area,
                                                    const int* __restrict__ flags, const unsigned long long* __restrict__ best,
                                                    unsigned char* __restrict__ masks) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= HW) return;
    const size_t base = (size_t)blockIdx.y * HW;
    const int l = lab[base + i], f = flags[blockIdx.y];
    if (l == SP_NONE || !(f & 2)) return;
    const bool keep = (f & 4) ? cnt[base + l] >= area : l == 0xffffff - (int)(best[blockIdx.y] & 0xffffffull);
    if (!keep) masks[base + i] = 0;
}

// ------------------------------------------------------------------------------------------ run-length coding
// grid (ceil(W / 64), n_out), 64 threads: column x of mask sel[j]: value changes on the way down, the step from the previous
// column's last pixel (column 0: from a 0 in front of the image) included, and the position (x * H + y) of the last one (-1: none)
__global__ __launch_bounds__(64) void k_sp_rle_count(const unsigned char* __restrict__ masks, const int* __restrict__ sel, int H, int W,
                                                     int* __restrict__ ntrans, int* __restrict__ lastpos) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
    if (x >= W) return;
    const unsigned char* m = masks + (size_t)sel[j] * H * W;
    unsigned char prev = x ? m[(size_t)(H - 1) * W + x - 1] : 0;
    int n = 0, last = -1;
    for (int y = 0; y < H; ++y) {
        const unsigned char v = m[(size_t)y * W + x];
        if (v != prev) ++n, last = x * H + y;
        prev = v;
    }
    ntrans[(size_t)j * W + x] = n;
    lastpos[(size_t)j * W + x] = last;
}
// a wave per mask (grid n_out, 64 threads): col_off = counts in front of the column, prevpos = position of the last change in
// front of the column (0: the start of the image), total[j] = changes + 1 = the mask's counts
__global__ __launch_bounds__(64) void k_sp_rle_scan(int W, const int* __restrict__ ntrans, const int* __restrict__ lastpos,
                                                    int* __restrict__ col_off, int* __restrict__ prevpos, int* __restrict__ total) {
    const int lane = threadIdx.x, j = blockIdx.x;
    int carry = 0, carry_pos = 0;
    for (int x0 = 0; x0 < W; x0 += 64) {
        const int x = x0 + lane;
        const int n = x < W ? ntrans[(size_t)j * W + x] : 0, lp = x < W ? lastpos[(size_t)j * W + x] : -1;
        int incl = n, mx = lp;
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, (unsigned)d), upm = __shfl_up(mx, (unsigned)d);
            if (lane >= d) incl += up, mx = max(mx, upm);
        }
        int before = __shfl_up(mx, 1u);                  // inclusive maximum of the lanes in front
        if (lane == 0) before = -1;
        if (x < W) {
            col_off[(size_t)j * W + x] = carry + incl - n;
            prevpos[(size_t)j * W + x] = max(carry_pos, before);
        }
        carry += __shfl(incl, 63);
        carry_pos = max(carry_pos, __shfl(mx, 63));
    }
    if (lane == 0) total[j] = carry + 1;
}
// the walk of k_sp_rle_count again: counts[run_off[j] + col_off + n] = position - previous position; the last column's lane
// closes the record with H * W - last position
__global__ __launch_bounds__(64) void k_sp_rle_write(const unsigned char* __restrict__ masks, const int* __restrict__ sel, int H, int W,
                                                     const int* __restrict__ col_off, const int* __restrict__ prevpos,
                                                     const long long* __restrict__ run_off, unsigned* __restrict__ counts) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
    if (x >= W) return;
    const unsigned char* m = masks + (size_t)sel[j] * H * W;
    unsigned* out = counts + run_off[j] + col_off[(size_t)j * W + x];
    unsigned char prev = x ? m[(size_t)(H - 1) * W + x - 1] : 0;
    int pos = prevpos[(size_t)j * W + x];
    for (int y = 0; y < H; ++y) {
        const unsigned char v = m[(size_t)y * W + x];
        if (v != prev) {
            const int t = x * H + y;
            *out++ = (unsigned)(t - pos);
            pos = t;
        }
        prev = v;
    }
    if (x == W - 1) *out = (unsigned)(H * W - pos);
}

// ------------------------------------------------------------------------------------------ the call
namespace {
struct SpLast {                 // what hmsg_test_sam_post_last reports: the last call of this thread
    int rounds_holes = 0, rounds_islands = 0;
    double stats_ms = 0.0;
};
thread_local SpLast g_sp_last;

struct SpWork {
    hipStream_t s;
    int H, W, HW;
    DevBuf<int> flag;
    // seven integers per mask of `data` (rows: which rows, or all n in order), read back
    template <typename T>
    std::vector<SpStats> stats(const T* data, const int* d_rows, int n, float t_hi, float t_mid, float t_lo, hipEvent_t before = nullptr,
                               hipEvent_t after = nullptr) {
        std::vector<SpStats> st((size_t)n, SP_STATS_INIT);
        if (!n) return st;
        DevBuf<int> d;
        d.alloc((size_t)n * 7);
        HIP_TRY(hipMemcpyAsync(d.p, st.data(), (size_t)n * 28, hipMemcpyHostToDevice, s));
        if (before) HIP_TRY(hipEventRecord(before, s));
        hipLaunchKernelGGL(k_sp_stats<T>, dim3(sp_stats_blocks(HW), (unsigned)n), dim3(SP_STATS_THREADS), 0, s, data, d_rows, HW, W, t_hi, t_mid,
                           t_lo, d.p);
        if (after) HIP_TRY(hipEventRecord(after, s));
        HMSG_CHECK_LAUNCH();
        HIP_TRY(hipMemcpyAsync(st.data(), d.p, (size_t)n * 28, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        return st;
    }
    // labels of the class fg of all K masks; returns the rounds it took
    int components(const unsigned char* masks, int K, int fg, int* lab, int* cnt) {
        const dim3 g(cdiv((size_t)HW, SP_T), (unsigned)K), b(SP_T);
        flag.ensure(4);
        hipLaunchKernelGGL(k_spcc_init, g, b, 0, s, masks, HW, W, fg, lab, cnt);
        int round = 0;
        for (; round < 4096;) {
            ++round;
            HIP_TRY(hipMemsetAsync(flag.p, 0, 16, s));
            for (int k = 0; k < 4; ++k) {               // every scan of the round has a flag of its own in the one read-back:
                hipLaunchKernelGGL(k_spcc_scan, g, b, 0, s, H, W, lab, flag.p + k);
                hipLaunchKernelGGL(k_spcc_flatten, g, b, 0, s, HW, lab);
            }
            int ch[4] = {0, 0, 0, 0};
            HIP_TRY(hipMemcpyAsync(ch, flag.p, 16, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            if (!ch[3]) break;                          // the last one changed nothing: the labels are final
        }
        hipLaunchKernelGGL(k_spcc_count, g, b, 0, s, HW, (const int*)lab, cnt);
        HMSG_CHECK_LAUNCH();
        return round;
    }
};

bool finite_f(float v) { return std::isfinite(v); }

void sam_post(const hmsg_sam_post_params& prm, int N, int H, int W, const float* logits, const float* iou_preds, int max_out,
              long long counts_cap, int32_t* n_out, int64_t* n_counts, int32_t* keep_idx, uint32_t* counts, int64_t* run_off,
              double* bbox_xywh, int32_t* area, float* stability_score, uint8_t* out_masks, double* device_ms) {
    HMSG_REQUIRE(N >= 0 && H >= 1 && W >= 1 && max_out >= 0, HMSG_ERR_INVALID, "hmsg_sam_postprocess: N, max_out >= 0 and H, W >= 1");
    HMSG_REQUIRE(finite_f(prm.pred_iou_thresh) && finite_f(prm.stability_score_thresh) && finite_f(prm.stability_score_offset) &&
                     finite_f(prm.mask_threshold) && finite_f(prm.box_nms_thresh),
                 HMSG_ERR_INVALID, "hmsg_sam_postprocess: a parameter is not finite");
    HMSG_REQUIRE(prm.min_mask_region_area >= 0, HMSG_ERR_INVALID, "hmsg_sam_postprocess: min_mask_region_area < 0");
    HMSG_REQUIRE((long long)H * W < (1ll << 24), HMSG_ERR_UNSUPPORTED,
                 "hmsg_sam_postprocess: H * W >= 2^24 (the float32 pixel counts of the stability score would not be exact)");
    g_sp_last = SpLast();
    const int HW = H * W;
    ScopedStream s(hipStreamNonBlocking);
    ScopedEvent ev0, ev1, ev2, ev3;
    SpWork wk{s, H, W, HW};
    // the three thresholds, formed in float32
    const float t_mid = prm.mask_threshold;
    const float t_hi = prm.mask_threshold + prm.stability_score_offset, t_lo = prm.mask_threshold - prm.stability_score_offset;

    // ---- step 1 on the host, steps 2 - 4 from the statistics of the rows it kept
    std::vector<float> iou((size_t)N);
    if (N) read_in(iou.data(), iou_preds, (size_t)N * 4);
    const std::vector<int32_t> rows = sp_iou_filter(N, iou.data(), prm.pred_iou_thresh);
    const int R = (int)rows.size();
    DevBuf<float> own_logits;
    DevBuf<int> d_rows;
    const float* d_logits = nullptr;
    std::vector<SpStats> st;
    HIP_TRY(hipEventRecord(ev0, s));
    if (R) {
        d_logits = stage_in(own_logits, logits, (size_t)N * HW, s, Up::bounce);
        d_rows.alloc((size_t)R);
        HIP_TRY(hipMemcpyAsync(d_rows.p, rows.data(), (size_t)R * 4, hipMemcpyHostToDevice, s));
        st = wk.stats(d_logits, (const int*)d_rows.p, R, t_hi, t_mid, t_lo, ev1, ev2);
    }
    const std::vector<int32_t> first = sp_first_pass(rows, st, iou.data(), prm.stability_score_thresh, prm.box_nms_thresh);
    const int K = (int)first.size();

    // ---- the survivors as 0/1 bytes, step 5 on them
    DevBuf<unsigned char> masks;
    std::vector<SpStats> st_fin((size_t)K);
    std::vector<int32_t> final_k((size_t)K);            // positions in `first`, in output order
    for (int k = 0; k < K; ++k) st_fin[(size_t)k] = st[(size_t)first[(size_t)k]], final_k[(size_t)k] = k;
    if (K) {
        std::vector<int32_t> krows((size_t)K);
        for (int k = 0; k < K; ++k) krows[(size_t)k] = rows[(size_t)first[(size_t)k]];
        DevBuf<int> d_krows;
        d_krows.alloc((size_t)K);
        HIP_TRY(hipMemcpyAsync(d_krows.p, krows.data(), (size_t)K * 4, hipMemcpyHostToDevice, s));
        masks.alloc((size_t)K * HW);
        const dim3 g(cdiv((size_t)HW, SP_T), (unsigned)K), b(SP_T);
        hipLaunchKernelGGL(k_sp_threshold, g, b, 0, s, d_logits, (const int*)d_krows.p, HW, t_mid, masks.p);
        HMSG_CHECK_LAUNCH();
        HIP_TRY(hipStreamSynchronize(s));              // (krows is free again)
        if (prm.min_mask_region_area > 0) {
            const int A = prm.min_mask_region_area;
            DevBuf<int> lab, cnt, flags;
            DevBuf<unsigned long long> best;
            lab.alloc((size_t)K * HW);
            cnt.alloc((size_t)K * HW);
            flags.alloc((size_t)K);
            best.alloc((size_t)K);
            flags.zero(s);
            best.zero(s);
            g_sp_last.rounds_holes = wk.components(masks.p, K, 0, lab.p, cnt.p);
            hipLaunchKernelGGL(k_spcc_fill, g, b, 0, s, HW, (const int*)lab.p, (const int*)cnt.p, A, masks.p, flags.p);
            g_sp_last.rounds_islands = wk.components(masks.p, K, 1, lab.p, cnt.p);
            hipLaunchKernelGGL(k_spcc_roots, g, b, 0, s, HW, (const int*)lab.p, (const int*)cnt.p, A, flags.p, best.p);
            hipLaunchKernelGGL(k_spcc_drop, g, b, 0, s, HW, (const int*)lab.p, (const int*)cnt.p, A, (const int*)flags.p,
                               (const unsigned long long*)best.p, masks.p);
            HMSG_CHECK_LAUNCH();
            std::vector<int> fl((size_t)K);
            HIP_TRY(hipMemcpyAsync(fl.data(), flags.p, (size_t)K * 4, hipMemcpyDeviceToHost, s));
            st_fin = wk.stats((const unsigned char*)masks.p, (const int*)nullptr, K, 0.5f, 0.5f, 0.5f);     // (waits for the stream)
            std::vector<char> changed((size_t)K);
            for (int k = 0; k < K; ++k) changed[(size_t)k] = (fl[(size_t)k] & 3) ? 1 : 0;
            final_k = sp_second_pass(st_fin, changed, prm.box_nms_thresh);
        }
    }
    const int n = (int)final_k.size();

    // ---- step 6: the records.  Their sizes first: nothing of the caller's is written before both capacities are known to do
    DevBuf<int> d_sel, ntrans, lastpos, col_off, prevpos, total;
    std::vector<long long> roff((size_t)n + 1, 0);
    if (n) {
        d_sel.alloc((size_t)n);
        HIP_TRY(hipMemcpyAsync(d_sel.p, final_k.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
        ntrans.alloc((size_t)n * W);
        lastpos.alloc((size_t)n * W);
        col_off.alloc((size_t)n * W);
        prevpos.alloc((size_t)n * W);
        total.alloc((size_t)n);
        hipLaunchKernelGGL(k_sp_rle_count, dim3(cdiv((size_t)W, 64), (unsigned)n), dim3(64), 0, s, (const unsigned char*)masks.p,
                           (const int*)d_sel.p, H, W, ntrans.p, lastpos.p);
        hipLaunchKernelGGL(k_sp_rle_scan, dim3((unsigned)n), dim3(64), 0, s, W, (const int*)ntrans.p, (const int*)lastpos.p, col_off.p,
                           prevpos.p, total.p);
        HMSG_CHECK_LAUNCH();
        std::vector<int> tot((size_t)n);
        HIP_TRY(hipMemcpyAsync(tot.data(), total.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (int j = 0; j < n; ++j) roff[(size_t)j + 1] = roff[(size_t)j] + tot[(size_t)j];
    }
    *n_out = n;
    if (n_counts) *n_counts = roff[(size_t)n];
    if (n > max_out || roff[(size_t)n] > counts_cap)
        throw hmsg_error{HMSG_ERR_INVALID, "hmsg_sam_postprocess: " + std::to_string(n) + " masks with " + std::to_string(roff[(size_t)n]) +
                                               " counts survive, the arrays hold max_out = " + std::to_string(max_out) +
                                               " masks and counts_cap = " + std::to_string(counts_cap) +
                                               " counts (n_out and n_counts say what is needed)"};
    if (n) {
        HMSG_REQUIRE(keep_idx && bbox_xywh && area && stability_score, HMSG_ERR_INVALID,
                     "hmsg_sam_postprocess: null keep_idx / bbox_xywh / area / stability_score");
        DevBuf<long long> d_roff;
        DevBuf<unsigned> own_counts;
        DevBuf<unsigned char> own_out;
        d_roff.alloc((size_t)n + 1);
        HIP_TRY(hipMemcpyAsync(d_roff.p, roff.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, s));
        unsigned* p_counts = stage_out(own_counts, counts, (size_t)roff[(size_t)n]);
        hipLaunchKernelGGL(k_sp_rle_write, dim3(cdiv((size_t)W, 64), (unsigned)n), dim3(64), 0, s, (const unsigned char*)masks.p,
                           (const int*)d_sel.p, H, W, (const int*)col_off.p, (const int*)prevpos.p, (const long long*)d_roff.p, p_counts);
        HMSG_CHECK_LAUNCH();
        unstage_out(counts, p_counts, (size_t)roff[(size_t)n], s);
        if (out_masks) {
            unsigned char* p_out = stage_out(own_out, out_masks, (size_t)n * HW);
            hipLaunchKernelGGL(k_sp_gather, dim3(cdiv((size_t)HW, SP_T), (unsigned)n), dim3(SP_T), 0, s, (const unsigned char*)masks.p,
                               (const int*)d_sel.p, HW, p_out);
            HMSG_CHECK_LAUNCH();
            unstage_out(out_masks, p_out, (size_t)n * HW, s);
        }
        HIP_TRY(hipEventRecord(ev3, s));
        HIP_TRY(hipStreamSynchronize(s));
        std::vector<int32_t> o_keep((size_t)n), o_area((size_t)n);
        std::vector<float> o_stab((size_t)n);
        std::vector<double> o_box((size_t)n * 4);
        for (int j = 0; j < n; ++j) {
            const size_t k = (size_t)final_k[(size_t)j], r = (size_t)first[k];
            const SpBox bx = sp_box(st_fin[k]);
            o_keep[(size_t)j] = rows[r];
            o_area[(size_t)j] = st_fin[k].n_mid;
            o_stab[(size_t)j] = sp_stability(st[r]);
            o_box[(size_t)j * 4 + 0] = bx.x0;                       // box_xyxy_to_xywh
            o_box[(size_t)j * 4 + 1] = bx.y0;
            o_box[(size_t)j * 4 + 2] = bx.x1 - bx.x0;
            o_box[(size_t)j * 4 + 3] = bx.y1 - bx.y0;
        }
        write_out(keep_idx, o_keep.data(), (size_t)n * 4);
        write_out(area, o_area.data(), (size_t)n * 4);
        write_out(stability_score, o_stab.data(), (size_t)n * 4);
        write_out(bbox_xywh, o_box.data(), (size_t)n * 32);
    } else {
        HIP_TRY(hipEventRecord(ev3, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    write_out(run_off, roff.data(), ((size_t)n + 1) * 8);
    float ms = 0.0f;
    if (R) {
        HIP_TRY(hipEventElapsedTime(&ms, ev1, ev2));
        g_sp_last.stats_ms = ms;
    }
    HIP_TRY(hipEventElapsedTime(&ms, ev0, ev3));
    if (device_ms) *device_ms = ms;
}
}  // namespace

extern "C" void hmsg_sam_post_default_params(hmsg_sam_post_params* p) {
    if (!p) return;
    p->pred_iou_thresh = 0.88f;
    p->stability_score_thresh = 0.95f;
    p->stability_score_offset = 1.0f;
    p->mask_threshold = 0.0f;
    p->box_nms_thresh = 0.7f;
    p->min_mask_region_area = 0;
}

extern "C" int hmsg_sam_postprocess(int32_t device_id, const hmsg_sam_post_params* prm, int32_t N, int32_t H, int32_t W, const float* logits,
                                    const float* iou_preds, int32_t max_out, int64_t counts_cap, int32_t* n_out, int64_t* n_counts,
                                    int32_t* keep_idx, uint32_t* counts, int64_t* run_off, double* bbox_xywh, int32_t* area,
                                    float* stability_score, uint8_t* out_masks, double* device_ms) {
    if (!prm || !logits || !iou_preds || !n_out || !run_off || !counts) return HMSG_ERR_INVALID;
    return hmsg_boundary("hmsg_sam_postprocess", device_id, [&] {
        sam_post(*prm, N, H, W, logits, iou_preds, max_out, counts_cap, n_out, n_counts, keep_idx, counts, run_off, bbox_xywh, area,
                 stability_score, out_masks, device_ms);
    });
}

extern "C" int hmsg_test_sam_post_last(int32_t* rounds_holes, int32_t* rounds_islands, double* stats_ms) {
    if (rounds_holes) *rounds_holes = g_sp_last.rounds_holes;
    if (rounds_islands) *rounds_islands = g_sp_last.rounds_islands;
    if (stats_ms) *stats_ms = g_sp_last.stats_ms;
    return HMSG_OK;
}

// the labelling for the library's other image stages (hmsg_common.h)
int hmsg_cc8_components(hipStream_t s, const unsigned char* masks, int K, int H, int W, int fg, int* lab, int* cnt) {
    SpWork wk{s, H, W, H * W};
    return wk.components(masks, K, fg, lab, cnt);
}
