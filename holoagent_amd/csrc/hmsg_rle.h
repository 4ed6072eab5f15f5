// Masks handed over as SAM's uncompressed run-length records (include/hmsg.h: hmsg_add_frame_features_rle; the format is
// stated there).  hmsg_rle.hip holds the kernels; this is what the entry points drive them through.
#pragma once
#include "hmsg_common.h"

// One hand-over: n frames, T = sum of their mask counts, the caller's counts / run_off (host or device memory).
//   hmsg_rle_begin    reads and checks run_off on the host, cuts the frames into chunks whose counts fit the staging budget, runs
//                     k_rle_scan over every chunk and reads ONE flag back: a mask without counts or whose counts do not sum to
//                     H * W is HMSG_ERR_INVALID naming the mask, before any bitset is written.
//   hmsg_rle_decode   k_rle_bitset for the frames of chunk c into `bits` (u64 [frames of the chunk][H*W][NW]).  With a single
//                     chunk -- every hand-over but a very large one -- its run starts are still resident from the check.
struct hmsg_rle_handover {
    int H = 0, W = 0, n = 0;
    const uint32_t* counts = nullptr;      // the caller's
    bool counts_dev = false;
    std::vector<long long> run_off;        // host copy [T + 1]
    std::vector<int> mask_off;             // [n + 1]: first mask of frame f in the hand-over's mask order
    std::vector<int> chunk_first;          // [chunks + 1]: first frame of every chunk
    int resident = -1;                     // the chunk whose run starts are in `starts`
    DevBuf<uint32_t> st_counts, starts;
    DevBuf<long long> d_run_off;
    DevBuf<int> d_mask_off, d_nmask, d_bad;
    DevBuf<unsigned long long> totals;     // [T] sum of every mask's counts
    int chunks() const { return (int)chunk_first.size() - 1; }
};
// nm [n]: masks per frame, already known to lie in [0, M]; max_chunk_frames: the caller's own bound on a chunk
void hmsg_rle_begin(hmsg_rle_handover& r, int H, int W, int n, const int* nm, const uint32_t* counts, const int64_t* run_off,
                    int max_chunk_frames, hipStream_t s, Prof* prof);
void hmsg_rle_decode(hmsg_rle_handover& r, int c, int M, int NW, unsigned long long* bits, hipStream_t s, Prof* prof);
