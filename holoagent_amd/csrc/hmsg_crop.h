// The crop / resize of hmsg_crop.hip in the three steps both of its callers take (hmsg_crop_resize_batch, and
// hmsg_frame_encoder_inputs of hmsg_clip_preprocess.hip): one statement of the rectangles and one kernel.
#pragma once
#include "hmsg_common.h"

#include <vector>

struct hmsg_crop_scratch {          // the rectangle table of one launch, host and device side: keep it until the stream has passed the launch
    std::vector<unsigned char> host;
    DevBuf<unsigned char> dev;
};

// 1. Host work only: the rectangles of the crops asked for (bbox f64 [M][4], host memory).  An empty crop throws HMSG_ERR_INVALID:
//    call it before a stream exists or anything is staged, so that a refused call leaves no work behind.
void hmsg_crop_rects(int H, int W, int M, const double* bbox, double bbox_margin, bool want_plain, bool want_masked,
                     hmsg_crop_scratch& scratch);
// 2. The table goes up on s.
void hmsg_crop_upload(hmsg_crop_scratch& scratch, hipStream_t s);
// 3. The launch on s.  image / segs / out_* are device memory; an output not asked for in step 1 is null.
void hmsg_crop_launch(int H, int W, const unsigned char* p_img, const unsigned char* p_seg, int out_size, unsigned char* p_plain,
                      unsigned char* p_masked, const hmsg_crop_scratch& scratch, hipStream_t s);
