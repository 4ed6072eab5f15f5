// The CLIP preprocess on the device: uint8 images -> the encoder-ready tensor, every bit equal to open_clip's inference
// transform on a PIL image -- Resize(S, BICUBIC), CenterCrop(S), ToTensor, Normalize(mean, std) -- which the reference runs on
// the host, one image at a time, on every crop and every frame (utils/clip_utils.py:72-73, 88-89, called from
// perception/models/sam_clip_feats_extractor.py:147-158, and graph.py:1127 for the room level's view embeddings).
//
// What is pinned: Pillow 12.2's 8-bit BICUBIC resample (ImagingResample: horizontal pass, a uint8 image, vertical pass; a pass
// whose lengths are equal is skipped) and torchvision's Resize / CenterCrop size rules as hmsg_resample_coef.h states them.
// The coefficient tables are made on the host in double (hmsg_resample_coef.h) and uploaded with the call; the kernel does
// integer multiply-adds, shifts and clamps, and looks the float up in a 3 x 256 table that the host made as well.
//
// k_clip_preprocess: one workgroup per (image, tile of output rows).  Only the S x S pixels inside the centre crop are
// computed.  Pass 1 resamples, along x, the source rows that the tile's vertical taps need, for the S surviving columns, into
// LDS as bytes; pass 2 runs the vertical taps from LDS, and its epilogue writes the NCHW planes (and the bytes, if asked).
// The tile's rows are chosen at launch from the LDS budget, so a large down-scale gets fewer rows per tile.
#include "hmsg_boundary.h"
#include "hmsg_crop.h"
#include "hmsg_resample_coef.h"

#include <cmath>

namespace {

constexpr int CLIP_MAX_SIDE = 16384;             // source sides above this: HMSG_ERR_UNSUPPORTED
constexpr int CLIP_MAX_SIZE = 1024;              // output side
constexpr int CLIP_TILE_ROWS = 16;
constexpr size_t CLIP_LDS_BUDGET = 60 * 1024;    // bytes of dynamic LDS per workgroup (64 KB need no opt-in; 3 KB are the table's)
constexpr int PB = hmsg_resample::PRECISION_BITS;

struct ClipGeom {
    int H, W, S;
    int left, top;            // of the centre crop, in the resized image
    int skip;                 // no resampling: with Resize's size rule either both passes have equal lengths (Pillow copies) or neither
    int hks, vks;             // row length of hk / vk: the taps of an output index, zero-padded to a multiple of 4
    int tile_rows, f16;
    int o_hb, o_hk, o_vb, o_vk, o_lut;   // offsets (int32 units) into the table
    unsigned long long src_bytes;        // of the whole batch: no 4-byte load may pass it
};

__device__ __forceinline__ int clip8(int v) { return min(max(v >> PB, 0), 255); }

__global__ void __launch_bounds__(256) k_clip_preprocess(const unsigned char* __restrict__ images, ClipGeom g, const int* __restrict__ tab,
                                                         void* __restrict__ out, unsigned char* __restrict__ out_u8, size_t out_first) {
    HIP_DYNAMIC_SHARED(unsigned char, rows_lds)
    __shared__ unsigned s_lut[768];
    const int S = g.S, tid = threadIdx.x, b = blockIdx.y;
    const int y0 = blockIdx.x * g.tile_rows, ny = min(g.tile_rows, S - y0);
    const int* __restrict__ hb = tab + g.o_hb;
    const int* __restrict__ hk = tab + g.o_hk;
    const int* __restrict__ vb = tab + g.o_vb;
    const int* __restrict__ vk = tab + g.o_vk;
    for (int i = tid; i < 768; i += 256) s_lut[i] = (unsigned)tab[g.o_lut + i];
    // the source rows of this tile: bounds are non-decreasing in the output index
    const int r0 = g.skip ? g.top + y0 : vb[2 * y0];
    const int r1 = g.skip ? r0 + ny : vb[2 * (y0 + ny - 1)] + vb[2 * (y0 + ny - 1) + 1];
    const int nr = r1 - r0;
    const size_t img_off = (size_t)b * g.H * g.W * 3;
    if (g.skip) {                                      // equal lengths: Pillow copies
        const int rowb = S * 3;
        for (int i = tid; i < nr * rowb; i += 256) {
            const int r = i / rowb, o = i - r * rowb;
            rows_lds[i] = images[img_off + ((size_t)(r0 + r) * g.W + g.left) * 3 + o];
        }
    } else if (g.src_bytes >= 4) {
        // A pixel's taps are neighbouring pixels of one row: one unaligned 4-byte load per tap (3 bytes used).  The trip count is
        // the table's row length (a multiple of 4, zero coefficients behind the taps) for every pixel, and a tap behind the last
        // reads the last one again, so the loads of four taps are independent of everything and in flight together.  The load
        // that would pass the end of the batch starts a byte early instead.
        const size_t last4 = (size_t)g.src_bytes - 4;
        for (int i = tid; i < nr * S; i += 256) {
            const int r = i / S, x = i - r * S;
            const int xmin = hb[2 * x], nm1 = hb[2 * x + 1] - 1;
            const int4* __restrict__ k4 = (const int4*)(hk + (size_t)x * g.hks);
            const size_t p = img_off + ((size_t)(r0 + r) * g.W + xmin) * 3;
            int a0 = 1 << (PB - 1), a1 = a0, a2 = a0;
            for (int t = 0; t < g.hks; t += 4) {
                const int4 kv = k4[t >> 2];
                const int kk[4] = {kv.x, kv.y, kv.z, kv.w};
                unsigned px[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const size_t q = p + (size_t)min(t + j, nm1) * 3, a = q < last4 ? q : last4;
                    unsigned w;
                    __builtin_memcpy(&w, images + a, 4);
                    px[j] = w >> ((unsigned)(q - a) * 8);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    a0 += (int)(px[j] & 0xff) * kk[j];
                    a1 += (int)((px[j] >> 8) & 0xff) * kk[j];
                    a2 += (int)((px[j] >> 16) & 0xff) * kk[j];
                }
            }
            unsigned char* d = rows_lds + (size_t)i * 3;
            d[0] = (unsigned char)clip8(a0);
            d[1] = (unsigned char)clip8(a1);
            d[2] = (unsigned char)clip8(a2);
        }
    } else {                                           // a batch of one 1 x 1 image
        for (int i = tid; i < nr * S; i += 256) {
            const int r = i / S, x = i - r * S;
            const int xmin = hb[2 * x], n = hb[2 * x + 1];
            const int* __restrict__ k = hk + (size_t)x * g.hks;
            const unsigned char* p = images + img_off + ((size_t)(r0 + r) * g.W + xmin) * 3;
            int a0 = 1 << (PB - 1), a1 = a0, a2 = a0;
            for (int t = 0; t < n; ++t, p += 3) {
                a0 += (int)p[0] * k[t];
                a1 += (int)p[1] * k[t];
                a2 += (int)p[2] * k[t];
            }
            unsigned char* d = rows_lds + (size_t)i * 3;
            d[0] = (unsigned char)clip8(a0);
            d[1] = (unsigned char)clip8(a1);
            d[2] = (unsigned char)clip8(a2);
        }
    }
    __syncthreads();
    const size_t plane = (size_t)S * S, ob = out_first + (size_t)b;
    for (int i = tid; i < ny * S; i += 256) {
        const int yl = i / S, x = i - yl * S, y = y0 + yl;
        int v0, v1, v2;
        if (g.skip) {
            const unsigned char* p = rows_lds + (size_t)i * 3;
            v0 = p[0];
            v1 = p[1];
            v2 = p[2];
        } else {
            const int nm1 = vb[2 * y + 1] - 1, rowb = S * 3;           // (uniform trip count, taps clamped: as in pass 1)
            const int4* __restrict__ k4 = (const int4*)(vk + (size_t)y * g.vks);
            const unsigned char* p = rows_lds + ((size_t)(vb[2 * y] - r0) * S + x) * 3;
            int a0 = 1 << (PB - 1), a1 = a0, a2 = a0;
            for (int t = 0; t < g.vks; t += 4) {
                const int4 kv = k4[t >> 2];
                const int kk[4] = {kv.x, kv.y, kv.z, kv.w};
                int c0[4], c1[4], c2[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const unsigned char* q = p + min(t + j, nm1) * rowb;
                    c0[j] = q[0];
                    c1[j] = q[1];
                    c2[j] = q[2];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    a0 += c0[j] * kk[j];
                    a1 += c1[j] * kk[j];
                    a2 += c2[j] * kk[j];
                }
            }
            v0 = clip8(a0);
            v1 = clip8(a1);
            v2 = clip8(a2);
        }
        const size_t pix = (size_t)y * S + x;
        if (out_u8) {
            unsigned char* d = out_u8 + (ob * plane + pix) * 3;
            d[0] = (unsigned char)v0;
            d[1] = (unsigned char)v1;
            d[2] = (unsigned char)v2;
        }
        const unsigned f0 = s_lut[v0], f1 = s_lut[256 + v1], f2 = s_lut[512 + v2];
        if (g.f16) {
            unsigned short* d = (unsigned short*)out + ob * 3 * plane + pix;
            d[0] = (unsigned short)f0;
            d[plane] = (unsigned short)f1;
            d[2 * plane] = (unsigned short)f2;
        } else {
            unsigned* d = (unsigned*)out + ob * 3 * plane + pix;
            d[0] = f0;
            d[plane] = f1;
            d[2 * plane] = f2;
        }
    }
}

bool params_ok(const hmsg_clip_preprocess* p) {
    if (!p || p->size < 1 || p->size > CLIP_MAX_SIZE) return false;
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(p->mean[c]) || !std::isfinite(p->std[c]) || p->std[c] == 0.0f) return false;
    return true;
}

// One launch in three steps, so that an entry point has done all of its host work -- and refused what it cannot do -- before it
// creates a stream, stages an array or launches anything: plan() makes the geometry and the table of B images of H x W (host only;
// the one place that throws for a shape); upload() sends the table up on s; run() launches: `images` (device) -> rows
// [out_first, out_first + B) of out / out_u8 (device).  The object must live until the stream has passed the launch.
struct ClipLaunch {
    ClipGeom g{};
    int B = 0;
    size_t lds = 0;
    std::vector<int32_t> host;
    DevBuf<int32_t> dev;
    const int* d_tab = nullptr;
    void plan(const hmsg_clip_preprocess& prm, int B, int H, int W);
    void upload(hipStream_t s) {
        dev.alloc(host.size() + 4);             // (the kernel reads int4 rows: start at a multiple of 16 bytes)
        int32_t* up = dev.p + ((16 - (uintptr_t)dev.p % 16) % 16) / sizeof(int32_t);
        HIP_TRY(hipMemcpyAsync(up, host.data(), host.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
        d_tab = up;
    }
    void run(const unsigned char* images, void* out, unsigned char* out_u8, size_t out_first, hipStream_t s) const {
        hipLaunchKernelGGL(k_clip_preprocess, dim3(cdiv((size_t)g.S, (size_t)g.tile_rows), (unsigned)B), dim3(256), lds + 16, s, images, g, d_tab,
                           out, out_u8, out_first);
        HMSG_CHECK_LAUNCH();
    }
};
void ClipLaunch::plan(const hmsg_clip_preprocess& prm, int B_, int H, int W) {
    namespace R = hmsg_resample;
    B = B_;
    HMSG_REQUIRE(H <= CLIP_MAX_SIDE && W <= CLIP_MAX_SIDE, HMSG_ERR_UNSUPPORTED,
                 "image side above " + std::to_string(CLIP_MAX_SIDE) + " (" + std::to_string(H) + " x " + std::to_string(W) + ")");
    HMSG_REQUIRE(B <= 65535, HMSG_ERR_UNSUPPORTED, "more than 65535 images in one call");
    const int S = prm.size;
    int w2, h2;
    R::resize_dims(H, W, S, w2, h2);
    g.H = H;
    g.W = W;
    g.S = S;
    g.left = R::center_crop_offset(w2, S);
    g.top = R::center_crop_offset(h2, S);
    g.skip = w2 == W && h2 == H;          // (w2 == W <=> h2 == H: the shorter side equals S, and then int(S * long / S) = long)
    g.f16 = prm.out_f16 != 0;
    g.src_bytes = (unsigned long long)B * H * W * 3;
    std::vector<int32_t> hb, hk, vb, vk;
    // coefficient rows padded with zeros to a multiple of four taps: the kernel reads them as int4
    auto pad_rows = [&](std::vector<int32_t>& kk, int ks) {
        const int kp = (ks + 3) & ~3;
        std::vector<int32_t> o((size_t)S * kp, 0);
        for (int i = 0; i < S; ++i) std::copy(kk.begin() + (size_t)i * ks, kk.begin() + (size_t)(i + 1) * ks, o.begin() + (size_t)i * kp);
        kk.swap(o);
        return kp;
    };
    if (!g.skip) g.hks = pad_rows(hk, R::coefficients(W, w2, g.left, S, hb, hk));
    if (!g.skip) g.vks = pad_rows(vk, R::coefficients(H, h2, g.top, S, vb, vk));
    // rows per tile: the most that the tile's source rows, S x 3 bytes each, leave inside the LDS budget
    for (g.tile_rows = std::min(CLIP_TILE_ROWS, S);; g.tile_rows /= 2) {
        int most = g.tile_rows;
        if (!g.skip) {
            most = 0;
            for (int y0 = 0; y0 < S; y0 += g.tile_rows) {
                const int y1 = std::min(y0 + g.tile_rows, S) - 1;
                most = std::max(most, vb[2 * y1] + vb[2 * y1 + 1] - vb[2 * y0]);
            }
        }
        lds = (size_t)most * S * 3;
        if (lds <= CLIP_LDS_BUDGET) break;
        HMSG_REQUIRE(g.tile_rows > 1, HMSG_ERR_UNSUPPORTED,
                     "one output row of this resize needs " + std::to_string(lds) + " bytes of LDS (" + std::to_string(H) + " x " + std::to_string(W) +
                         " -> " + std::to_string(S) + "): down-scale in two steps");
    }
    float lut[768];
    R::normalize_table(prm.mean, prm.std, lut);
    std::vector<int32_t>& t = host;
    t.clear();
    auto put = [&](const std::vector<int32_t>& v) {             // (every section starts at a multiple of 16 bytes)
        t.resize((t.size() + 3) & ~(size_t)3, 0);
        const int o = (int)t.size();
        t.insert(t.end(), v.begin(), v.end());
        return o;
    };
    g.o_hb = put(hb);
    g.o_hk = put(hk);
    g.o_vb = put(vb);
    g.o_vk = put(vk);
    g.o_lut = (int)t.size();
    for (int i = 0; i < 768; ++i) {
        uint32_t bits;
        if (g.f16) bits = R::f32_to_f16_bits(lut[i]);
        else memcpy(&bits, &lut[i], 4);
        t.push_back((int32_t)bits);
    }
}

size_t out_elem(const hmsg_clip_preprocess* p) { return p->out_f16 ? 2 : 4; }

}  // namespace

extern "C" void hmsg_clip_default_preprocess(hmsg_clip_preprocess* p) {
    if (!p) return;
    p->size = 224;
    p->out_f16 = 0;
    const float mean[3] = {0.48145466f, 0.4578275f, 0.40821073f}, stdv[3] = {0.26862954f, 0.26130258f, 0.27577711f};
    for (int c = 0; c < 3; ++c) {
        p->mean[c] = mean[c];
        p->std[c] = stdv[c];
    }
}

extern "C" int hmsg_clip_preprocess_batch(int32_t device_id, const hmsg_clip_preprocess* prm, int32_t B, int32_t H, int32_t W,
                                          const uint8_t* images, void* out, uint8_t* out_u8, double* device_ms) {
    if (!params_ok(prm) || B < 0 || H <= 0 || W <= 0) return HMSG_ERR_INVALID;
    if (B == 0) return HMSG_OK;
    if (!images || !out) return HMSG_ERR_INVALID;
    return hmsg_boundary("hmsg_clip_preprocess_batch", device_id, [&] {
        ClipLaunch launch;
        launch.plan(*prm, B, H, W);                            // (refuses a shape it cannot do before anything is staged)
        ScopedStream s(hipStreamNonBlocking);
        ScopedEvent ev0, ev1;
        const size_t S = (size_t)prm->size, n_out = (size_t)B * 3 * S * S * out_elem(prm), n_u8 = (size_t)B * S * S * 3;
        DevBuf<unsigned char> d_img, d_out, d_u8;
        launch.upload(s);
        const unsigned char* p_img = stage_in(d_img, images, (size_t)B * H * W * 3, s, Up::bounce);
        unsigned char* p_out = stage_out(d_out, (unsigned char*)out, n_out);
        unsigned char* p_u8 = stage_out(d_u8, out_u8, n_u8);
        HIP_TRY(hipEventRecord(ev0, s));
        launch.run(p_img, p_out, p_u8, 0, s);
        HIP_TRY(hipEventRecord(ev1, s));
        unstage_out((unsigned char*)out, p_out, n_out, s);
        unstage_out(out_u8, p_u8, n_u8, s);
        HIP_TRY(hipStreamSynchronize(s));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, ev0, ev1));
        if (device_ms) *device_ms = ms;
    });
}

extern "C" int hmsg_frame_encoder_inputs(int32_t device_id, const hmsg_clip_preprocess* prm, int32_t H, int32_t W, const uint8_t* image,
                                         int32_t M, const uint8_t* segs, const double* bbox, double bbox_margin, int32_t crop_size,
                                         void* out, double* device_ms) {
    if (!params_ok(prm) || H <= 0 || W <= 0 || !image || !out || M < 0 || (M > 0 && (!bbox || !segs))) return HMSG_ERR_INVALID;
    if (crop_size <= 0 || (crop_size & 3)) return HMSG_ERR_INVALID;
    return hmsg_boundary("hmsg_frame_encoder_inputs", device_id, [&] {
        HMSG_REQUIRE(H <= CLIP_MAX_SIDE && W <= CLIP_MAX_SIDE && crop_size <= CLIP_MAX_SIDE, HMSG_ERR_UNSUPPORTED,
                     "image or crop side above " + std::to_string(CLIP_MAX_SIDE));
        // all host work first, and every refusal (an empty crop, a shape) with it: nothing is staged or launched before
        hmsg_crop_scratch rects;
        ClipLaunch frame, crops;
        frame.plan(*prm, 1, H, W);
        if (M) {
            crops.plan(*prm, 2 * M, crop_size, crop_size);
            hmsg_crop_rects(H, W, M, bbox, bbox_margin, true, true, rects);
        }
        ScopedStream s(hipStreamNonBlocking);
        ScopedEvent ev0, ev1;
        const size_t S = (size_t)prm->size, n_out = (size_t)(1 + 2 * M) * 3 * S * S * out_elem(prm), crop_bytes = (size_t)crop_size * crop_size * 3;
        DevBuf<unsigned char> d_img, d_seg, d_out, d_crops;
        const unsigned char* p_img = stage_in(d_img, image, (size_t)H * W * 3, s, Up::direct);
        const unsigned char* p_seg = M ? stage_in(d_seg, segs, (size_t)M * H * W, s, Up::bounce) : nullptr;
        unsigned char* p_out = stage_out(d_out, (unsigned char*)out, n_out);
        frame.upload(s);
        if (M) {
            crops.upload(s);
            hmsg_crop_upload(rects, s);
            d_crops.alloc(crop_bytes * 2 * M);                                                 // masked crops, then plain crops
        }
        HIP_TRY(hipEventRecord(ev0, s));                                                       // three launches, no host work between them
        frame.run(p_img, p_out, nullptr, 0, s);                                                // row 0: F_g's input
        if (M) {
            hmsg_crop_launch(H, W, p_img, p_seg, crop_size, d_crops.p + crop_bytes * M, d_crops.p, rects, s);
            crops.run(d_crops.p, p_out, nullptr, 1, s);
        }
        HIP_TRY(hipEventRecord(ev1, s));
        unstage_out((unsigned char*)out, p_out, n_out, s);
        HIP_TRY(hipStreamSynchronize(s));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, ev0, ev1));
        if (device_ms) *device_ms = ms;
    });
}
