// The host arithmetic of the CLIP preprocess (include/hmsg.h: hmsg_clip_preprocess_batch), in plain C++ without any HIP: the
// size rules of torchvision's Resize / CenterCrop, the coefficient tables of Pillow's 8-bit BICUBIC resample
// (src/libImaging/Resample.c: precompute_coeffs + normalize_coeffs_8bpc) and the 3 x 256 table of ToTensor + Normalize.
// The device does integer work on these tables only, so no result depends on device double arithmetic.
//
// Everything here is double (or float) arithmetic in Pillow's / torch's operation order, one rounding per operation: compile
// with floating-point contraction off (-ffp-contract=off, as every source of the library is), and never with -ffast-math.
// tests/host_cpp/resample_coef.cpp prints these tables for tests/test_resample_coef.py.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace hmsg_resample {

constexpr int PRECISION_BITS = 32 - 8 - 2;      // Pillow's: coefficients are rounded to 1 / 2^22

// Resize(S) on a PIL image (torchvision, a single int size): the shorter side becomes S, the other int(S * long / short)
inline void resize_dims(int H, int W, int S, int& w2, int& h2) {
    if (W <= H) {
        w2 = S;
        h2 = (int)((double)((int64_t)S * H) / (double)W);
    } else {
        h2 = S;
        w2 = (int)((double)((int64_t)S * W) / (double)H);
    }
}
// CenterCrop(S): int(round((n - S) / 2.0)), Python's round: halves go to the even integer.  n >= S.
inline int center_crop_offset(int n, int S) {
    const int d = n - S, q = d / 2;
    return (d & 1) ? q + (q & 1) : q;
}

inline double bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// One axis inSize -> outSize, output indices [first, first + count): bounds[2 i] = first source index, bounds[2 i + 1] =
// number of taps, kk[i * ksize + x] = the int32 coefficient of tap x (zero past the taps).  Returns ksize.
inline int coefficients(int inSize, int outSize, int first, int count, std::vector<int32_t>& bounds, std::vector<int32_t>& kk) {
    double scale, filterscale;
    scale = filterscale = (double)inSize / outSize;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = 2.0 * filterscale;
    const int ksize = (int)std::ceil(support) * 2 + 1;
    bounds.assign((size_t)count * 2, 0);
    kk.assign((size_t)count * ksize, 0);
    std::vector<double> w((size_t)ksize);
    for (int i = 0; i < count; ++i) {
        const int xx = first + i;
        const double center = (xx + 0.5) * scale;
        const double ss = 1.0 / filterscale;
        double ww = 0.0;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > inSize) xmax = inSize;
        xmax -= xmin;
        for (int x = 0; x < xmax; ++x) {
            w[x] = bicubic((x + xmin - center + 0.5) * ss);
            ww += w[x];
        }
        for (int x = 0; x < xmax; ++x) {
            if (ww != 0.0) w[x] /= ww;
            kk[(size_t)i * ksize + x] = w[x] < 0 ? (int32_t)(-0.5 + w[x] * (1 << PRECISION_BITS)) : (int32_t)(0.5 + w[x] * (1 << PRECISION_BITS));
        }
        bounds[(size_t)i * 2] = xmin;
        bounds[(size_t)i * 2 + 1] = xmax;
    }
    return ksize;
}

// float32 -> float16 bits, round to nearest even (what torch's .half() and numpy's astype(float16) do)
inline uint16_t f32_to_f16_bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    const uint32_t sign = (u >> 16) & 0x8000u;
    u &= 0x7fffffffu;
    if (u >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | (u > 0x7f800000u ? 0x200u : 0u));   // inf / nan
    if (u >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                                       // rounds to inf
    if (u < 0x33000001u) return (uint16_t)sign;                                                    // rounds to zero
    int e = (int)(u >> 23) - 127;
    uint32_t m = (u & 0x7fffffu) | 0x800000u;
    int shift = 13;
    if (e < -14) {                       // subnormal half
        shift += -14 - e;
        e = -15;
    }
    const uint32_t half = 1u << (shift - 1), rest = m & ((1u << shift) - 1);
    uint32_t r = m >> shift;
    if (rest > half || (rest == half && (r & 1))) ++r;
    // r carries the implicit bit for normals: (e + 15) << 10 plus r - 0x400; a mantissa overflow carries into the exponent
    return (uint16_t)(sign | (uint32_t)(((e + 15) << 10) + (int)r - (e == -15 ? 0 : 0x400)));
}

// ToTensor + Normalize per byte value: lut[c * 256 + v] = ((float)v / 255.0f - mean[c]) / std[c], float32 operations
inline void normalize_table(const float mean[3], const float stdv[3], float lut[768]) {
    for (int c = 0; c < 3; ++c)
        for (int v = 0; v < 256; ++v) {
            const float x = (float)v / 255.0f;
            const float y = x - mean[c];
            lut[c * 256 + v] = y / stdv[c];
        }
}

}  // namespace hmsg_resample
