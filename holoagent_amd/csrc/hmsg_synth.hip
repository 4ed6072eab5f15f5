// Benchmark utility (NOT part of the hot path): renders the synthetic posed RGB-D + mask stream of
// SURVEY.md section 8d directly into HBM so that the 1000-frame workload of BASELINE.json is resident
// before the timed region starts (a numpy renderer needs minutes for it).  Same scene model as
// holoagent_amd/synth.py: closed axis-aligned box rooms, K object boxes per room, camera inside one room
// per frame, depth = z of the first hit + Gaussian sensor noise, u16 millimetres.
//   masks 0..n_ent-1 : silhouettes of the room's entities (its objects, then its 6 faces)
//   masks n_ent..M-1 : pseudo-random rectangular tiles (overlaps allowed)
#include "hmsg_boundary.h"

#include <algorithm>

struct SynthParams {
    int H, W, M, n_frames, n_obj_total;
    double fx, fy, cx, cy;
    double noise_mm;
    unsigned long long seed;
};

__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}

__global__ void k_synth(SynthParams P, const double* __restrict__ poses, const int* __restrict__ room_of_frame,
                        const double* __restrict__ room_boxes, const double* __restrict__ obj_boxes,
                        const int* __restrict__ room_obj_off, unsigned char* __restrict__ rgb, unsigned short* __restrict__ depth,
                        unsigned char* __restrict__ masks, int* __restrict__ mask_entity) {
    const size_t HW = (size_t)P.H * P.W;
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= HW * P.n_frames) return;
    const int f = (int)(t / HW);
    const int p = (int)(t - (size_t)f * HW);
    const int y = p / P.W, x = p - y * P.W;
    const double* T = poses + (size_t)f * 16;
    const int rid = room_of_frame[f];
    double dc[3] = {((double)x + 0.5 - P.cx) / P.fx, ((double)y + 0.5 - P.cy) / P.fy, 1.0};
    double dw[3], o[3] = {T[3], T[7], T[11]};
    for (int a = 0; a < 3; ++a) dw[a] = T[a * 4] * dc[0] + T[a * 4 + 1] * dc[1] + T[a * 4 + 2] * dc[2];
    double inv[3];
    for (int a = 0; a < 3; ++a) inv[a] = 1.0 / (fabs(dw[a]) < 1e-12 ? 1e-12 : dw[a]);
    const double* rb = room_boxes + (size_t)rid * 6;
    double tfar = 1e300;
    int face_axis = 0;
    for (int a = 0; a < 3; ++a) {
        double t1 = (rb[a] - o[a]) * inv[a], t2 = (rb[3 + a] - o[a]) * inv[a];
        double tm = t1 > t2 ? t1 : t2;
        if (tm < tfar) {
            tfar = tm;
            face_axis = a;
        }
    }
    int ent = P.n_obj_total + rid * 6 + face_axis * 2 + (dw[face_axis] > 0 ? 1 : 0);
    double d = tfar;
    const int ob = room_obj_off[rid], oe = room_obj_off[rid + 1];
    for (int k = ob; k < oe; ++k) {
        const double* bx = obj_boxes + (size_t)k * 6;
        double tn = -1e300, tf = 1e300;
        for (int a = 0; a < 3; ++a) {
            double t1 = (bx[a] - o[a]) * inv[a], t2 = (bx[3 + a] - o[a]) * inv[a];
            tn = fmax(tn, fmin(t1, t2));
            tf = fmin(tf, fmax(t1, t2));
        }
        if (tn < tf && tn > 0.05 && tn < d) {
            d = tn;
            ent = k;
        }
    }
    // sensor noise
    unsigned long long h1 = mix64(P.seed ^ (0x9e3779b97f4a7c15ull * (t + 1)));
    unsigned long long h2 = mix64(h1 + 0x632be59bd9b4e019ull);
    double u1 = ((double)(h1 >> 11) + 1.0) / 9007199254740993.0, u2 = (double)(h2 >> 11) / 9007199254740992.0;
    double g = sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
    double mm = rint(d * 1000.0 + P.noise_mm * g);
    unsigned short du = (mm < 1.0 || mm > 65535.0 || d > 10.0) ? 0 : (unsigned short)mm;
    depth[t] = du;
    rgb[t * 3 + 0] = (unsigned char)((ent * 53 + 17) % 256);
    rgb[t * 3 + 1] = (unsigned char)((ent * 97 + 101) % 256);
    rgb[t * 3 + 2] = (unsigned char)((ent * 193 + 7) % 256);
    const int n_ent = (oe - ob) + 6;
    unsigned char* mf = masks + (size_t)f * P.M * HW;
    for (int i = 0; i < P.M; ++i) {
        unsigned char v;
        if (i < n_ent) {
            int e = i < (oe - ob) ? ob + i : P.n_obj_total + rid * 6 + (i - (oe - ob));
            v = ent == e;
            if (p == 0) mask_entity[(size_t)f * P.M + i] = e;
        } else {
            unsigned long long hh = mix64(P.seed * 31 + (unsigned long long)f * 1315423911ull + i);
            int hgt = P.H / 8 + (int)(hh % (unsigned)(P.H / 3 - P.H / 8));
            int wid = P.W / 8 + (int)((hh >> 16) % (unsigned)(P.W / 3 - P.W / 8));
            int y0 = (int)((hh >> 32) % (unsigned)(P.H - hgt)), x0 = (int)((hh >> 48) % (unsigned)(P.W - wid));
            v = (y >= y0 && y < y0 + hgt && x >= x0 && x < x0 + wid);
            if (y == y0 + hgt / 2 && x == x0 + wid / 2) mask_entity[(size_t)f * P.M + i] = ent;
        }
        mf[(size_t)i * HW + p] = v;
    }
}

extern "C" int hmsg_synth_render(int32_t device_id, int32_t n_frames, int32_t H, int32_t W, int32_t M, const double* K,
                                 const double* poses, const int32_t* room_of_frame, int32_t n_rooms, const double* room_boxes,
                                 int32_t n_obj, const double* obj_boxes, const int32_t* room_obj_off, double depth_noise_mm,
                                 uint64_t seed, uint8_t* rgb_dev, uint16_t* depth_dev, uint8_t* masks_dev, int32_t* mask_entity_host) {
    return hmsg_boundary("hmsg_synth_render", device_id, [&] {
        DevBuf<double> dp, drb, dob;
        DevBuf<int> drf, doff, dme;
        dp.alloc((size_t)n_frames * 16);
        drb.alloc((size_t)n_rooms * 6);
        dob.alloc((size_t)std::max(n_obj, 1) * 6);
        drf.alloc(n_frames);
        doff.alloc(n_rooms + 1);
        dme.alloc((size_t)n_frames * M);
        HIP_TRY(hipMemcpy(dp.p, poses, (size_t)n_frames * 128, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(drb.p, room_boxes, (size_t)n_rooms * 48, hipMemcpyHostToDevice));
        if (n_obj) HIP_TRY(hipMemcpy(dob.p, obj_boxes, (size_t)n_obj * 48, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(drf.p, room_of_frame, (size_t)n_frames * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(doff.p, room_obj_off, (size_t)(n_rooms + 1) * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(dme.p, 0, (size_t)n_frames * M * 4));
        SynthParams P{H, W, M, n_frames, n_obj, K[0], K[4], K[2], K[5], depth_noise_mm, seed};
        const size_t total = (size_t)H * W * n_frames;
        hipLaunchKernelGGL(k_synth, dim3(cdiv(total, 256)), dim3(256), 0, 0, P, (const double*)dp.p, (const int*)drf.p,
                           (const double*)drb.p, (const double*)dob.p, (const int*)doff.p, rgb_dev, depth_dev, masks_dev, dme.p);
        HMSG_CHECK_LAUNCH();
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(mask_entity_host, dme.p, (size_t)n_frames * M * 4, hipMemcpyDeviceToHost));
    });
}
