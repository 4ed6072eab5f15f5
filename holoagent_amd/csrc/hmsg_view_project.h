// The point transform of check_object_in_view (utils/graph_utils.py:123-141), stated once as device code: hmsg_object_views
// (hmsg_graph.hip) and the slow path's cloud-in-view distances (hmsg_query_views.hip) both decide "in front" and "inside the
// image" through it.  The reference's two matmuls go through BLAS dgemm, whose micro-kernel keeps one accumulator per output
// element and feeds it with fused multiply-adds in k order; the chain fma(a3, b3, fma(a2, b2, fma(a1, b1, a0 * b0)))
// reproduces numpy + OpenBLAS bit for bit (tests/test_object_views.py), so a point on the image border decides as it does there.
#pragma once
#include "hmsg_common.h"

struct ViewCam {
    double P[12];      // world -> camera, rows 0..2 of the 4x4
    double K[9];
    double W, H;
};
__device__ __forceinline__ ViewCam view_cam_load(const double* __restrict__ pose_inv, const double* __restrict__ Kmat, const int* __restrict__ wh) {
    ViewCam c;
    for (int i = 0; i < 12; ++i) c.P[i] = pose_inv[i];
    for (int i = 0; i < 9; ++i) c.K[i] = Kmat[i];
    c.W = (double)wh[0];
    c.H = (double)wh[1];
    return c;
}
#define VIEW_POINT_BEHIND 0      // camera z <= 0 (or NaN): the reference drops the point
#define VIEW_POINT_FRONT 1       // in front of the camera, outside the image
#define VIEW_POINT_INSIDE 2      // 0 <= u < W and 0 <= v < H
// point q (x, y, z) -> one of the three; *cz = its camera z
__device__ __forceinline__ int view_point(const ViewCam& cam, const double* __restrict__ q, double* cz) {
    const double x = q[0], y = q[1], z = q[2];
    double c[3];
    for (int r = 0; r < 3; ++r)
        c[r] = fma(cam.P[r * 4 + 3], 1.0, fma(cam.P[r * 4 + 2], z, fma(cam.P[r * 4 + 1], y, __dmul_rn(cam.P[r * 4], x))));
    *cz = c[2];
    if (!(c[2] > 0.0)) return VIEW_POINT_BEHIND;
    double ph[3];
    for (int r = 0; r < 3; ++r)
        ph[r] = fma(cam.K[r * 3 + 2], c[2], fma(cam.K[r * 3 + 1], c[1], __dmul_rn(cam.K[r * 3], c[0])));
    const double u = __ddiv_rn(ph[0], ph[2]), v = __ddiv_rn(ph[1], ph[2]);
    return (u >= 0.0 && u < cam.W && v >= 0.0 && v < cam.H) ? VIEW_POINT_INSIDE : VIEW_POINT_FRONT;
}
