// One vertex into one view by THE RULE of sg_render (include/seggroup_hip.h: CAMERA SPACE, REJECTION, SCREEN), shared by the rasteriser
// (kernels_render.hip, k_rd_project) and the 2D-to-3D lift (kernels_lift.hip, k_lift_pairs): one function, so the two agree to the byte on
// where a vertex lands.  Double arithmetic, each operation rounded once; the library is built with nothing contracted.
#pragma once
#include <hip/hip_runtime.h>

#include "box_iou_device.h"
#include "overseg_device.h"

namespace sgrd {

constexpr int kCamDoubles = 16;                // a view: T row-major 3 x 4 world->camera, then fx fy cx cy
constexpr double kGuard = 16384.0;             // |u|, |v| above it: far
enum { kInView = 0, kBehind = 1, kFar = 2 };

// p: the vertex's three floats; c: the view's 16 doubles.  -> kInView with X, Y (1/256 pixel) and c2 (camera-space depth) set, or
// kBehind (a coordinate or a c_k that is not finite, or c_2 <= near) or kFar (|u| or |v| above the guard band, or NaN) with them untouched.
__device__ __forceinline__ int project(const float* __restrict__ p, const double* __restrict__ c, int ortho, double near, int& X, int& Y, double& c2) {
    if (!(sgos::finite_f32(p[0]) && sgos::finite_f32(p[1]) && sgos::finite_f32(p[2]))) return kBehind;
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    const double c0 = ((c[0] * x + c[1] * y) + c[2] * z) + c[3];
    const double c1 = ((c[4] * x + c[5] * y) + c[6] * z) + c[7];
    const double cz = ((c[8] * x + c[9] * y) + c[10] * z) + c[11];
    if (!(sg_box::finite_f64(c0) && sg_box::finite_f64(c1) && sg_box::finite_f64(cz) && cz > near)) return kBehind;
    const double fx = c[12], fy = c[13], cx = c[14], cy = c[15];
    const double u = ortho ? fx * c0 + cx : fx * (c0 / cz) + cx;
    const double w = ortho ? fy * c1 + cy : fy * (c1 / cz) + cy;
    if (!(fabs(u) <= kGuard && fabs(w) <= kGuard)) return kFar;       // a NaN fails both: far
    X = (int)floor(u * 256.0 + 0.5);
    Y = (int)floor(w * 256.0 + 0.5);
    c2 = cz;
    return kInView;
}

}  // namespace sgrd
