// The rigid pose that carries one triangle onto another: written once, for the RANSAC kernels (kernels_register.hip) and
// for the host (sg_triangle_pose in align.cpp), so that a hypothesis' pose can be rebuilt without a device round trip.
//
// A triangle is x[9] = x0 | x1 | x2.  Its frame: e1 = (x1 - x0) / |x1 - x0|, c = e1 x (x2 - x0), e3 = c / |c|, e2 = e3 x e1; |c| is the
// triangle's height over its first edge.  With F = [e1 e2 e3] as columns, R = F_b F_a^T and t = mean(b) - R mean(a).  Every operation is
// a double operation rounded once, in the order written here (the build contracts nothing): dot(a, b) = (a0*b0 + a1*b1) + a2*b2,
// mean[r] = ((x0[r] + x1[r]) + x2[r]) / 3.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

namespace sgtri {

__host__ __device__ inline double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

__host__ __device__ inline void cross3(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

struct Frame {
    double e[3][3];            // e[0] = e1, e[1] = e2, e[2] = e3
    double mean[3];
    double edge;               // |x1 - x0|
    double height;             // |e1 x (x2 - x0)|
};

// the frame of a triangle; with edge == 0 or height == 0 the axes are not finite and the caller must not use them
__host__ __device__ inline void frame(const double* x, Frame& f) {
    double d1[3], d2[3], c[3];
    for (int r = 0; r < 3; ++r) {
        d1[r] = x[3 + r] - x[r];
        d2[r] = x[6 + r] - x[r];
        f.mean[r] = ((x[r] + x[3 + r]) + x[6 + r]) / 3.0;
    }
    f.edge = sqrt(dot3(d1, d1));
    for (int r = 0; r < 3; ++r) f.e[0][r] = d1[r] / f.edge;
    cross3(f.e[0], d2, c);
    f.height = sqrt(dot3(c, c));
    for (int r = 0; r < 3; ++r) f.e[2][r] = c[r] / f.height;
    cross3(f.e[2], f.e[0], f.e[1]);
}

// T = row-major 3x4 [R|t] with R = F_b F_a^T, t = mean(b) - R mean(a)
__host__ __device__ inline void pose_of_frames(const Frame& fa, const Frame& fb, double* T) {
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) T[4 * r + c] = (fb.e[0][r] * fa.e[0][c] + fb.e[1][r] * fa.e[1][c]) + fb.e[2][r] * fa.e[2][c];
        T[4 * r + 3] = fb.mean[r] - ((T[4 * r] * fa.mean[0] + T[4 * r + 1] * fa.mean[1]) + T[4 * r + 2] * fa.mean[2]);
    }
}

__host__ __device__ inline void triangle_pose(const double* a, const double* b, double* T) {
    Frame fa, fb;
    frame(a, fa);
    frame(b, fb);
    pose_of_frames(fa, fb, T);
}

}  // namespace sgtri
