// Rigid alignment of two clouds, device side: what a point-to-point ICP needs around sg_nearest_point_grid.
//
//   k_rigid_apply     out[u] = (float)(R x[u] + t) in double, one thread a point, every operation rounded once in the order the header
//                     states (-ffp-contract=off: no fma), so the bytes are those of the element-wise NumPy statement.
//   k_align_moments   the 17 sums of the closed-form fit (n | sum a | sum b | sum a b^T | sum d2) over the inlier pairs, in double.  A
//                     workgroup folds 1,024 consecutive pairs into ONE partial row of the workspace: thread t accumulates pairs t, t + 256,
//                     .. of its block in order and sgmom::block_row (moments_device.h) is the first tree.  An index outside 0..N-1 raises
//                     the flag word before anything is read through it.
//   sgmom::k_fold     (moments_device.h) the second tree over the partial rows, templated on the row width: 17 sums here, 31 for the
//                     point-to-plane fit below.  sgmom::reduce is the host sequence around both: workspace, launches, one copy back.
// No floating-point atomics; grid, block and both trees are functions of U alone, so the 17 doubles do not depend on the device or the stream.
// The kernel is a gather: 12 B of x, 8 B of idx and 4 B of d2 streamed per pair, 12 B of y read at random; the ~30 double operations per
// pair hide under it.
//
// Point-to-plane:
//   k_plane_moments   the 31 sums of a Gauss-Newton step on the point-to-plane residual (usable | skipped | upper triangle of sum J J^T |
//                     sum J r | sum r r | sum d2) over the candidate pairs, with the moving point taken through the current pose in double
//                     (sg_rigid_apply's statement without its final rounding).  Launch shape, pair order, both trees and the index flag are
//                     k_align_moments'; 24 B of y and its normal are read at random per pair, ~130 double operations hide under them.
#include <cmath>

#include "moments_device.h"
#include "sg_common.h"

namespace {

using sgmom::kBlock;
using sgmom::kPer;
using sgmom::Origin;
using sgmom::Rigid;

constexpr int kMom = 17;
constexpr int kPlaneMom = 31;                 // usable | skipped | 21 of J J^T | 6 of J r | r r | d2

struct Origins { double x[3], y[3]; };

__global__ __launch_bounds__(kBlock) void k_rigid_apply(const float* __restrict__ x, int xs, int U, Rigid T, float* __restrict__ out) {
    const int u = blockIdx.x * kBlock + threadIdx.x;
    if (u >= U) return;
    const float* p = x + (size_t)u * xs;
    const double px = (double)p[0], py = (double)p[1], pz = (double)p[2];
    float* o = out + (size_t)u * 3;
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = (float)(((T.m[4 * r] * px + T.m[4 * r + 1] * py) + T.m[4 * r + 2] * pz) + T.m[4 * r + 3]);
}

// every thread reaches block_row: a pair past U, outside the radius or with a bad index adds 0
__global__ __launch_bounds__(kBlock) void k_align_moments(const float* __restrict__ x, int xs, int U, const float* __restrict__ y, int ys, int N,
                                                          const int64_t* __restrict__ idx, const float* __restrict__ d2, float max_d2, Origins o,
                                                          double* __restrict__ partial, int* __restrict__ flag) {
    double acc[kMom];
#pragma unroll
    for (int m = 0; m < kMom; ++m) acc[m] = 0.0;
    const long long base = (long long)blockIdx.x * sgmom::kItems + threadIdx.x;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const long long u = base + (long long)j * kBlock;
        if (u >= (long long)U) continue;
        const int64_t i = idx[u];
        if (i < 0 || i >= (int64_t)N) { bad = true; continue; }
        const float dd = d2[u];
        if (!(dd <= max_d2)) continue;                         // a NaN compares false: never an inlier
        const float* px = x + (size_t)u * xs;
        const float* py = y + (size_t)i * ys;
        const double a[3] = {(double)px[0] - o.x[0], (double)px[1] - o.x[1], (double)px[2] - o.x[2]};
        const double b[3] = {(double)py[0] - o.y[0], (double)py[1] - o.y[1], (double)py[2] - o.y[2]};
        acc[0] += 1.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            acc[1 + r] += a[r];
            acc[4 + r] += b[r];
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[7 + 3 * r + c] += a[r] * b[c];
        }
        acc[16] += (double)dd;
    }
    if (bad) *flag = 1;
    sgmom::block_row(acc, partial + (size_t)blockIdx.x * kMom);
}

// the point-to-plane twin of k_align_moments: the same blocks, the same pair order, the same two trees, 31 sums.  R, t and the origin are
// wave-uniform (kernel arguments: scalar registers); every operation is written once, in the order the header states, and nothing contracts.
__global__ __launch_bounds__(kBlock) void k_plane_moments(const float* __restrict__ x, int xs, int U, Rigid T, const float* __restrict__ y, int ys,
                                                          int N, const float* __restrict__ nrm, int ns, const int64_t* __restrict__ idx,
                                                          const float* __restrict__ d2, float max_d2, Origin o, double* __restrict__ partial,
                                                          int* __restrict__ flag) {
    double acc[kPlaneMom];
#pragma unroll
    for (int m = 0; m < kPlaneMom; ++m) acc[m] = 0.0;
    const long long base = (long long)blockIdx.x * sgmom::kItems + threadIdx.x;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const long long u = base + (long long)j * kBlock;
        if (u >= (long long)U) continue;
        const int64_t i = idx[u];
        if (i < 0 || i >= (int64_t)N) { bad = true; continue; }
        const float dd = d2[u];
        if (!(dd <= max_d2)) continue;                         // a NaN compares false: never a candidate
        const float* pn = nrm + (size_t)i * ns;
        const double n[3] = {(double)pn[0], (double)pn[1], (double)pn[2]};
        const double nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
        if (!(nn >= 0.25 && nn <= 4.0)) {                       // a NaN or an infinite component fails one of the two compares
            acc[1] += 1.0;
            continue;
        }
        const float* px = x + (size_t)u * xs;
        const float* py = y + (size_t)i * ys;
        const double qx = (double)px[0], qy = (double)px[1], qz = (double)px[2];
        double a[3], e[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double p = ((T.m[4 * r] * qx + T.m[4 * r + 1] * qy) + T.m[4 * r + 2] * qz) + T.m[4 * r + 3];
            a[r] = p - o.c[r];
            e[r] = a[r] - ((double)py[r] - o.c[r]);
        }
        const double res = (e[0] * n[0] + e[1] * n[1]) + e[2] * n[2];
        const double J[6] = {a[1] * n[2] - a[2] * n[1], a[2] * n[0] - a[0] * n[2], a[0] * n[1] - a[1] * n[0], n[0], n[1], n[2]};
        acc[0] += 1.0;
        int k = 2;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
#pragma unroll
            for (int c = r; c < 6; ++c) acc[k++] += J[r] * J[c];
        }
#pragma unroll
        for (int r = 0; r < 6; ++r) acc[23 + r] += J[r] * res;
        acc[29] += res * res;
        acc[30] += (double)dd;
    }
    if (bad) *flag = 1;
    sgmom::block_row(acc, partial + (size_t)blockIdx.x * kPlaneMom);
}

}  // namespace

extern "C" {

int sg_rigid_apply(const float* d_x, int x_stride, int U, const double* h_T, float* d_out, void* stream) {
    const char* who = "sg_rigid_apply";
    SG_REQUIRE(U >= 0 && x_stride >= 3 && h_T, "%s: bad arguments (%d points, rows of %d floats)", who, U, x_stride);
    if (U > SG_MAX_CLOUD_POINTS) return sg::fail(SG_EUNSUP, "%s: %d points; a call takes at most %d", who, U, SG_MAX_CLOUD_POINTS);
    Rigid T;
    if (int rc = sgmom::read_rigid(who, h_T, &T)) return rc;
    if (U == 0) return SG_OK;
    SG_REQUIRE(d_x && d_out, "%s: bad arguments", who);
    k_rigid_apply<<<sg::cdiv(U, kBlock), kBlock, 0, sg::as_stream(stream)>>>(d_x, x_stride, U, T, d_out);
    SG_LAUNCH_CHECK();
    return SG_OK;
}

size_t sg_align_moments_ws_bytes(int U) { return (U < 0 || U > SG_MAX_CLOUD_POINTS) ? 0 : sgmom::ws_bytes<kMom>(U); }

int sg_align_moments(const float* d_x, int x_stride, int U, const float* d_y, int y_stride, int N, const int64_t* d_idx, const float* d_d2,
                     float max_d2, const double* h_origin_x, const double* h_origin_y, double* h_out, void* d_ws, size_t ws_bytes, void* stream) {
    const char* who = "sg_align_moments";
    SG_REQUIRE(U >= 0 && N >= 1, "%s: bad arguments (%d pairs, %d candidates)", who, U, N);
    if (U > SG_MAX_CLOUD_POINTS || N > SG_MAX_CLOUD_POINTS)
        return sg::fail(SG_EUNSUP, "%s: %d pairs into %d candidates; a call takes at most %d of either", who, U, N, SG_MAX_CLOUD_POINTS);
    SG_REQUIRE(x_stride >= 3 && y_stride >= 3, "%s: rows of at least 3 floats (x: %d, y: %d)", who, x_stride, y_stride);
    SG_REQUIRE(h_origin_x && h_origin_y && h_out, "%s: bad arguments", who);
    SG_REQUIRE(!std::isnan(max_d2), "%s: max_d2 is not a number", who);
    SG_REQUIRE(sgmom::finite_n<3>(h_origin_x) && sgmom::finite_n<3>(h_origin_y), "%s: an origin that is not finite", who);
    if (U == 0) {
        for (int m = 0; m < kMom; ++m) h_out[m] = 0.0;
        return SG_OK;
    }
    SG_REQUIRE(d_x && d_y && d_idx && d_d2 && d_ws, "%s: bad arguments", who);
    Origins o;
    for (int i = 0; i < 3; ++i) { o.x[i] = h_origin_x[i]; o.y[i] = h_origin_y[i]; }
    hipStream_t st = sg::as_stream(stream);
    int flag = 0;
    auto first = [&](int rows, double* d_partial, int* d_flag) {
        k_align_moments<<<rows, kBlock, 0, st>>>(d_x, x_stride, U, d_y, y_stride, N, d_idx, d_d2, max_d2, o, d_partial, d_flag);
    };
    if (int rc = sgmom::reduce<kMom>(who, U, d_ws, ws_bytes, st, first, h_out, &flag)) return rc;
    if (flag) return sg::fail(SG_EINVAL, "%s: an index outside 0..%d", who, N - 1);
    return SG_OK;
}

size_t sg_align_plane_moments_ws_bytes(int U) { return (U < 0 || U > SG_MAX_CLOUD_POINTS) ? 0 : sgmom::ws_bytes<kPlaneMom>(U); }

int sg_align_plane_moments(const float* d_x, int x_stride, int U, const double* h_T, const float* d_y, int y_stride, int N, const float* d_n,
                           int n_stride, const int64_t* d_idx, const float* d_d2, float max_d2, const double* h_origin, double* h_out, void* d_ws,
                           size_t ws_bytes, void* stream) {
    const char* who = "sg_align_plane_moments";
    SG_REQUIRE(U >= 0 && N >= 1, "%s: bad arguments (%d pairs, %d candidates)", who, U, N);
    if (U > SG_MAX_CLOUD_POINTS || N > SG_MAX_CLOUD_POINTS)
        return sg::fail(SG_EUNSUP, "%s: %d pairs into %d candidates; a call takes at most %d of either", who, U, N, SG_MAX_CLOUD_POINTS);
    SG_REQUIRE(x_stride >= 3 && y_stride >= 3 && n_stride >= 3, "%s: rows of at least 3 floats (x: %d, y: %d, normals: %d)", who, x_stride, y_stride,
               n_stride);
    SG_REQUIRE(h_T && h_origin && h_out, "%s: bad arguments", who);
    SG_REQUIRE(!std::isnan(max_d2), "%s: max_d2 is not a number", who);
    SG_REQUIRE(sgmom::finite_n<3>(h_origin), "%s: an origin that is not finite", who);
    Rigid T;
    if (int rc = sgmom::read_rigid(who, h_T, &T)) return rc;
    if (U == 0) {
        for (int m = 0; m < kPlaneMom; ++m) h_out[m] = 0.0;
        return SG_OK;
    }
    SG_REQUIRE(d_x && d_y && d_n && d_idx && d_d2 && d_ws, "%s: bad arguments", who);
    const Origin o = sgmom::origin_of(h_origin);
    hipStream_t st = sg::as_stream(stream);
    int flag = 0;
    auto first = [&](int rows, double* d_partial, int* d_flag) {
        k_plane_moments<<<rows, kBlock, 0, st>>>(d_x, x_stride, U, T, d_y, y_stride, N, d_n, n_stride, d_idx, d_d2, max_d2, o, d_partial, d_flag);
    };
    if (int rc = sgmom::reduce<kPlaneMom>(who, U, d_ws, ws_bytes, st, first, h_out, &flag)) return rc;
    if (flag) return sg::fail(SG_EINVAL, "%s: an index outside 0..%d", who, N - 1);
    return SG_OK;
}

}  // extern "C"
