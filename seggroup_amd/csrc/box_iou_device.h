// IoU of one pair of upright boxes, device side: THE pair function, shared by kernels_boxiou.hip (sg_box_iou, sg_box_best)
// and kernels_boxnms.hip (sg_box_nms), so a matrix entry, a best partner and a suppression bit come from the same bits.  A box is 8
// doubles, cx cy cz sx sy sz c s; include/seggroup_hip.h spells the operation sequence out and pair_iou follows it statement by statement.
// The clipped footprint has at most 8 vertices.  It lives in two sets of eight NAMED slots (every index below is a compile-time constant
// once the loops are unrolled): an append is a predicated move into the slot whose number equals the running count, so nothing is
// indexed at run time and nothing goes to scratch.  Double arithmetic, nothing contracted (-ffp-contract=off).
//
// Also here, for both files: the check of one box (upright_flags) and the refusal its flag bits become on the host (upright_refusal).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "sg_common.h"

namespace sg_box {

using sg::finite_f64;

constexpr int kSlots = 8;
constexpr int kNotFinite = 1, kNegative = 2, kNotUnit = 4;   // upright_flags' bits
constexpr double kUnitTol = 1e-6;

// the 8 doubles of one box -> its flag bits: a value that is not finite (nothing else is looked at then), a negative size,
// |c*c + s*s - 1| > 1e-6.  A size of zero is valid.
__device__ __forceinline__ int upright_flags(const double* __restrict__ p) {
    int bad = 0;
#pragma unroll
    for (int r = 0; r < 8; ++r)
        if (!finite_f64(p[r])) bad = kNotFinite;
    if (!bad) {
        if (p[3] < 0.0 || p[4] < 0.0 || p[5] < 0.0) bad |= kNegative;
        const double n = p[6] * p[6] + p[7] * p[7];
        if (fabs(n - 1.0) > kUnitTol) bad |= kNotUnit;
    }
    return bad;
}

// the refusal of a set whose boxes ORed these bits together, SG_OK for none: not finite before negative size before the unit circle.
// `set` is "A" or "B", or null where the entry takes one set.
inline int upright_refusal(const char* who, const char* set, int bits) {
    const char* of = set ? " of set " : "";
    if (!set) set = "";
    if (bits & kNotFinite) return sg::fail(SG_EINVAL, "%s: a box%s%s has a value that is not finite", who, of, set);
    if (bits & kNegative) return sg::fail(SG_EINVAL, "%s: a box%s%s has a negative size", who, of, set);
    if (bits & kNotUnit) return sg::fail(SG_EINVAL, "%s: a box%s%s has (c, s) off the unit circle: |c*c + s*s - 1| > 1e-6", who, of, set);
    return SG_OK;
}

// slot m of the polygon <- (x, y): eight predicated moves, no run-time index.  An append past slot 7 is dropped (the contract says so).
__device__ __forceinline__ void put(double (&u)[kSlots], double (&v)[kSlots], int m, double x, double y) {
#pragma unroll
    for (int j = 0; j < kSlots; ++j)
        if (j == m) { u[j] = x; v[j] = y; }
}

// the signed distance of (u, v) to side SIDE of the rectangle |u| <= hu, |v| <= hv, >= 0 inside: hu - u, u + hu, hv - v, v + hv
template <int SIDE>
__device__ __forceinline__ double side_dist(double u, double v, double h) {
    return SIDE == 0 ? h - u : SIDE == 1 ? u + h : SIDE == 2 ? h - v : v + h;
}

// One side of Sutherland-Hodgman.  The polygon (iu, iv)[0..n-1] has at most MAXIN vertices; (ou, ov)[0..m-1] is what is left of it.
template <int SIDE, int MAXIN>
__device__ __forceinline__ int clip_side(const double (&iu)[kSlots], const double (&iv)[kSlots], int n, double h, double (&ou)[kSlots],
                                         double (&ov)[kSlots]) {
    int m = 0;
    double pu = iu[0], pv = iv[0];                       // the vertex before vertex 0 is vertex n - 1
#pragma unroll
    for (int j = 1; j < MAXIN; ++j)
        if (j == n - 1) { pu = iu[j]; pv = iv[j]; }
    double dp = side_dist<SIDE>(pu, pv, h);
#pragma unroll
    for (int i = 0; i < MAXIN; ++i) {
        if (i < n) {
            const double qu = iu[i], qv = iv[i];
            const double dq = side_dist<SIDE>(qu, qv, h);
            const bool in_p = dp >= 0.0, in_q = dq >= 0.0;
            if (in_p != in_q) {
                const double t = dp / (dp - dq);
                double xu, xv;
                if (SIDE < 2) {
                    xu = SIDE == 0 ? h : -h;              // on the side itself, exactly
                    xv = pv + t * (qv - pv);
                } else {
                    xu = pu + t * (qu - pu);
                    xv = SIDE == 2 ? h : -h;
                }
                put(ou, ov, m, xu, xv);
                ++m;
            }
            if (in_q) {
                put(ou, ov, m, qu, qv);
                ++m;
            }
            pu = qu;
            pv = qv;
            dp = dq;
        }
    }
    return min(m, kSlots);
}

// IoU(a, b): include/seggroup_hip.h, statement by statement
__device__ __forceinline__ double pair_iou(const double* __restrict__ a, const double* __restrict__ b) {
    const double ax = a[0], ay = a[1], az = a[2], asx = a[3], asy = a[4], asz = a[5], ac = a[6], as = a[7];
    const double bx = b[0], by = b[1], bz = b[2], bsx = b[3], bsy = b[4], bsz = b[5], bc = b[6], bs = b[7];
    const double dx = ax - bx, dy = ay - by;
    const double hax = 0.5 * asx, hay = 0.5 * asy, hbx = 0.5 * bsx, hby = 0.5 * bsy;
    const double ex = hax * ac, ey = hax * as, fx = hay * as, fy = hay * ac;
    // the corners of a about b's centre: (-,-), (+,-), (+,+), (-,+) along (u, v) of a, counter-clockwise
    const double wx[4] = {(dx - ex) + fx, (dx + ex) + fx, (dx + ex) - fx, (dx - ex) - fx};
    const double wy[4] = {(dy - ey) - fy, (dy + ey) - fy, (dy + ey) + fy, (dy - ey) + fy};
    double pu[kSlots], pv[kSlots], qu[kSlots], qv[kSlots];
#pragma unroll
    for (int k = 0; k < kSlots; ++k) pu[k] = pv[k] = qu[k] = qv[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        pu[k] = bc * wx[k] + bs * wy[k];
        pv[k] = bc * wy[k] - bs * wx[k];
    }
    int n = 4;
    n = clip_side<0, 4>(pu, pv, n, hbx, qu, qv);
    n = clip_side<1, 5>(qu, qv, n, hbx, pu, pv);
    n = clip_side<2, 6>(pu, pv, n, hby, qu, qv);
    n = clip_side<3, 7>(qu, qv, n, hby, pu, pv);
    double acc = 0.0;
#pragma unroll
    for (int i = 1; i + 1 < kSlots; ++i) {
        if (i + 1 < n) {
            const double e0 = pu[i] - pu[0], e1 = pv[i] - pv[0], g0 = pu[i + 1] - pu[0], g1 = pv[i + 1] - pv[0];
            acc = acc + (e0 * g1 - e1 * g0);
        }
    }
    double area = 0.5 * acc;
    if (!(area > 0.0)) area = 0.0;
    const double haz = 0.5 * asz, hbz = 0.5 * bsz;
    const double top = fmin(az + haz, bz + hbz), bottom = fmax(az - haz, bz - hbz);
    double h = top - bottom;
    if (!(h > 0.0)) h = 0.0;
    const double inter = area * h;
    const double va = (asx * asy) * asz, vb = (bsx * bsy) * bsz;
    const double uni = (va + vb) - inter;
    return uni > 0.0 ? inter / uni : 0.0;
}

// the first s in 0..B-1 with off[s + 1] > x; the caller knows that x < off[B]
__device__ __forceinline__ int scene_of(const int32_t* __restrict__ off, int B, int x) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (off[mid + 1] > x) hi = mid; else lo = mid + 1;
    }
    return lo;
}

}  // namespace sg_box
