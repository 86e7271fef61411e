// The eigenvector step of the point-cloud normals, shared by the kNN form (k_pc_normals) and the form over
// neighbourhoods of variable length (k_pc_normals_csr): the same code, so the same bytes from the same six sums.
#pragma once
#include <hip/hip_runtime.h>

namespace sgpc {

constexpr int kSweeps = 5;          // after five sweeps every off-diagonal is exactly 0 on the measured clouds

// one Jacobi rotation of the pair (p, q); r is the third index.  a_rp, a_rq: the two off-diagonals that share r; v_ip, v_iq: the columns
// p and q of the accumulated rotation.  A pair whose off-diagonal is exactly 0 is skipped.
__device__ __forceinline__ void rotate(float& app, float& aqq, float& apq, float& arp, float& arq, float& v0p, float& v0q, float& v1p,
                                       float& v1q, float& v2p, float& v2q) {
    if (apq == 0.0f) return;
    const float theta = (aqq - app) / (2.0f * apq);
    const float sgn = theta >= 0.0f ? 1.0f : -1.0f;
    const float t = sgn / (__builtin_fabsf(theta) + __builtin_sqrtf(theta * theta + 1.0f));      // theta * theta = +inf gives t = 0
    const float c = 1.0f / __builtin_sqrtf(t * t + 1.0f);
    const float s = t * c;
    const float h = t * apq;
    app = app - h;
    aqq = aqq + h;
    apq = 0.0f;
    const float rp = arp, rq = arq;
    arp = c * rp - s * rq;
    arq = s * rp + c * rq;
    const float x0 = v0p, y0 = v0q, x1 = v1p, y1 = v1q, x2 = v2p, y2 = v2q;
    v0p = c * x0 - s * y0; v0q = s * x0 + c * y0;
    v1p = c * x1 - s * y1; v1q = s * x1 + c * y1;
    v2p = c * x2 - s * y2; v2q = s * x2 + c * y2;
}

// c2 if b2, else c1 if b1, else c0
__device__ __forceinline__ float pick(float c0, float c1, float c2, bool b1, bool b2) {
    const unsigned int m1 = b1 ? ~0u : 0u, m2 = b2 ? ~0u : 0u;
    const unsigned int lo = (__float_as_uint(c1) & m1) | (__float_as_uint(c0) & ~m1);
    return __uint_as_float((__float_as_uint(c2) & m2) | (lo & ~m2));
}

// the six covariance sums -> the column of the accumulated rotation whose diagonal entry is smallest; not re-normalised
__device__ __forceinline__ void smallest_eigenvector(float a00, float a01, float a02, float a11, float a12, float a22, float& nx, float& ny,
                                                     float& nz) {
    // 4. cyclic Jacobi, pairs (0,1), (0,2), (1,2); v_rc = row r, column c of the accumulated rotation
    float v00 = 1.0f, v01 = 0.0f, v02 = 0.0f, v10 = 0.0f, v11 = 1.0f, v12 = 0.0f, v20 = 0.0f, v21 = 0.0f, v22 = 1.0f;
#pragma unroll 1
    for (int sweep = 0; sweep < kSweeps; ++sweep) {
        rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
        rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
        rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
    }
    // the column whose diagonal entry is smallest, the lowest index among equal entries
    // (selected by masks: written as branches, the compiler turns the three candidates into a table in scratch)
    const bool b1 = a11 < a00;
    const float dm = b1 ? a11 : a00;
    const bool b2 = a22 < dm;
    nx = pick(v00, v01, v02, b1, b2); ny = pick(v10, v11, v12, b1, b2); nz = pick(v20, v21, v22, b1, b2);
}

}  // namespace sgpc
