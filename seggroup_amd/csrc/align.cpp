// Rigid alignment of two clouds, host side: the closed-form fit from sg_align_moments' 17 sums.  No HIP call in this file:
// it is part of the host-only sanitizer build and runs without a device.
//
// Kabsch from the moments: with a = x - origin_x, b = y - origin_y over the n inlier pairs,  H = sum a b^T - (sum a)(sum b)^T / n  is the
// cross-covariance of the centred pairs, H = U S V^T, and the rotation that minimises sum |R a + t - b|^2 is R = V diag(1, 1, d) U^T with
// d = det(V) det(U).  The SVD is a one-sided (Hestenes) Jacobi on the columns of H: plane rotations from the right until the columns are
// orthogonal, H J = U S with J = V accumulated -- the small singular values keep their relative accuracy, which forming H^T H would
// square away, and the degeneracy threshold below is stated on their ratio.  Only the two leading pairs (u1, v1), (u2, v2) are used:
//     R = v1 u1^T + v2 u2^T + (v1 x v2)(u1 x u2)^T
// is V diag(1, 1, d) U^T whatever the signs of u3 and v3 (u3 = det(U) u1 x u2, v3 = det(V) v1 x v2), so a reflection is corrected by
// flipping the smallest singular direction without ever normalising a third column that may be zero (a planar set).  Both pairs are
// re-orthonormalised (Gram-Schmidt) first, so R^T R - I stays at a few units of the last place.
//
// Point-to-plane: one Gauss-Newton step from sg_align_plane_moments' 31 sums.  The 6x6 normal matrix, with its rotational
// rows and columns scaled into length units, is diagonalised by cyclic Jacobi (symmetric, so the eigenvalues -- negative rounding residue
// of a singular matrix included -- come out to a few units of the last place of the LARGEST one, which is what the degeneracy ratio needs),
// the step is solved in the eigenbasis, applied about the origin by Rodrigues' formula and the rotation re-orthonormalised, so that fifty
// composed steps are still a rotation.
//
// Global registration: sg_triangle_pose is triangle_pose.h's function for the host, the one the RANSAC kernels run.
//
// Plane extraction: sg_plane_fit is the least-squares plane through the inliers that sg_plane_moments summed -- the
// covariance from the 11 sums, the same cyclic Jacobi on 3x3, the eigenvector of the smallest eigenvalue.
//
// Oriented boxes: sg_box_axes is the frame of one label from sg_label_moments' ten sums -- the covariance, the same Jacobi,
// the eigenvectors as rows by descending eigenvalue, signs fixed, the third row the cross product of the first two.
#include "sg_common.h"
#include "triangle_pose.h"

#include <cmath>

namespace {

constexpr double kLineRatio = 0x1p-40;         // second singular value at or below this share of the first: the pairs lie on a line
constexpr int kMaxSweeps = 64;

struct Vec3 { double v[3]; };

double dot(const Vec3& a, const Vec3& b) { return (a.v[0] * b.v[0] + a.v[1] * b.v[1]) + a.v[2] * b.v[2]; }
Vec3 cross(const Vec3& a, const Vec3& b) {
    return {{a.v[1] * b.v[2] - a.v[2] * b.v[1], a.v[2] * b.v[0] - a.v[0] * b.v[2], a.v[0] * b.v[1] - a.v[1] * b.v[0]}};
}
void normalise(Vec3& a) {
    const double n = std::sqrt(dot(a, a));
    for (double& c : a.v) c /= n;
}
// a and b orthonormal, a's direction kept
void orthonormalise(Vec3& a, Vec3& b) {
    normalise(a);
    const double p = dot(a, b);
    for (int i = 0; i < 3; ++i) b.v[i] -= p * a.v[i];
    normalise(b);
}
// the largest-magnitude component is made positive, ties to the lowest axis
void fix_sign(Vec3& a) {
    int big = 0;
    for (int i = 1; i < 3; ++i)
        if (std::fabs(a.v[i]) > std::fabs(a.v[big])) big = i;
    if (a.v[big] < 0.0)
        for (double& c : a.v) c = -c;
}
// count | sum q [3] | sum q q^T (xx xy xz yy yz zz) -> A = sum q q^T - (sum q)(sum q)^T / count
void scatter(const double* h_m, double A[3][3]) {
    const double n = h_m[0];
    const double* sq = h_m + 1;
    const int at[3][3] = {{4, 5, 6}, {5, 7, 8}, {6, 8, 9}};
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) A[r][c] = h_m[at[r][c]] - sq[r] * sq[c] / n;
}

constexpr int kPlaneMom = 31;
constexpr double kPlaneRatio = 0x1p-40;        // smallest eigenvalue at or below this share of the largest: some motion costs nothing
constexpr double kSeriesBelow = 1e-8;          // radians: below it sin and cos come from their series

// eigenvalues and eigenvectors (the columns of V) of the symmetric A by cyclic Jacobi; A is destroyed.  false: not converged (non-finite input)
template <int kN>
bool jacobi(double A[kN][kN], double V[kN][kN], double lambda[kN]) {
    for (int i = 0; i < kN; ++i)
        for (int j = 0; j < kN; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kMaxSweeps; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < kN - 1; ++p)
            for (int q = p + 1; q < kN; ++q) off += std::fabs(A[p][q]);
        if (off == 0.0) {
            for (int i = 0; i < kN; ++i) lambda[i] = A[i][i];
            return true;
        }
        if (!std::isfinite(off)) return false;
        for (int p = 0; p < kN - 1; ++p) {
            for (int q = p + 1; q < kN; ++q) {
                const double apq = A[p][q];
                if (apq == 0.0) continue;
                // an entry that no longer changes either diagonal value is set to zero, not rotated away
                const double g = 128.0 * std::fabs(apq);
                if (sweep > 3 && std::fabs(A[p][p]) + g == std::fabs(A[p][p]) && std::fabs(A[q][q]) + g == std::fabs(A[q][q])) {
                    A[p][q] = A[q][p] = 0.0;
                    continue;
                }
                const double zeta = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = c * t;
                A[p][p] -= t * apq;
                A[q][q] += t * apq;
                A[p][q] = A[q][p] = 0.0;
                for (int k = 0; k < kN; ++k) {
                    if (k != p && k != q) {
                        const double akp = A[k][p], akq = A[k][q];
                        A[k][p] = A[p][k] = c * akp - s * akq;
                        A[k][q] = A[q][k] = s * akp + c * akq;
                    }
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
        }
    }
    return false;
}

}  // namespace

extern "C" {

int sg_align_solve(const double* h_m, const double* h_origin_x, const double* h_origin_y, double* h_T) {
    const char* who = "sg_align_solve";
    SG_REQUIRE(h_m && h_origin_x && h_origin_y && h_T, "%s: bad arguments", who);
    for (int i = 0; i < 17; ++i) SG_REQUIRE(std::isfinite(h_m[i]), "%s: moment %d is not finite", who, i);
    for (int i = 0; i < 3; ++i)
        SG_REQUIRE(std::isfinite(h_origin_x[i]) && std::isfinite(h_origin_y[i]), "%s: an origin that is not finite", who);
    const double n = h_m[0];
    SG_REQUIRE(n >= 0.0, "%s: a negative pair count (%g)", who, n);
    if (n < 3.0) return sg::fail(SG_EUNSUP, "%s: degenerate: %g pairs; a rigid fit needs at least 3", who, n);
    const double *sa = h_m + 1, *sb = h_m + 4, *sab = h_m + 7;
    // the columns of H, rotated in place; J accumulates the rotations
    Vec3 col[3], jc[3];
    for (int c = 0; c < 3; ++c) {
        for (int r = 0; r < 3; ++r) {
            col[c].v[r] = sab[3 * r + c] - sa[r] * sb[c] / n;
            jc[c].v[r] = r == c ? 1.0 : 0.0;
        }
    }
    for (int sweep = 0; sweep < kMaxSweeps; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 2; ++p) {
            for (int q = p + 1; q < 3; ++q) {
                const double alpha = dot(col[p], col[p]), beta = dot(col[q], col[q]), gamma = dot(col[p], col[q]);
                if (gamma == 0.0 || std::fabs(gamma) <= 0x1p-53 * (std::sqrt(alpha) * std::sqrt(beta))) continue;
                rotated = true;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = c * t;
                for (int i = 0; i < 3; ++i) {
                    const double hp = col[p].v[i], hq = col[q].v[i];
                    col[p].v[i] = c * hp - s * hq;
                    col[q].v[i] = s * hp + c * hq;
                    const double jp = jc[p].v[i], jq = jc[q].v[i];
                    jc[p].v[i] = c * jp - s * jq;
                    jc[q].v[i] = s * jp + c * jq;
                }
            }
        }
        if (!rotated) break;
    }
    double sv[3];
    for (int c = 0; c < 3; ++c) sv[c] = std::sqrt(dot(col[c], col[c]));
    if (!(std::isfinite(sv[0]) && std::isfinite(sv[1]) && std::isfinite(sv[2])))
        return sg::fail(SG_EINVAL, "%s: the moments overflow the fit", who);
    int first = 0;
    for (int c = 1; c < 3; ++c)
        if (sv[c] > sv[first]) first = c;
    int second = first == 0 ? 1 : 0;
    for (int c = 0; c < 3; ++c)
        if (c != first && sv[c] > sv[second]) second = c;
    if (!(sv[second] > kLineRatio * sv[first]))
        return sg::fail(SG_EUNSUP, "%s: degenerate: singular values %g, %g of the pairs' cross-covariance -- they lie on a line or in a point, "
                                   "the rotation about it is free", who, sv[first], sv[second]);
    Vec3 u1 = col[first], u2 = col[second], v1 = jc[first], v2 = jc[second];
    orthonormalise(u1, u2);
    orthonormalise(v1, v2);
    const Vec3 u3 = cross(u1, u2), v3 = cross(v1, v2);
    double R[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[r][c] = (v1.v[r] * u1.v[c] + v2.v[r] * u2.v[c]) + v3.v[r] * u3.v[c];
    for (int r = 0; r < 3; ++r) {
        double rx = 0.0;                                        // (R xbar)[r] with xbar = sum a / n + origin_x
        for (int c = 0; c < 3; ++c) {
            h_T[4 * r + c] = R[r][c];
            rx += R[r][c] * (sa[c] / n + h_origin_x[c]);
        }
        h_T[4 * r + 3] = (sb[r] / n + h_origin_y[r]) - rx;
    }
    return SG_OK;
}

int sg_align_plane_solve(const double* h_m, const double* h_origin, double length, const double* h_T, double* h_T_new, double* h_step) {
    const char* who = "sg_align_plane_solve";
    SG_REQUIRE(h_m && h_origin && h_T && h_T_new, "%s: bad arguments", who);
    for (int i = 0; i < kPlaneMom; ++i) SG_REQUIRE(std::isfinite(h_m[i]), "%s: moment %d is not finite", who, i);
    for (int i = 0; i < 3; ++i) SG_REQUIRE(std::isfinite(h_origin[i]), "%s: an origin that is not finite", who);
    for (int i = 0; i < 12; ++i) SG_REQUIRE(std::isfinite(h_T[i]), "%s: entry %d of the transform is not finite", who, i);
    SG_REQUIRE(std::isfinite(length) && length > 0.0, "%s: the length scale must be finite and > 0 (%g)", who, length);
    const double n = h_m[0];
    SG_REQUIRE(n >= 0.0, "%s: a negative pair count (%g)", who, n);
    if (n < 6.0) return sg::fail(SG_EUNSUP, "%s: degenerate: %g usable pairs; a point-to-plane step needs at least 6", who, n);
    const double scale[6] = {1.0 / length, 1.0 / length, 1.0 / length, 1.0, 1.0, 1.0};
    double A[6][6], V[6][6], lambda[6], g[6];
    int k = 2;
    for (int r = 0; r < 6; ++r) {
        for (int c = r; c < 6; ++c) A[r][c] = A[c][r] = (scale[r] * h_m[k++]) * scale[c];
        g[r] = scale[r] * h_m[23 + r];
    }
    if (!jacobi<6>(A, V, lambda)) return sg::fail(SG_EINVAL, "%s: the moments overflow the fit", who);
    double lmax = lambda[0], lmin = lambda[0];
    for (int i = 1; i < 6; ++i) {
        lmax = std::fmax(lmax, lambda[i]);
        lmin = std::fmin(lmin, lambda[i]);
    }
    if (!(lmax > 0.0) || !(lmin > kPlaneRatio * lmax))
        return sg::fail(SG_EUNSUP, "%s: degenerate: eigenvalues %g .. %g of the scaled normal matrix -- the planes the pairs lie on leave a "
                                   "motion free (one plane, parallel planes, two plane directions only)", who, lmin, lmax);
    double step[6];                                             // s = -D V diag(1 / lambda) V^T D g
    for (int i = 0; i < 6; ++i) step[i] = 0.0;
    for (int e = 0; e < 6; ++e) {
        double proj = 0.0;
        for (int i = 0; i < 6; ++i) proj += V[i][e] * g[i];
        proj /= lambda[e];
        for (int i = 0; i < 6; ++i) step[i] -= V[i][e] * proj;
    }
    for (int i = 0; i < 6; ++i) step[i] *= scale[i];
    for (int i = 0; i < 6; ++i)
        if (!std::isfinite(step[i])) return sg::fail(SG_EINVAL, "%s: the moments overflow the fit", who);
    // Rodrigues: Rw = I + (sin th / th) K + ((1 - cos th) / th^2) K K with K the cross-product matrix of w
    const double* w = step;
    const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2], th = std::sqrt(th2);
    const double sa = th < kSeriesBelow ? 1.0 - th2 / 6.0 : std::sin(th) / th;
    const double sb = th < kSeriesBelow ? 0.5 - th2 / 24.0 : (1.0 - std::cos(th)) / th2;
    const double K[3][3] = {{0.0, -w[2], w[1]}, {w[2], 0.0, -w[0]}, {-w[1], w[0], 0.0}};
    double Rw[3][3];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) {
            const double kk = (K[r][0] * K[0][c] + K[r][1] * K[1][c]) + K[r][2] * K[2][c];
            Rw[r][c] = ((r == c ? 1.0 : 0.0) + sa * K[r][c]) + sb * kk;
        }
    }
    Vec3 row[3];
    double tn[3];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) row[r].v[c] = (Rw[r][0] * h_T[c] + Rw[r][1] * h_T[4 + c]) + Rw[r][2] * h_T[8 + c];
        const double d[3] = {h_T[3] - h_origin[0], h_T[7] - h_origin[1], h_T[11] - h_origin[2]};
        tn[r] = (((Rw[r][0] * d[0] + Rw[r][1] * d[1]) + Rw[r][2] * d[2]) + h_origin[r]) + step[3 + r];
    }
    orthonormalise(row[0], row[1]);                             // rows 0 and 1, then row 2 as their cross product: a proper rotation
    row[2] = cross(row[0], row[1]);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) {
            SG_REQUIRE(std::isfinite(row[r].v[c]), "%s: the transform is not a rotation with a translation", who);
            h_T_new[4 * r + c] = row[r].v[c];
        }
        h_T_new[4 * r + 3] = tn[r];
        h_T_new[12 + r] = 0.0;
    }
    h_T_new[15] = 1.0;
    if (h_step)
        for (int i = 0; i < 6; ++i) h_step[i] = step[i];
    return SG_OK;
}

int sg_plane_fit(const double* h_m, const double* h_origin, double* h_plane, double* h_centroid, double* h_rms) {
    const char* who = "sg_plane_fit";
    SG_REQUIRE(h_m && h_origin && h_plane, "%s: bad arguments", who);
    for (int i = 0; i < 11; ++i) SG_REQUIRE(std::isfinite(h_m[i]), "%s: moment %d is not finite", who, i);
    for (int i = 0; i < 3; ++i) SG_REQUIRE(std::isfinite(h_origin[i]), "%s: an origin that is not finite", who);
    const double n = h_m[0];
    SG_REQUIRE(n >= 0.0, "%s: a negative point count (%g)", who, n);
    if (n < 3.0) return sg::fail(SG_EUNSUP, "%s: degenerate: %g points; a plane needs at least 3", who, n);
    const double* sq = h_m + 1;
    double A[3][3], V[3][3], lambda[3];
    scatter(h_m, A);
    if (!jacobi<3>(A, V, lambda)) return sg::fail(SG_EINVAL, "%s: the moments overflow the fit", who);
    int lo = 0, hi = 0;
    for (int i = 1; i < 3; ++i) {
        if (lambda[i] < lambda[lo]) lo = i;
        if (lambda[i] > lambda[hi]) hi = i;
    }
    if (lo == hi) hi = (lo + 1) % 3;                              // three equal eigenvalues
    const int mid = 3 - lo - hi;
    // the middle eigenvalue is what separates a plane from a line; Jacobi leaves rounding residue of either sign where it is zero
    if (!(lambda[hi] > 0.0) || !(lambda[mid] > kLineRatio * lambda[hi]))
        return sg::fail(SG_EUNSUP, "%s: degenerate: eigenvalues %g, %g, %g of the points' covariance -- they lie on a line or in a point, the "
                                   "plane through them is free", who, lambda[lo], lambda[mid], lambda[hi]);
    Vec3 nrm = {{V[0][lo], V[1][lo], V[2][lo]}};
    normalise(nrm);
    fix_sign(nrm);
    Vec3 centre;
    for (int i = 0; i < 3; ++i) centre.v[i] = h_origin[i] + sq[i] / n;
    const double d = -dot(nrm, centre);
    SG_REQUIRE(std::isfinite(d) && std::isfinite(nrm.v[0]) && std::isfinite(nrm.v[1]) && std::isfinite(nrm.v[2]), "%s: the moments overflow the fit",
               who);
    for (int i = 0; i < 3; ++i) h_plane[i] = nrm.v[i];
    h_plane[3] = d;
    if (h_centroid)
        for (int i = 0; i < 3; ++i) h_centroid[i] = centre.v[i];
    if (h_rms) *h_rms = std::sqrt(std::fmax(lambda[lo], 0.0) / n);
    return SG_OK;
}

int sg_box_axes(const double* h_m, double* h_R, double* h_eig) {
    const char* who = "sg_box_axes";
    SG_REQUIRE(h_m && h_R, "%s: bad arguments", who);
    for (int i = 0; i < 10; ++i) SG_REQUIRE(std::isfinite(h_m[i]), "%s: moment %d is not finite", who, i);
    const double n = h_m[0];
    SG_REQUIRE(n >= 1.0, "%s: a box needs at least one point (count %g)", who, n);
    double A[3][3], V[3][3], lambda[3];
    scatter(h_m, A);
    for (auto& row : A)
        for (double& a : row) a /= n;
    if (!jacobi<3>(A, V, lambda)) return sg::fail(SG_EINVAL, "%s: the moments overflow the covariance", who);
    int ord[3] = {0, 1, 2};                                       // descending eigenvalue, the lower index first among equals
    for (int i = 1; i < 3; ++i)
        for (int j = i; j > 0 && lambda[ord[j]] > lambda[ord[j - 1]]; --j) std::swap(ord[j], ord[j - 1]);
    Vec3 row[3];
    if (!(lambda[ord[0]] > 0.0)) {
        // one point, or points that coincide: no direction is singled out, the frame is the identity
        for (int r = 0; r < 3; ++r) row[r] = {{r == 0 ? 1.0 : 0.0, r == 1 ? 1.0 : 0.0, r == 2 ? 1.0 : 0.0}};
    } else {
        for (int r = 0; r < 2; ++r) {
            row[r] = {{V[0][ord[r]], V[1][ord[r]], V[2][ord[r]]}};
            fix_sign(row[r]);
        }
        row[2] = cross(row[0], row[1]);
    }
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            SG_REQUIRE(std::isfinite(row[r].v[c]), "%s: the moments overflow the covariance", who);
            h_R[3 * r + c] = row[r].v[c];
        }
    if (h_eig)
        for (int r = 0; r < 3; ++r) h_eig[r] = lambda[ord[r]];
    return SG_OK;
}

int sg_triangle_pose(const double* h_a, const double* h_b, double* h_T) {
    const char* who = "sg_triangle_pose";
    SG_REQUIRE(h_a && h_b && h_T, "%s: bad arguments", who);
    for (int i = 0; i < 9; ++i) SG_REQUIRE(std::isfinite(h_a[i]) && std::isfinite(h_b[i]), "%s: a coordinate that is not finite", who);
    sgtri::Frame fa, fb;
    sgtri::frame(h_a, fa);
    sgtri::frame(h_b, fb);
    if (!(fa.edge > 0.0 && fa.height > 0.0 && fb.edge > 0.0 && fb.height > 0.0))
        return sg::fail(SG_EUNSUP, "%s: degenerate: a triangle with a zero first edge or with its corners on a line has no frame", who);
    double T[12];
    sgtri::pose_of_frames(fa, fb, T);
    for (int i = 0; i < 12; ++i) SG_REQUIRE(std::isfinite(T[i]), "%s: the coordinates overflow the pose", who);
    for (int i = 0; i < 12; ++i) h_T[i] = T[i];
    return SG_OK;
}

}  // extern "C"
