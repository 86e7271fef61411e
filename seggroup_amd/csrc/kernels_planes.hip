// Plane extraction, device side: hypothesise-and-count RANSAC over the free points of a cloud, the 11 sums of a
// least-squares refit over one plane's inliers, and the labelling of those inliers.
//
//   k_pl_flag / k_pl_compact  the free points (label < 0, or all of them) in ASCENDING index into dense rows of xyz (and normals): 1 / 0 per
//                      point, scan64_device.h's exclusive sum, a scatter.  Triples index this list, so its order is part of the contract.
//   k_pl_generate      one thread per hypothesis: the triple (ransac_draw_device.h with C := M: splitmix64 of the seed, or the caller's
//                      row, checked against 0..M-1 before anything is read through it), the rejection rules in double, the unit normal
//                      and offset into d_plane[h], count[h] = 0 / -1, and the kept h compacted through one integer counter (their order
//                      may vary; every result is stored at [h], so nothing depends on it).
//   k_pl_count         over the kept hypotheses only.  The shape sg_feature_nearest measured: a thread holds kHyp planes in registers
//                      (4 x 4 doubles), the free points go through LDS in tiles of kTile, widened to double once when the tile is filled,
//                      and every lane reads the same address (a broadcast: no bank conflict whatever the layout).  1,024 hypotheses do
//                      not fill the device, so the free list is cut into segments of whole tiles over blockIdx.y and a hypothesis' partial
//                      counts meet in an integer atomicAdd -- the sum does not depend on the order of arrival.
//   k_pl_best          the highest count, the lowest h among equals: one 64-bit integer maximum over (count, ~h).
//   k_pl_moments       n | sum q | sum q q^T (xx xy xz yy yz zz) | sum r^2 over the free inliers of ONE plane, q = p - origin; the launch
//                      shape and both reduction trees are moments_device.h's: a workgroup folds 1,024 consecutive points into one partial
//                      row (sgmom::block_row), sgmom::k_fold adds the rows, sgmom::reduce is the host sequence.
//   k_pl_assign        label[i] = id at the free inliers of one plane; the number labelled through a ballot and one integer atomicAdd.
// The inlier test is one function, inlier(), for the count, the moments and the labelling.  No floating-point atomics: two calls on the
// same input write the same bytes.
#include <cmath>

#include "moments_device.h"
#include "overseg_device.h"
#include "ransac_draw_device.h"
#include "scan64_device.h"
#include "sg_common.h"

namespace {

using sgmom::kBlock;
using sgmom::Origin;

constexpr int kWave = 64;
constexpr int kMaxPoints = 1 << 24;
constexpr int kMaxHypotheses = 1 << 20;
constexpr int kHyp = 4;                       // hypotheses per thread of the counting kernel
constexpr int kTile = 1024;                   // free points per LDS tile: 1,024 x 3 doubles = 24 KiB (48 KiB with normals)
constexpr int kCountWaves = 2048;             // the segments are cut so that about this many waves are in flight
constexpr int kMom = 11;

struct Flags { int flag; int kept; unsigned long long best; int labelled; int pad; };
struct Plane { double n[3], d; };
struct GenParams { double min_edge, min_sine; };
struct Test { double dist, min_cos; };

__device__ __forceinline__ double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// |n.p + d| <= dist, and with a normal |n.nrm| >= min_cos; a NaN fails either compare, and a normal with an infinite component gives an
// infinite or NaN product, which the second compare of that line turns away
__device__ __forceinline__ bool inlier(const Plane& pl, const double* p, const double* nrm, bool with_normals, const Test& t, double* r) {
    *r = dot3(pl.n, p) + pl.d;
    bool in = fabs(*r) <= t.dist;
    if (with_normals) {
        const double a = fabs(dot3(pl.n, nrm));
        in = in && a >= t.min_cos && a < INFINITY;
    }
    return in;
}

__global__ __launch_bounds__(kBlock) void k_pl_flag(const int32_t* __restrict__ label, int N, int32_t* __restrict__ flag) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < N) flag[i] = (!label || label[i] < 0) ? 1 : 0;
}

__global__ __launch_bounds__(kBlock) void k_pl_compact(const float* __restrict__ xyz, int xs, const float* __restrict__ normals, int N,
                                                       const int32_t* __restrict__ flag, const int64_t* __restrict__ off,
                                                       float* __restrict__ pts, float* __restrict__ nrm) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N || !flag[i]) return;
    const size_t m = (size_t)off[i];                                  // < off[N] <= N: the scan of N flags of 0 / 1
    for (int r = 0; r < 3; ++r) {
        pts[m * 3 + r] = xyz[(size_t)i * xs + r];
        if (normals) nrm[m * 3 + r] = normals[(size_t)i * 3 + r];
    }
}

__global__ __launch_bounds__(kBlock) void k_pl_fill(int32_t* __restrict__ count, double* __restrict__ plane, int H) {
    const int h = blockIdx.x * kBlock + threadIdx.x;
    if (h >= H) return;
    count[h] = -1;
    for (int r = 0; r < 4; ++r) plane[(size_t)h * 4 + r] = 0.0;
}

__global__ __launch_bounds__(kBlock) void k_pl_generate(const float* __restrict__ pts, const int64_t* __restrict__ d_M, int H,
                                                        const int32_t* __restrict__ triples, unsigned long long seed, GenParams prm,
                                                        int compact, int32_t* __restrict__ count, double* __restrict__ plane,
                                                        int32_t* __restrict__ kept, Flags* __restrict__ fl) {
    const int h = blockIdx.x * kBlock + threadIdx.x;
    if (h >= H) return;
    const long long M = (long long)*d_M;
    double out[4] = {0.0, 0.0, 0.0, 0.0};
    bool keep = M >= 3;
    int t[3] = {0, 0, 0};
    if (keep) {                                                          // the flag is raised only with three free points or more
        bool distinct;
        keep = sgdraw::triple_of(h, triples, seed, (int)M, t, &distinct);  // M <= N <= 2^24: the sum of N flags of 0 / 1
        if (!keep) atomicOr(&fl->flag, 2);
        keep = keep && distinct;
    }
    if (keep) {
        double p[3][3];
        for (int e = 0; e < 3; ++e)
            for (int r = 0; r < 3; ++r) p[e][r] = (double)pts[(size_t)t[e] * 3 + r];
        double u[3], v[3], w[3];
        for (int r = 0; r < 3; ++r) {
            u[r] = p[1][r] - p[0][r];
            v[r] = p[2][r] - p[0][r];
            w[r] = p[2][r] - p[1][r];
        }
        const double c[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
        const double lu = sqrt(dot3(u, u)), lv = sqrt(dot3(v, v)), lw = sqrt(dot3(w, w)), lc = sqrt(dot3(c, c));
        // written so that a NaN rejects; every edge is at least min_edge > 0 and min_sine > 0, so a kept |c| is > 0
        keep = lu >= prm.min_edge && lv >= prm.min_edge && lw >= prm.min_edge && lc >= (prm.min_sine * lu) * lv && lc > 0.0;
        if (keep) {
            for (int r = 0; r < 3; ++r) out[r] = c[r] / lc;
            out[3] = -dot3(out, p[0]);
            keep = out[3] == out[3];                                      // an overflow in the products: not a plane
            if (!keep) out[0] = out[1] = out[2] = out[3] = 0.0;
        }
    }
    for (int r = 0; r < 4; ++r) plane[(size_t)h * 4 + r] = out[r];
    count[h] = keep ? 0 : -1;
    if (compact) {
        if (keep) kept[atomicAdd(&fl->kept, 1)] = h;
    } else {
        kept[h] = h;
    }
}

// thread t of workgroup (bx, by) owns kept[bx * 1024 + k * 256 + t], k < kHyp, over the free points [by * seg_pts, (by + 1) * seg_pts)
template <bool kNormals>
__global__ __launch_bounds__(kBlock) void k_pl_count(const float* __restrict__ pts, const float* __restrict__ nrm, int M, int seg_pts,
                                                     const int32_t* __restrict__ kept, int nkept, const double* __restrict__ plane, Test test,
                                                     int32_t* __restrict__ count) {
    __shared__ double s_p[kTile * 3];
    __shared__ double s_n[kNormals ? kTile * 3 : 1];
    Plane pl[kHyp];
    int h[kHyp], cnt[kHyp];
#pragma unroll
    for (int k = 0; k < kHyp; ++k) {
        const int s = blockIdx.x * (kBlock * kHyp) + k * kBlock + threadIdx.x;
        h[k] = s < nkept ? kept[s] : -1;
        if (h[k] >= 0 && count[h[k]] < 0) h[k] = -1;                     // uncompacted list: a rejected hypothesis (its -1 is never added to)
        cnt[k] = 0;
        for (int r = 0; r < 3; ++r) pl[k].n[r] = h[k] >= 0 ? plane[(size_t)h[k] * 4 + r] : 0.0;
        pl[k].d = h[k] >= 0 ? plane[(size_t)h[k] * 4 + 3] : 0.0;
    }
    const int m_end = min(M, ((int)blockIdx.y + 1) * seg_pts);          // seg_pts * gridDim.y < M + seg_pts <= 2^25
    for (int m0 = (int)blockIdx.y * seg_pts; m0 < m_end; m0 += kTile) {
        const int rows = min(kTile, m_end - m0);
        __syncthreads();
        for (int e = threadIdx.x; e < rows * 3; e += kBlock) {
            s_p[e] = (double)pts[(size_t)m0 * 3 + e];
            if (kNormals) s_n[e] = (double)nrm[(size_t)m0 * 3 + e];
        }
        __syncthreads();
        for (int r = 0; r < rows; ++r) {
            const double p[3] = {s_p[3 * r], s_p[3 * r + 1], s_p[3 * r + 2]};
            double q[3] = {0.0, 0.0, 0.0};
            if (kNormals) { q[0] = s_n[3 * r]; q[1] = s_n[3 * r + 1]; q[2] = s_n[3 * r + 2]; }
#pragma unroll
            for (int k = 0; k < kHyp; ++k) {
                double res;
                cnt[k] += inlier(pl[k], p, q, kNormals, test, &res) ? 1 : 0;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kHyp; ++k)
        if (h[k] >= 0 && cnt[k] > 0) atomicAdd(&count[h[k]], cnt[k]);
}

__global__ __launch_bounds__(kBlock) void k_pl_best(const int32_t* __restrict__ count, int H, unsigned long long* __restrict__ best) {
    const int h = blockIdx.x * kBlock + threadIdx.x;
    unsigned long long key = 0ull;                                       // 0: no kept hypothesis (a kept one has a low word >= 1)
    if (h < H && count[h] >= 0) key = ((unsigned long long)(unsigned int)count[h] << 32) | (0xffffffffu - (unsigned int)h);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long other = __shfl_xor(key, o);
        key = other > key ? other : key;
    }
    if (threadIdx.x % kWave == 0 && key) atomicMax(best, key);
}

// every thread reaches block_row: a point past N, not free or outside the plane adds 0
__global__ __launch_bounds__(kBlock) void k_pl_moments(const float* __restrict__ xyz, int xs, const int32_t* __restrict__ label,
                                                       const float* __restrict__ normals, int N, Plane pl, Test test, Origin o,
                                                       double* __restrict__ partial) {
    double acc[kMom];
#pragma unroll
    for (int m = 0; m < kMom; ++m) acc[m] = 0.0;
    const long long base = (long long)blockIdx.x * sgmom::kItems + threadIdx.x;
#pragma unroll
    for (int j = 0; j < sgmom::kPer; ++j) {
        const long long i = base + (long long)j * kBlock;
        if (i >= (long long)N) continue;
        if (label && label[i] >= 0) continue;
        const float* pp = xyz + (size_t)i * xs;
        const double p[3] = {(double)pp[0], (double)pp[1], (double)pp[2]};
        double nr[3] = {0.0, 0.0, 0.0};
        if (normals)
            for (int r = 0; r < 3; ++r) nr[r] = (double)normals[(size_t)i * 3 + r];
        double res;
        if (!inlier(pl, p, nr, normals != nullptr, test, &res)) continue;
        const double q[3] = {p[0] - o.c[0], p[1] - o.c[1], p[2] - o.c[2]};
        acc[0] += 1.0;
        int k = 4;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            acc[1 + r] += q[r];
#pragma unroll
            for (int c = r; c < 3; ++c) acc[k++] += q[r] * q[c];
        }
        acc[10] += res * res;
    }
    sgmom::block_row(acc, partial + (size_t)blockIdx.x * kMom);
}

__global__ __launch_bounds__(kBlock) void k_pl_assign(const float* __restrict__ xyz, int xs, const float* __restrict__ normals, int N, Plane pl,
                                                      Test test, int id, int32_t* __restrict__ label, int* __restrict__ labelled) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    bool in = false;
    if (i < N && label[i] < 0) {
        const float* pp = xyz + (size_t)i * xs;
        const double p[3] = {(double)pp[0], (double)pp[1], (double)pp[2]};
        double nr[3] = {0.0, 0.0, 0.0};
        if (normals)
            for (int r = 0; r < 3; ++r) nr[r] = (double)normals[(size_t)i * 3 + r];
        double res;
        in = inlier(pl, p, nr, normals != nullptr, test, &res);
        if (in) label[i] = id;
    }
    const int n = __popcll(__ballot(in));
    if (threadIdx.x % kWave == 0 && n) atomicAdd(labelled, n);
}

constexpr int kStages = 5;
const char* const kStageNames[kStages] = {"compact", "generate", "count", "moments", "assign"};
thread_local sgos::StageTimes<kStages> t_plane;
thread_local bool t_compact = true;

// what the three entry points share: the plane, the distance and the optional normal test, checked
int read_test(const char* who, const double* h_plane, double dist, const float* d_normals, double min_cos, Plane* pl, Test* test) {
    SG_REQUIRE(h_plane && sgmom::finite_n<4>(h_plane), "%s: the plane is four finite numbers (n, d)", who);
    SG_REQUIRE(std::isfinite(dist) && dist >= 0.0, "%s: dist must be a finite length >= 0 (%g)", who, dist);
    SG_REQUIRE(!d_normals || (min_cos >= 0.0 && min_cos <= 1.0), "%s: min_cos must be in 0..1 (%g)", who, min_cos);
    for (int r = 0; r < 3; ++r) pl->n[r] = h_plane[r];
    pl->d = h_plane[3];
    test->dist = dist;
    test->min_cos = d_normals ? min_cos : 0.0;
    return SG_OK;
}

}  // namespace

extern "C" {

SG_STAGE_TIMER_API(plane, t_plane, kStageNames)

int sg_plane_set_tuning(int compact) {
    t_compact = compact != 0;
    return SG_OK;
}

size_t sg_plane_ransac_ws_bytes(int N, int H, int with_normals) {
    if (N < 0 || N > kMaxPoints || H < 0 || H > kMaxHypotheses) return 0;
    const size_t n = (size_t)std::max(N, 1);
    return sg::align_up(sizeof(Flags)) + sg::align_up(n * sizeof(int32_t)) + sg::align_up((n + 1) * sizeof(int64_t)) +
           sg::align_up((size_t)(sgscan::tiles_of(N) + 1) * sizeof(long long)) + (with_normals ? 2 : 1) * sg::align_up(n * 3 * sizeof(float)) +
           sg::align_up((size_t)std::max(H, 1) * sizeof(int32_t));
}

int sg_plane_ransac(const float* d_xyz, int stride, int N, const int32_t* d_label, const float* d_normals, double min_cos, int H, uint64_t seed,
                    const int32_t* d_triples, double dist, double min_edge, double min_sine, int32_t* d_count, double* d_plane, int* h_free,
                    int* h_best, void* d_ws, size_t ws_bytes, void* stream) {
    const char* who = "sg_plane_ransac";
    SG_REQUIRE(N >= 0 && H >= 0 && stride >= 3, "%s: bad arguments (%d points in rows of %d floats, %d hypotheses)", who, N, stride, H);
    if (N > kMaxPoints || H > kMaxHypotheses)
        return sg::fail(SG_EUNSUP, "%s: %d points, %d hypotheses; a call takes at most %d and %d", who, N, H, kMaxPoints, kMaxHypotheses);
    SG_REQUIRE(std::isfinite(dist) && dist >= 0.0 && std::isfinite(min_edge) && min_edge > 0.0 && min_sine > 0.0 && min_sine <= 1.0,
               "%s: dist must be a finite length >= 0, min_edge a finite length > 0 and min_sine in (0, 1] (%g, %g, %g)", who, dist, min_edge,
               min_sine);
    SG_REQUIRE(!d_normals || (min_cos >= 0.0 && min_cos <= 1.0), "%s: min_cos must be in 0..1 (%g)", who, min_cos);
    SG_REQUIRE(h_free && h_best, "%s: bad arguments", who);
    SG_REQUIRE(H == 0 || (d_count && d_plane), "%s: bad arguments", who);
    *h_free = 0;
    *h_best = -1;
    hipStream_t st = sg::as_stream(stream);
    if (N == 0) {
        if (H) k_pl_fill<<<sg::cdiv(H, kBlock), kBlock, 0, st>>>(d_count, d_plane, H);
        SG_HIP(hipStreamSynchronize(st));
        SG_LAUNCH_CHECK();
        return SG_OK;
    }
    SG_REQUIRE(d_xyz && d_ws, "%s: bad arguments", who);
    const size_t need = sg_plane_ransac_ws_bytes(N, H, d_normals != nullptr);
    SG_REQUIRE(ws_bytes >= need, "%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
    sg::Carver cv(d_ws, ws_bytes);
    Flags* fl = cv.take<Flags>(1);
    int32_t* flag = cv.take<int32_t>((size_t)N);
    int64_t* off = cv.take<int64_t>((size_t)N + 1);
    long long* tsum = cv.take<long long>((size_t)sgscan::tiles_of(N) + 1);
    float* pts = cv.take<float>((size_t)N * 3);
    float* nrm = d_normals ? cv.take<float>((size_t)N * 3) : nullptr;
    int32_t* kept = cv.take<int32_t>((size_t)std::max(H, 1));
    SG_REQUIRE(cv.ok, "%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
    const Test test{dist, d_normals ? min_cos : 0.0};
    sgos::StageClock<3> clock(st, t_plane.timing, t_plane.us);
    SG_HIP(hipMemsetAsync(fl, 0, sizeof(Flags), st));
    k_pl_flag<<<sg::cdiv(N, kBlock), kBlock, 0, st>>>(d_label, N, flag);
    sgscan::exclusive_scan64(flag, N, tsum, off, st);
    k_pl_compact<<<sg::cdiv(N, kBlock), kBlock, 0, st>>>(d_xyz, stride, d_normals, N, flag, off, pts, nrm);
    clock.tick();
    if (H)
        k_pl_generate<<<sg::cdiv(H, kBlock), kBlock, 0, st>>>(pts, off + N, H, d_triples, (unsigned long long)seed, GenParams{min_edge, min_sine},
                                                               t_compact ? 1 : 0, d_count, d_plane, kept, fl);
    Flags land{};
    int64_t M64 = 0;
    SG_HIP(hipMemcpyAsync(&land, fl, sizeof(Flags), hipMemcpyDeviceToHost, st));
    SG_HIP(hipMemcpyAsync(&M64, off + N, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    clock.tick();
    SG_HIP(hipStreamSynchronize(st));
    SG_LAUNCH_CHECK();
    if (M64 < 0 || M64 > (int64_t)N) return sg::fail(SG_EINTERNAL, "%s: %lld free points of %d", who, (long long)M64, N);
    const int M = (int)M64;
    *h_free = M;
    if (land.flag & 2) return sg::fail(SG_EINVAL, "%s: a triple names a free point outside 0..%d", who, M - 1);
    const int nkept = t_compact ? land.kept : H;
    if (nkept < 0 || nkept > H) return sg::fail(SG_EINTERNAL, "%s: %d kept of %d hypotheses", who, nkept, H);
    if (M < 3 || nkept == 0) return SG_OK;
    const int tiles = sg::cdiv(M, kTile);
    const int segments = std::min(tiles, std::max(1, kCountWaves / sg::cdiv(nkept, kWave * kHyp)));
    const int seg_pts = sg::cdiv(tiles, segments) * kTile;              // whole tiles; the last segment may be short
    const dim3 grid(sg::cdiv(nkept, kBlock * kHyp), sg::cdiv(M, seg_pts));
    if (d_normals) k_pl_count<true><<<grid, kBlock, 0, st>>>(pts, nrm, M, seg_pts, kept, nkept, d_plane, test, d_count);
    else k_pl_count<false><<<grid, kBlock, 0, st>>>(pts, nrm, M, seg_pts, kept, nkept, d_plane, test, d_count);
    k_pl_best<<<sg::cdiv(H, kBlock), kBlock, 0, st>>>(d_count, H, &fl->best);
    SG_HIP(hipMemcpyAsync(&land, fl, sizeof(Flags), hipMemcpyDeviceToHost, st));
    clock.tick();
    SG_HIP(hipStreamSynchronize(st));
    SG_LAUNCH_CHECK();
    if (land.best) *h_best = (int)(0xffffffffu - (unsigned int)(land.best & 0xffffffffull));
    return SG_OK;
}

size_t sg_plane_moments_ws_bytes(int N) { return (N < 0 || N > kMaxPoints) ? 0 : sgmom::ws_bytes<kMom>(N); }

int sg_plane_moments(const float* d_xyz, int stride, int N, const int32_t* d_label, const float* d_normals, double min_cos, const double* h_plane,
                     double dist, const double* h_origin, double* h_out, void* d_ws, size_t ws_bytes, void* stream) {
    const char* who = "sg_plane_moments";
    SG_REQUIRE(N >= 0 && stride >= 3, "%s: bad arguments (%d points in rows of %d floats)", who, N, stride);
    if (N > kMaxPoints) return sg::fail(SG_EUNSUP, "%s: %d points; a call takes at most %d", who, N, kMaxPoints);
    Plane pl;
    Test test;
    if (int rc = read_test(who, h_plane, dist, d_normals, min_cos, &pl, &test)) return rc;
    SG_REQUIRE(h_origin && h_out, "%s: bad arguments", who);
    SG_REQUIRE(sgmom::finite_n<3>(h_origin), "%s: an origin that is not finite", who);
    if (N == 0) {
        for (int m = 0; m < kMom; ++m) h_out[m] = 0.0;
        return SG_OK;
    }
    SG_REQUIRE(d_xyz && d_ws, "%s: bad arguments", who);
    const Origin o = sgmom::origin_of(h_origin);
    hipStream_t st = sg::as_stream(stream);
    sgos::StageClock<1> clock(st, t_plane.timing, t_plane.us + 3);
    auto first = [&](int rows, double* d_partial, int*) {
        k_pl_moments<<<rows, kBlock, 0, st>>>(d_xyz, stride, d_label, d_normals, N, pl, test, o, d_partial);
    };
    return sgmom::reduce<kMom>(who, N, d_ws, ws_bytes, st, first, h_out, nullptr, [&] { clock.tick(); });   // no flag: k_pl_moments raises none
}

size_t sg_plane_assign_ws_bytes(int N) { return (N < 0 || N > kMaxPoints) ? 0 : sg::align_up(sizeof(Flags)); }

int sg_plane_assign(const float* d_xyz, int stride, int N, const float* d_normals, double min_cos, const double* h_plane, double dist, int id,
                    int32_t* d_label, int* h_labelled, void* d_ws, size_t ws_bytes, void* stream) {
    const char* who = "sg_plane_assign";
    SG_REQUIRE(N >= 0 && stride >= 3, "%s: bad arguments (%d points in rows of %d floats)", who, N, stride);
    if (N > kMaxPoints) return sg::fail(SG_EUNSUP, "%s: %d points; a call takes at most %d", who, N, kMaxPoints);
    Plane pl;
    Test test;
    if (int rc = read_test(who, h_plane, dist, d_normals, min_cos, &pl, &test)) return rc;
    SG_REQUIRE(id >= 0, "%s: the id must be >= 0 (%d): a negative label is a free point", who, id);
    SG_REQUIRE(h_labelled, "%s: bad arguments", who);
    *h_labelled = 0;
    if (N == 0) return SG_OK;
    SG_REQUIRE(d_xyz && d_label && d_ws, "%s: bad arguments", who);
    SG_REQUIRE(ws_bytes >= sg_plane_assign_ws_bytes(N), "%s: workspace too small (%zu < %zu)", who, ws_bytes, sg_plane_assign_ws_bytes(N));
    Flags* fl = (Flags*)d_ws;
    hipStream_t st = sg::as_stream(stream);
    Flags land{};
    {
        sgos::StageClock<1> clock(st, t_plane.timing, t_plane.us + 4);
        SG_HIP(hipMemsetAsync(fl, 0, sizeof(Flags), st));
        k_pl_assign<<<sg::cdiv(N, kBlock), kBlock, 0, st>>>(d_xyz, stride, d_normals, N, pl, test, id, d_label, &fl->labelled);
        SG_HIP(hipMemcpyAsync(&land, fl, sizeof(Flags), hipMemcpyDeviceToHost, st));
        clock.tick();
        SG_HIP(hipStreamSynchronize(st));
    }
    SG_LAUNCH_CHECK();
    *h_labelled = land.labelled;
    return SG_OK;
}

}  // extern "C"
