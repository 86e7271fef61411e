// Global (init-free) registration, device side: the three stages a coarse pose needs besides the tree's own thinning,
// radius lists, normals and nearest-point search.
//
//   k_spfh             the simplified point feature histogram of every point over its radius row: one WAVE per point, lanes take pairs, the
//                      three angular features of a pair in double, 3 x 11 integer bins and the pair count in the wave's LDS row (integer
//                      atomics: the counts do not depend on the order).  The lists are checked here: a row outside
//                      0 <= lo <= hi <= off[N] (or off[0] != 0) raises flag 8 and counts as empty, an entry outside 0..N-1 raises flag 4 and
//                      is left out -- nothing is read through either.
//   k_fpfh             the weighted sum of the neighbours' normalised histograms: one wave per point, lanes 0..32 own a bin and walk the row in
//                      stored order (a double accumulator each), 64 entries' index, squared distance and pair count fetched at a time by
//                      the whole wave and handed round by readlane; the neighbour's 136-byte row is one coalesced read.
//   k_feature_nearest  brute-force nearest row of b for every row of a: a thread holds its query in registers, b goes through LDS in tiles
//                      that every lane reads at the same address; channels past C are zeros on both sides, which add +0 to a sum that is
//                      never negative, so the fp32 statement keeps its bytes.  U / 64 waves do not fill the device, so the rows of b are cut
//                      into segments (blockIdx.y) and a query's answers meet in one 64-bit integer minimum over (d2 bits, index): d2 >= +0
//                      orders as its bits do, the index in the low word sends ties to the lowest -- whatever the order of arrival.
//   k_ransac_gather    the C correspondences' points packed into two dense arrays; an index out of range raises the flag first.
//   k_ransac_filter    one thread per hypothesis: the triple (ransac_draw_device.h: splitmix64 of the seed, or the caller's), the
//                      pre-rejection in double, and the surviving h compacted through one integer counter (their order may vary;
//                      nothing depends on it).
//   k_ransac_count     over the survivors only: the pose of triangle_pose.h again from the triple, the correspondences tiled through LDS,
//                      one wave (or, by sg_ransac_set_tuning, one thread) per survivor.  The result is stored at [h].
// No floating-point atomics anywhere: two calls on the same input write the same bytes.
#include <cmath>

#include "overseg_device.h"
#include "ransac_draw_device.h"
#include "sg_common.h"
#include "triangle_pose.h"
#include "wave_ops.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWave = 64;
constexpr int kWaves = kBlock / kWave;
constexpr int kBins = 11;
constexpr int kHist = 3 * kBins;              // 33 bins
constexpr int kRow = kHist + 1;               // ... and the number of counted pairs
constexpr double kPi = 3.14159265358979323846;
constexpr int kMaxFeaturePoints = 1 << 18;    // sg_feature_nearest, sg_ransac_count: rows / correspondences
constexpr int kMaxHypotheses = 1 << 24;

struct Flags { int flag; int survivors; };

__device__ __forceinline__ int bin_of(double x) {
    const int b = (int)floor(11.0 * x);
    return min(max(b, 0), kBins - 1);
}

__device__ __forceinline__ double bcast_d(double v, int lane) {
    const long long x = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(x & 0xffffffffll), lane), hi = __builtin_amdgcn_readlane((int)(x >> 32), lane);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// the row of point i, checked: (lo, hi) with lo == hi for a row that does not hold together
__device__ __forceinline__ void checked_row(const int64_t* __restrict__ off, int N, int i, bool has_idx, int lane, int* flag, int64_t& lo, int64_t& hi) {
    const int64_t T = off[N];
    lo = off[i];
    hi = off[i + 1];
    if (!(lo >= 0 && lo <= hi && hi <= T) || (i == 0 && lo != 0) || (hi > lo && !has_idx)) {
        if (lane == 0) atomicOr(flag, 8);
        lo = 0;
        hi = 0;
    }
}

__global__ __launch_bounds__(kBlock) void k_spfh(const float* __restrict__ xyz, int xs, const float* __restrict__ nrm, int N,
                                                 const int64_t* __restrict__ off, const int32_t* __restrict__ idx, int32_t* __restrict__ spfh,
                                                 int* __restrict__ flag) {
    __shared__ int s_h[kWaves][kRow];
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    const int i = blockIdx.x * kWaves + wave;
    const bool active = i < N;
    if (lane < kRow) s_h[wave][lane] = 0;
    __syncthreads();
    if (active) {
        int64_t lo, hi;
        checked_row(off, N, i, idx != nullptr, lane, flag, lo, hi);
        const float* pi = xyz + (size_t)i * xs;
        const float* qi = nrm + (size_t)i * 3;
        const double p[3] = {(double)pi[0], (double)pi[1], (double)pi[2]};
        const double ni[3] = {(double)qi[0], (double)qi[1], (double)qi[2]};
        bool bad = false;
        for (int64_t e = lo + lane; e < hi; e += kWave) {
            const int j = idx[e];
            if ((unsigned)j >= (unsigned)N) { bad = true; continue; }
            const float* pj = xyz + (size_t)j * xs;
            const float* qj = nrm + (size_t)j * 3;
            const double nj[3] = {(double)qj[0], (double)qj[1], (double)qj[2]};
            double d[3] = {(double)pj[0] - p[0], (double)pj[1] - p[1], (double)pj[2] - p[2]};
            const double len = sqrt(sgtri::dot3(d, d));
            if (len == 0.0) continue;
            for (int r = 0; r < 3; ++r) d[r] = d[r] / len;
            const double a1 = sgtri::dot3(ni, d), a2 = sgtri::dot3(nj, d);
            const bool swap = fabs(a1) < fabs(a2);
            double u[3], t[3];
            for (int r = 0; r < 3; ++r) {
                u[r] = swap ? nj[r] : ni[r];
                t[r] = swap ? ni[r] : nj[r];
                d[r] = swap ? -d[r] : d[r];
            }
            const double phi = sgtri::dot3(u, d);
            double v[3], w[3];
            sgtri::cross3(d, u, v);
            const double vl = sqrt(sgtri::dot3(v, v));
            if (vl == 0.0) continue;
            for (int r = 0; r < 3; ++r) v[r] = v[r] / vl;
            sgtri::cross3(u, v, w);
            const double alpha = sgtri::dot3(v, t);
            const double theta = atan2(sgtri::dot3(w, t), sgtri::dot3(u, t));
            atomicAdd(&s_h[wave][bin_of((theta + kPi) / (2.0 * kPi))], 1);
            atomicAdd(&s_h[wave][kBins + bin_of((alpha + 1.0) / 2.0)], 1);
            atomicAdd(&s_h[wave][2 * kBins + bin_of((phi + 1.0) / 2.0)], 1);
            atomicAdd(&s_h[wave][kHist], 1);
        }
        if (bad) atomicOr(flag, 4);
    }
    __syncthreads();
    if (active && lane < kRow) spfh[(size_t)i * kRow + lane] = s_h[wave][lane];
}

__global__ __launch_bounds__(kBlock) void k_fpfh(const float* __restrict__ xyz, int xs, int N, const int64_t* __restrict__ off,
                                                 const int32_t* __restrict__ idx, const int32_t* __restrict__ spfh, float* __restrict__ fpfh,
                                                 int* __restrict__ flag) {
    __shared__ double s_s[kWaves][kHist];
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    const int i = blockIdx.x * kWaves + wave;
    const bool active = i < N;
    double S = 0.0;
    if (active) {
        int64_t lo, hi;
        checked_row(off, N, i, idx != nullptr, lane, flag, lo, hi);
        const float* pi = xyz + (size_t)i * xs;
        const double p[3] = {(double)pi[0], (double)pi[1], (double)pi[2]};
        for (int64_t base = lo; base < hi; base += kWave) {
            const int64_t e = base + lane;
            int j = -1, pairs = 0;
            double dd = 0.0;
            if (e < hi) {
                j = idx[e];
                if ((unsigned)j >= (unsigned)N) j = -1;                  // flagged by k_spfh; left out here as there
            }
            if (j >= 0) {
                const float* pj = xyz + (size_t)j * xs;
                const double d[3] = {(double)pj[0] - p[0], (double)pj[1] - p[1], (double)pj[2] - p[2]};
                dd = sgtri::dot3(d, d);
                pairs = spfh[(size_t)j * kRow + kHist];
            }
            const int use = (j >= 0 && dd > 0.0 && pairs > 0) ? 1 : 0;
            const int cnt = (int)min((int64_t)kWave, hi - base);
            for (int t = 0; t < cnt; ++t) {
                if (!__builtin_amdgcn_readlane(use, t)) continue;         // wave-uniform
                const int jt = __builtin_amdgcn_readlane(j, t), pt = __builtin_amdgcn_readlane(pairs, t);
                const double dt = bcast_d(dd, t);
                if (lane < kHist) S = S + ((100.0 * (double)spfh[(size_t)jt * kRow + lane]) / (double)pt) / dt;
            }
        }
        if (lane < kHist) s_s[wave][lane] = S;
    }
    __syncthreads();
    if (active && lane < kHist) {
        const int g = lane / kBins;
        double tot = 0.0;
        for (int b = 0; b < kBins; ++b) tot = tot + s_s[wave][g * kBins + b];
        fpfh[(size_t)i * kHist + lane] = tot > 0.0 ? (float)((100.0 * S) / tot) : 0.0f;
    }
}

// ---- nearest descriptor ----------------------------------------------------------------------------------------------------------------------
constexpr int kFnBlock = 128;                 // queries per workgroup, one a thread
constexpr int kFnTile = 128;                  // rows of b per LDS tile: 128 x 64 floats = 32 KiB at the widest

constexpr int kFnWaves = 2048;                // the segments are cut so that about this many waves are in flight

__global__ __launch_bounds__(kBlock) void k_fn_init(unsigned long long* __restrict__ key, int U) {
    const int u = blockIdx.x * kBlock + threadIdx.x;
    if (u < U) key[u] = ~0ull;
}

// the key buffer IS out_idx: every key is read before its place is written
__global__ __launch_bounds__(kBlock) void k_fn_finish(int64_t* __restrict__ out_idx, float* __restrict__ out_d2, int U) {
    const int u = blockIdx.x * kBlock + threadIdx.x;
    if (u >= U) return;
    const unsigned long long k = (unsigned long long)out_idx[u];
    out_idx[u] = (int64_t)(k & 0xffffffffull);
    out_d2[u] = __uint_as_float((unsigned int)(k >> 32));
}

template <int CT>
__global__ __launch_bounds__(kFnBlock) void k_feature_nearest(const float* __restrict__ a, const float* __restrict__ b, int U, int N, int C,
                                                              int seg_rows, unsigned long long* __restrict__ key) {
    __shared__ __attribute__((aligned(16))) float s_b[kFnTile * CT];
    const int u = blockIdx.x * kFnBlock + threadIdx.x;
    float q[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) q[c] = (u < U && c < C) ? a[(size_t)u * C + c] : 0.0f;
    float best = 0.0f;
    int bi = -1;
    const int n_end = min(N, ((int)blockIdx.y + 1) * seg_rows);         // seg_rows * gridDim.y < N + seg_rows <= 2^18 + 2^18
    for (int n0 = (int)blockIdx.y * seg_rows; n0 < n_end; n0 += kFnTile) {
        const int rows = min(kFnTile, n_end - n0);
        __syncthreads();
        for (int e = threadIdx.x; e < rows * CT; e += kFnBlock) {
            const int r = e / CT, c = e % CT;
            s_b[e] = c < C ? b[(size_t)(n0 + r) * C + c] : 0.0f;
        }
        __syncthreads();
        for (int r = 0; r < rows; ++r) {
            float d = 0.0f;
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                const float t = q[c] - s_b[r * CT + c];
                d = d + t * t;
            }
            if (bi < 0 || d < best) { best = d; bi = n0 + r; }
        }
    }
    if (u < U && bi >= 0) atomicMin(&key[u], ((unsigned long long)__float_as_uint(best) << 32) | (unsigned int)bi);
}

// ---- RANSAC ---------------------------------------------------------------------------------------------------------------------------------
constexpr int kRcTile = 1024;                 // correspondences per LDS tile: 2 x 1024 x 3 floats = 24 KiB

__global__ __launch_bounds__(kBlock) void k_ransac_gather(const float* __restrict__ m, int ms, int U, const float* __restrict__ f, int fs, int N,
                                                          const int32_t* __restrict__ ci, const int32_t* __restrict__ cj, int C,
                                                          float* __restrict__ pa, float* __restrict__ pb, int* __restrict__ flag) {
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= C) return;
    const int i = ci[c], j = cj[c];
    const bool ok = (unsigned)i < (unsigned)U && (unsigned)j < (unsigned)N;
    if (!ok) atomicOr(flag, 1);
    for (int r = 0; r < 3; ++r) {
        pa[(size_t)c * 3 + r] = ok ? m[(size_t)i * ms + r] : 0.0f;
        pb[(size_t)c * 3 + r] = ok ? f[(size_t)j * fs + r] : 0.0f;
    }
}

__device__ __forceinline__ void load_triangle(const float* __restrict__ p, const int* t, double* x) {
    for (int e = 0; e < 3; ++e)
        for (int r = 0; r < 3; ++r) x[3 * e + r] = (double)p[(size_t)t[e] * 3 + r];
}

struct RansacParams { double max_d2, similarity, min_edge; };

__global__ __launch_bounds__(kBlock) void k_ransac_filter(const float* __restrict__ pa, const float* __restrict__ pb, int C, int H,
                                                          const int32_t* __restrict__ triples, unsigned long long seed, RansacParams prm,
                                                          int32_t* __restrict__ count, int32_t* __restrict__ surv, Flags* __restrict__ fl) {
    const int h = blockIdx.x * kBlock + threadIdx.x;
    if (h >= H) return;
    int t[3];
    bool keep;
    if (!sgdraw::triple_of(h, triples, seed, C, t, &keep)) {
        atomicOr(&fl->flag, 2);
        count[h] = -1;
        return;
    }
    if (keep) {
        double a[9], b[9];
        load_triangle(pa, t, a);
        load_triangle(pb, t, b);
        for (int e = 0; e < 3; ++e) {
            const int p = e, q = (e + 1) % 3;
            const double da[3] = {a[3 * q] - a[3 * p], a[3 * q + 1] - a[3 * p + 1], a[3 * q + 2] - a[3 * p + 2]};
            const double db[3] = {b[3 * q] - b[3 * p], b[3 * q + 1] - b[3 * p + 1], b[3 * q + 2] - b[3 * p + 2]};
            const double la = sqrt(sgtri::dot3(da, da)), lb = sqrt(sgtri::dot3(db, db));
            // written so that a NaN rejects
            keep = keep && la >= prm.min_edge && lb >= prm.min_edge && la >= prm.similarity * lb && lb >= prm.similarity * la;
        }
        if (keep) {                                                  // every edge is at least min_edge > 0: the frames divide by no zero
            sgtri::Frame fa, fb;
            sgtri::frame(a, fa);
            sgtri::frame(b, fb);
            keep = fa.height >= prm.min_edge / 8.0 && fb.height >= prm.min_edge / 8.0;
        }
    }
    if (keep) surv[atomicAdd(&fl->survivors, 1)] = h;
    else count[h] = -1;
}

// kG lanes per survivor: 64 (a wave walks the tile, 64 correspondences a step) or 1 (a thread walks it alone)
template <int kG>
__global__ __launch_bounds__(kBlock) void k_ransac_count(const float* __restrict__ pa, const float* __restrict__ pb, int C,
                                                         const int32_t* __restrict__ triples, unsigned long long seed, RansacParams prm,
                                                         const int32_t* __restrict__ surv, int nsurv, int32_t* __restrict__ count) {
    __shared__ float s_a[kRcTile * 3];
    __shared__ float s_b[kRcTile * 3];
    const int s = blockIdx.x * (kBlock / kG) + threadIdx.x / kG, lg = threadIdx.x % kG;
    const bool active = s < nsurv;
    double T[12];
    for (int k = 0; k < 12; ++k) T[k] = 0.0;
    int h = 0;
    if (active) {
        h = surv[s];
        int t[3];
        bool distinct;
        sgdraw::triple_of(h, triples, seed, C, t, &distinct);        // a survivor's triple passed the filter's checks
        double a[9], b[9];
        load_triangle(pa, t, a);
        load_triangle(pb, t, b);
        sgtri::triangle_pose(a, b, T);
    }
    int cnt = 0;
    for (int c0 = 0; c0 < C; c0 += kRcTile) {
        const int rows = min(kRcTile, C - c0);
        __syncthreads();
        for (int e = threadIdx.x; e < rows * 3; e += kBlock) {
            s_a[e] = pa[(size_t)c0 * 3 + e];
            s_b[e] = pb[(size_t)c0 * 3 + e];
        }
        __syncthreads();
        for (int r0 = 0; r0 < rows; r0 += kG) {
            const int r = r0 + lg;
            bool in = false;
            if (r < rows) {
                const double x = (double)s_a[3 * r], y = (double)s_a[3 * r + 1], z = (double)s_a[3 * r + 2];
                double d[3];
                for (int k = 0; k < 3; ++k)
                    d[k] = ((((T[4 * k] * x + T[4 * k + 1] * y) + T[4 * k + 2] * z) + T[4 * k + 3])) - (double)s_b[3 * r + k];
                in = active && sgtri::dot3(d, d) <= prm.max_d2;
            }
            if constexpr (kG == kWave) cnt += __popcll(__ballot(in));
            else cnt += in ? 1 : 0;
        }
    }
    if (active && lg == 0) count[h] = cnt;
}

constexpr int kRansacStages = 3;
const char* const kRansacStageNames[kRansacStages] = {"gather", "filter", "count"};
thread_local sgos::StageTimes<kRansacStages> t_ransac;
thread_local int t_ransac_lanes = kWave;

template <int CT>
void launch_feature_nearest(const float* a, const float* b, int U, int N, int C, int64_t* idx, float* d2, hipStream_t st) {
    const int tiles = sg::cdiv(N, kFnTile);
    const int segments = std::min(tiles, std::max(1, kFnWaves / sg::cdiv(U, kWave)));
    const int seg_rows = sg::cdiv(tiles, segments) * kFnTile;           // whole tiles; the last segment may be short
    unsigned long long* key = reinterpret_cast<unsigned long long*>(idx);
    k_fn_init<<<sg::cdiv(U, kBlock), kBlock, 0, st>>>(key, U);
    k_feature_nearest<CT><<<dim3(sg::cdiv(U, kFnBlock), sg::cdiv(N, seg_rows)), kFnBlock, 0, st>>>(a, b, U, N, C, seg_rows, key);
    k_fn_finish<<<sg::cdiv(U, kBlock), kBlock, 0, st>>>(idx, d2, U);
}

}  // namespace

extern "C" {

size_t sg_fpfh_ws_bytes(int N) { return (N < 0 || N > SG_MAX_GRID_POINTS) ? 0 : sg::align_up(sizeof(Flags)); }

int sg_fpfh(const float* d_xyz, int stride, int N, const float* d_normals, const int64_t* d_off, const int32_t* d_idx, int32_t* d_spfh,
            float* d_fpfh, void* d_ws, size_t ws_bytes, void* stream) {
    const char* who = "sg_fpfh";
    SG_REQUIRE(N >= 0 && stride >= 3, "%s: bad arguments (%d points, rows of %d floats)", who, N, stride);
    if (N > SG_MAX_GRID_POINTS) return sg::fail(SG_EUNSUP, "%s: %d points; a call takes at most %d", who, N, SG_MAX_GRID_POINTS);
    if (N == 0) return SG_OK;
    SG_REQUIRE(d_xyz && d_normals && d_off && d_spfh && d_fpfh && d_ws, "%s: bad arguments", who);
    SG_REQUIRE(ws_bytes >= sg_fpfh_ws_bytes(N), "%s: workspace too small (%zu < %zu)", who, ws_bytes, sg_fpfh_ws_bytes(N));
    Flags* fl = (Flags*)d_ws;
    hipStream_t st = sg::as_stream(stream);
    SG_HIP(hipMemsetAsync(fl, 0, sizeof(Flags), st));
    const int blocks = sg::cdiv(N, kWaves);
    k_spfh<<<blocks, kBlock, 0, st>>>(d_xyz, stride, d_normals, N, d_off, d_idx, d_spfh, &fl->flag);
    k_fpfh<<<blocks, kBlock, 0, st>>>(d_xyz, stride, N, d_off, d_idx, d_spfh, d_fpfh, &fl->flag);
    Flags land{};
    SG_HIP(hipMemcpyAsync(&land, fl, sizeof(Flags), hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    SG_LAUNCH_CHECK();
    if (land.flag & 8) return sg::fail(SG_EINVAL, "%s: the offsets of the rows do not ascend from 0 to off[N]", who);
    if (land.flag & 4) return sg::fail(SG_EINVAL, "%s: a row names a point outside 0..%d", who, N - 1);
    return SG_OK;
}

int sg_feature_nearest(const float* d_a, int U, const float* d_b, int N, int C, int64_t* d_idx, float* d_d2, void* stream) {
    const char* who = "sg_feature_nearest";
    SG_REQUIRE(U >= 0 && N >= 1 && C >= 1 && C <= 64, "%s: bad arguments (%d queries, %d candidates, %d channels; 1..64 channels)", who, U, N, C);
    if (U > kMaxFeaturePoints || N > kMaxFeaturePoints)
        return sg::fail(SG_EUNSUP, "%s: %d queries against %d candidates; the brute-force search takes at most %d of either -- thin the "
                                   "clouds first (a larger voxel)", who, U, N, kMaxFeaturePoints);
    if (U == 0) return SG_OK;
    SG_REQUIRE(d_a && d_b && d_idx && d_d2, "%s: bad arguments", who);
    hipStream_t st = sg::as_stream(stream);
    if (C <= 4) launch_feature_nearest<4>(d_a, d_b, U, N, C, d_idx, d_d2, st);
    else if (C <= 16) launch_feature_nearest<16>(d_a, d_b, U, N, C, d_idx, d_d2, st);
    else if (C <= 36) launch_feature_nearest<36>(d_a, d_b, U, N, C, d_idx, d_d2, st);
    else launch_feature_nearest<64>(d_a, d_b, U, N, C, d_idx, d_d2, st);
    SG_LAUNCH_CHECK();
    return SG_OK;
}

SG_STAGE_TIMER_API(ransac, t_ransac, kRansacStageNames)

int sg_ransac_set_tuning(int lanes_per_survivor) {
    SG_REQUIRE(lanes_per_survivor == 0 || lanes_per_survivor == 1 || lanes_per_survivor == kWave,
               "sg_ransac_set_tuning: 1 or 64 lanes per survivor (0: the default), not %d", lanes_per_survivor);
    t_ransac_lanes = lanes_per_survivor ? lanes_per_survivor : kWave;
    return SG_OK;
}

size_t sg_ransac_ws_bytes(int C, int H) {
    if (C < 3 || C > kMaxFeaturePoints || H < 0 || H > kMaxHypotheses) return 0;
    return sg::align_up(sizeof(Flags)) + 2 * sg::align_up((size_t)C * 3 * sizeof(float)) + sg::align_up((size_t)std::max(H, 1) * sizeof(int32_t));
}

int sg_ransac_count(const float* d_m, int m_stride, int U, const float* d_f, int f_stride, int N, const int32_t* d_ci, const int32_t* d_cj, int C,
                    int H, uint64_t seed, const int32_t* d_triples, double max_dist, double similarity, double min_edge, int32_t* d_count,
                    int* h_survivors, void* d_ws, size_t ws_bytes, void* stream) {
    const char* who = "sg_ransac_count";
    SG_REQUIRE(U >= 1 && N >= 1 && m_stride >= 3 && f_stride >= 3 && C >= 3 && H >= 0,
               "%s: bad arguments (%d and %d points, %d correspondences (3 at least), %d hypotheses)", who, U, N, C, H);
    if (C > kMaxFeaturePoints || H > kMaxHypotheses)
        return sg::fail(SG_EUNSUP, "%s: %d correspondences, %d hypotheses; a call takes at most %d and %d", who, C, H, kMaxFeaturePoints,
                        kMaxHypotheses);
    SG_REQUIRE(std::isfinite(max_dist) && max_dist > 0.0 && std::isfinite(min_edge) && min_edge > 0.0 && similarity > 0.0 && similarity <= 1.0,
               "%s: max_dist and min_edge must be finite lengths > 0 and similarity in (0, 1] (%g, %g, %g)", who, max_dist, min_edge, similarity);
    if (h_survivors) *h_survivors = 0;
    if (H == 0) return SG_OK;
    SG_REQUIRE(d_m && d_f && d_ci && d_cj && d_count && d_ws, "%s: bad arguments", who);
    const size_t need = sg_ransac_ws_bytes(C, H);
    SG_REQUIRE(ws_bytes >= need, "%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
    sg::Carver cv(d_ws, ws_bytes);
    Flags* fl = cv.take<Flags>(1);
    float* pa = cv.take<float>((size_t)C * 3);
    float* pb = cv.take<float>((size_t)C * 3);
    int32_t* surv = cv.take<int32_t>((size_t)H);
    SG_REQUIRE(cv.ok, "%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
    const RansacParams prm{max_dist * max_dist, similarity, min_edge};
    hipStream_t st = sg::as_stream(stream);
    sgos::StageClock<kRansacStages> clock(st, t_ransac.timing, t_ransac.us);
    SG_HIP(hipMemsetAsync(fl, 0, sizeof(Flags), st));
    k_ransac_gather<<<sg::cdiv(C, kBlock), kBlock, 0, st>>>(d_m, m_stride, U, d_f, f_stride, N, d_ci, d_cj, C, pa, pb, &fl->flag);
    clock.tick();
    k_ransac_filter<<<sg::cdiv(H, kBlock), kBlock, 0, st>>>(pa, pb, C, H, d_triples, (unsigned long long)seed, prm, d_count, surv, fl);
    Flags land{};
    SG_HIP(hipMemcpyAsync(&land, fl, sizeof(Flags), hipMemcpyDeviceToHost, st));
    clock.tick();
    SG_HIP(hipStreamSynchronize(st));
    SG_LAUNCH_CHECK();
    if (land.flag & 1) return sg::fail(SG_EINVAL, "%s: a correspondence outside 0..%d (moving) or 0..%d (fixed)", who, U - 1, N - 1);
    if (land.flag & 2) return sg::fail(SG_EINVAL, "%s: a triple names a correspondence outside 0..%d", who, C - 1);
    if (land.survivors < 0 || land.survivors > H) return sg::fail(SG_EINTERNAL, "%s: %d survivors of %d hypotheses", who, land.survivors, H);
    if (land.survivors > 0) {
        if (t_ransac_lanes == 1)
            k_ransac_count<1><<<sg::cdiv(land.survivors, kBlock), kBlock, 0, st>>>(pa, pb, C, d_triples, (unsigned long long)seed, prm, surv,
                                                                                   land.survivors, d_count);
        else
            k_ransac_count<kWave><<<sg::cdiv(land.survivors, kWaves), kBlock, 0, st>>>(pa, pb, C, d_triples, (unsigned long long)seed, prm, surv,
                                                                                       land.survivors, d_count);
    }
    clock.tick();
    SG_HIP(hipStreamSynchronize(st));
    SG_LAUNCH_CHECK();
    if (h_survivors) *h_survivors = land.survivors;
    return SG_OK;
}

}  // extern "C"
