// 2D label images onto a scan's vertices, device side: every vertex is projected into every view by sg_render's own rule
// (render_project_device.h), tested against the view's depth image, and votes with the label under it; then a vote per vertex.
//
//   k_lift_pairs   one thread a (view, vertex), vertex fastest: the camera is wave-uniform, the coordinates coalesce.  It projects, tests
//                  and adds in one pass -- no projected record is written --: d_seen[v] += 1 and d_counts[v*C + l] += 1 through integer
//                  atomics (a vertex meets itself in another view's workgroup), the seven counts through one ballot and one atomic a wave.
//                  A label >= C raises the flag word and adds nothing.
//   k_lift_vote    one wave a vertex: lanes stride over the row's C counts (coalesced for any C), a lane keeps its best as one 64-bit key
//                  (count << 32 | ~class), the wave's maximum is the most votes and at a tie the lowest class; a wave sum is the total; a
//                  second pass over the row (it is in cache) counts the classes that hold as many.
//
// Every loop has a bound (cdiv(C, 64)); no cooperative launch, no device-wide barrier.  Double arithmetic with nothing contracted; the only
// atomics are integer ones, so the same bytes come back under any schedule.  sg_lift synchronises once, at its end, which also brings the
// flag word and the seven counts; sg_lift_vote does not synchronise.
#include <cmath>

#include "sg_common.h"
#include "render_project_device.h"
#include "wave_ops.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWave = 64;
constexpr long long kMaxPixels = 1ll << 26;
constexpr long long kMaxCells = 1ll << 31;     // V * C
constexpr int kMaxViews = 64, kMaxSide = 4096, kMaxClasses = 4096;
enum { mFlag = 0, mBehind = 1, mFar = 2, mOutside = 3, mNoDepth = 4, mOccluded = 5, mVisible = 6, mLabelled = 7, kMisc = 8 };
constexpr int kStats = 7;

typedef unsigned long long u64;
typedef unsigned int u32;

struct Frame {
    int W, H, ortho, C;
    double near, tol;
};

__device__ __forceinline__ void count_wave(bool mine, u64* counter) {
    const int n = __popcll(__ballot(mine));
    if (n && threadIdx.x % kWave == 0) atomicAdd(counter, (u64)n);
}

__global__ __launch_bounds__(kBlock) void k_lift_pairs(const float* __restrict__ xyz, int stride, int V, const double* __restrict__ cam, Frame fr,
                                                       const int32_t* __restrict__ label, const float* __restrict__ depth,
                                                       u32* __restrict__ counts, int32_t* __restrict__ seen, u64* __restrict__ misc) {
    const int v = blockIdx.x * kBlock + threadIdx.x;
    const int b = blockIdx.y;
    bool behind = false, far = false, outside = false, nodepth = false, occluded = false, visible = false, labelled = false;
    if (v < V) {
        int X = 0, Y = 0;
        double c2 = 0.0;
        const int code = sgrd::project(xyz + (size_t)v * stride, cam + (size_t)b * sgrd::kCamDoubles, fr.ortho, fr.near, X, Y, c2);
        behind = code == sgrd::kBehind;
        far = code == sgrd::kFar;
        if (code == sgrd::kInView) {
            const int px = X >> 8, py = Y >> 8;              // the pixel a splat of size 1 lands on
            if ((unsigned)px >= (unsigned)fr.W || (unsigned)py >= (unsigned)fr.H) {
                outside = true;
            } else {
                const size_t at = ((size_t)b * fr.H + py) * fr.W + px;       // inside the image: below B * H * W
                const float d = depth[at];
                if (!(sgos::finite_f32(d) && d > 0.0f)) {
                    nodepth = true;
                } else if (fabs(c2 - (double)d) > fr.tol) {
                    occluded = true;
                } else {
                    const int l = label[at];
                    if (l >= fr.C) {
                        atomicOr(&misc[mFlag], 1ull);        // refused: the pair adds nothing, and nothing is indexed by l
                    } else {
                        atomicAdd(&seen[v], 1);
                        labelled = l >= 0;
                        visible = !labelled;                 // the seven counts are disjoint: visible here is "seen, no vote"
                        if (labelled) atomicAdd(&counts[(size_t)v * fr.C + l], 1u);
                    }
                }
            }
        }
    }
    count_wave(behind, &misc[mBehind]);
    count_wave(far, &misc[mFar]);
    count_wave(outside, &misc[mOutside]);
    count_wave(nodepth, &misc[mNoDepth]);
    count_wave(occluded, &misc[mOccluded]);
    count_wave(visible, &misc[mVisible]);
    count_wave(labelled, &misc[mLabelled]);
}

// the wave's reductions on the DPP network of wave_ops.h, for the two types it has no entry for
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ u64 dpp_u64(u64 old, u64 v) {
    const int lo = sgw::dpp_i<CTRL, ROW_MASK>((int)(u32)old, (int)(u32)v);
    const int hi = sgw::dpp_i<CTRL, ROW_MASK>((int)(u32)(old >> 32), (int)(u32)(v >> 32));
    return ((u64)(u32)hi << 32) | (u32)lo;
}
__device__ __forceinline__ u64 op_maxu64(u64 a, u64 b) { return a > b ? a : b; }
__device__ __forceinline__ int op_addi(int a, int b) { return a + b; }

__device__ __forceinline__ u64 wave_max_u64(u64 v) {
    using namespace sgw;
    SGW_REDUCE(u64, dpp_u64, v, op_maxu64, v);
    const int lo = __builtin_amdgcn_readlane((int)(u32)v, 63), hi = __builtin_amdgcn_readlane((int)(u32)(v >> 32), 63);
    return ((u64)(u32)hi << 32) | (u32)lo;
}
__device__ __forceinline__ int wave_sum_i(int v) {
    using namespace sgw;
    SGW_REDUCE(int, dpp_i, v, op_addi, 0);
    return __builtin_amdgcn_readlane(v, 63);
}

__global__ __launch_bounds__(kBlock) void k_lift_vote(const u32* __restrict__ counts, int V, int C, int32_t* __restrict__ winner, int32_t* __restrict__ votes,
                                                      int32_t* __restrict__ total, int32_t* __restrict__ tied) {
    const int lane = threadIdx.x % kWave;
    const long long v = (long long)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
    if (v >= V) return;                                      // the whole wave: the reductions below run with all 64 lanes
    const u32* row = counts + (size_t)v * C;
    u64 best = 0;                                            // no class: below every key of a class (~c != 0 for c < 2^32 - 1)
    int sum = 0;
    for (int c = lane; c < C; c += kWave) {                  // at most cdiv(C, 64) <= 64 rounds
        const u32 n = row[c];
        const u64 key = ((u64)n << 32) | (u32)~(u32)c;
        best = key > best ? key : best;
        sum += (int)n;
    }
    best = wave_max_u64(best);
    sum = wave_sum_i(sum);
    const u32 most = (u32)(best >> 32);
    int same = 0;
    if (most) {                                              // wave-uniform
        for (int c = lane; c < C; c += kWave) same += row[c] == most;
    }
    same = wave_sum_i(same);
    if (lane == 0) {
        winner[v] = most ? (int32_t)~(u32)best : -1;
        votes[v] = (int32_t)most;
        total[v] = sum;
        tied[v] = same > 1;
    }
}

bool sizes_ok(int V, int B) { return V >= 1 && V <= SG_MAX_CLOUD_POINTS && B >= 1 && B <= kMaxViews; }

// counters | cameras
size_t need_bytes(int B) { return sg::align_up(kMisc * sizeof(u64)) + sg::align_up((size_t)B * sgrd::kCamDoubles * sizeof(double)); }

thread_local int64_t t_stats[kStats] = {0, 0, 0, 0, 0, 0, 0};

}  // namespace

extern "C" {

size_t sg_lift_ws_bytes(int V, int B) { return sizes_ok(V, B) ? need_bytes(B) : 0; }

int sg_lift_stats(int64_t* h, int cap) {
    SG_REQUIRE(h && cap >= kStats, "sg_lift_stats: room for %d values is needed (%d at %p)", kStats, cap, (const void*)h);
    for (int i = 0; i < kStats; ++i) h[i] = t_stats[i];
    return kStats;
}

int sg_lift(const float* d_xyz, int stride, int V, int B, const double* h_cam, int ortho, double near, int W, int H, const int32_t* d_label,
            const float* d_depth, double tol, int C, uint32_t* d_counts, int32_t* d_seen, void* d_ws, size_t ws_bytes, void* stream) {
    const char* who = "sg_lift";
    SG_REQUIRE(V >= 1 && B >= 1 && W >= 1 && H >= 1 && C >= 1, "%s: %d vertices, %d views of %d x %d pixels, %d classes; each is at least 1", who, V, B, W, H, C);
    if (V > SG_MAX_CLOUD_POINTS) return sg::fail(SG_EUNSUP, "%s: %d vertices; a scan holds at most %d", who, V, SG_MAX_CLOUD_POINTS);
    if (B > kMaxViews || W > kMaxSide || H > kMaxSide || (long long)B * H * W > kMaxPixels)
        return sg::fail(SG_EUNSUP, "%s: %d views of %d x %d pixels; a call takes at most %d views, sides of %d and 2^26 pixels in all", who, B, W, H, kMaxViews,
                        kMaxSide);
    if (C > kMaxClasses || (long long)V * C > kMaxCells)
        return sg::fail(SG_EUNSUP, "%s: %d classes over %d vertices; a call takes at most %d classes and 2^31 counts in all", who, C, V, kMaxClasses);
    SG_REQUIRE(d_xyz && h_cam && d_label && d_depth && d_counts && d_seen && d_ws, "%s: a null pointer", who);
    SG_REQUIRE(stride >= 3, "%s: rows of %d floats; a point is at least 3", who, stride);
    SG_REQUIRE(std::isfinite(near) && near > 0.0, "%s: near must be finite and > 0 (%g)", who, near);
    SG_REQUIRE(std::isfinite(tol) && tol >= 0.0, "%s: tol must be finite and >= 0 (%g)", who, tol);
    for (int b = 0; b < B; ++b) {
        const double* c = h_cam + (size_t)b * sgrd::kCamDoubles;
        for (int k = 0; k < sgrd::kCamDoubles; ++k) SG_REQUIRE(std::isfinite(c[k]), "%s: camera %d holds a number that is not finite (entry %d)", who, b, k);
        SG_REQUIRE(c[12] != 0.0 && c[13] != 0.0, "%s: camera %d has fx = %g, fy = %g; neither may be 0", who, b, c[12], c[13]);
    }
    const size_t need = need_bytes(B);
    SG_REQUIRE(ws_bytes >= need, "%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
    sg::Carver cv(d_ws, ws_bytes);
    u64* misc = cv.take<u64>(kMisc);
    double* cam = cv.take<double>((size_t)B * sgrd::kCamDoubles);
    SG_REQUIRE(cv.ok, "%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
    for (int i = 0; i < kStats; ++i) t_stats[i] = 0;

    hipStream_t st = sg::as_stream(stream);
    const Frame fr{W, H, ortho ? 1 : 0, C, near, tol};
    SG_HIP(hipMemsetAsync(misc, 0, kMisc * sizeof(u64), st));
    SG_HIP(hipMemcpyAsync(cam, h_cam, (size_t)B * sgrd::kCamDoubles * sizeof(double), hipMemcpyHostToDevice, st));
    k_lift_pairs<<<dim3(sg::cdiv(V, kBlock), B), kBlock, 0, st>>>(d_xyz, stride, V, cam, fr, d_label, d_depth, d_counts, d_seen, misc);
    SG_LAUNCH_CHECK();
    u64 land[kMisc] = {0};
    SG_HIP(hipMemcpyAsync(land, misc, sizeof(land), hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    SG_LAUNCH_CHECK();
    if (land[mFlag]) return sg::fail(SG_EINVAL, "%s: a visible pixel's label is outside the %d classes (labels are < C; negative is no label)", who, C);
    for (int i = 0; i < kStats; ++i) t_stats[i] = (int64_t)land[mBehind + i];
    return SG_OK;
}

int sg_lift_vote(const uint32_t* d_counts, int V, int C, int32_t* d_winner, int32_t* d_votes, int32_t* d_total, int32_t* d_tied, void* stream) {
    const char* who = "sg_lift_vote";
    SG_REQUIRE(V >= 1 && C >= 1, "%s: %d vertices, %d classes; each is at least 1", who, V, C);
    if (V > SG_MAX_CLOUD_POINTS) return sg::fail(SG_EUNSUP, "%s: %d vertices; a scan holds at most %d", who, V, SG_MAX_CLOUD_POINTS);
    if (C > kMaxClasses || (long long)V * C > kMaxCells)
        return sg::fail(SG_EUNSUP, "%s: %d classes over %d vertices; a call takes at most %d classes and 2^31 counts in all", who, C, V, kMaxClasses);
    SG_REQUIRE(d_counts && d_winner && d_votes && d_total && d_tied, "%s: a null pointer", who);
    k_lift_vote<<<sg::cdiv(V, kBlock / kWave), kBlock, 0, sg::as_stream(stream)>>>(d_counts, V, C, d_winner, d_votes, d_total, d_tied);
    SG_LAUNCH_CHECK();
    return SG_OK;
}

}  // extern "C"
