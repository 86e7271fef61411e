// Which boxes hold a point, device side: the way back from the boxes of kernels_boxes.hip / kernels_boxiou.hip to the points.
// A box is 15 doubles, cx cy cz sx sy sz r00 .. r22 (the rows of R are its axes); include/seggroup_hip.h spells the test of one point
// against one box out, and holds() below follows it statement by statement.
//
//   k_pb_prepare       one thread a box: the 16 doubles the test reads (c | h = 0.5*s + margin | R | vol), and the flag bits of a value that
//                      is not finite, a negative size, a frame that is not orthonormal to 1e-6
//   k_pb_test<HELD>    one workgroup of 256 threads takes up to 256 consecutive points of ONE scene; the host's workgroup table (one int4 a
//                      workgroup: first point, points, first box, end of the boxes) says which.  The scene's prepared boxes go through LDS in
//                      tiles of 128 (16 KiB); every lane reads the same box (a broadcast), its point stays in registers, boxes are visited in
//                      ascending index.  HELD adds the per-box counts: a ballot per box and wave, integer adds into 128 LDS words, one
//                      integer add per workgroup and box that holds something into d_held.
// Double arithmetic, nothing contracted (-ffp-contract=off), no floating-point atomics.  The table and the flag word are ONE upload: entry 0
// of the table is the flag word's landing, uploaded as zeros.
#include <cmath>
#include <vector>

#include "sg_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWave = 64;
constexpr int kTile = 128;                    // boxes in LDS at a time
constexpr int kPrep = 16;                     // doubles of a prepared box
constexpr int kMaxPoints = 1 << 24;
constexpr int kBoxNotFinite = 1, kNegative = 2, kNotFrame = 4, kPointNotFinite = 8;
constexpr double kFrameTol = 1e-6;

__device__ __forceinline__ double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

__global__ __launch_bounds__(kBlock) void k_pb_prepare(const double* __restrict__ box, int K, double margin, double* __restrict__ prep,
                                                       int* __restrict__ flag) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= K) return;
    double v[15];
    int bad = 0;
#pragma unroll
    for (int r = 0; r < 15; ++r) {
        v[r] = box[(size_t)i * 15 + r];
        if (!sg::finite_f64(v[r])) bad = kBoxNotFinite;
    }
    if (!bad) {
        if (v[3] < 0.0 || v[4] < 0.0 || v[5] < 0.0) bad |= kNegative;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (fabs(dot3(v + 6 + 3 * a, v + 6 + 3 * a) - 1.0) > kFrameTol) bad |= kNotFrame;
#pragma unroll
            for (int b = a + 1; b < 3; ++b)
                if (fabs(dot3(v + 6 + 3 * a, v + 6 + 3 * b)) > kFrameTol) bad |= kNotFrame;
        }
    }
    double* o = prep + (size_t)i * kPrep;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        o[a] = v[a];
        o[3 + a] = 0.5 * v[3 + a] + margin;
    }
#pragma unroll
    for (int r = 0; r < 9; ++r) o[6 + r] = v[6 + r];
    o[15] = (v[3] * v[4]) * v[5];
    if (bad) atomicOr(flag, bad);
}

// include/seggroup_hip.h, statement by statement: b = c (3) | h (3) | R (9) | vol
__device__ __forceinline__ bool holds(const double* b, double x, double y, double z) {
    const double d0 = x - b[0], d1 = y - b[1], d2 = z - b[2];
    bool in = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double l = (b[6 + 3 * k] * d0 + b[7 + 3 * k] * d1) + b[8 + 3 * k] * d2;
        in = in && fabs(l) <= b[3 + k];
    }
    return in;
}

template <bool HELD>
__global__ __launch_bounds__(kBlock) void k_pb_test(const float* __restrict__ xyz, int stride, const int4* __restrict__ table,
                                                    const double* __restrict__ prep, int32_t* __restrict__ count, int32_t* __restrict__ first,
                                                    int32_t* __restrict__ inner, int32_t* __restrict__ held, int* __restrict__ flag) {
    __shared__ double tile[kTile * kPrep];
    __shared__ int tile_held[HELD ? kTile : 1];
    const int4 job = table[1 + blockIdx.x];                // x: first point, y: points (1..256), z: first box, w: end of the scene's boxes
    const int t = threadIdx.x;
    const bool live = t < job.y;
    const int p = job.x + t;                                // < N where live: the host laid the table out from checked offsets
    double x = 0.0, y = 0.0, z = 0.0;
    if (live && job.w > job.z) {
        const float* q = xyz + (size_t)p * stride;
        const float fx = q[0], fy = q[1], fz = q[2];
        if (!(sg::finite_f32(fx) && sg::finite_f32(fy) && sg::finite_f32(fz))) atomicOr(flag, kPointNotFinite);
        x = (double)fx;
        y = (double)fy;
        z = (double)fz;
    }
    int n = 0, lowest = -1, best = -1;
    double best_vol = 0.0;
    for (int at = job.z; at < job.w; at += kTile) {        // uniform over the workgroup
        const int nb = min(kTile, job.w - at);
        const double* src = prep + (size_t)at * kPrep;
        for (int i = t; i < nb * kPrep; i += kBlock) tile[i] = src[i];
        if (HELD && t < kTile) tile_held[t] = 0;
        __syncthreads();
        for (int j = 0; j < nb; ++j) {
            const double* b = tile + j * kPrep;             // the same address in every lane
            const bool in = live && holds(b, x, y, z);
            if (in) {
                const double vol = b[15];
                ++n;
                if (lowest < 0) lowest = at - job.z + j;
                if (best < 0 || vol < best_vol) { best = at - job.z + j; best_vol = vol; }   // ascending j: the lowest among equal volumes stays
            }
            if (HELD) {
                const unsigned long long m = __ballot(in);
                if (m && t % kWave == 0) atomicAdd(&tile_held[j], __popcll(m));
            }
        }
        __syncthreads();                                    // the tile is read (and its counts are whole) before it is replaced
        if (HELD && t < nb && tile_held[t]) atomicAdd(&held[at + t], tile_held[t]);     // thread t alone zeroes word t for the next tile
    }
    if (live) {
        count[p] = n;
        first[p] = lowest;
        inner[p] = best;
    }
}

bool sizes_ok(int N, int K, int B) { return N >= 0 && N <= kMaxPoints && K >= 0 && K <= sg::kMaxBoxes && B >= 0 && B <= sg::kMaxScenes; }

// entry 0 is the flag word's landing; a scene of n points has cdiv(n, 256) workgroups, so there are at most cdiv(N, 256) + B of them
size_t table_entries(int N, int B) { return 1 + (size_t)sg::cdiv(N, kBlock) + (size_t)B; }
size_t need_bytes(int N, int K, int B) { return sg::align_up(table_entries(N, B) * sizeof(int4)) + sg::align_up((size_t)std::max(K, 1) * kPrep * sizeof(double)); }

}  // namespace

extern "C" {

size_t sg_points_in_boxes_ws_bytes(int N, int K, int B) { return sizes_ok(N, K, B) ? need_bytes(N, K, B) : 0; }

int sg_points_in_boxes(const float* d_xyz, int stride, int N, const double* d_box, int K, const int32_t* h_off_p, const int32_t* h_off_b, int B,
                       double margin, int32_t* d_count, int32_t* d_first, int32_t* d_inner, int32_t* d_held, void* d_ws, size_t ws_bytes,
                       void* stream) {
    const char* who = "sg_points_in_boxes";
    SG_REQUIRE(N >= 0 && K >= 0 && B >= 0 && stride >= 3 && h_off_p && h_off_b, "%s: bad arguments (%d points of stride %d, %d boxes, %d scenes)",
               who, N, stride, K, B);
    SG_REQUIRE(margin >= 0.0 && std::isfinite(margin), "%s: the margin is negative or not finite (%g)", who, margin);
    if (!sizes_ok(N, K, B))
        return sg::fail(SG_EUNSUP, "%s: %d points and %d boxes in %d scenes; a call takes at most 2^24 points, 2^20 boxes and 2^16 scenes", who, N, K, B);
    if (int rc = sg::check_offsets(who, "the points", h_off_p, B, N)) return rc;
    if (int rc = sg::check_offsets(who, "the boxes", h_off_b, B, K)) return rc;
    SG_REQUIRE((d_xyz && d_count && d_first && d_inner) || !N, "%s: bad arguments (a null pointer)", who);
    SG_REQUIRE((d_box || !K) && d_ws, "%s: bad arguments (a null pointer)", who);
    const size_t need = need_bytes(N, K, B);
    SG_REQUIRE(ws_bytes >= need, "%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
    hipStream_t st = sg::as_stream(stream);
    if (d_held && K) SG_HIP(hipMemsetAsync(d_held, 0, (size_t)K * sizeof(int32_t), st));
    if (!N) {
        if (d_held && K) SG_HIP(hipStreamSynchronize(st));
        return SG_OK;
    }
    sg::Carver cv(d_ws, ws_bytes);
    int4* table = cv.take<int4>(table_entries(N, B));
    double* prep = cv.take<double>((size_t)std::max(K, 1) * kPrep);
    SG_REQUIRE(cv.ok, "%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
    std::vector<int4> host(1, make_int4(0, 0, 0, 0));       // alive until the call has synchronised
    host.reserve(table_entries(N, B));
    for (int s = 0; s < B; ++s)
        for (int at = h_off_p[s]; at < h_off_p[s + 1]; at += kBlock)
            host.push_back(make_int4(at, std::min(kBlock, h_off_p[s + 1] - at), h_off_b[s], h_off_b[s + 1]));
    const int groups = (int)host.size() - 1;                 // >= 1: N > 0 and the offsets end at N
    SG_HIP(hipMemcpyAsync(table, host.data(), host.size() * sizeof(int4), hipMemcpyHostToDevice, st));
    int* flag = &table->x;
    if (K) k_pb_prepare<<<sg::cdiv(K, kBlock), kBlock, 0, st>>>(d_box, K, margin, prep, flag);
    if (d_held && K)
        k_pb_test<true><<<groups, kBlock, 0, st>>>(d_xyz, stride, table, prep, d_count, d_first, d_inner, d_held, flag);
    else
        k_pb_test<false><<<groups, kBlock, 0, st>>>(d_xyz, stride, table, prep, d_count, d_first, d_inner, nullptr, flag);
    int4 land = make_int4(0, 0, 0, 0);
    const hipError_t copied = hipMemcpyAsync(&land, table, sizeof(int4), hipMemcpyDeviceToHost, st);
    SG_HIP(hipStreamSynchronize(st));                                            // whatever the copy said: the upload out of `host` ends here
    SG_HIP(copied);
    SG_LAUNCH_CHECK();
    if (land.x & kPointNotFinite) return sg::fail(SG_EINVAL, "%s: a point of a scene that has boxes has a coordinate that is not finite", who);
    if (land.x & kBoxNotFinite) return sg::fail(SG_EINVAL, "%s: a box has a value that is not finite", who);
    if (land.x & kNegative) return sg::fail(SG_EINVAL, "%s: a box has a negative size", who);
    if (land.x & kNotFrame)
        return sg::fail(SG_EINVAL, "%s: a box has a frame that is not orthonormal: |r.r - 1| or |r_i.r_j| > 1e-6 for rows of R", who);
    return SG_OK;
}

}  // extern "C"
