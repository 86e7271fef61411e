// Scans and their labels as images, device side: a z-buffer rasteriser of triangles and point splats by THE RULE of
// include/seggroup_hip.h.  Screen coordinates are fixed point (1/256 pixel), coverage is three int64 edge functions, a pixel keeps the
// minimum of a 64-bit key (float depth bits << 32 | primitive index) through an integer atomic minimum: one answer whatever the schedule.
//
//   k_rd_project   one thread a (view, vertex): camera space in double, the reject code, X, Y (fixed point) and z -> one 16-byte record
//   k_rd_prims     one thread a (view, primitive): refused through the flag word (a face index outside 0..V-1: dropped, never used as an
//                  index), dropped and counted (behind, far, degenerate), or kept.  The box of the pixel centres inside the corners' bounding
//                  box is clipped to the image; a box of at most `small` x `small` pixels is walked by the thread itself (edge functions
//                  stepped incrementally: integers, so exact), a larger one goes to the call's queue through an atomic cursor.  The
//                  queue's order varies from run to run; a minimum does not depend on it.  A splat is never large (15 x 15 at most).
//   k_rd_large     a fixed grid of workgroups strides over the queue; a workgroup walks its primitive's box in tiles of 16 x 16 pixels, a
//                  thread a pixel; a tile that lies wholly outside one edge is skipped (the edge function at the tile's best corner).
//   k_rd_resolve   one thread a pixel: the key decoded, the winner's three edge functions recomputed for `vert`, the outputs written with
//                  plain stores, `hits` and the covered pixels counted with integer atomic adds.
//   k_rd_colour    sg_render_colour: one thread a pixel, three bytes.
//
// Every loop has a bound (a box holds at most W * H pixels, the queue at most B * F entries); no cooperative launch, no device-wide
// barrier, no workgroup waits for another.  Double arithmetic with nothing contracted; the only atomics are integer ones.  One stream
// synchronisation per call, at its end, which also brings the flag word and the six counts.
#include <atomic>
#include <cmath>

#include "sg_common.h"
#include "box_iou_device.h"
#include "overseg_device.h"
#include "palette_device.h"
#include "render_project_device.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWave = 64;
constexpr int kTileSide = 16;                  // k_rd_large: a workgroup's tile is 16 x 16 pixels, a thread a pixel
constexpr int kSmall = 8;                      // a clipped box of at most kSmall x kSmall pixels is rasterised by its own thread.  MEASURED (tools/
                                               // time_render.py, profiles/render_time.json): 8 beat 16 and 32 on every mesh with faces
                                               // of more than 8 pixels a side (up to 3.4 times), and a ScanNet-sized mesh has none, so all time alike
constexpr int kSmallMax = 32;                  // sg_render_set_tuning's largest: the thread's loop stays below 1,024 pixels
constexpr int kLargeGrid = 2048;               // workgroups of k_rd_large: 256 CUs x 8, striding over the queue
constexpr long long kMaxFaces = 1ll << 26;
constexpr long long kMaxPixels = 1ll << 26;
constexpr int kMaxViews = 64, kMaxSide = 4096, kMaxPointSize = 15;
constexpr int kPrimBits = 26;                  // a queue entry: view << 26 | face (F <= 2^26, B <= 64)
enum { mFlag = 0, mCursor = 1, mKept = 2, mBehind = 3, mFar = 4, mDegenerate = 5, mLarge = 6, mCovered = 7, kMisc = 8 };
constexpr int kCamDoubles = sgrd::kCamDoubles;

typedef unsigned long long u64;
typedef unsigned int u32;
constexpr u64 kEmpty = ~0ull;

struct __align__(16) Proj {                    // z > 0: in view; z == 0: behind; z < 0: far
    int X, Y;
    double z;
};

struct View {
    int W, H, ortho;
    double near;
};

__global__ __launch_bounds__(kBlock) void k_rd_project(const float* __restrict__ xyz, int stride, int V, const double* __restrict__ cam, View vw,
                                                       Proj* __restrict__ proj) {
    const int v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= V) return;
    const int b = blockIdx.y;
    const double* c = cam + (size_t)b * kCamDoubles;
    const float* p = xyz + (size_t)v * stride;
    Proj out{0, 0, 0.0};
    if (sgrd::project(p, c, vw.ortho, vw.near, out.X, out.Y, out.z) == sgrd::kFar) out.z = -1.0;      // the rule itself: render_project_device.h
    proj[(size_t)b * V + v] = out;
}

// A kept triangle over the pixel grid: the three edge functions at the centre of pixel (x0, y0) of its clipped box, their steps a pixel
// to the right and a pixel down, all with A > 0 (negated where the corners came clockwise), and the per-corner depth factor.
struct Tri {
    long long w[3], sx[3], sy[3], A;
    double q[3];                                 // 1 / z_i (perspective) or z_i (orthographic)
    int x0, y0, x1, y1;                          // the clipped box, inclusive; empty iff x0 > x1 or y0 > y1
};

// -> false iff A == 0 (degenerate)
__device__ __forceinline__ bool tri_setup(const Proj& a, const Proj& b, const Proj& c, const View& vw, Tri& t) {
    const long long X[3] = {a.X, b.X, c.X}, Y[3] = {a.Y, b.Y, c.Y};
    const long long A = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0]);
    if (A == 0) return false;
    const long long sgn = A < 0 ? -1 : 1;
    t.A = sgn * A;
    const int xmin = min(a.X, min(b.X, c.X)), xmax = max(a.X, max(b.X, c.X));
    const int ymin = min(a.Y, min(b.Y, c.Y)), ymax = max(a.Y, max(b.Y, c.Y));
    t.x0 = max((xmin + 127) >> 8, 0);            // the first centre 256 px + 128 >= xmin
    t.x1 = min((xmax - 128) >> 8, vw.W - 1);     // the last centre <= xmax
    t.y0 = max((ymin + 127) >> 8, 0);
    t.y1 = min((ymax - 128) >> 8, vw.H - 1);
    const long long px = 256ll * t.x0 + 128, py = 256ll * t.y0 + 128;
#pragma unroll
    for (int i = 0; i < 3; ++i) {                // w_i: the edge from corner i+1 to corner i+2, opposite corner i
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        const long long ex = X[k] - X[j], ey = Y[k] - Y[j];
        t.w[i] = sgn * (ex * (py - Y[j]) - ey * (px - X[j]));
        t.sx[i] = -sgn * ey * 256;
        t.sy[i] = sgn * ex * 256;
    }
    t.q[0] = vw.ortho ? a.z : 1.0 / a.z;
    t.q[1] = vw.ortho ? b.z : 1.0 / b.z;
    t.q[2] = vw.ortho ? c.z : 1.0 / c.z;
    return true;
}

__device__ __forceinline__ u64 depth_key(const Tri& t, long long w0, long long w1, long long w2, int ortho, u32 prim) {
    const double s = ((double)w0 * t.q[0] + (double)w1 * t.q[1]) + (double)w2 * t.q[2];
    const double r = s / (double)t.A;
    const float depth = (float)(ortho ? r : 1.0 / r);
    return ((u64)__float_as_uint(depth) << 32) | prim;
}

__device__ __forceinline__ void keep_min(u64* slot, u64 key) {
    if (key < *slot) atomicMin(slot, key);       // the slot only falls: a stale read can only cost an atomic, never lose a key
}

__device__ __forceinline__ void count_wave(bool mine, u64* counter) {
    const int n = __popcll(__ballot(mine));
    if (n && threadIdx.x % kWave == 0) atomicAdd(counter, (u64)n);
}

// faces: corners a, b, c of face p in view b, or false with the flag raised (an index outside 0..V-1: nothing is read through it)
__device__ __forceinline__ bool face_corners(const int32_t* __restrict__ faces, long long p, int V, const Proj* __restrict__ proj, int i[3], Proj c[3]) {
    i[0] = faces[3 * p], i[1] = faces[3 * p + 1], i[2] = faces[3 * p + 2];
    if ((unsigned)i[0] >= (unsigned)V || (unsigned)i[1] >= (unsigned)V || (unsigned)i[2] >= (unsigned)V) return false;
    c[0] = proj[i[0]], c[1] = proj[i[1]], c[2] = proj[i[2]];
    return true;
}

template <bool kFaces>
__global__ __launch_bounds__(kBlock) void k_rd_prims(const int32_t* __restrict__ faces, long long P, int V, const Proj* __restrict__ proj, View vw,
                                                     int point_size, int small, u64* __restrict__ keys, u32* __restrict__ queue,
                                                     u64* __restrict__ misc) {
    const long long p = (long long)blockIdx.x * kBlock + threadIdx.x;
    const int b = blockIdx.y;
    const Proj* pv = proj + (size_t)b * V;
    u64* img = keys + (size_t)b * vw.H * vw.W;
    bool behind = false, far = false, degenerate = false, kept = false, large = false;
    if (p < P) {
        if constexpr (kFaces) {
            int idx[3];
            Proj c[3];
            if (!face_corners(faces, p, V, pv, idx, c)) {
                atomicOr(&misc[mFlag], 1ull);
            } else {
                behind = c[0].z == 0.0 || c[1].z == 0.0 || c[2].z == 0.0;
                far = !behind && (c[0].z < 0.0 || c[1].z < 0.0 || c[2].z < 0.0);
                Tri t;
                if (!behind && !far) {
                    kept = tri_setup(c[0], c[1], c[2], vw, t);
                    degenerate = !kept;
                }
                if (kept && t.x0 <= t.x1 && t.y0 <= t.y1) {
                    const int bw = t.x1 - t.x0 + 1, bh = t.y1 - t.y0 + 1;
                    large = bw > small || bh > small;
                    if (large) {
                        queue[atomicAdd(&misc[mCursor], 1ull)] = ((u32)b << kPrimBits) | (u32)p;      // at most B * F entries: the queue's size
                    } else {
                        for (int y = 0; y < bh; ++y) {                                              // bh, bw <= small <= 32
                            long long w0 = t.w[0] + y * t.sy[0], w1 = t.w[1] + y * t.sy[1], w2 = t.w[2] + y * t.sy[2];
                            for (int x = 0; x < bw; ++x) {
                                if ((w0 | w1 | w2) >= 0) keep_min(img + (size_t)(t.y0 + y) * vw.W + (t.x0 + x), depth_key(t, w0, w1, w2, vw.ortho, (u32)p));
                                w0 += t.sx[0], w1 += t.sx[1], w2 += t.sx[2];
                            }
                        }
                    }
                }
            }
        } else {
            const Proj c = pv[p];
            behind = c.z == 0.0;
            far = c.z < 0.0;
            kept = !behind && !far;
            if (kept) {
                const int half = point_size >> 1, cx = c.X >> 8, cy = c.Y >> 8;
                const int x0 = max(cx - half, 0), x1 = min(cx + half, vw.W - 1), y0 = max(cy - half, 0), y1 = min(cy + half, vw.H - 1);
                const u64 key = ((u64)__float_as_uint((float)c.z) << 32) | (u32)p;
                for (int y = y0; y <= y1; ++y)                                                      // at most 15 x 15
                    for (int x = x0; x <= x1; ++x) keep_min(img + (size_t)y * vw.W + x, key);
            }
        }
    }
    count_wave(kept, &misc[mKept]);
    count_wave(behind, &misc[mBehind]);
    count_wave(far, &misc[mFar]);
    count_wave(degenerate, &misc[mDegenerate]);
    count_wave(large, &misc[mLarge]);
}

__global__ __launch_bounds__(kBlock) void k_rd_large(const int32_t* __restrict__ faces, int V, const Proj* __restrict__ proj, View vw,
                                                     u64* __restrict__ keys, const u32* __restrict__ queue, const u64* __restrict__ misc) {
    const u64 count = misc[mCursor];
    const int tx = threadIdx.x % kTileSide, ty = threadIdx.x / kTileSide;
    for (u64 n = blockIdx.x; n < count; n += gridDim.x) {          // at most B * F entries
        const u32 e = queue[n];
        const int b = (int)(e >> kPrimBits);
        const long long p = e & ((1u << kPrimBits) - 1);
        int idx[3];
        Proj c[3];
        Tri t;
        face_corners(faces, p, V, proj + (size_t)b * V, idx, c);      // queued: the indices were inside, the triangle kept
        tri_setup(c[0], c[1], c[2], vw, t);
        u64* img = keys + (size_t)b * vw.H * vw.W;
        const int bw = t.x1 - t.x0 + 1, bh = t.y1 - t.y0 + 1;
        const int ntx = (bw + kTileSide - 1) / kTileSide, nty = (bh + kTileSide - 1) / kTileSide;
        for (int tile = 0; tile < ntx * nty; ++tile) {             // at most W * H / 256 + W / 16 + H / 16 + 1 tiles
            const int ox = (tile % ntx) * kTileSide, oy = (tile / ntx) * kTileSide;
            bool outside = false;
#pragma unroll
            for (int i = 0; i < 3; ++i) {                          // the edge function at the tile's corner that is best for it
                const long long best = t.w[i] + ox * t.sx[i] + oy * t.sy[i] + max(t.sx[i], 0ll) * (kTileSide - 1) + max(t.sy[i], 0ll) * (kTileSide - 1);
                outside |= best < 0;
            }
            if (outside) continue;                                 // uniform over the workgroup
            const int x = ox + tx, y = oy + ty;
            if (x < bw && y < bh) {
                const long long w0 = t.w[0] + x * t.sx[0] + y * t.sy[0], w1 = t.w[1] + x * t.sx[1] + y * t.sy[1], w2 = t.w[2] + x * t.sx[2] + y * t.sy[2];
                if ((w0 | w1 | w2) >= 0) keep_min(img + (size_t)(t.y0 + y) * vw.W + (t.x0 + x), depth_key(t, w0, w1, w2, vw.ortho, (u32)p));
            }
        }
    }
}

template <bool kFaces>
__global__ __launch_bounds__(kBlock) void k_rd_resolve(const int32_t* __restrict__ faces, int V, const Proj* __restrict__ proj, View vw,
                                                       const u64* __restrict__ keys, long long pixels, int32_t* __restrict__ d_prim,
                                                       float* __restrict__ d_depth, int32_t* __restrict__ d_vert, int32_t* __restrict__ d_hits,
                                                       u64* __restrict__ misc) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    bool covered = false;
    if (i < pixels) {
        const u64 key = keys[i];
        covered = key != kEmpty;
        int prim = -1, vert = -1;
        float depth = INFINITY;
        if (covered) {
            prim = (int)(u32)key;
            depth = __uint_as_float((u32)(key >> 32));
            if constexpr (kFaces) {
                const long long per = (long long)vw.H * vw.W;
                const int b = (int)(i / per);
                const int at = (int)(i - b * per), y = at / vw.W, x = at - y * vw.W;
                int idx[3];
                Proj c[3];
                Tri t;
                face_corners(faces, prim, V, proj + (size_t)b * V, idx, c);       // a winner: the indices were inside, the triangle kept
                tri_setup(c[0], c[1], c[2], vw, t);
                const int dx = x - t.x0, dy = y - t.y0;
                const long long w0 = t.w[0] + dx * t.sx[0] + dy * t.sy[0], w1 = t.w[1] + dx * t.sx[1] + dy * t.sy[1], w2 = t.w[2] + dx * t.sx[2] + dy * t.sy[2];
                vert = w1 > w0 ? (w2 > w1 ? idx[2] : idx[1]) : (w2 > w0 ? idx[2] : idx[0]);      // the largest, a tie to the lower corner
            } else {
                vert = prim;
            }
            if (d_hits) atomicAdd(&d_hits[vert], 1);
        }
        d_prim[i] = prim;
        if (d_depth) d_depth[i] = depth;
        if (d_vert) d_vert[i] = vert;
    }
    count_wave(covered, &misc[mCovered]);
}

struct Rgb { uint8_t c[3]; };

__global__ __launch_bounds__(kBlock) void k_rd_colour(const int32_t* __restrict__ vert, long long n, const uint8_t* __restrict__ cidx,
                                                      const uint8_t* __restrict__ rgb, int V, Rgb background, uint8_t* __restrict__ img) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int v = vert[i];
    Rgb out = background;
    if ((unsigned)v < (unsigned)V) {
        if (cidx) {
            const uint32_t c = sgpal::kPalette[min((int)cidx[v], SG_NUM_COLOURS)];
            out.c[0] = (uint8_t)c, out.c[1] = (uint8_t)(c >> 8), out.c[2] = (uint8_t)(c >> 16);
        } else {
            out.c[0] = rgb[3 * (size_t)v], out.c[1] = rgb[3 * (size_t)v + 1], out.c[2] = rgb[3 * (size_t)v + 2];
        }
    }
    img[3 * i] = out.c[0], img[3 * i + 1] = out.c[1], img[3 * i + 2] = out.c[2];
}

bool sizes_ok(int V, long long P, int B, int W, int H) {
    return V >= 1 && V <= SG_MAX_CLOUD_POINTS && P >= 0 && P <= kMaxFaces && B >= 1 && B <= kMaxViews && W >= 1 && W <= kMaxSide && H >= 1 &&
           H <= kMaxSide && (long long)B * H * W <= kMaxPixels;
}

// counters | cameras | projected vertices | keys | queue
size_t need_bytes(int V, long long P, int B, int W, int H) {
    return sg::align_up(kMisc * sizeof(u64)) + sg::align_up((size_t)B * kCamDoubles * sizeof(double)) + sg::align_up((size_t)B * V * sizeof(Proj)) +
           sg::align_up((size_t)B * H * W * sizeof(u64)) + sg::align_up(std::max<size_t>((size_t)B * P, 1) * sizeof(u32));
}

std::atomic<int> g_small{kSmall};
thread_local int64_t t_stats[6] = {0, 0, 0, 0, 0, 0};

}  // namespace

extern "C" {

size_t sg_render_ws_bytes(int V, long long P, int B, int W, int H) { return sizes_ok(V, P, B, W, H) ? need_bytes(V, P, B, W, H) : 0; }

int sg_render_stats(int64_t* h, int cap) {
    SG_REQUIRE(h && cap >= 6, "sg_render_stats: room for 6 values is needed (%d at %p)", cap, (const void*)h);
    for (int i = 0; i < 6; ++i) h[i] = t_stats[i];
    return 6;
}

int sg_render_set_tuning(int small) {
    SG_REQUIRE(small >= 0 && small <= kSmallMax, "sg_render_set_tuning: the small-primitive threshold is 1..%d pixels, or 0 for the build's %d (%d)", kSmallMax,
               kSmall, small);
    g_small.store(small ? small : kSmall);
    return SG_OK;
}

int sg_render(const float* d_xyz, int stride, int V, const int32_t* d_faces, long long F, int point_size, int B, const double* h_cam, int ortho,
              double near, int W, int H, int32_t* d_prim, float* d_depth, int32_t* d_vert, int32_t* d_hits, void* d_ws, size_t ws_bytes, void* stream) {
    const char* who = "sg_render";
    SG_REQUIRE(V >= 1 && F >= 0 && B >= 1 && W >= 1 && H >= 1, "%s: %d vertices, %lld faces, %d views of %d x %d pixels", who, V, F, B, W, H);
    if (V > SG_MAX_CLOUD_POINTS) return sg::fail(SG_EUNSUP, "%s: %d vertices; a scan holds at most %d", who, V, SG_MAX_CLOUD_POINTS);
    if (F > kMaxFaces) return sg::fail(SG_EUNSUP, "%s: %lld faces; a call takes at most 2^26", who, F);
    if (B > kMaxViews || W > kMaxSide || H > kMaxSide || (long long)B * H * W > kMaxPixels)
        return sg::fail(SG_EUNSUP, "%s: %d views of %d x %d pixels; a call takes at most %d views, sides of %d and 2^26 pixels in all", who, B, W, H, kMaxViews,
                        kMaxSide);
    SG_REQUIRE(d_xyz && h_cam && d_prim && d_ws, "%s: a null pointer", who);
    SG_REQUIRE(stride >= 3, "%s: rows of %d floats; a point is at least 3", who, stride);
    SG_REQUIRE((d_faces != nullptr) == (F > 0), "%s: faces %p with F = %lld; triangles are d_faces with F > 0, splats NULL with F == 0", who,
               (const void*)d_faces, F);
    const bool is_faces = F > 0;
    SG_REQUIRE(is_faces || (point_size >= 1 && point_size <= kMaxPointSize && (point_size & 1)), "%s: point_size %d; a splat's side is odd, 1..%d", who,
               point_size, kMaxPointSize);
    SG_REQUIRE(std::isfinite(near) && near > 0.0, "%s: near must be finite and > 0 (%g)", who, near);
    for (int b = 0; b < B; ++b) {
        const double* c = h_cam + (size_t)b * kCamDoubles;
        for (int k = 0; k < kCamDoubles; ++k) SG_REQUIRE(std::isfinite(c[k]), "%s: camera %d holds a number that is not finite (entry %d)", who, b, k);
        SG_REQUIRE(c[12] != 0.0 && c[13] != 0.0, "%s: camera %d has fx = %g, fy = %g; neither may be 0", who, b, c[12], c[13]);
    }
    const long long P = is_faces ? F : (long long)V;
    const size_t need = need_bytes(V, F, B, W, H);
    SG_REQUIRE(ws_bytes >= need, "%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
    sg::Carver cv(d_ws, ws_bytes);
    u64* misc = cv.take<u64>(kMisc);
    double* cam = cv.take<double>((size_t)B * kCamDoubles);
    Proj* proj = cv.take<Proj>((size_t)B * V);
    u64* keys = cv.take<u64>((size_t)B * H * W);
    u32* queue = cv.take<u32>(std::max<size_t>((size_t)B * F, 1));
    SG_REQUIRE(cv.ok, "%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
    for (int i = 0; i < 6; ++i) t_stats[i] = 0;

    hipStream_t st = sg::as_stream(stream);
    const View vw{W, H, ortho ? 1 : 0, near};
    const long long pixels = (long long)B * H * W;
    SG_HIP(hipMemsetAsync(misc, 0, kMisc * sizeof(u64), st));
    SG_HIP(hipMemsetAsync(keys, 0xff, (size_t)pixels * sizeof(u64), st));
    if (d_hits) SG_HIP(hipMemsetAsync(d_hits, 0, (size_t)V * sizeof(int32_t), st));
    SG_HIP(hipMemcpyAsync(cam, h_cam, (size_t)B * kCamDoubles * sizeof(double), hipMemcpyHostToDevice, st));
    k_rd_project<<<dim3(sg::cdiv(V, kBlock), B), kBlock, 0, st>>>(d_xyz, stride, V, cam, vw, proj);
    const dim3 gp(sg::cdiv(P, kBlock), B);
    const int nbp = sg::cdiv(pixels, kBlock);
    if (is_faces) {
        k_rd_prims<true><<<gp, kBlock, 0, st>>>(d_faces, P, V, proj, vw, 0, g_small.load(), keys, queue, misc);
        k_rd_large<<<(int)std::min<long long>(kLargeGrid, (long long)B * F), kBlock, 0, st>>>(d_faces, V, proj, vw, keys, queue, misc);
        k_rd_resolve<true><<<nbp, kBlock, 0, st>>>(d_faces, V, proj, vw, keys, pixels, d_prim, d_depth, d_vert, d_hits, misc);
    } else {
        k_rd_prims<false><<<gp, kBlock, 0, st>>>(nullptr, P, V, proj, vw, point_size, kMaxPointSize, keys, queue, misc);
        k_rd_resolve<false><<<nbp, kBlock, 0, st>>>(nullptr, V, proj, vw, keys, pixels, d_prim, d_depth, d_vert, d_hits, misc);
    }
    SG_LAUNCH_CHECK();
    u64 land[kMisc] = {0};
    SG_HIP(hipMemcpyAsync(land, misc, sizeof(land), hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    SG_LAUNCH_CHECK();
    if (land[mFlag]) return sg::fail(SG_EINVAL, "%s: a face names a vertex outside 0..%d", who, V - 1);
    for (int i = 0; i < 6; ++i) t_stats[i] = (int64_t)land[mKept + i];
    return SG_OK;
}

int sg_render_colour(const int32_t* d_vert, long long n, const uint8_t* d_cidx, const uint8_t* d_rgb, int V, const uint8_t* h_background, uint8_t* d_img,
                     void* stream) {
    const char* who = "sg_render_colour";
    SG_REQUIRE(n >= 0 && V >= 1, "%s: %lld pixels over %d vertices", who, n, V);
    if (n > kMaxPixels) return sg::fail(SG_EUNSUP, "%s: %lld pixels; a call takes at most 2^26", who, n);
    SG_REQUIRE((d_cidx != nullptr) != (d_rgb != nullptr), "%s: exactly one of d_cidx (a palette index per vertex) and d_rgb ([V,3]) is needed", who);
    SG_REQUIRE(h_background && (n == 0 || (d_vert && d_img)), "%s: a null pointer", who);
    if (n == 0) return SG_OK;
    const Rgb bg{{h_background[0], h_background[1], h_background[2]}};
    k_rd_colour<<<sg::cdiv(n, kBlock), kBlock, 0, sg::as_stream(stream)>>>(d_vert, n, d_cidx, d_rgb, V, bg, d_img);
    SG_LAUNCH_CHECK();
    return SG_OK;
}

}  // extern "C"
