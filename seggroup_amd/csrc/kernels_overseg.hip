// Mesh over-segmentation, device side: everything of the graph-based segmenter that is V- or E-sized arithmetic or sorting.
//
//   k_os_check          coordinates finite, face ids inside 0..V-1                                   (one flag word)
//   k_os_face_normals   n = e1 x e2, normalised; a degenerate face gives exact zeros
//   incidence           (vertex, face) pairs in face-major order, stable radix sort by vertex (sort_device.h): a vertex's faces
//                       come out in ascending face index, a face that names the vertex twice is there twice
//   k_os_vertex_normals one thread per vertex: lower bound of its run, ONE sequential sum in that order, normalised -- no float atomics,
//                       the sum has one order
//   edges               sg_mesh_adjacency's raw list: unique undirected a < b in lexicographic order
//   k_os_weights        w = 1 - Na.Nb, squared when the edge is convex; the sort key is the sign-aware monotone map of w's bits
//                       (w may be slightly negative)
//   sort + gather       stable sort of (key, edge index) over the key's 32 bits -- three 11-bit passes -- then (a, b, w) in that order:
//                       ascending (w, a, b)
//
// Every fp32 operation is written op by op and rounded once (-ffp-contract=off; sqrt and / are the correctly rounded expansions, which
// tests/test_gpu_overseg.py holds to the NumPy statement of the specification bit for bit).  The order-dependent merge chain over the
// sorted edges runs on the host (overseg.cpp).
#include "sg_common.h"
#include "sort_device.h"
#include "overseg_device.h"

namespace {

constexpr int kBlock = 256;

struct F3 { float x, y, z; };

// n / |n| with |n| = sqrt((x*x + y*y) + z*z); exact zeros when the length is not positive
__device__ __forceinline__ F3 normalised(float x, float y, float z) {
    const float len = __builtin_sqrtf((x * x + y * y) + z * z);
    if (len > 0.0f) return F3{x / len, y / len, z / len};
    return F3{0.0f, 0.0f, 0.0f};
}

using sgos::finite_f32;

// flag |= 1: a coordinate is not finite; flag |= 2: a face id is outside 0..V-1
__global__ __launch_bounds__(kBlock) void k_os_check(const float* __restrict__ xyz, int V, const int32_t* __restrict__ faces, int F,
                                                     int* __restrict__ flag) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    int bad = 0;
    if (i < (size_t)V * 3 && !finite_f32(xyz[i])) bad |= 1;
    if (i < (size_t)F * 3) {
        const int v = faces[i];
        if (v < 0 || v >= V) bad |= 2;
    }
    if (bad) atomicOr(flag, bad);
}

// face normals [F,3], and the incidence pairs of the face: key = vertex, value = face, at 3f + corner
__global__ __launch_bounds__(kBlock) void k_os_face_normals(const float* __restrict__ xyz, const int32_t* __restrict__ faces, int F,
                                                            float* __restrict__ fn, unsigned int* __restrict__ inc_key,
                                                            int* __restrict__ inc_face) {
    const int f = blockIdx.x * kBlock + threadIdx.x;
    if (f >= F) return;
    const int i0 = faces[(size_t)f * 3], i1 = faces[(size_t)f * 3 + 1], i2 = faces[(size_t)f * 3 + 2];
    const float p0x = xyz[(size_t)i0 * 3], p0y = xyz[(size_t)i0 * 3 + 1], p0z = xyz[(size_t)i0 * 3 + 2];
    const float e1x = xyz[(size_t)i1 * 3] - p0x, e1y = xyz[(size_t)i1 * 3 + 1] - p0y, e1z = xyz[(size_t)i1 * 3 + 2] - p0z;
    const float e2x = xyz[(size_t)i2 * 3] - p0x, e2y = xyz[(size_t)i2 * 3 + 1] - p0y, e2z = xyz[(size_t)i2 * 3 + 2] - p0z;
    const float nx = e1y * e2z - e1z * e2y;
    const float ny = e1z * e2x - e1x * e2z;
    const float nz = e1x * e2y - e1y * e2x;
    const F3 n = normalised(nx, ny, nz);
    fn[(size_t)f * 3] = n.x; fn[(size_t)f * 3 + 1] = n.y; fn[(size_t)f * 3 + 2] = n.z;
    inc_key[(size_t)f * 3] = (unsigned)i0; inc_key[(size_t)f * 3 + 1] = (unsigned)i1; inc_key[(size_t)f * 3 + 2] = (unsigned)i2;
    inc_face[(size_t)f * 3] = f; inc_face[(size_t)f * 3 + 1] = f; inc_face[(size_t)f * 3 + 2] = f;
}

// the sum of the normals of the faces that name v, in the sorted incidence list's order (ascending face index), from +0
__global__ __launch_bounds__(kBlock) void k_os_vertex_normals(const unsigned int* __restrict__ key, const int* __restrict__ face, int n,
                                                              const float* __restrict__ fn, int V, float* __restrict__ vn) {
    const int v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= V) return;
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
        if (key[mid] < (unsigned)v) lo = mid + 1; else hi = mid;
    }
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    for (int i = lo; i < n && key[i] == (unsigned)v; ++i) {
        const int f = face[i];
        sx = sx + fn[(size_t)f * 3];
        sy = sy + fn[(size_t)f * 3 + 1];
        sz = sz + fn[(size_t)f * 3 + 2];
    }
    const F3 nv = normalised(sx, sy, sz);
    vn[(size_t)v * 3] = nv.x; vn[(size_t)v * 3 + 1] = nv.y; vn[(size_t)v * 3 + 2] = nv.z;
}

// weight and sort key of edge e = (a, b) of the lexicographic list [E,2] int64; idx[e] = e
__global__ __launch_bounds__(kBlock) void k_os_weights(const int64_t* __restrict__ adj, int E, const float* __restrict__ xyz,
                                                       const float* __restrict__ vn, float* __restrict__ w_out,
                                                       unsigned int* __restrict__ key, int* __restrict__ idx) {
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= E) return;
    const size_t a = (size_t)adj[(size_t)e * 2], b = (size_t)adj[(size_t)e * 2 + 1];
    const float nax = vn[a * 3], nay = vn[a * 3 + 1], naz = vn[a * 3 + 2];
    const float nbx = vn[b * 3], nby = vn[b * 3 + 1], nbz = vn[b * 3 + 2];
    const float d = (nax * nbx + nay * nby) + naz * nbz;
    float w = 1.0f - d;
    const float dx = xyz[b * 3] - xyz[a * 3], dy = xyz[b * 3 + 1] - xyz[a * 3 + 1], dz = xyz[b * 3 + 2] - xyz[a * 3 + 2];
    const float c = (nbx * dx + nby * dy) + nbz * dz;
    if (c > 0.0f) w = w * w;
    w_out[e] = w;
    key[e] = sgos::weight_key(w);
    idx[e] = e;
}

__global__ __launch_bounds__(kBlock) void k_os_gather(const int* __restrict__ idx, int E, const int64_t* __restrict__ adj,
                                                      const float* __restrict__ w, int32_t* __restrict__ edges, float* __restrict__ w_sorted) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= E) return;
    const int e = idx[i];
    edges[(size_t)i * 2] = (int32_t)adj[(size_t)e * 2];
    edges[(size_t)i * 2 + 1] = (int32_t)adj[(size_t)e * 2 + 1];
    w_sorted[i] = w[e];
}

int bits_for(long long n) {
    int b = 1;
    while ((1ll << b) < n) ++b;
    return b;
}

struct Plan {                       // the workspace of one scan
    size_t n;                       // 3F, at least 1
    float* fn;                      // [F,3] face normals
    unsigned int *k0, *k1;          // incidence keys, then the weight keys
    int *v0, *v1;                   // incidence faces, then the edge indices
    int* hist;
    float* w;                       // [E] weights in lexicographic edge order
    int64_t* adj;                   // [3F,2] sg_mesh_adjacency's raw list
    int* flag;
    void* adj_ws;
    size_t adj_ws_bytes;
    // outputs of sg_overseg_scan, which has no caller's buffers for them
    float* vn;
    int32_t* edges;
    float* w_sorted;
    bool ok;
};

Plan carve(void* d_ws, size_t ws_bytes, int V, int F) {
    Plan p{};
    p.n = (size_t)std::max(F, 1) * 3;
    sg::Carver cv(d_ws, ws_bytes);
    p.fn = cv.take<float>(p.n);
    p.k0 = cv.take<unsigned int>(p.n);
    p.k1 = cv.take<unsigned int>(p.n);
    p.v0 = cv.take<int>(p.n);
    p.v1 = cv.take<int>(p.n);
    p.hist = cv.take<int>(sgsort::hist_ints((long long)p.n));
    p.w = cv.take<float>(p.n);
    p.adj = cv.take<int64_t>(p.n * 2);
    p.flag = cv.take<int>(1);
    p.adj_ws_bytes = sg_mesh_adjacency_ws_bytes(F);
    p.adj_ws = cv.take<char>(p.adj_ws_bytes);
    p.vn = cv.take<float>((size_t)std::max(V, 1) * 3);
    p.edges = cv.take<int32_t>(p.n * 2);
    p.w_sorted = cv.take<float>(p.n);
    p.ok = cv.ok;
    return p;
}

// sg_overseg_set_timing(1): the calling thread's next sg_overseg_edges calls bracket their stages with events (tools/time_overseg.py)
constexpr int kStages = 8;
const char* const kStageNames[kStages] = {"check", "face_normals", "incidence_sort", "vertex_normals", "edges", "weights", "weight_sort", "gather"};
thread_local sgos::StageTimes<kStages> t_times;

using StageClock = sgos::StageClock<kStages>;

}  // namespace

// the stages both segmenters share (overseg_device.h)
const int* sgos::sort_by_weight(unsigned int* k0, unsigned int* k1, int* v0, int* v1, int* hist, int E, hipStream_t st) {
    auto W = sgsort::one_list<unsigned int, int>(k0, k1, v0, v1, hist, E);
    sgsort::radix_sort<unsigned int, int, true>(W, 1, 0, 32, st);
    return W.vin[0];
}

void sgos::gather_edges(const int* idx, int E, const int64_t* adj, const float* w, int32_t* edges, float* w_sorted, hipStream_t st) {
    k_os_gather<<<sg::cdiv(E, kBlock), kBlock, 0, st>>>(idx, E, adj, w, edges, w_sorted);
}

extern "C" {

// the stage times in microseconds of this thread's last timed sg_overseg_edges -> number of stages; names through sg_overseg_stage_name
SG_STAGE_TIMER_API(overseg, t_times, kStageNames)

size_t sg_overseg_ws_bytes(int V, int F) {
    const size_t n = (size_t)std::max(F, 1) * 3;
    return 7 * sg::align_up(n * 4) + sg::align_up(sgsort::hist_ints((long long)n) * 4) + 2 * sg::align_up(n * 16) + 256 +
           sg::align_up(sg_mesh_adjacency_ws_bytes(F)) + sg::align_up((size_t)std::max(V, 1) * 12);
}

int sg_overseg_edges(const float* d_xyz, int V, const int32_t* d_faces, int F, float* d_face_normals, float* d_normals, int32_t* d_edges,
                     float* d_w, int* h_E, void* d_ws, size_t ws_bytes, void* stream) {
    SG_REQUIRE(V > 0 && F >= 0 && d_xyz && (F == 0 || d_faces) && d_normals && h_E && d_ws && (F == 0 || (d_edges && d_w)),
               "sg_overseg_edges: bad arguments");
    SG_REQUIRE((long long)F * 3 <= 0x7fffffffll && (long long)V * 3 <= 0x7fffffffll, "sg_overseg_edges: the mesh is too large");
    *h_E = 0;
    const Plan p = carve(d_ws, ws_bytes, V, F);
    if (!p.ok) return sg::fail(SG_ENOMEM, "sg_overseg_edges: workspace too small (%zu < %zu)", ws_bytes, sg_overseg_ws_bytes(V, F));
    hipStream_t st = sg::as_stream(stream);
    const int n = 3 * F;
    StageClock clock(st, t_times.timing, t_times.us);
    // 0. the inputs are the caller's: nothing reads through a face id before this check has passed
    SG_HIP(hipMemsetAsync(p.flag, 0, 4, st));
    k_os_check<<<sg::cdiv(3ll * std::max(V, F), kBlock), kBlock, 0, st>>>(d_xyz, V, d_faces, F, p.flag);
    int flag = 0;
    SG_HIP(hipMemcpyAsync(&flag, p.flag, 4, hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    if (flag & 1) return sg::fail(SG_EINVAL, "sg_overseg_edges: a vertex coordinate is not finite");
    if (flag & 2) return sg::fail(SG_EINVAL, "sg_overseg_edges: a face names a vertex outside 0..%d", V - 1);
    clock.tick();
    // 1. face normals + incidence pairs, 2. stable sort by vertex, ordered sum per vertex
    const unsigned int* skey = p.k0;
    const int* sface = p.v0;
    if (F > 0) {
        k_os_face_normals<<<sg::cdiv(F, kBlock), kBlock, 0, st>>>(d_xyz, d_faces, F, p.fn, p.k0, p.v0);
        clock.tick();
        auto L = sgsort::one_list<unsigned int, int>(p.k0, p.k1, p.v0, p.v1, p.hist, n);
        sgsort::radix_sort<unsigned int, int, true>(L, 1, 0, bits_for((long long)V + 1), st);
        skey = L.kin[0];
        sface = L.vin[0];
        clock.tick();
        if (d_face_normals) SG_HIP(hipMemcpyAsync(d_face_normals, p.fn, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    }
    k_os_vertex_normals<<<sg::cdiv(V, kBlock), kBlock, 0, st>>>(skey, sface, n, p.fn, V, d_normals);
    SG_LAUNCH_CHECK();
    if (F == 0) return SG_OK;
    clock.tick();
    // 3. the unique undirected edges in lexicographic order: sg_mesh_adjacency's raw list, with its limits and its errors
    int E = 0;
    const int rc = sg_mesh_adjacency(d_faces, F, nullptr, V, p.adj, &E, nullptr, nullptr, p.adj_ws, p.adj_ws_bytes, stream);
    if (rc < 0) return rc;
    if (E < 0 || E > n) return sg::fail(SG_EHIP, "sg_overseg_edges: %d edges from %d faces", E, F);
    clock.tick();
    if (E == 0) return SG_OK;
    // 4. weights and keys, 5. ascending (w, a, b): a stable sort of the lexicographic list by the key (the incidence buffers are free again)
    k_os_weights<<<sg::cdiv(E, kBlock), kBlock, 0, st>>>(p.adj, E, d_xyz, d_normals, p.w, p.k0, p.v0);
    clock.tick();
    const int* order = sgos::sort_by_weight(p.k0, p.k1, p.v0, p.v1, p.hist, E, st);
    clock.tick();
    sgos::gather_edges(order, E, p.adj, p.w, d_edges, d_w, st);
    clock.tick();
    SG_LAUNCH_CHECK();
    *h_E = E;
    return SG_OK;
}

int sg_overseg_scan(const float* d_xyz, int V, const int32_t* d_faces, int F, float k_thresh, int seg_min_verts, int32_t* h_seg_indices,
                    void* d_ws, size_t ws_bytes, void* stream) {
    SG_REQUIRE(V > 0 && F >= 0 && h_seg_indices && d_ws, "sg_overseg_scan: bad arguments");
    const Plan p = carve(d_ws, ws_bytes, V, F);
    if (!p.ok) return sg::fail(SG_ENOMEM, "sg_overseg_scan: workspace too small (%zu < %zu)", ws_bytes, sg_overseg_ws_bytes(V, F));
    int E = 0;
    int rc = sg_overseg_edges(d_xyz, V, d_faces, F, nullptr, p.vn, p.edges, p.w_sorted, &E, d_ws, ws_bytes, stream);
    if (rc < 0) return rc;
    std::vector<int32_t> h_edges((size_t)E * 2);
    std::vector<float> h_w((size_t)E);
    if (E > 0) {
        hipStream_t st = sg::as_stream(stream);
        SG_HIP(hipMemcpyAsync(h_edges.data(), p.edges, (size_t)E * 8, hipMemcpyDeviceToHost, st));
        SG_HIP(hipMemcpyAsync(h_w.data(), p.w_sorted, (size_t)E * 4, hipMemcpyDeviceToHost, st));
        SG_HIP(hipStreamSynchronize(st));
    }
    return sg_overseg_merge(h_edges.data(), h_w.data(), E, V, k_thresh, seg_min_verts, h_seg_indices);
}

}  // extern "C"
