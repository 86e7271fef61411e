// Connected components of a scan's graph: comp[v] = the lowest vertex index of v's component, size[v] = its vertex count,
// C = the number of components.  The graph is an edge list, the sides of a face list, or a kNN table cut at a length; an optional label
// vector keeps only the pairs whose ends hold the same value.  One pass over the pairs, no iteration to convergence:
//
//   k_cc_init      parent[v] = v, the counters zeroed
//   k_cc_hook      per pair: both roots (path halving), the HIGHER root hooked under the LOWER with atomicCAS(&parent[hi], hi, lo)
//   k_cc_flatten   (its own launch: every hook is visible) comp[v] = v's root, the roots counted, one integer add per wave and root
//   k_cc_sizes     size[v] = count[comp[v]]
//
// The invariant: every write to parent[x] after k_cc_init stores a value BELOW x (a hook writes lo < hi, a halving writes the parent of
// x's parent, and x's parent was below x already).  So parent[x] <= x always, parent[x] == x exactly while x was never written -- once
// hooked, never a root again -- and there are no cycles.  A component's minimum is never the higher of two roots, so it is never hooked:
// it is the final root.  Any value parent[x] ever held is a vertex of x's tree, so a stale read names a vertex with the same root: a find
// over stale values ends at a vertex that was a root once, the CAS (decided at the memory side) then fails and hands back the present
// parent, and the pair goes on from there.  Both sides of a pair only move to lower indices, which bounds the work per pair by 2 V steps;
// the budget below is that bound, and a thread that runs out of it sets the flag word instead of spinning (SG_EINTERNAL).
// Finds read parent with relaxed agent-scope loads (served by L2, not by a CU's L1) so that a retry is rare, not for correctness.
// A halving store goes to a vertex that is not a root (its parent was read as another vertex), and no CAS can succeed on such a vertex:
// a halving cannot undo a hook.  Two halvings of one vertex may land in either order; both values are ancestors.
//
// Results are integers and independent of the order of the atomics: the same bytes on every run.
//
// The hook with its budget and flag word, and the init, flatten and sizes kernels, live in components_device.h: the radius graph
// (kernels_radius.hip) runs the same hook from inside its search and launches the same three kernels.
#include <cmath>

#include "sg_common.h"
#include "overseg_device.h"
#include "components_device.h"

namespace {

using namespace sgcc;

constexpr int kMaxBlocks = 16384;              // grid-stride above this many blocks of pairs
constexpr long long kMaxEdges = 1ll << 30;

enum class Src : int { Edges, Faces, Knn };

struct Graph {
    const int32_t* pairs;           // edges [E,2] | faces [F,3] | kNN table [N,row]
    long long count;                // E | F | N * row
    int row;                        // kNN: entries per row
    const float* points;            // kNN: rows of `stride` floats
    int stride;
    float r2;                       // kNN: max_edge * max_edge, rounded once on the host
    const int32_t* label;           // the filter, or NULL
};

__device__ __forceinline__ void join(int* parent, int a, int b, int V, const int32_t* label, Misc* m, bool& bad) {
    if ((unsigned)a >= (unsigned)V || (unsigned)b >= (unsigned)V) { bad = true; return; }
    if (a == b) return;
    if (label && label[a] != label[b]) return;
    hook(parent, a, b, V, m);
}

template <Src kSrc>
__global__ __launch_bounds__(kBlock) void k_cc_hook(Graph g, int V, int* parent, Misc* m) {
    bool bad_index = false, bad_coord = false;
    for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < g.count; e += (long long)gridDim.x * kBlock) {
        if constexpr (kSrc == Src::Edges) {
            join(parent, g.pairs[2 * e], g.pairs[2 * e + 1], V, g.label, m, bad_index);
        } else if constexpr (kSrc == Src::Faces) {
            const int a = g.pairs[3 * e], b = g.pairs[3 * e + 1], c = g.pairs[3 * e + 2];
            join(parent, a, b, V, g.label, m, bad_index);
            join(parent, b, c, V, g.label, m, bad_index);
            join(parent, a, c, V, g.label, m, bad_index);
        } else {
            const int i = (int)(e / g.row), t = (int)(e - (long long)i * g.row);
            const float* pi = g.points + (size_t)i * g.stride;
            const float x = pi[0], y = pi[1], z = pi[2];
            if (t == 0) {                        // entry 0 is skipped whatever it holds; its thread looks at the point itself
                bad_coord |= !(sgos::finite_f32(x) && sgos::finite_f32(y) && sgos::finite_f32(z));
                continue;
            }
            const int j = g.pairs[e];
            if ((unsigned)j >= (unsigned)V) { bad_index = true; continue; }
            if (j == i) continue;
            const float* pj = g.points + (size_t)j * g.stride;
            const float d0 = pj[0] - x, d1 = pj[1] - y, d2 = pj[2] - z;
            const float dd = (d0 * d0 + d1 * d1) + d2 * d2;
            if (dd <= g.r2) join(parent, i, j, V, g.label, m, bad_index);       // NaN (a coordinate that is not finite, flagged by its own thread): no pair
        }
    }
    if (bad_index) atomicOr(&m->flag, kFlagIndex);
    if (bad_coord) atomicOr(&m->flag, kFlagCoord);
}

struct Plan {
    Misc* misc;
    int* parent;
    int* count;
    bool ok;
};

Plan carve(void* d_ws, size_t ws_bytes, int V) {
    Plan p{};
    sg::Carver cv(d_ws, ws_bytes);
    p.misc = cv.take<Misc>(1);
    p.parent = cv.take<int>((size_t)V);
    p.count = cv.take<int>((size_t)V);
    p.ok = cv.ok;
    return p;
}

// sg_components_set_timing(1): the calling thread's next calls bracket their stages with events (tools/time_components.py)
constexpr int kStages = 4;
const char* const kStageNames[kStages] = {"init", "hook", "flatten", "sizes"};
thread_local sgos::StageTimes<kStages> t_times;

int check_tail(const char* who, int V, int32_t* d_comp, int* h_C, void* d_ws) {
    SG_REQUIRE(d_comp && h_C && d_ws, "%s: a null pointer", who);
    *h_C = 0;
    SG_REQUIRE(V >= 1, "%s: %d vertices", who, V);
    if (V > SG_MAX_CLOUD_POINTS) return sg::fail(SG_EUNSUP, "%s: %d vertices; a graph holds at most %d", who, V, SG_MAX_CLOUD_POINTS);
    return SG_OK;
}

template <Src kSrc>
int run(const char* who, const Graph& g, int V, int32_t* d_comp, int32_t* d_size, int* h_C, void* d_ws, size_t ws_bytes, void* stream) {
    const Plan p = carve(d_ws, ws_bytes, V);
    SG_REQUIRE(p.ok, "%s: workspace too small (%zu < %zu)", who, ws_bytes, sg_components_ws_bytes(V));
    hipStream_t st = sg::as_stream(stream);
    const int nb = sg::cdiv(V, kBlock);
    sgos::StageClock<kStages> clock(st, t_times.timing, t_times.us);
    k_cc_init<<<nb, kBlock, 0, st>>>(p.parent, p.count, V, p.misc);
    clock.tick();
    if (g.count > 0) {
        const int hb = (int)std::min<long long>((g.count + kBlock - 1) / kBlock, kMaxBlocks);
        k_cc_hook<kSrc><<<hb, kBlock, 0, st>>>(g, V, p.parent, p.misc);
    }
    clock.tick();
    k_cc_flatten<<<nb, kBlock, 0, st>>>(p.parent, V, d_comp, d_size ? p.count : nullptr, p.misc);
    clock.tick();
    if (d_size) k_cc_sizes<<<nb, kBlock, 0, st>>>(d_comp, p.count, V, d_size);
    clock.tick();
    Misc hm{};
    SG_HIP(hipMemcpyAsync(&hm, p.misc, sizeof(Misc), hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    SG_LAUNCH_CHECK();
    if (hm.flag & kFlagIndex) return sg::fail(SG_EINVAL, "%s: a vertex index outside 0..%d", who, V - 1);
    if (hm.flag & kFlagCoord) return sg::fail(SG_EINVAL, "%s: a coordinate is not finite", who);
    if (hm.flag & kFlagBudget) return sg::fail(SG_EINTERNAL, "%s: a chase ran out of its %d steps", who, 2 * V + 4);
    if (hm.roots < 1 || hm.roots > V) return sg::fail(SG_EINTERNAL, "%s: %d components from %d vertices", who, hm.roots, V);
    *h_C = hm.roots;
    return SG_OK;
}

}  // namespace

extern "C" {

SG_STAGE_TIMER_API(components, t_times, kStageNames)

size_t sg_components_ws_bytes(int V) {
    if (V < 1 || V > SG_MAX_CLOUD_POINTS) return 0;
    return sg::align_up(sizeof(Misc)) + 2 * sg::align_up((size_t)V * 4);
}

int sg_components_edges(const int32_t* d_edges, long long E, int V, const int32_t* d_label, int32_t* d_comp, int32_t* d_size, int* h_C,
                        void* d_ws, size_t ws_bytes, void* stream) {
    const char* who = "sg_components_edges";
    if (const int rc = check_tail(who, V, d_comp, h_C, d_ws)) return rc;
    SG_REQUIRE(E >= 0 && (E == 0 || d_edges), "%s: %lld edges at %p", who, E, (const void*)d_edges);
    if (E >= kMaxEdges) return sg::fail(SG_EUNSUP, "%s: %lld edges; a list holds fewer than %lld", who, E, kMaxEdges);
    Graph g{};
    g.pairs = d_edges; g.count = E; g.label = d_label;
    return run<Src::Edges>(who, g, V, d_comp, d_size, h_C, d_ws, ws_bytes, stream);
}

int sg_components_faces(const int32_t* d_faces, int F, int V, const int32_t* d_label, int32_t* d_comp, int32_t* d_size, int* h_C, void* d_ws,
                        size_t ws_bytes, void* stream) {
    const char* who = "sg_components_faces";
    if (const int rc = check_tail(who, V, d_comp, h_C, d_ws)) return rc;
    SG_REQUIRE(F >= 0 && (F == 0 || d_faces), "%s: %d faces at %p", who, F, (const void*)d_faces);
    Graph g{};
    g.pairs = d_faces; g.count = F; g.label = d_label;
    return run<Src::Faces>(who, g, V, d_comp, d_size, h_C, d_ws, ws_bytes, stream);
}

int sg_components_knn(const float* d_points, int stride, const int32_t* d_knn, int N, int row, float max_edge, const int32_t* d_label,
                      int32_t* d_comp, int32_t* d_size, int* h_C, void* d_ws, size_t ws_bytes, void* stream) {
    const char* who = "sg_components_knn";
    if (const int rc = check_tail(who, N, d_comp, h_C, d_ws)) return rc;
    SG_REQUIRE(d_points && d_knn, "%s: a null pointer", who);
    SG_REQUIRE(stride >= 3 && row >= 2, "%s: rows of %d floats, lists of %d entries", who, stride, row);
    SG_REQUIRE(max_edge > 0.0f, "%s: max_edge must be +inf or finite and positive (%g)", who, (double)max_edge);     // NaN fails the comparison
    Graph g{};
    g.pairs = d_knn; g.count = (long long)N * row; g.row = row; g.points = d_points; g.stride = stride; g.label = d_label;
    g.r2 = max_edge * max_edge;                  // one fp32 multiplication; +inf stays +inf and admits every pair
    return run<Src::Knn>(who, g, N, d_comp, d_size, h_C, d_ws, ws_bytes, stream);
}

}  // extern "C"
