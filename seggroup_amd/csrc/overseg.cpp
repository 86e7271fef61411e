// Mesh over-segmentation, host side: the order-dependent part of the graph-based segmenter.  The device hands over the
// unique mesh edges in ascending (w, a, b) (kernels_overseg.hip); what follows is a chain in which every decision depends on the unions
// before it -- Felzenszwalb-Huttenlocher merging, then the small-segment pass over the same edges -- so it is walked by one host thread
// (such a chain is not walked by one lane).  No HIP call in this file: it is part of the host-only sanitizer build, and its
// arrays are treated as untrusted.
#include <cmath>

#include "sg_common.h"

namespace {

struct Forest {
    std::vector<int32_t> parent, size;
    std::vector<float> thr;
    Forest(int V, float k) : parent((size_t)V), size((size_t)V, 1), thr((size_t)V, k) {
        for (int v = 0; v < V; ++v) parent[(size_t)v] = v;
    }
    int find(int v) {
        while (parent[(size_t)v] != v) {
            parent[(size_t)v] = parent[(size_t)parent[(size_t)v]];         // path halving
            v = parent[(size_t)v];
        }
        return v;
    }
    int join(int ra, int rb) {                                             // the larger tree keeps its root; ids do not depend on that choice
        if (size[(size_t)ra] < size[(size_t)rb]) std::swap(ra, rb);
        parent[(size_t)rb] = ra;
        size[(size_t)ra] += size[(size_t)rb];
        return ra;
    }
};

}  // namespace

extern "C" {

int sg_overseg_merge(const int32_t* h_edges, const float* h_w, int E, int V, float k_thresh, int seg_min_verts, int32_t* h_seg_indices) {
    SG_REQUIRE(V > 0 && E >= 0 && h_seg_indices && (E == 0 || (h_edges && h_w)), "sg_overseg_merge: bad arguments");
    SG_REQUIRE(std::isfinite(k_thresh) && k_thresh >= 0.0f, "sg_overseg_merge: k_thresh must be finite and not negative");
    SG_REQUIRE(seg_min_verts >= 0, "sg_overseg_merge: seg_min_verts must not be negative");
    for (int e = 0; e < E; ++e) {
        const int32_t a = h_edges[(size_t)e * 2], b = h_edges[(size_t)e * 2 + 1];
        if (a < 0 || b < 0 || a >= V || b >= V) return sg::fail(SG_EINVAL, "sg_overseg_merge: edge %d names a vertex outside 0..%d", e, V - 1);
        if (a >= b) return sg::fail(SG_EINVAL, "sg_overseg_merge: edge %d is not a < b", e);
        if (e > 0 && !(h_w[e - 1] <= h_w[e])) return sg::fail(SG_EINVAL, "sg_overseg_merge: the weights are not ascending at edge %d", e);
    }
    if (E > 0 && !(h_w[0] == h_w[0])) return sg::fail(SG_EINVAL, "sg_overseg_merge: the weights are not ascending at edge 0");
    Forest uf(V, k_thresh);
    // 6. merge while the edge is no heavier than both components' thresholds
    for (int e = 0; e < E; ++e) {
        const int ra = uf.find(h_edges[(size_t)e * 2]), rb = uf.find(h_edges[(size_t)e * 2 + 1]);
        const float w = h_w[e];
        if (ra != rb && w <= uf.thr[(size_t)ra] && w <= uf.thr[(size_t)rb]) {
            const int r = uf.join(ra, rb);
            const float q = k_thresh / (float)uf.size[(size_t)r];
            uf.thr[(size_t)r] = w + q;
        }
    }
    // 7. the same edges in the same order: a component below seg_min_verts joins its neighbour
    for (int e = 0; e < E; ++e) {
        const int ra = uf.find(h_edges[(size_t)e * 2]), rb = uf.find(h_edges[(size_t)e * 2 + 1]);
        if (ra != rb && (uf.size[(size_t)ra] < seg_min_verts || uf.size[(size_t)rb] < seg_min_verts)) uf.join(ra, rb);
    }
    // 8. a component's id is its lowest vertex: vertices are visited in ascending order, so the first one to reach a root names it
    std::vector<int32_t> lowest((size_t)V, -1);
    for (int v = 0; v < V; ++v) {
        const int r = uf.find(v);
        if (lowest[(size_t)r] < 0) lowest[(size_t)r] = v;
        h_seg_indices[v] = lowest[(size_t)r];
    }
    return SG_OK;
}

}  // extern "C"
