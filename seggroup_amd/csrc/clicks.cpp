// Simulated clicks, host side: the clusters of an instance's segments over the scan's segment graph, in the list order and
// the member order of the reference's group_adjacency_segs -- which its argmax (the first of equally large clusters), its unstable
// argsort (member order, past 16 members) and its random draws (consumed cluster by cluster) all depend on.  The device has contracted the
// scan's edges to segment pairs (kernels_seggraph.hip); what is left is sized by segments.  No HIP call in this file: it is part of the
// host-only sanitizer build, and its arrays are treated as untrusted.
//
// The rule: instances in ascending value, inside an instance its segments in ascending number.  Segment s opens the list [s]; then, over its
// neighbours t < s of the same instance in ascending t, the list that holds t -- unless it is s's already -- is appended to s's whole, in
// its own order, and stops being a list.  What remains are the clusters, in the order their opening segments were visited.  Lists are
// linked with a tail pointer and found through a union-find, so a chain of k segments costs O(k alpha(k)) where the reference's list
// surgery costs O(k^2).
#include "sg_common.h"

#include <numeric>

namespace {

int find_root(std::vector<int32_t>& parent, int32_t x) {
    int32_t r = x;
    while (parent[r] != r) r = parent[r];
    while (parent[x] != r) { const int32_t up = parent[x]; parent[x] = r; x = up; }
    return r;
}

}  // namespace

extern "C" {

int sg_click_clusters(const int32_t* h_pairs, long long P, const int32_t* h_seg_ins, int S, int32_t* h_cl_off, int32_t* h_cl_members,
                      int32_t* h_cl_ins, int* h_C) {
    SG_REQUIRE(S >= 1 && P >= 0 && (P == 0 || h_pairs) && h_seg_ins && h_cl_off && h_cl_members && h_cl_ins && h_C,
               "sg_click_clusters: bad arguments");
    *h_C = 0;
    for (long long i = 0; i < P; ++i) {
        const int32_t a = h_pairs[2 * i], b = h_pairs[2 * i + 1];
        if (a < 0 || b >= S) return sg::fail(SG_EINVAL, "sg_click_clusters: pair %lld names a segment outside 0..%d", i, S - 1);
        if (a >= b) return sg::fail(SG_EINVAL, "sg_click_clusters: pair %lld is not (lower, higher)", i);
        if (i > 0 && (h_pairs[2 * i - 2] > a || (h_pairs[2 * i - 2] == a && h_pairs[2 * i - 1] >= b)))
            return sg::fail(SG_EINVAL, "sg_click_clusters: the pairs do not ascend at pair %lld", i);
    }
    // the lower neighbours of every segment inside its instance: the pairs ascend by (a, b), so a segment's row fills in ascending a
    std::vector<int32_t> row(S + 1, 0);
    const auto inside = [&](long long i) {
        const int32_t ia = h_seg_ins[h_pairs[2 * i]];
        return ia > 0 && ia == h_seg_ins[h_pairs[2 * i + 1]];
    };
    for (long long i = 0; i < P; ++i)
        if (inside(i)) ++row[h_pairs[2 * i + 1] + 1];
    for (int s = 0; s < S; ++s) row[s + 1] += row[s];
    std::vector<int32_t> lower(row[S]), fill(row.begin(), row.end() - 1);
    for (long long i = 0; i < P; ++i)
        if (inside(i)) lower[fill[h_pairs[2 * i + 1]]++] = h_pairs[2 * i];
    // the visiting order: (instance, segment) ascending over the segments that have an instance
    std::vector<int32_t> order;
    order.reserve(S);
    for (int s = 0; s < S; ++s)
        if (h_seg_ins[s] > 0) order.push_back(s);
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return h_seg_ins[x] < h_seg_ins[y]; });
    // union-find over segments; per root the segment that opened its list, per opener the list's tail, per segment its successor
    std::vector<int32_t> parent(S), size(S, 1), opener(S), tail(S), next(S, -1);
    std::iota(parent.begin(), parent.end(), 0);
    std::iota(opener.begin(), opener.end(), 0);
    std::iota(tail.begin(), tail.end(), 0);
    std::vector<char> alive(S, 0);
    for (const int32_t s : order) {
        alive[s] = 1;
        for (int32_t j = row[s]; j < row[s + 1]; ++j) {
            const int32_t rs = find_root(parent, s), rt = find_root(parent, lower[j]);
            if (rs == rt) continue;
            const int32_t o = opener[rt];                          // the absorbed list: o .. tail[o]
            next[tail[s]] = o;
            tail[s] = tail[o];
            alive[o] = 0;
            const int32_t big = size[rs] >= size[rt] ? rs : rt, small = big == rs ? rt : rs;
            parent[small] = big;
            size[big] += size[small];
            opener[big] = s;
        }
    }
    int C = 0;
    int32_t n = 0;
    h_cl_off[0] = 0;
    for (const int32_t s : order) {
        if (!alive[s]) continue;
        for (int32_t m = s; m >= 0; m = next[m]) {
            if (n >= S) return sg::fail(SG_EINTERNAL, "sg_click_clusters: a list does not end");
            h_cl_members[n++] = m;
        }
        h_cl_ins[C] = h_seg_ins[s];
        h_cl_off[++C] = n;
    }
    *h_C = C;
    return SG_OK;
}

}  // extern "C"
