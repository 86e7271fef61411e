// Host grouping of one scene (reference seggroup/model.py:710-888), shared by the single-scene pipeline (pipeline.cpp) and the scene
// engine (engine.cpp): the disjoint set of the grouping engine (grouping.cpp), the cluster graph, the layer numberings and the [14,S]
// label tables, advanced step by step between the caller's launches, plus the descriptor arrays the device reads for a layer.  The
// callers keep their launches, buffers, stream synchronisations and the timing of the host work between them.
#pragma once
#include <memory>
#include <vector>

#include "sg_common.h"

namespace sgp {

struct LayerDesc {               // host view of one frozen numbering + what the device needs for it
    int C = 0;
    std::vector<int32_t> root, cl_of_seg, order, cl_seg_off, cl_pt_off, dst;
};

int freeze_layer(const sg_partition* part, int S, LayerDesc& L);

struct SceneGrouping {
    const sg_scene* sc = nullptr;
    int mode = SG_MODE_INS_INFER;
    sg_result* out = nullptr;                  // trace, stalled, used_fallback
    sg_debug* dbg = nullptr;                   // h_adj / h_dist / n_adj taps, usually none
    int32_t* tab = nullptr;                    // [14,S] label tables, in the caller's (pinned) memory
    int max_ins = 1, max_seg = 0;              // weak instance ids + 2 (the metric kernels' bound), largest over-segment
    LayerDesc Lcur, Lnew;                      // the numbering in front of / behind the latest grouping pass
    int E = 0;                                 // rows of adj: the cluster graph in Lnew's numbering
    std::vector<int32_t> adj, adj_next;
    std::vector<uint8_t> connected, keep;
    struct Rows { int first = 0, count = 0; } wrote;     // the table rows the latest step wrote (every step writes behind the previous one's)
    // final clustering: Feat_4 [C5,256] of the roots root5[0..C5) left by group_unlabeled; L5 = the clusters the FPS-1024 fallback samples
    std::vector<float> feat4;
    std::vector<int32_t> root5;
    int C5 = 0;
    LayerDesc L5;

    // rows written so far; the last two are the ins / sem vectors the metrics read
    int n_tables() const { return wrote.first + wrote.count; }
    int ins_row() const { return n_tables() - 2; }
    int sem_row() const { return n_tables() - 1; }
    const sg_partition* partition() const { return part.get(); }

    // The steps, in model.py order; each returns SG_OK or a negative error and leaves the rows it wrote in `wrote`.
    // begin: result fields cleared, max_ins / max_seg; create_partition: the disjoint set (model.py:712-721), a step of its own
    // because the single-scene pipeline builds it behind its first launches
    void begin(const sg_scene* scene, int mode, int32_t* tables, sg_result* result, sg_debug* taps);
    int create_partition();
    // layer 1: every segment its own cluster, rows 0-2 (needs no device result)
    int layer1();
    // structural layer (model.py:735-783): group the contracted segment graph h_adj1 [E1,2] at 6.0 (3.0 in sem_infer) on its decision
    // distances, rows 3-5
    int structural(const int32_t* h_adj1, const float* h_dist, int E1);
    // semantic layer 0 / 1 (model.py:802-815 / 843-856): group on the GCN decision distances [E] at 2.0, rows 6-8 / 9-11
    int semantic(int layer, const float* h_dist);
    // final clustering (model.py:868-888) from the last GCN output h_gcn [Lcur.C,256]: Feat_4, group_unlabeled, rows 12-13.  Returns 1
    // when the FPS-1024 fallback must run first: the caller samples L5 (fallback_fps1024), waits, and finishes with final_fallback.
    int final_clustering(const float* h_gcn);
    int final_fallback(const float* h_samples);

private:
    struct PartitionFree { void operator()(sg_partition* p) const { sg_partition_destroy(p); } };
    std::unique_ptr<sg_partition, PartitionFree> part;
    int regroup(int p, const float* h_dist, float th);
    int export_rows(int first_row, bool with_seg);
    int final_rows();
    void tap_adj(int i);
};

// Descriptor fillers: a layer's host-built arrays, written into memory the caller provides (the pipeline's descriptor block, the
// engine's parameter arena).
void fill_cl_of_order(const LayerDesc& L, int32_t* cl);                              // [S] cluster of every order slot
void fill_seg_prevcl(const LayerDesc& Lprev, int32_t* prevcl);                       // [S] former cluster of > 20 points, else -1
void fill_cl_mean(const LayerDesc& L, const double* seg_sums, float* mean);          // [C,3] centroids from [S,3] coordinate sums
void fill_parents(const LayerDesc& Lold, const LayerDesc& Lnew, int32_t* goff, int32_t* gidx);   // [Lnew.C+1], [Lold.C]
void fill_csr(const int32_t* adj, int E, int C, int32_t* rowptr, int32_t* col, int32_t* eid);   // [C+1], [2E], [2E]
int pos_of_point0(const LayerDesc& L);                                               // member-order position of point 0

// The FPS-1024 fallback's device step: the members of L's clusters, 1,024 XYZ samples of each, and their copy into pl->h_samples,
// enqueued on `st`; the caller waits for it its own way.
int fallback_fps1024(sg_pipeline* pl, const sg_scene* sc, const LayerDesc& L, hipStream_t st);

}  // namespace sgp
