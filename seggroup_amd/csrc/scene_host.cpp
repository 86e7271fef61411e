// Host grouping of one scene, shared by pipeline.cpp and engine.cpp (scene_host.h).
#include <cmath>

#include "pipeline_priv.h"
#include "scene_host.h"

namespace sgp {

int freeze_layer(const sg_partition* part, int S, LayerDesc& L) {
    L.root.resize(S); L.cl_of_seg.resize(S); L.order.resize(S); L.cl_seg_off.resize(S + 1); L.cl_pt_off.resize(S + 1); L.dst.resize(S);
    L.C = sg_partition_layer(part, L.root.data(), L.cl_of_seg.data(), L.order.data(), L.cl_seg_off.data(), L.cl_pt_off.data(), L.dst.data());
    return L.C;
}

void SceneGrouping::begin(const sg_scene* scene, int mode_, int32_t* tables, sg_result* result, sg_debug* taps) {
    sc = scene; mode = mode_; tab = tables; out = result; dbg = taps;
    part.reset();
    wrote = Rows();
    out->stalled = 0; out->used_fallback = 0;
    for (int i = 0; i < 5; ++i) out->trace[i] = 0;
    max_ins = 1; max_seg = 0;
    for (int s = 0; s < sc->S; ++s) { max_ins = std::max(max_ins, sc->h_seg_ins[s] + 2); max_seg = std::max(max_seg, sc->h_seg_size[s]); }
}

int SceneGrouping::create_partition() {
    part.reset(sg_partition_create(sc->S, sc->h_seg_first, sc->h_seg_size, sc->h_seg_ins, sc->h_seg_sem));
    return part ? SG_OK : SG_EINVAL;
}

int SceneGrouping::export_rows(int first_row, bool with_seg) {
    const int S = sc->S;
    int32_t* a = tab + (size_t)first_row * S;
    const int rc = sg_partition_export_tables(part.get(), with_seg ? a : nullptr, with_seg ? a + S : a, with_seg ? a + 2 * (size_t)S : a + S);
    if (rc < 0) return rc;
    wrote.first = first_row; wrote.count = with_seg ? 3 : 2;
    return SG_OK;
}

void SceneGrouping::tap_adj(int i) {
    if (!dbg) return;
    if (dbg->h_adj[i]) std::copy(adj.begin(), adj.begin() + 2 * (size_t)E, dbg->h_adj[i]);
    dbg->n_adj[i] = E;
}

// grouping pass p (0: structural, 1-2: semantic) on the decision distances h_dist [E] of Lcur's cluster graph: group + re-index + contract
// (model.py:218-258, 291-302, 759-768) into Lnew and adj, trace[p+1], the rows of layer_{p+2}, and the taps h_dist[p] / h_adj[p+1]
int SceneGrouping::regroup(int p, const float* h_dist, float th) {
    if (dbg && dbg->h_dist[p]) std::copy(h_dist, h_dist + E, dbg->h_dist[p]);
    connected.assign(std::max(E, 1), 0);
    int rc = sg_partition_group_nearby(part.get(), Lcur.root.data(), Lcur.C, h_dist, adj.data(), E, th, connected.data());
    if (rc == SG_ESTALL) { out->stalled = 1; rc = SG_OK; sg::err_buf()[0] = 0; }   // downgraded: no stale message stays behind
    if (rc < 0) return rc;
    keep.resize(connected.size());
    for (size_t i = 0; i < connected.size(); ++i) keep[i] = !connected[i];
    adj_next.resize(2 * (size_t)std::max(E, 1));
    const int En = sg_partition_contract(part.get(), Lcur.root.data(), adj.data(), E, keep.data(), adj_next.data());
    if (En < 0) return En;
    freeze_layer(part.get(), sc->S, Lnew);
    adj.assign(adj_next.begin(), adj_next.begin() + 2 * (size_t)En);
    E = En;
    out->trace[p + 1] = Lnew.C;
    rc = export_rows(3 + 3 * p, true);
    tap_adj(p + 1);
    return rc;
}

int SceneGrouping::layer1() {
    freeze_layer(part.get(), sc->S, Lcur);
    out->trace[0] = Lcur.C;
    return export_rows(0, true);                         // layer_1.{seg,ins,sem}
}

int SceneGrouping::structural(const int32_t* h_adj1, const float* h_dist, int E1) {
    adj.assign(h_adj1, h_adj1 + 2 * (size_t)E1);
    E = E1;
    tap_adj(0);
    return regroup(0, h_dist, mode == SG_MODE_SEM_INFER ? 3.0f : 6.0f);
}

int SceneGrouping::semantic(int layer, const float* h_dist) {
    Lcur = Lnew;
    return regroup(1 + layer, h_dist, 2.0f);
}

int SceneGrouping::final_clustering(const float* h_gcn) {
    // Feat_4 = max over absorbed rows of the gcn_3 output, adj_4 = current adj
    const int D4 = 256;
    feat4.assign((size_t)Lnew.C * D4, -INFINITY);
    for (int j = 0; j < Lcur.C; ++j) {
        float* dstp = &feat4[(size_t)Lnew.cl_of_seg[Lcur.root[j]] * D4];
        const float* src = h_gcn + (size_t)j * D4;
        for (int k = 0; k < D4; ++k) dstp[k] = std::max(dstp[k], src[k]);
    }
    root5.assign(Lnew.root.begin(), Lnew.root.begin() + Lnew.C);
    root5.resize(sc->S);
    C5 = Lnew.C;
    int E5 = E;
    adj.resize(2 * (size_t)std::max(E, 1));
    const int need_fallback = sg_partition_group_unlabeled(part.get(), root5.data(), &C5, feat4.data(), D4, adj.data(), &E5);
    if (need_fallback < 0) return need_fallback;
    if (need_fallback) {
        freeze_layer(part.get(), sc->S, L5);
        return 1;
    }
    return final_rows();
}

int SceneGrouping::final_fallback(const float* h_samples) {
    const int rc = sg_partition_unlabeled_fallback(part.get(), L5.root.data(), L5.C, h_samples, 1024);
    if (rc < 0) return rc;
    out->used_fallback = 1;
    return final_rows();
}

int SceneGrouping::final_rows() {
    out->trace[4] = sg_partition_num_clusters(part.get());
    return export_rows(12, false);                       // final.{ins,sem}
}

void fill_cl_of_order(const LayerDesc& L, int32_t* cl) {
    for (size_t i = 0; i < L.order.size(); ++i) cl[i] = L.cl_of_seg[L.order[i]];
}

// layer 3's seeded kNN starts from layer 2's table, which has no list for a cluster of <= 20 points
void fill_seg_prevcl(const LayerDesc& Lprev, int32_t* prevcl) {
    for (size_t s = 0; s < Lprev.cl_of_seg.size(); ++s) {
        const int pc = Lprev.cl_of_seg[s];
        prevcl[s] = Lprev.cl_pt_off[pc + 1] - Lprev.cl_pt_off[pc] > 20 ? pc : -1;
    }
}

// combine_centralized_pointcloud (model.py:429-436): the sum is carried in double, so its grouping does not show in the fp32 result
void fill_cl_mean(const LayerDesc& L, const double* seg_sums, float* mean) {
    for (int c = 0; c < L.C; ++c) {
        double sx = 0.0, sy = 0.0, sz = 0.0;
        for (int i = L.cl_seg_off[c]; i < L.cl_seg_off[c + 1]; ++i) {
            const double* q = seg_sums + 3 * (size_t)L.order[i];
            sx += q[0]; sy += q[1]; sz += q[2];
        }
        const double cnt = (double)(L.cl_pt_off[c + 1] - L.cl_pt_off[c]);
        mean[3 * c] = (float)(sx / cnt); mean[3 * c + 1] = (float)(sy / cnt); mean[3 * c + 2] = (float)(sz / cnt);
    }
}

// the clusters of Lold absorbed by each cluster of Lnew, in Lold order (model.py:766-768): a counting sort
void fill_parents(const LayerDesc& Lold, const LayerDesc& Lnew, int32_t* goff, int32_t* gidx) {
    std::fill(goff, goff + Lnew.C + 1, 0);
    for (int j = 0; j < Lold.C; ++j) ++goff[Lnew.cl_of_seg[Lold.root[j]] + 1];
    for (int c = 0; c < Lnew.C; ++c) goff[c + 1] += goff[c];
    std::vector<int32_t> fill(goff, goff + Lnew.C);
    for (int j = 0; j < Lold.C; ++j) gidx[fill[Lnew.cl_of_seg[Lold.root[j]]]++] = j;
}

// symmetric CSR of the cluster graph: both directions of every edge, rows in edge order
void fill_csr(const int32_t* adj, int E, int C, int32_t* rowptr, int32_t* col, int32_t* eid) {
    std::fill(rowptr, rowptr + C + 1, 0);
    for (int e = 0; e < E; ++e) { ++rowptr[adj[2 * e] + 1]; ++rowptr[adj[2 * e + 1] + 1]; }
    for (int c = 0; c < C; ++c) rowptr[c + 1] += rowptr[c];
    std::vector<int32_t> fill(rowptr, rowptr + C);
    for (int e = 0; e < E; ++e) {
        const int a = adj[2 * e], b = adj[2 * e + 1];
        col[fill[a]] = b; eid[fill[a]++] = e;
        col[fill[b]] = a; eid[fill[b]++] = e;
    }
}

// point 0 is the first member of segment 0; its member-order position is that segment's dst
int pos_of_point0(const LayerDesc& L) {
    for (size_t i = 0; i < L.order.size(); ++i) if (L.order[i] == 0) return L.dst[i];
    return 0;
}

// FPS-1024 over the current clusters (model.py:479), XYZ only, no transform
int fallback_fps1024(sg_pipeline* pl, const sg_scene* sc, const LayerDesc& L, hipStream_t st) {
    const int S = sc->S;
    size_t cur = 0;
    auto at = [&](size_t count) { const size_t a = cur; cur += (count + 3) / 4 * 4; return a; };
    const size_t o_order = at(S), o_dst = at(S), o_cl = at(S), o_off = at(L.C + 1);
    int32_t* h = pl->h_desc.p;
    std::copy_n(L.order.data(), S, h + o_order);
    std::copy_n(L.dst.data(), S, h + o_dst);
    fill_cl_of_order(L, h + o_cl);
    std::copy_n(L.cl_pt_off.data(), L.C + 1, h + o_off);
    SG_HIP(hipMemcpyAsync(pl->desc.p, h, cur * 4, hipMemcpyHostToDevice, st));
    const int32_t* dd = pl->desc.p;
    int rc = sg_gather_members(sc->d_seg_points, sc->d_seg_off, S, dd + o_order, dd + o_dst, dd + o_cl, pl->members.p, nullptr, nullptr, nullptr, (void*)st);
    if (rc < 0) return rc;
    int max_cl = 0;
    for (int c = 0; c < L.C; ++c) max_cl = std::max(max_cl, L.cl_pt_off[c + 1] - L.cl_pt_off[c]);
    if ((rc = pl->need_fallback_buffers()) < 0) return rc;
    rc = sg::fps_sample_hint(sc->d_data, sc->N, 6, pl->members.p, dd + o_off, L.C, 1024, 3, 0, pl->samples_big.p, nullptr, pl->ws_fps.p, pl->ws_fps.n,
                             (void*)st, max_cl);
    if (rc < 0) return rc;
    SG_HIP(hipMemcpyAsync(pl->h_samples.p, pl->samples_big.p, (size_t)L.C * 1024 * 3 * 4, hipMemcpyDeviceToHost, st));
    return SG_OK;
}

}  // namespace sgp
