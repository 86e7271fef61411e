/*
 * seggroup_hip.h -- C ABI of libseggroup_hip.so: the MI355X (gfx950) implementation of the SegGroup
 * pseudo-label generation hot path (reference: antao97/SegGroup, seggroup/model.py + seggroup/infer.py).
 *
 * The reference has no FFI; its operator seam is the set of module-level functions that
 * SegModel.forward resolves by global name.  Each entry point below replaces one (or a
 * fused run) of those functions; the citation names the reference lines it stands in for.  A
 * maintainer binds them from Python with ctypes (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - plain C types only; `d_` pointers are DEVICE pointers (tensor.data_ptr()), `h_` pointers are HOST.
 *   - every function returns 0 on success or a negative SG_E* code; sg_last_error() gives the
 *     message of the calling thread's last failure.  Nothing throws, nothing calls exit().
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream).  Device entry
 *     points only ENQUEUE work unless documented otherwise.
 *   - indices are int32 inside the library (N < 2^31); the Python layer converts from the
 *     reference's int64.  Features are float32.
 *   - functions never allocate or free caller-visible memory.  Scratch comes from the caller
 *     (`d_ws`, sizes from sg_*_ws_bytes) except for the sg_pipeline_* object, which owns its
 *     buffers between create and destroy.
 */
#ifndef SEGGROUP_HIP_H
#define SEGGROUP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SG_OK          0
#define SG_EINVAL     -1   /* bad argument / inconsistent sizes                                   */
#define SG_EHIP       -2   /* a HIP runtime call failed                                            */
#define SG_ENOMEM     -3   /* workspace too small / allocation failed                              */
#define SG_ESTALL     -4   /* reference would loop forever (model.py:228-239)       */
#define SG_EUNSUP     -5   /* size outside the supported envelope (documented per function)        */
#define SG_EINTERNAL  -6   /* a bounded device loop ran out of its budget: a defect, never the input */

#define SG_MODE_INS_INFER 0   /* infer.py --ins_infer : all five layers (model.py:684-897)         */
#define SG_MODE_SEM_INFER 1   /* infer.py --sem_infer : returns after layer 2 (model.py:781-783)   */

#define SG_NUM_LABEL_VECTORS 14 /* layer_{1..4}.{seg,ins,sem} + final.{ins,sem} (model.py:525-605) */
#define SG_RANGE_WORDS 256      /* words of every d_range_bits buffer below (zero-initialised by the caller)  */
#define SG_MAX_POINTS (1 << 20) /* points of one scene: the in-cluster kNN's list keys carry 20 index bits; sg_pipeline_create,
                                 * sg_engine_create and the trainers return NULL / SG_EUNSUP above it (the reference has no such limit;
                                 * ScanNet scenes stay below 600k points)                                     */

const char* sg_last_error(void);
int  sg_version(void);
/* number of visible HIP devices (0 when no GPU): lets callers fail loudly before first use */
int  sg_device_count(void);
/* device self-test of the DPP wave reductions the structural-layer kernels use (csrc/wave_ops.h) against the ds_bpermute
 * butterflies they replace; *h_mismatches = 0 on a healthy build.  Synchronises the stream. */
int  sg_selftest_wave_ops(int* h_mismatches, void* stream);
/* device self-test: the kNN's top-K list in double form (v_min_f64 / v_max_f64 insertion) against the 64-bit integer form, ties, signed
 * zeros, tiny positive scores and the empty key included; *h_mismatches = 0 when they agree */
int  sg_selftest_list_insert(int* h_mismatches, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a3  update_adj, first call (model.py:291-302 with model.py:724-733): contract the point-level
 * mesh adjacency through the over-segmentation.  d_adj is the [E,2] int64 tensor of <scene>.adj.pth;
 * d_seg_of_point maps point -> segment number (rank of the segment's first point).  Output rows are
 * (lo,hi) int32 pairs, lexicographically sorted and unique -- the order torch.unique(dim=0) gives.
 * Implementation: one bit per (lo,hi) pair in an S*S bitmap, then an ordered compaction.
 * Supported: S*S <= 2^31 bits.  d_ws needs sg_contract_ws_bytes(S).
 * ------------------------------------------------------------------------------------------- */
size_t sg_contract_ws_bytes(int S);
int sg_contract_point_edges(const int64_t* d_adj, int E, const int32_t* d_seg_of_point, int N, int S,
                            int32_t* d_out_adj, int out_capacity, int32_t* d_out_count,
                            void* d_ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a2/a10  member lists of one layer's clusters (DisjointSet.indexs / get_cluster_list, model.py:
 * 169-214; re-index blocks model.py:759-768).  A cluster is an ORDERED list of original segments
 * (model.py:191 concatenates member lists), so its member list is the concatenation of those
 * segments' ascending point lists.  h-side arrays come from sg_partition_layer().
 *   d_seg_points/d_seg_off : CSR of the original over-segmentation (points ascending per segment)
 *   d_order[S]  original segment ids in cluster-concatenated order
 *   d_dst[S]    destination offset (in points) of each of those segments
 *   d_cl[S]     cluster number of each of those segments
 * writes d_members[N] (point ids in member order), d_pos_of_point[N] (inverse permutation),
 * d_cluster_of_pos[N] and d_slot_of_pos[N] (index into d_order of the segment holding each position);
 * the last three may be NULL.
 * ------------------------------------------------------------------------------------------- */
int sg_gather_members(const int32_t* d_seg_points, const int32_t* d_seg_off, int S,
                      const int32_t* d_order, const int32_t* d_dst, const int32_t* d_cl,
                      int32_t* d_members, int32_t* d_pos_of_point, int32_t* d_cluster_of_pos,
                      int32_t* d_slot_of_pos, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a4+a5  get_cluster_pointcloud + farthest_point_sampling (model.py:319-426).  For every cluster
 * (member CSR d_members/d_cl_off, C clusters): rows = members tiled P/n times, then P%n FPS picks
 * (start at member 0, first pick = farthest from it with the min-distance array RESET to that pick,
 * first-index argmax, fp32 distances (dx2+dy2)+dz2 with individually rounded squares, trailing-zero
 * fix-up of model.py:407-412).  d_data is [N,ch_in] float32 (XYZ first); ch_out (3 or 6) channels are
 * copied.  transform != 0 applies model.py:421-423 (subtract mean XYZ of the P rows, divide by the
 * scalar max |XYZ|).  d_sel (may be NULL) receives the chosen point ids [C,P].
 * d_ws needs sg_fps_ws_bytes(N) (min-distance scratch for clusters that do not fit in LDS).
 * ------------------------------------------------------------------------------------------- */
size_t sg_fps_ws_bytes(int N);
int sg_fps_sample(const float* d_data, int N, int ch_in, const int32_t* d_members, const int32_t* d_cl_off, int C,
                  int P, int ch_out, int transform, float* d_samples, int32_t* d_sel,
                  void* d_ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a6+a7  MLP1 = knn(k=10) + get_graph_feature1 + conv1x1 6->64 + BatchNorm2d(batch statistics over
 * all C*64*10 rows, eps 1e-5, biased variance) + LeakyReLU(0.2) + max_k + [max | mean] over the 64
 * points (model.py:30-80).  d_samples [C,64,6] -> d_feat rows of 128 floats with row stride
 * feat_stride (floats).  d_w [64,6], d_gamma/d_beta [64].  d_ws needs sg_mlp1_ws_bytes(C).
 * ------------------------------------------------------------------------------------------- */
size_t sg_mlp1_ws_bytes(int C);
int sg_mlp1_forward(const float* d_samples, int C, const float* d_w, const float* d_gamma, const float* d_beta,
                    float* d_feat, int feat_stride, void* d_ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a8  calculate_distance (model.py:269-274): d[e] = || F[a] - F[b] + 1e-6 ||_2 for every edge.
 * ------------------------------------------------------------------------------------------- */
int sg_edge_distance(const float* d_feat, int feat_stride, int D, const int32_t* d_adj, int E,
                     float* d_dist, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a10  aggregate_cluster_feature (model.py:278-288): out[g] = element-wise max of rows[idx] over
 * group g (CSR d_goff[G+1], d_gidx).  Columns [0,D) of each output row (stride out_stride).
 * ------------------------------------------------------------------------------------------- */
int sg_group_max_rows(const float* d_rows, int row_stride, int D, const int32_t* d_goff, const int32_t* d_gidx,
                      int G, float* d_out, int out_stride, void* stream);

/* a10 point->cluster max (model.py:793,834): rows are in member order, i.e. clusters are contiguous ranges and
 * d_cluster_of_pos is non-decreasing along the rows (sg_gather_members produces exactly that).  Only D == 64.  Columns [0,64) of
 * every one of the C output rows are written: a cluster without a row stays -inf.  The maximum is by VALUE over arbitrary rows
 * (infinities, subnormals and both zeros included): the float max is an integer atomic on the bits, split on the value's sign
 * bit, so -0.0 orders above every negative and below +0.0; a cluster holding both zeros returns either. */
int sg_segment_max(const float* d_rows, int N, int D, const int32_t* d_cluster_of_pos,
                   float* d_out, int out_stride, int C, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a12  combine_centralized_pointcloud (model.py:429-436), written in MEMBER order:
 *   d_x9m [N,12]  = [XYZ, RGB, XYZ - mean XYZ of the point's cluster, 0,0,0]   (row pos)
 *   d_xyzw [N,4]  = [X, Y, Z, fl(fl(X2+Y2)+Z2)]                              (kNN operand)
 * d_tile_cl / d_tile_lo / d_tile_hi describe T tiles (<=256 consecutive positions of one cluster),
 * d_cl_tile_off[C+1] the tiles of each cluster (from sg_partition_layer); the two-level sum keeps
 * the mean bit-reproducible.  d_ws needs sg_center_ws_bytes(T, C).
 * ------------------------------------------------------------------------------------------- */
size_t sg_center_ws_bytes(int T, int C);
int sg_center_clusters(const float* d_data, int N, const int32_t* d_members, const int32_t* d_cl_off, int C,
                       const int32_t* d_tile_cl, const int32_t* d_tile_lo, const int32_t* d_tile_hi, int T,
                       const int32_t* d_cl_tile_off, float* d_x9m, float* d_xyzw,
                       void* d_ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a6+a11  get_knn (model.py:512-522) with knn (model.py:30-36), k = 20, in member-order positions.
 * Scores are evaluated in the reference's exact fp32 order:
 *   s_ij = ((-xx_j) - (-2 * fma(z_i,z_j, fma(y_i,y_j, fl(x_i*x_j))))) - xx_i
 * Clusters with n <= k list all members in member order and leave the remaining columns pointing at
 * GLOBAL POINT 0 (position pos0) -- the zero-initialised table quirk of model.py:513.
 * d_knn [N,k] int32 positions, row = query position, descending score.
 * ------------------------------------------------------------------------------------------- */
int sg_cluster_knn(const float* d_xyzw, int N, const int32_t* d_cl_off,
                   const int32_t* d_tile_cl, const int32_t* d_tile_lo, const int32_t* d_tile_hi, int T,
                   int k, int pos0, int32_t* d_knn, void* stream);

/* Same result as sg_cluster_knn (bit-identical tables, ties included), with whole over-segments skipped
 * when their bounding box proves that none of their points can enter any lane's top-k.  Tiles for THIS
 * entry point hold <= 64 positions (one workgroup = 64 queries x 4 candidate slices):
 *   d_segbox [S,8]   = {min xyz, max xyz, max |p|^2, 0} per ORIGINAL segment (sg_segment_boxes, once per scene)
 *   d_cl_seg_off[C+1], d_order[S], d_dst[S] : the layer's ordered segment lists (sg_partition_layer)
 *   d_seg_off[S+1]   : CSR offsets of the original segmentation (segment sizes)
 *   d_slot_of_pos[N] : from sg_gather_members (each wave scans its own segment first)                  */
int sg_segment_boxes(const float* d_data, const int32_t* d_seg_points, const int32_t* d_seg_off, int S,
                     float* d_box, void* stream);
int sg_cluster_knn_pruned(const float* d_xyzw, int N, const int32_t* d_cl_off,
                          const int32_t* d_tile_cl, const int32_t* d_tile_lo, const int32_t* d_tile_hi, int T,
                          const int32_t* d_cl_seg_off, const int32_t* d_order, const int32_t* d_dst,
                          const int32_t* d_seg_off, const float* d_segbox, const int32_t* d_slot_of_pos,
                          int k, int pos0, int32_t* d_knn, void* stream);

/* Fastest variant (same tables again).  Once per scene sg_segment_sort_boxes puts the points of every original
 * segment in Morton order (d_sperm[N]: sorted position -> index into d_seg_points; key = 30-bit Morton code inside the
 * segment's box, ties by CSR index) and boxes every run of 32 sorted points (d_chunk_box [(sum_s ceil(size_s/32)), 8];
 * d_seg_chunk_off[S+1] = first chunk of each segment, computed by the caller from the segment sizes).  Per layer
 * sg_knn_operands lays the kNN operand out in that order (d_sxyzw [N,4], d_smpos [N] = member position of each sorted
 * position) and sg_cluster_knn_sorted scans only chunks whose box can still beat a lane's 20th best.  Tiles hold <= 64
 * SORTED positions of one cluster (same ranges as member order: sorting only permutes inside a segment).
 * One launch (a block per segment: box, LDS bitonic sort, chunk boxes) when the largest segment (max_seg points, known
 * to the host) fits a block's LDS (2048 points); segments beyond that take a second launch that buckets by the top 12
 * Morton bits in d_ws (sg_segment_sort_ws_bytes(N) = 16 N bytes; unused otherwise) and sorts every run of cells in LDS.
 * Outputs: d_segbox [S,8], d_sperm [N], d_chunk_box.  d_seg_sums (may be NULL): [S,3] double, the sum of every
 * segment's xyz -- layer-invariant, so the host can form any cluster's centroid from it.
 * Segments of at most 256 points take a launch of their own in front of it: one wave per segment, four segments per block, box / keys /
 * bitonic network / chunk boxes in registers (same outputs, same bits); the block launch is skipped when max_seg says that no larger
 * segment exists.  sg_segment_sort_set_wave_max(64 | 128 | 256) sets that size for the whole PROCESS (this call and the scene engine),
 * 0 sends every segment through the block kernel: a knob of the tests and of A/B timing, not part of the interface.  SG_EINVAL for
 * any other value.  sg_segment_sort_get_wave_max returns the setting in force. */
size_t sg_segment_sort_ws_bytes(int N);
int sg_segment_sort_set_wave_max(int wave_max);
int sg_segment_sort_get_wave_max(void);
int sg_segment_sort_boxes(const float* d_data, int N, const int32_t* d_seg_points, const int32_t* d_seg_off,
                          const int32_t* d_seg_of_point, int S, const int32_t* d_seg_chunk_off, int max_seg, float* d_segbox,
                          int32_t* d_sperm, float* d_chunk_box, double* d_seg_sums, void* d_ws, size_t ws_bytes, void* stream);
/* One launch for what sg_gather_members + sg_center_clusters + sg_knn_operands produce for a layer (same arrays, same
 * bits): d_cl[i] = cluster of the i-th segment in member order, d_cl_mean [C,3] = the clusters' centroids as fp32
 * (= (float)(sum of the members' xyz in double / count), e.g. from sg_segment_sort_boxes' d_seg_sums).
 * d_point_rec (may be NULL): [N,4] = {x, y, z, bits of the point's member position in this layer}: the 16-byte record
 * sg_cluster_knn_seeded gathers per seed (instead of a row of d_data and an entry of d_pos_of_point).
 * d_seed_id (may be NULL): [N] by member position = the point's SEED ID, its place in the Morton-sorted CSR of the
 * over-segmentation (d_seg_off[s] + rank inside segment s): the same in every layer, consecutive for the queries of a kNN tile,
 * close for points that are close in space.  With d_seed_id the records are indexed by seed id (written in order), without by
 * point id.  Seed tables may use either id space -- whatever map the caller hands to sg_knn_seed_points / sg_cluster_knn_seeded.
 * d_range_bits (may be NULL): SG_RANGE_WORDS words, atomically raised to the bits of the largest |centred coordinate| / |feature| laid out
 * (the atomics are spread over the words; the range is their maximum, and 2 * range bounds every edge difference of the layer): the scale
 * sg_edgeconv_forward_r cuts conv1's operand with. */
int sg_layer_layout(const float* d_data, int N, const int32_t* d_seg_points, const int32_t* d_seg_off, const int32_t* d_sperm, int S,
                    const int32_t* d_order, const int32_t* d_dst, const int32_t* d_cl, const float* d_cl_mean, int32_t* d_members,
                    int32_t* d_pos_of_point, int32_t* d_cluster_of_pos, int32_t* d_slot_of_pos, float* d_x9m, float* d_sxyzw,
                    int32_t* d_smpos, float* d_point_rec, int32_t* d_seed_id, unsigned int* d_range_bits, void* stream);
int sg_knn_operands(const float* d_data, const int32_t* d_seg_points, const int32_t* d_seg_off, const int32_t* d_sperm, int S,
                    const int32_t* d_order, const int32_t* d_dst, float* d_sxyzw, int32_t* d_smpos, void* stream);
int sg_cluster_knn_sorted(const float* d_sxyzw, const int32_t* d_smpos, int N, const int32_t* d_cl_off,
                          const int32_t* d_tile_cl, const int32_t* d_tile_lo, const int32_t* d_tile_hi, int T,
                          const int32_t* d_cl_seg_off, const int32_t* d_order, const int32_t* d_dst,
                          const int32_t* d_seg_off, const int32_t* d_seg_chunk_off, const float* d_segbox,
                          const float* d_chunk_box, const int32_t* d_slot_of_pos, int k, int pos0, int32_t* d_knn, void* stream);
/* Seeded variant for a layer whose clusters are unions of the clusters of the PREVIOUS kNN layer (model.py:829 after
 * 788: the score of a pair depends on raw coordinates only and union() appends whole member lists, so a query's
 * previous list is the exact top k inside its former cluster).  sg_knn_seed_points turns the previous table (rows and
 * entries = member positions of that layer, d_members = its position -> id map: point ids (sg_layer_layout's d_members)
 * or seed ids (its d_seed_id: what the pipeline and the engine pass)) into d_seed [N,k] indexed by and holding those ids.
 * sg_cluster_knn_seeded = sg_cluster_knn_sorted with one wave per tile that starts every query from its seeds (d_members:
 * THIS layer's position -> id map in the same id space, d_point_rec: sg_layer_layout's records of THIS layer by id) and skips the chunks of
 * segments whose former cluster (d_seg_prevcl[S]) is the query's own; d_seg_prevcl = -1 marks segments of former
 * clusters with <= k points, which have no kNN list (model.py:516-518).  Same table as every other variant. */
int sg_knn_seed_points(const int32_t* d_knn, const int32_t* d_members, int N, int k, int32_t* d_seed, void* stream);
int sg_cluster_knn_seeded(const float* d_sxyzw, const int32_t* d_smpos, int N, const int32_t* d_cl_off,
                          const int32_t* d_tile_cl, const int32_t* d_tile_lo, const int32_t* d_tile_hi, int T,
                          const int32_t* d_cl_seg_off, const int32_t* d_order, const int32_t* d_dst,
                          const int32_t* d_seg_off, const int32_t* d_seg_chunk_off, const float* d_segbox,
                          const float* d_chunk_box, const int32_t* d_slot_of_pos, const int32_t* d_seed,
                          const int32_t* d_seg_prevcl, const int32_t* d_members, const float* d_point_rec,
                          int k, int pos0, int32_t* d_knn, void* stream);

/* Two-pass kernel over a cluster-ordered chunk table (same tables once more; variant 0 of sg_pipeline_set_knn_variant:
 * faster on 500k-point scenes and on large segments, on par with the one-pass kernel at 150k / 1.5k).  Per layer the host provides d_slot_chunk0[S+1] (exclusive prefix, in cluster slot order, of the
 * 32-point chunk counts of the segments d_order[slot]), d_cl_chunk_off[C+1] (= slot_chunk0 at each cluster's first
 * slot) and d_tile_chunk0[T] (cluster-relative number of the chunk holding the tile's first sorted position).
 * sg_knn_chunk_table writes d_cc [(slot_chunk0[S]), 8]: {box min xyz, box max xyz, max |p|^2, bits: first sorted
 * position << 6 | points - 1} of every chunk in that order (needs N < 2^25).  sg_cluster_knn_2pass: pass 1 keeps the
 * k best SCORES per query (one v_med3_f32 per list slot), pass 2 rescans with that floor and inserts only the ~k
 * survivors as exact (score, index) keys; 64 chunk boxes are tested per coalesced load and the next surviving
 * chunk's operands are prefetched while the current one is scanned. */
int sg_knn_chunk_table(const int32_t* d_order, const int32_t* d_dst, const int32_t* d_seg_off, const int32_t* d_seg_chunk_off,
                       const float* d_chunk_box, int S, const int32_t* d_slot_chunk0, float* d_cc, void* stream);
int sg_cluster_knn_2pass(const float* d_sxyzw, const int32_t* d_smpos, int N, const int32_t* d_cl_off,
                         const int32_t* d_tile_cl, const int32_t* d_tile_lo, const int32_t* d_tile_hi,
                         const int32_t* d_tile_chunk0, int T, const int32_t* d_cl_chunk_off, const float* d_cc,
                         int k, int pos0, int32_t* d_knn, void* stream);
/* sg_cluster_knn_sorted with an explicit number of waves per 64-query tile (1, 2 or 4; anything else = by tile count:
 * 1 when T >= 2048 tiles fill the GPU, else 2 or 4).  More waves shorten a tile's critical path, but every wave warms
 * up its own top-k list.  Same table for every choice (the GPU tests compare them). */
int sg_cluster_knn_sorted_w(const float* d_sxyzw, const int32_t* d_smpos, int N, const int32_t* d_cl_off,
                            const int32_t* d_tile_cl, const int32_t* d_tile_lo, const int32_t* d_tile_hi, int T,
                            const int32_t* d_cl_seg_off, const int32_t* d_order, const int32_t* d_dst,
                            const int32_t* d_seg_off, const int32_t* d_seg_chunk_off, const float* d_segbox,
                            const float* d_chunk_box, const int32_t* d_slot_of_pos, int k, int pos0, int waves_per_tile,
                            int32_t* d_knn, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a13  get_graph_feature2 + MLP2 / MLP3 (model.py:83-138): edge features [x_j - x_i, x_i] over the
 * k=20 table, conv1x1 18->64 (+ conv1x1 64->64 for layers == 2), BatchNorm2d with batch statistics
 * over all N*k rows, LeakyReLU(0.2), max over k.  fp32 MFMA (v_mfma_f32_32x32x2_f32).
 * d_out [N,64] in member order.  d_w2/d_g2/d_b2 are ignored when layers == 1.
 * d_ws needs sg_edgeconv_ws_bytes(N).
 * ------------------------------------------------------------------------------------------- */
size_t sg_edgeconv_ws_bytes(int N);
int sg_edgeconv_forward(const float* d_x9m, const int32_t* d_knn, int N, int k, int layers,
                        const float* d_w1, const float* d_g1, const float* d_b1,
                        const float* d_w2, const float* d_g2, const float* d_b2,
                        float* d_out, void* d_ws, size_t ws_bytes, void* stream);
/* The same with conv1's operand on fp16 pieces scaled by the layer's range (4 instead of 8 MFMAs per neighbour slot, same accuracy: the
 * pieces keep 22 bits and the scale is a power of two).  d_range_bits: a ZERO-INITIALISED buffer of SG_RANGE_WORDS (256) words whose
 * maximum is the bits of a float R with |x_j - x_i| <= 2 R for every edge and channel -- sg_layer_layout raises them while it writes
 * d_x9m, sg_edge_range computes one from d_x9m alone (max |x9m[p][c] - x9m[0][c]|; the words must be 0 or smaller bounds before).
 * BOTH layer counts use the range: MLP2 scales conv1's operand with it, MLP3's fold kernel reads it to choose the scale of conv1' and
 * writes the fp16 weight image accordingly.  Every kernel involved reads or clears all SG_RANGE_WORDS words (a smaller buffer is read
 * and written out of bounds); the op clears them when it is done.  NULL = sg_edgeconv_forward (bf16 pieces, no range needed).
 * With k == 20 the neighbour-slot loop runs as a hand-scheduled gfx950 instruction stream (csrc/edgeconv_slots_gen.h); other k take
 * the compiler-scheduled loop.  Both compute the same bits. */
int sg_edgeconv_forward_r(const float* d_x9m, const int32_t* d_knn, int N, int k, int layers, const float* d_w1, const float* d_g1,
                          const float* d_b1, const float* d_w2, const float* d_g2, const float* d_b2, float* d_out, void* d_ws,
                          size_t ws_bytes, unsigned int* d_range_bits, void* stream);
/* sg_edgeconv_forward_r with flags: SG_EDGECONV_COMPILER_LOOP forces the compiler-scheduled slot loop also for k == 20 (the
 * cross-check of the hand-scheduled one: tests compare the two bit for bit). */
#define SG_EDGECONV_COMPILER_LOOP 1u
int sg_edgeconv_forward_x(const float* d_x9m, const int32_t* d_knn, int N, int k, int layers, const float* d_w1, const float* d_g1,
                          const float* d_b1, const float* d_w2, const float* d_g2, const float* d_b2, float* d_out, void* d_ws,
                          size_t ws_bytes, unsigned int* d_range_bits, unsigned int flags, void* stream);
int sg_edge_range(const float* d_x9m, int N, unsigned int* d_range_bits, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a14  calculate_similarity + build_similarity_matrix + GCN (model.py:262-265,305-309,141-151):
 * out = relu( ((I + sym(exp(-alpha*d))) row-normalised) @ X @ W^T ), evaluated sparsely over the
 * symmetric CSR (d_rowptr[S+1], d_col, d_eid -> index into the edge list) built by the host.
 * d_ws needs sg_gcn_ws_bytes(S, D, E).
 * ------------------------------------------------------------------------------------------- */
size_t sg_gcn_ws_bytes(int S, int D, int E);
int sg_gcn_forward(const float* d_x, int S, int D, const int32_t* d_adj, int E,
                   const int32_t* d_rowptr, const int32_t* d_col, const int32_t* d_eid,
                   const float* d_w, float alpha, float* d_out, void* d_ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a16  export_{segment,instance,semantic}_label (model.py:525-605), gather only:
 *   out[t][v] = tables[t][ seg_of_point[ unmap[v] ] ]      t < T label vectors, v < V raw vertices
 * d_tables [T,S] int32 holds each original segment's exported value for that vector.
 * ------------------------------------------------------------------------------------------- */
int sg_export_labels(const int32_t* d_unmap, int V, const int32_t* d_seg_of_point, int N,
                     const int32_t* d_tables, int T, int S, int32_t* d_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a17  evaluate (model.py:608-655): integer counts on the device, ratios on the host.
 * d_gt [V,2] int32 (sem, ins), predictions int32 [V].  Writes the three reference return values
 * to HOST buffers h_iou_sem[2*40], h_iou_ins[2*40], h_acc[4]; SYNCHRONISES the stream.
 * max_ins = upper bound (exclusive) of predicted instance ids.  d_ws needs sg_eval_ws_bytes(max_ins).
 * ------------------------------------------------------------------------------------------- */
size_t sg_eval_ws_bytes(int max_ins);
int sg_evaluate(const int32_t* d_gt, const int32_t* d_sem_pred, const int32_t* d_ins_pred, int V, int max_ins,
                float* h_iou_sem, float* h_iou_ins, float* h_acc, void* d_ws, size_t ws_bytes, void* stream);

/* =============================================================================================
 * Host-side grouping engine (a2, a3 later calls, a9, a10 re-index, a15): the serial, order-dependent
 * core of the reference, restated over SEGMENT-level arrays (S <= a few thousand), plain C++.
 * ============================================================================================= */
typedef struct sg_partition sg_partition;

/* DisjointSet + graph initialisation (model.py:169-214,712-721).  seg_first[s] = index of the first
 * point of segment s (strictly ascending), seg_size[s] its point count, seg_ins/seg_sem the weak
 * labels of that first point (-1 = unlabeled). */
sg_partition* sg_partition_create(int S, const int32_t* h_seg_first, const int32_t* h_seg_size,
                                  const int32_t* h_seg_ins, const int32_t* h_seg_sem);
void sg_partition_destroy(sg_partition* p);
int  sg_partition_num_clusters(const sg_partition* p);

/* DisjointSet.union(id1,id2) on cluster roots given as SEGMENT numbers (model.py:181-192);
 * returns 1 if points moved, 0 if no-op / vetoed. */
int sg_partition_union(sg_partition* p, int seg_root1, int seg_root2);
/* find(): root segment of the cluster that currently owns segment s (model.py:178-179) */
int sg_partition_find(const sg_partition* p, int s);
/* current weak labels / point count of the cluster rooted at segment r (stale for dead roots) */
int sg_partition_label(const sg_partition* p, int r, int32_t* ins, int32_t* sem, double* npts);

/* Freeze the current numbering (get_cluster_list order, model.py:209-214; re-index blocks 759-768):
 *   h_root[C]        root segment of cluster c (ascending)
 *   h_cl_of_seg[S]   cluster number of every original segment
 *   h_order[S]       original segments in cluster-concatenated (member) order
 *   h_cl_seg_off[C+1] range of h_order belonging to cluster c
 *   h_cl_pt_off[C+1]  range of member positions (points) belonging to cluster c
 *   h_dst[S]         point offset of h_order[i] in the member array
 * returns C, or a negative error. */
int sg_partition_layer(const sg_partition* p, int32_t* h_root, int32_t* h_cl_of_seg, int32_t* h_order,
                       int32_t* h_cl_seg_off, int32_t* h_cl_pt_off, int32_t* h_dst);

/* group_nearby_clusters (model.py:218-258).  adj rows index the layer frozen in h_root (C clusters).
 * h_connected[E] receives 1 for edges whose endpoints ended in one cluster.  Returns 0, or SG_ESTALL
 * when the reference's pass 2 would never terminate (the sweep that made no progress is the last). */
int sg_partition_group_nearby(sg_partition* p, const int32_t* h_root, int C, const float* h_dist,
                              const int32_t* h_adj, int E, float th, uint8_t* h_connected);

/* update_adj for layers >= 2 (model.py:291-302): contract the edges with h_keep[e] != 0 (NULL = all)
 * from the numbering h_root_old to the CURRENT partition's numbering; sorted unique rows.
 * Returns the number of rows written (<= E) or a negative error. */
int sg_partition_contract(const sg_partition* p, const int32_t* h_root_old, const int32_t* h_adj, int E,
                          const uint8_t* h_keep, int32_t* h_adj_out);

/* group_unlabeled_clusters, first loop (model.py:447-477): iterated nearest-feature-neighbour merges
 * of unlabeled clusters.  h_feat [C,D] / h_adj [E,2] are updated IN PLACE to the new numbering
 * (feature = max of absorbed rows); *C_io / *E_io likewise.  Returns 1 if an unlabeled cluster
 * remains (the caller must then sample with P=1024 and call ..._fallback), 0 if none. */
int sg_partition_group_unlabeled(sg_partition* p, int32_t* h_root_io, int* C_io, float* h_feat, int D,
                                 int32_t* h_adj, int* E_io);
/* second half (model.py:479-507): h_samples [C,1024,3] fp32 XYZ of every cluster in the numbering
 * left by the call above. */
int sg_partition_unlabeled_fallback(sg_partition* p, const int32_t* h_root, int C, const float* h_samples, int P);

/* Export tables for one layer (model.py:525-605): per ORIGINAL segment the values that
 * export_segment_label / export_instance_label / export_semantic_label write for its points. */
int sg_partition_export_tables(const sg_partition* p, int32_t* h_seg_tab, int32_t* h_ins_tab, int32_t* h_sem_tab);

/* =============================================================================================
 * Whole-scene pipeline: SegModel.forward (model.py:684-897) for one scene on one stream.
 * ============================================================================================= */
typedef struct sg_pipeline sg_pipeline;

typedef struct sg_weights {       /* HOST pointers, float32, row-major (checkpoint contract) */
    const float* mlp1_w;  const float* mlp1_g;  const float* mlp1_b;      /* [64,6]  [64] [64]        */
    const float* mlp2_w;  const float* mlp2_g;  const float* mlp2_b;      /* [64,18] [64] [64]        */
    const float* gcn2_w;                                                  /* [192,192]                */
    const float* mlp3_w1; const float* mlp3_g1; const float* mlp3_b1;     /* [64,18] [64] [64]        */
    const float* mlp3_w2; const float* mlp3_g2; const float* mlp3_b2;     /* [64,64] [64] [64]        */
    const float* gcn3_w;                                                  /* [256,256]                */
} sg_weights;

typedef struct sg_scene {         /* one scene, DEVICE-resident inputs (staged by the loader)          */
    int N, S, E0, V;
    const float*   d_data;          /* [N,6]   <scene>.pcl.pth                 (data.py:34)            */
    const int64_t* d_adj;           /* [E0,2]  <scene>.adj.pth                 (model.py:724)          */
    const int32_t* d_seg_of_point;  /* [N]     segment number per point        (.seg.json, model.py:714)*/
    const int32_t* d_seg_points;    /* [N]     CSR of the .seg.json lists: points ascending per segment */
    const int32_t* d_seg_off;       /* [S+1]                                                            */
    const int32_t* d_unmap;         /* [V]     <scene>.unmap.pth               (model.py:533)          */
    const int32_t* d_gt;            /* [V,2]   label/real/raw .label.pth (sem, ins) (model.py:612)     */
    /* HOST, segment level (derived by the loader from weak_label and the segment lists) */
    const int32_t* h_seg_first;     /* [S] first point of each segment                                 */
    const int32_t* h_seg_size;      /* [S]                                                             */
    const int32_t* h_seg_ins;       /* [S] weak instance label of the first point (weak_label[:,1])   */
    const int32_t* h_seg_sem;       /* [S] weak semantic label of the first point (weak_label[:,0])   */
    /* HOST, optional (NULL = not given): the over-segment of every raw vertex, seg_of_point[unmap[v]] (-1 where unmap[v] is not a
     * point).  Needed by the engine's compact label transfer (sg_engine_set_label_transfer): a label vector is a table look-up
     * through this array, so the look-up can run on the host and only the [14,S] tables have to cross PCIe. */
    const int32_t* h_seg_of_vertex; /* [V]                                                             */
} sg_scene;

typedef struct sg_result {        /* HOST outputs                                                       */
    int32_t* h_labels;              /* [14,V] int32, pinned or pageable; order: layer_1.seg, layer_1.ins,
                                       layer_1.sem, layer_2.*, layer_3.*, layer_4.*, final.ins, final.sem.
                                       sem_infer fills the first 6 and leaves the rest untouched.        */
    float iou_sem[80];              /* [2,40] I then U  (model.py:628)                                   */
    float iou_ins[80];              /* [2,40]           (model.py:640)                                   */
    float acc[4];                   /* model.py:654                                                      */
    int32_t trace[5];               /* cluster counts of layers 1..5                                     */
    int32_t stalled;                /* 1 if a pass-2 sweep was cut short (SG_ESTALL condition)           */
    int32_t used_fallback;          /* 1 if the FPS-1024 fallback of model.py:479-494 ran                */
    int32_t* h_tables;              /* optional [14,S] int32 (NULL = not wanted; sg_pipeline_forward, the engine and the trainer fill it): the label tables the vectors are looked up in,
                                       h_labels[t][v] = s >= 0 ? h_tables[t][s] : -1 with s = h_seg_of_vertex[v] (sg_expand_labels) */
} sg_result;

typedef struct sg_debug {         /* optional taps for stage-level parity tests (every pointer may be NULL) */
    float*   d_samples1;            /* DEVICE [S,64,6]                                                   */
    float*   d_feat1;               /* DEVICE [S,128]                                                    */
    float*   d_pointfeat[2];        /* DEVICE [N,64] MLP2 / MLP3 output, MEMBER order of that layer      */
    int32_t* d_knn[2];              /* DEVICE [N,20] member-order positions                              */
    int32_t* d_members[2];          /* DEVICE [N]    point id at each member-order position              */
    float*   h_gcn[2];              /* HOST [S2,192] / [S3,256]                                          */
    float*   h_dist[3];             /* HOST distance vectors of the three group_nearby calls            */
    int32_t* h_adj[4];              /* HOST adjacency lists adj_1..adj_4 ([E,2])                         */
    int32_t  n_adj[4];              /* rows written to h_adj[i]                                          */
    /* train-mode inputs of the classifier tail (model.py:900-914), ins_infer forward only: */
    float*   h_feat5;               /* HOST [S,256] Feat_5: features of the final clusters                */
    int32_t* h_ins5;                /* HOST [S] weak instance label of every final cluster (-1 = none)    */
    int32_t* h_sem5;                /* HOST [S] weak semantic label of every final cluster                */
    int32_t  n5;                    /* final clusters written                                             */
    void*    tape;                  /* library-internal (sg_trainer): the training step's record of this forward; NULL otherwise */
    float*   d_cat[2];              /* DEVICE [C2,192] / [C3,256] cluster features in front of each GCN: the previous layer's
                                       features grouped (max) | the EdgeConv point features' max per cluster, after its BN + LReLU */
} sg_debug;

sg_pipeline* sg_pipeline_create(int max_points, int max_segments, int max_edges, int max_vertices,
                                const sg_weights* w, void* stream);
void sg_pipeline_destroy(sg_pipeline* pl);
/* device + pinned bytes owned by the pipeline (for capacity planning against 288 GB HBM) */
size_t sg_pipeline_device_bytes(const sg_pipeline* pl);

/* SegModel.forward for one scene.  Blocks the calling thread until the results are in `out`
 * (it synchronises `stream` at each of the 3-5 points where the serial grouping needs distances).
 * Thread-safe across DIFFERENT pipeline objects (one pipeline per in-flight scene). */
int sg_pipeline_forward(sg_pipeline* pl, const sg_scene* scene, int mode, sg_result* out, sg_debug* dbg);

/* Many scenes through `npipes` pipelines: one native host thread per pipeline pulls scenes until all `count` are
 * done (the infer.py:149-152 loop without the interpreter in it).  results[i].h_labels must point at [14,V_i]
 * int32 host buffers, vector v at h_labels + v * V_i (pinned for full D2H speed).  h_stage_ms_sum (may be NULL) accumulates the per-stage device
 * times of every forward (same order as sg_pipeline_stage_name).  Blocks until every scene is done. */
struct sg_writer;   /* asynchronous label-file writer pool, declared below */
/* writer / out_dirs / formats (all optional): after each scene its label vectors are submitted to `writer` as
 * <out_dirs[i]>/<layer_k.seg|ins|sem, final.ins|sem>.{txt,npy} (formats: 1 txt | 2 npy); directories must exist. */
int sg_batch_forward(sg_pipeline* const* pipes, int npipes, const sg_scene* scenes, int count, int mode,
                     sg_result* results, float* h_stage_ms_sum,
                     struct sg_writer* writer, const char* const* out_dirs, int formats);

/* =============================================================================================
 * Scene engine: SegModel.forward for MANY scenes with the scene index as a grid dimension (infer.py:149-152 loop body,
 * model.py:684-897).  `groups` persistent host threads (one HIP stream each) pull up to `scenes_per_group` scenes at a
 * time from a job queue and advance them in lock-step: every kernel is launched ONCE per phase for all scenes of the
 * group (csrc/engine_ctx.h), with one host->device copy, one device->host copy and one stream synchronisation per
 * phase; the serial grouping of a group's scenes runs on its thread while the other groups' kernels occupy the GPU.
 * groups x scenes_per_group scenes are in flight.  Labels, metrics, traces, kNN tables and adjacency lists are bit-identical
 * to sg_pipeline_forward (same kernel bodies; tests/test_gpu_scene.py, tests/test_gpu_engine_taps.py).  So are the float
 * stages (MLP1 features, cluster features, GCN outputs, decision distances) as long as every scene's EdgeConv tile groups
 * (ceil(N / 128)) fit in the launch's per-scene grid, 2 x CUs / scenes in the super-step: each group is then one workgroup's
 * row of BatchNorm partial sums in both paths.  A larger scene in a group of several is walked by fewer workgroups than in
 * sg_pipeline_forward and its fp64 partials are summed in another association: a fold value may then round to a neighbouring
 * float, and the scene's float stages may differ from the single-scene ones in the last bits (the tests bound this by 1e-5;
 * observed: none, at 150k and 2^20 points beside other scenes).
 *
 * sg_engine_submit enqueues `count` scenes and returns a ticket at once (the arrays must stay valid until the ticket
 * has been waited for; results[i].h_labels as for sg_batch_forward); sg_engine_wait blocks until every scene of the
 * ticket is done and returns the first error.  A driver keeps the GPU busy across batches by submitting batch k+1
 * before it waits for batch k.  writer / out_dirs / formats as for sg_batch_forward.
 * ============================================================================================= */
typedef struct sg_engine sg_engine;
sg_engine* sg_engine_create(int max_points, int max_segments, int max_edges, int max_vertices, const sg_weights* w,
                            int groups, int scenes_per_group);
void sg_engine_destroy(sg_engine* e);
int sg_engine_submit(sg_engine* e, const sg_scene* scenes, int count, int mode, sg_result* results,
                     struct sg_writer* writer, const char* const* out_dirs, int formats);
int sg_engine_wait(sg_engine* e, int ticket);
/* sg_engine_submit with stage taps (a test hook): dbg (may be NULL) holds `count` pointers, dbg[i] (may be NULL) receives scene i's
 * taps in the sg_debug layouts: d_samples1, d_feat1, d_knn / d_members, d_cat, h_gcn, h_dist, h_adj / n_adj.  The engine has no
 * per-point features: d_pointfeat, the train-mode tail (h_feat5, h_ins5, h_sem5, n5) and tape are left untouched (tape must be NULL).
 * A tapped group copies the taps behind each phase and waits for them; without taps the launches are those of sg_engine_submit. */
int sg_engine_submit_debug(sg_engine* e, const sg_scene* scenes, int count, int mode, sg_result* results, sg_debug* const* dbg,
                           struct sg_writer* writer, const char* const* out_dirs, int formats);
/* 0 = no stage timing (default), 1 | 2 = HIP events around the stages of every batched launch.  Returns the previous level. */
int sg_engine_set_timing(sg_engine* e, int level);
/* 0 (default): every scene's 14 label vectors are copied to results[i].h_labels (8.4 MB per 150k-vertex scene).  1 = compact: the
 * vectors stay on the device; results[i].h_tables (if given) receives the [14,S] tables, the writer pool is handed tables + the scene's
 * h_seg_of_vertex and expands while it writes, results[i].h_labels is left untouched (may be NULL).  Scenes without h_seg_of_vertex
 * fall back to the full copy.  Returns the previous setting.  (Round 4: at the headline rate the full copy is 24 GB/s of D2H per GPU.) */
int sg_engine_set_label_transfer(sg_engine* e, int compact);
/* sg_pipeline_set_knn_variant for every slot (the two-pass kernel, 0, has no batched twin: the seeded kernel runs instead) */
int sg_engine_set_knn_variant(sg_engine* e, int variant);
/* accumulated device time per stage (ms; a batched launch counts once, whatever the number of scenes in it) since the
 * last reset, in sg_pipeline_stage_name order; returns the number of scenes those launches covered */
long long sg_engine_stage_times(sg_engine* e, double* h_ms_sum, int capacity, int reset);
size_t sg_engine_device_bytes(const sg_engine* e);
/* development aid: wall time of the group threads since the last reset -- out[0] super-steps, [1] scenes, [2] ms inside
 * super-steps, [3] of which blocked in stream synchronisation, [4] ms waiting for work; enable != 0 turns the accounting on */
int sg_engine_profile(sg_engine* e, double* out, int reset, int enable);

/* per-stage device time of the last forward, in milliseconds (HIP events on the pipeline's stream);
 * names via sg_pipeline_stage_name(i), count returned. */
int sg_pipeline_stage_times(const sg_pipeline* pl, float* h_ms, int capacity);
/* How many HIP events a forward records for sg_pipeline_stage_times: 2 (default) one after every stage, 1 only around
 * the in-cluster kNN and the EdgeConv passes (the other stages read 0), 0 none.  With many pipelines in flight the
 * ~25 events of level 2 cost ~6 % of the throughput.  Returns the previous level. */
int sg_pipeline_set_timing(sg_pipeline* pl, int level);
/* Which in-cluster kNN kernel THIS pipeline uses for a layer of T tiles (all variants give the same table; the GPU
 * tests compare them).  Per pipeline: the library keeps no process-wide state.
 *   -1  by tile count (default): 8 when T >= 2048 tiles fill the GPU, else one-pass with 2 or 4 waves per tile
 *    0  two-pass (sg_cluster_knn_2pass)
 *    1 | 2 | 4  one-pass (sg_cluster_knn_sorted_w) with that many waves per 64-query tile
 *    8  one-pass, 1 wave per tile, seeded from the previous kNN layer where there is one (sg_cluster_knn_seeded:
 *       layer 3 starts from layer 2's table)
 * Returns the previous setting. */
int sg_pipeline_set_knn_variant(sg_pipeline* pl, int variant);
const char* sg_pipeline_stage_name(int i);

/* =============================================================================================
 * Output writers (a16 file side, model.py:536-547): one decimal integer per line, '\n' terminated;
 * and the .npy twin (v1.0 header, '<i4', shape (V,)).  Host only.
 * ============================================================================================= */
int sg_write_label_txt(const char* path, const int32_t* h_vec, int V);
int sg_write_label_npy(const char* path, const int32_t* h_vec, int V);

/* Asynchronous writer pool: submit() copies h_vec and returns; `formats` = 1 txt | 2 npy | 3 both, written to
 * <path_without_ext>.txt / .npy by one of `threads` native threads.  At most `max_queue` vectors are pending
 * (submit blocks beyond that).  flush() waits for everything submitted so far and reports the first error. */
/* ---------------------------------------------------------------------------------------------
 * Native scene-pack loader (csrc/loader.cpp; reference data.py:28-38 + the per-forward file reads of model.py:696-724).
 * `threads` workers, each with a pinned staging buffer of `slot_bytes` (>= the largest pack file) and a copy stream; `slots` device blobs
 * of 3 x `slot_bytes` (one allocation) made at creation (nothing allocates per scene): packs written from round 4 on store the [E0,2] adjacency as int32
 * (half the bytes of the reference's int64 rows) and the loader widens it to int64 behind the upload, inside the slot -- sg_scene.d_adj is
 * int64 either way; packs with int64 rows still load.  sg_loader_submit queues a `.sgpack` (seggroup_amd/cache.py) and returns a ticket at once;
 * sg_loader_wait blocks until that pack is resident and fills *out (device arrays inside the slot's blob, the four per-segment host
 * arrays and h_seg_of_vertex owned by the slot), *slot and the scene's name.  The slot belongs to the caller until
 * sg_loader_release(slot): release it when the engine has finished the scene.  A worker takes a job only when a slot is free.
 * Call on the thread / device context the engine uses (the device current at creation is the loader's).
 * ------------------------------------------------------------------------------------------- */
typedef struct sg_loader sg_loader;
sg_loader* sg_loader_create(int threads, int slots, size_t slot_bytes);
/* The same with the device slots sized for packs of at most `max_edges` adjacency rows (slot_bytes + 16 max_edges instead of 3 x slot_bytes;
 * 0 = unknown = sg_loader_create).  A pack with more edges fails its ticket with SG_ENOMEM. */
sg_loader* sg_loader_create_sized(int threads, int slots, size_t slot_bytes, size_t max_edges);
/* At most `uploads_in_flight` workers (default 2; env SG_LOADER_COPIES) are between the start and the end of a pack's host-to-device copy at a
 * time: more bulk copies in flight saturate the copy engines and starve the scene engine's own small transfers (csrc/loader.cpp). */
int  sg_loader_set_copy_limit(sg_loader* l, int uploads_in_flight);
int  sg_loader_submit(sg_loader* l, const char* pack_path);
int  sg_loader_wait(sg_loader* l, int ticket, sg_scene* out, int* slot, char* name, int name_capacity);
int  sg_loader_release(sg_loader* l, int slot);
void sg_loader_destroy(sg_loader* l);

typedef struct sg_writer sg_writer;
sg_writer* sg_writer_create(int threads, int max_queue);
int  sg_writer_submit(sg_writer* w, const char* path_without_ext, const int32_t* h_vec, int V, int formats);
/* A whole scene BY REFERENCE (model.py:533-547: the 14 files of one export directory): h_labels = nvec vectors of V values, stride V,
 * written as <out_dir>/<layer_1.seg ... final.sem>.{txt,npy} by one worker (openat on the directory's descriptor, writev).  Nothing is
 * copied: the buffer must stay untouched until sg_writer_wait_tag(w, tag) or sg_writer_flush returned.  tag >= 0, ascending over time
 * (the engine passes its ticket number); sg_writer_wait_tag blocks until every scene with a tag <= `tag` is on disk. */
int  sg_writer_submit_scene(sg_writer* w, const char* out_dir, const int32_t* h_labels, int V, int nvec, int formats, long long tag);
/* The same scene given as label TABLES [nvec,S] + the over-segment of every vertex [V] (both copied: ~0.7 MB instead of a reference
 * to 8.4 MB of vectors that had to cross PCIe first); the worker expands vector by vector while it formats.  Files byte-identical to
 * sg_writer_submit_scene's. */
int  sg_writer_submit_scene_tables(sg_writer* w, const char* out_dir, const int32_t* h_tables, int S, const int32_t* h_seg_of_vertex, int V,
                                   int nvec, int formats, long long tag);
/* h_out[t][v] = (s >= 0 && s < S) ? h_tables[t][s] : -1, s = h_seg_of_vertex[v]: what k_export computes on the device (model.py:525-605) */
int  sg_expand_labels(const int32_t* h_tables, int nvec, int S, const int32_t* h_seg_of_vertex, int V, int32_t* h_out);
/* The same scene written as ONE compact file, <out_dir>/pseudo_labels.sgl (sg_write_sgl), instead of per-vector files; tables and
 * seg_of_vertex are copied (tag and flush semantics as sg_writer_submit_scene_tables). */
int  sg_writer_submit_scene_sgl(sg_writer* w, const char* out_dir, const int32_t* h_tables, int S, const int32_t* h_seg_of_vertex, int V,
                                int nvec, long long tag);
/* One coloured mesh (label visualisation, below): <path> = head | vertex block | tail, the three pieces BY REFERENCE with the tag / flush
 * semantics of sg_writer_submit_scene (untouched until sg_writer_wait_tag(w, tag) for a tag >= 0, or sg_writer_flush, returned).  The
 * file is written under a temporary name in the same directory and renamed; its directory (the reference's visualize/) is created if
 * it is missing. */
int  sg_writer_submit_ply(sg_writer* w, const char* path, const void* h_head, long long head_bytes, const void* h_vertices,
                          long long vertex_bytes, const void* h_tail, long long tail_bytes, long long tag);
int  sg_writer_wait_tag(sg_writer* w, long long tag);
int  sg_writer_flush(sg_writer* w);
void sg_writer_destroy(sg_writer* w);

/* =============================================================================================
 * Compact pseudo-label file `pseudo_labels.sgl` (one per export directory, results/<exp>/<scene>/<stage>/): the label tables and the
 * over-segment of every raw vertex, from which every label vector is a look-up (sg_expand_labels).  All fields little-endian:
 *   header, 48 bytes:  char magic[8] = "SGLABEL\0" | u32 version (SG_SGL_VERSION) | u32 nvec (14 ins_infer / train, 6 sem_infer) | u32 S |
 *                      u32 V | u32 sov_width (2 when S < 65535, else 4) | u32 0 | u64 payload_bytes (= nvec*S*4 + V*sov_width) |
 *                      u32 CRC-32 of the payload (IEEE 802.3 polynomial, zlib.crc32) | u32 0
 *   payload:           int32 tables [nvec,S] (rows in layer_1.seg ... final.sem order) | seg_of_vertex [V]: uint16 with 0xFFFF = -1
 *                      (sov_width 2) or int32 (sov_width 4)
 * sg_write_sgl writes atomically (a temporary name in the same directory, then renameat over `path`).  The readers treat the file as
 * untrusted: magic, version, every size (64-bit, overflow-checked) against the file's length, the CRC and every seg_of_vertex entry
 * (-1 or < S) are checked; any mismatch is SG_EINVAL.  sg_read_sgl_header: h_info[5] = {version, nvec, S, V, sov_width} (CRC not
 * checked).  sg_read_sgl: h_tables [nvec*S], h_seg_of_vertex [V] widened to int32; capacities in elements.
 * ============================================================================================= */
#define SG_SGL_VERSION 1
#define SG_SGL_HEADER_BYTES 48
int sg_write_sgl(const char* path, const int32_t* h_tables, int nvec, int S, const int32_t* h_seg_of_vertex, int V);
int sg_read_sgl_header(const char* path, int* h_info);
int sg_read_sgl(const char* path, int32_t* h_tables, long long tables_capacity, int32_t* h_seg_of_vertex, long long V_capacity);

/* The label vectors on the device from the compact form (csrc/kernels_sgl.hip): d_out[t][v] = tables[t][s] (s = seg_of_vertex[v] in
 * [0,S)) or -1, t < nvec, as int32 (out_elem_bytes 4) or int64 (8).  d_seg_of_vertex is uint16 with 0xFFFF = -1 (sov_width 2) or int32
 * (4).  The tables are staged in LDS when nvec*S*4 <= 128 KiB.  Enqueue only.
 * _batch: B scenes in one launch (scene = grid.y); d_desc DEVICE [B,5] int64 = {table offset (elements of d_tables), S, seg_of_vertex
 * offset (entries), V, output offset (elements)}: scene b's row t starts at d_out + out_off + t*V.  max_V / max_S bound the batch. */
int sg_expand_labels_device(const int32_t* d_tables, int nvec, int S, const void* d_seg_of_vertex, int sov_width, int V, void* d_out,
                            int out_elem_bytes, void* stream);
int sg_expand_labels_device_batch(int B, const long long* d_desc, int max_V, int max_S, const int32_t* d_tables, int nvec,
                                  const void* d_seg_of_vertex, int sov_width, void* d_out, int out_elem_bytes, void* stream);

/* evaluate (model.py:608-655) of `nlayers` layers of B scenes from their tables, one pass over each scene's vertices: gt[v] and
 * seg_of_vertex[v] are read once and every layer's (ins, sem) prediction is a look-up in its table rows h_layer_rows[2l], [2l+1].  Counts
 * as k_eval_counts (integers: bitwise reproducible), ratios on the host as sg_evaluate forms them, so every float equals sg_evaluate's
 * on the expanded vectors.  h_desc HOST [B,6] int64 = {table offset, S, seg_of_vertex offset, V, gt offset (vertices of d_gt [*,2]
 * int32), max_ins (> every predicted instance id of the scene's layers)}.  Outputs [B, nlayers] x {80, 80, 4}.  SYNCHRONISES the stream.
 * d_ws needs sg_eval_tables_ws_bytes(B, nlayers, h_desc). */
size_t sg_eval_tables_ws_bytes(int B, int nlayers, const long long* h_desc);
int sg_eval_tables(int B, const long long* h_desc, const int32_t* d_tables, int nvec, const void* d_seg_of_vertex, int sov_width,
                   const int32_t* d_gt, int nlayers, const int* h_layer_rows, float* h_iou_sem, float* h_iou_ins, float* h_acc,
                   void* d_ws, size_t ws_bytes, void* stream);

/* =============================================================================================
 * ScanNet instance AP / AP50 / AP25 of pseudo labels (csrc/kernels_ap.hip, csrc/ap.cpp).  Ground-truth id of a vertex:
 * gt_id = sem*1000 + ins where ins > 0, else 0; sem outside 0..40 or ins >= 1000 is SG_EINVAL.  ALL vertices count.
 *
 * sg_ap_contingency: B scenes, h_desc HOST [B,6] int64 as sg_eval_tables' ({-, S, seg_of_vertex offset, V, gt offset, -}; entries 0 and 5
 * are not read).  Per scene: the sorted ground-truth list, G entries (id, count), entry 0 = id 0 (count may be 0); first_vertex [S+1]
 * (lowest vertex of every slot, -1 for none; slot = the vertex's segment, S for a vertex without one); the non-zero cells of the
 * [S+1, G] contingency as (slot, g, count) int32 triples in (slot, g) order.  Outputs are concatenated in scene order:
 * h_counts [B,2] int64 = {G, triples}, h_gt [sum G, 2], h_first_vertex [sum (S+1)], h_triples [sum triples, 3] (at most V per scene;
 * triples_cap in triples).  gt_cap bounds G and sizes the workspace ((S+1) * gt_cap cells per scene): a scene with more ids is
 * SG_ENOMEM with h_counts[.,0] filled, so the caller can size a second call.  flags bit 0: plain per-vertex atomics (no in-wave merge of
 * equal keys; same results, for measurement).  Integer atomics only: the same bytes on every run.  SYNCHRONISES the stream.
 * _vectors: one scene from an instance vector, slot(v) = d_ins[v] (values <= 0 -> slot 0), S = the largest value (a larger one is
 * SG_EINVAL); its workspace is sg_ap_contingency_ws_bytes(1, {0, S, 0, V, 0, 0}, gt_cap).
 *
 * sg_ap_fold (host): one layer's match record from a scene's triples and that layer's table rows h_ins_row / h_sem_row [n_row]
 * (n_slots = n_row + 1: the last slot has no label; n_slots = n_row: the vector form, ins_row[slot] = slot, sem_row[slot] = the sem
 * value at first_vertex[slot]).  Predicted instances = distinct ins values > 0 in ascending order (mask order); label = sem at the lowest
 * vertex; kept when the label is one of the 18 benchmark classes and the instance has >= 100 vertices.
 *   h_pred  [P,6] = {mask index, ins value, label id, vertex count, void intersection, matches}      h_n[3] = {P, M, Gv}
 *   h_match [M,2] = {ground-truth record, intersection}, per prediction in ascending ground-truth id, same class only
 *   h_gtrec [Gv,3] = {gt_id, class id, vertex count} of the ground-truth instances of the 18 classes, ascending gt_id
 * sg_ap_match (host): greedy matching of a record (ScanNet's evaluate_semantic_instance) at n_overlaps thresholds; h_conf [P] or NULL
 * (1.0).  Pairs of (class c, overlap o) are h_y_true / h_y_score [h_y_off[c*n+o], h_y_off[c*n+o+1]); h_info [18*n, 3] = {hard false
 * negatives, has_gt, has_pred}.  y_cap >= n_overlaps * (Gv + M + P) always suffices.
 * ============================================================================================= */
size_t sg_ap_contingency_ws_bytes(int B, const long long* h_desc, int gt_cap);
int sg_ap_contingency(int B, const long long* h_desc, const void* d_seg_of_vertex, int sov_width, const int32_t* d_gt, int gt_cap, int flags,
                      long long* h_counts, int32_t* h_gt, int32_t* h_first_vertex, int32_t* h_triples, long long triples_cap, void* d_ws,
                      size_t ws_bytes, void* stream);
int sg_ap_contingency_vectors(const int32_t* d_ins, int V, int S, const int32_t* d_gt, int gt_cap, int flags, long long* h_counts, int32_t* h_gt,
                              int32_t* h_first_vertex, int32_t* h_triples, long long triples_cap, void* d_ws, size_t ws_bytes, void* stream);
int sg_ap_fold(const int32_t* h_triples, long long T, const int32_t* h_first_vertex, int n_slots, const int32_t* h_gt, int G,
               const int32_t* h_ins_row, const int32_t* h_sem_row, int n_row, int32_t* h_pred, long long pred_cap, int32_t* h_match,
               long long match_cap, int32_t* h_gtrec, long long gtrec_cap, long long* h_n);
int sg_ap_match(const int32_t* h_pred, long long P, const int32_t* h_match, long long M, const int32_t* h_gtrec, long long Gv,
                const double* h_conf, const double* h_overlaps, int n_overlaps, double* h_y_score, uint8_t* h_y_true, long long y_cap,
                long long* h_y_off, int32_t* h_info);

/* =============================================================================================
 * Label visualisation (reference seggroup/dataset/scannet/util.py:431-527: visualize_labels, visualize_grouping_process; csrc/
 * kernels_visualize.hip, csrc/visualize.cpp).  A vertex takes one of 41 palette colours (index 0 white, 1..40 ScanNet's class colours)
 * chosen by its label; the coloured mesh is the source PLY with the red / green / blue byte of every vertex record replaced.  Colours travel
 * as one-byte palette INDICES until the record kernel writes them.
 *   semantic  -1, 0 -> white; l -> colour l (1..40; anything else is SG_EINVAL, the reference raises IndexError)
 *   instance  -1, 0 -> white; white where the semantic label is 1 or 2 (if one is given); l -> colour (l - 1) mod 40 + 1
 *   segment   -1 -> white; l -> colour rank mod 40 + 1, rank = position of l among the ascending distinct values that OCCUR among the
 *             vertices (an occurring -1 counts as rank 0); with shuffled positions h_perm: colour h_perm[rank] mod 40 + 1
 *   grouping  (vector form only; second = the segment labels) ins != -1 -> colour (rank - 1) mod 40 + 1, otherwise (seg * mult) mod 40 + 1
 * Two calls per form: *_unique sorts the occurring values (radix sort + adjacent-unique, integer work only), keeps them in the workspace
 * and returns their number, the length over which the caller draws the reference's shuffle; *_apply forms the colours.  Both SYNCHRONISE
 * the stream; the workspace must stay untouched between them.
 * ============================================================================================= */
#define SG_NUM_COLOURS 40
#define SG_COLOUR_MAX_ROWS 16   /* rows of one table-form call / of one record launch */
#define SG_COLOUR_SEMANTIC 0
#define SG_COLOUR_INSTANCE 1
#define SG_COLOUR_SEGMENT 2
#define SG_COLOUR_GROUPING 3

/* Table form: d_tables [nvec,S] + d_seg_of_vertex [V] (sov_width 2: uint16 with 0xFFFF = -1, or 4: int32), h_types [nvec] = SG_COLOUR_*.
 * _unique: h_counts [nvec] = distinct occurring values of every segment row (0 for the others).  _apply: d_cidx [nvec, S+1] palette
 * indices, slot S = a vertex without a segment; h_sem_rows [nvec] (may be NULL) = per instance row the semantic row that whitens it, or -1;
 * h_perm / h_perm_off [nvec] (may be NULL): row r's shuffled positions start at h_perm[h_perm_off[r]] (h_counts[r] of them), -1 = none. */
size_t sg_colour_tables_ws_bytes(int S);
int sg_colour_tables_unique(const int32_t* d_tables, int nvec, int S, const void* d_seg_of_vertex, int sov_width, int V, const int* h_types,
                            int* h_counts, void* d_ws, size_t ws_bytes, void* stream);
int sg_colour_tables_apply(const int32_t* d_tables, int nvec, int S, const int* h_types, const int* h_sem_rows, const int* h_counts,
                           const int32_t* h_perm, const long long* h_perm_off, uint8_t* d_cidx, void* d_ws, size_t ws_bytes, void* stream);

/* Vector form: d_labels [V] int32 of one type.  d_second [V] (instance: the semantic labels, may be NULL; grouping: the segment labels). */
size_t sg_colour_vector_ws_bytes(int V);
int sg_colour_vector_unique(const int32_t* d_labels, int V, int type, int* h_count, void* d_ws, size_t ws_bytes, void* stream);
int sg_colour_vector_apply(const int32_t* d_labels, int V, int type, const int32_t* d_second, int count, const int32_t* h_perm, int mult,
                           uint8_t* d_cidx, void* d_ws, size_t ws_bytes, void* stream);

/* The per-vertex hot path: for every requested row r a complete vertex block d_out[r] = [V, stride] bytes, equal to d_src with the bytes at
 * off_r / off_g / off_b of every record replaced by the row's colour of that vertex -- ONE launch for all rows (the source record and
 * seg_of_vertex[v] are read once).  Table form: d_cidx [*, ld] with ld >= S + 1, vertex v reads d_cidx[h_rows[r] * ld + slot(v)].  Vector
 * form (d_seg_of_vertex NULL): ld >= V, vertex v reads d_cidx[h_rows[r] * ld + v].  A 16-byte record with the colour in its last word
 * (ScanNet's float x, y, z; uchar r, g, b, a) takes a path of 16-byte loads and stores when d_src / d_out are 16-byte aligned.
 * _batch: B scenes in one launch (scene = grid.y); d_desc DEVICE [B,7] int64 = {source offset (bytes), V, seg_of_vertex offset (entries), S,
 * d_cidx offset (bytes), ld, output offset (bytes)}; scene b's row r starts at d_out + out_off + r * V * stride.  For the 16-byte path the
 * source and output offsets must be multiples of 16.  No synchronisation. */
int sg_ply_vertex_records_device(const void* d_src, int V, int stride, int off_r, int off_g, int off_b, const void* d_seg_of_vertex, int sov_width,
                                 int S, const uint8_t* d_cidx, long long ld, int nrows, const int* h_rows, void* d_out, void* stream);
int sg_ply_vertex_records_device_batch(int B, const long long* d_desc, int max_V, int max_S, const void* d_src, int stride, int off_r, int off_g,
                                       int off_b, const void* d_seg_of_vertex, int sov_width, const uint8_t* d_cidx, int nrows, const int* h_rows,
                                       void* d_out, void* stream);

/* Plan of a binary_little_endian PLY file (untrusted: every size in 64-bit arithmetic against the file's length).  h_plan [SG_PLY_PLAN_WORDS]
 * = {offset of the vertex block, V, bytes per vertex, offset of red, green, blue inside a vertex, offset of what follows the vertex block,
 * its length, the file's length, length of the header text}.  SG_EINVAL for ASCII / big-endian files, a truncated header, a vertex
 * element with a list property, missing or non-uchar colour properties, more than SG_MAX_POINTS vertices, a vertex block beyond the file. */
#define SG_PLY_PLAN_WORDS 10
int sg_ply_plan(const char* path, long long* h_plan);

/* visualize_labels' adj_path step (util.py:445-454) over a CSR of the symmetric adjacency: every vertex that carries a label (!= -1) when
 * the call starts hands, in ascending vertex order, the value it holds at its turn to all of its neighbours -- order-dependent, exactly
 * the reference's result, in O(V + E) instead of a dense [V,V] matrix.  In place. */
int sg_dilate_labels(int32_t* h_labels, int V, const long long* h_indptr, const int32_t* h_indices);

/* =============================================================================================
 * Raw scan -> hot-path inputs (reference seggroup/dataset/scannet/util.py).  The compute parts
 * of the reference's offline pre-processing; file formats stay on the Python side (seggroup_amd/prepare.py).
 * Index types follow the reference's tensors: mapper / unmapper / adjacency are int64 (LongTensor), the raw
 * inputs (PLY faces, segIndices) int32.  Every function synchronises the stream before it returns host counts.
 * ============================================================================================= */

/* get_unmapper (util.py:538-550, cal_pairwise_distance 530-535): d_idx[u] = argmax_j ((-|x_u|^2) - (-2 x_u.y_j)) - |y_j|^2
 * in the reference's fp32 operation order, lowest j among equal maxima.  d_x [U,3]; d_y rows of `y_stride` floats
 * (>= 3: xyz first).  Brute force: U*N pair evaluations. */
size_t sg_nearest_point_ws_bytes(int N);
int sg_nearest_point(const float* d_x, int U, const float* d_y, int y_stride, int N, int64_t* d_idx,
                     void* d_ws, size_t ws_bytes, void* stream);

/* generate_pointcloud_pth (util.py:633-693) without the file I/O and the random draw: given the mapper (which
 * raw vertex every sampled point copies), d_pcl [Np,6] = [xyz, rgb / 127.5 - 1 (evaluated in double, stored fp32)]
 * and d_unmap [V] = the LAST sampled point that copies the vertex (687-689) or, for a vertex that was not sampled,
 * its nearest sampled point (sg_nearest_point against d_pcl).  *h_unsampled = number of such vertices. */
size_t sg_prep_sample_ws_bytes(int V, int Np);
int sg_prep_sample_points(const float* d_xyz, const uint8_t* d_rgb, int V, const int64_t* d_mapper, int Np,
                          float* d_pcl, int64_t* d_unmap, int* h_unsampled, void* d_ws, size_t ws_bytes, void* stream);

/* get_adj_from_pointcloud (dataset/scannet/util.py:814-834; optional in the reference -- nothing calls it): the k nearest
 * neighbours of every point against the whole cloud in cal_pairwise_distance's exact fp32 formula (the best-scoring entry of
 * topk(k + 1), normally the point itself, is dropped), as per-row sorted, lexicographically sorted, unique [*, 2] int64 rows.
 * d_points rows of `stride` floats, xyz first; k in {5, 10, 20}; d_adj needs room for [N*k,2]; *h_n = rows written.
 * Equal scores: the lower index ranks first (torch.topk leaves that order unspecified). */
size_t sg_pointcloud_adjacency_ws_bytes(int N, int k);
int sg_pointcloud_adjacency(const float* d_points, int stride, int N, int k, int64_t* d_adj, int* h_n, void* d_ws, size_t ws_bytes, void* stream);

/* get_adj_from_mesh (util.py:771-792).  d_faces [F,3]: edges (0,1), (0,2), (1,2) of every face, zero-length ones
 * dropped (783); d_adj_raw = ascending ids per row, unique rows in lexicographic order; d_adj_res (may be NULL)
 * = the same rows mapped through d_unmap first (rows that collapse to (a, a) only then are kept, as in the
 * reference).  Both need room for [3F,2] int64; the row counts come back in *h_n_raw / *h_n_res. */
size_t sg_mesh_adjacency_ws_bytes(int F);
int sg_mesh_adjacency(const int32_t* d_faces, int F, const int64_t* d_unmap, int V, int64_t* d_adj_raw, int* h_n_raw,
                      int64_t* d_adj_res, int* h_n_res, void* d_ws, size_t ws_bytes, void* stream);

/* generate_seg_labels_and_ds_set (util.py:174-220) without the file I/O.  d_seg_indices [V] (non-negative raw
 * segment ids) -> d_raw_label [V] = rank of the id among the sorted unique ids (the `.seg.txt` column), and the
 * member lists of the SAMPLED cloud as a CSR: d_seg_points [Np] grouped by ascending compacted id, ascending point
 * index inside a group, d_seg_off [G+1] (room for min(V, Np) + 1).  h_counts[0] = number of raw segments,
 * h_counts[1] = G (a segment none of whose vertices was sampled has no group). */
size_t sg_segment_lists_ws_bytes(int V, int Np);
int sg_segment_lists(const int32_t* d_seg_indices, int V, const int64_t* d_mapper, int Np, int32_t* d_raw_label,
                     int32_t* d_seg_points, int32_t* d_seg_off, int* h_counts, void* d_ws, size_t ws_bytes, void* stream);

/* `.seg.json` exactly as json.dump writes it (util.py:205-220): one list per sampled point, a segment's members at
 * the index of its smallest member, [] elsewhere.  Host arrays of sg_segment_lists (any group order). */
int sg_write_seg_json(const char* path, const int32_t* h_seg_points, const int32_t* h_seg_off, int G, int Np);

/* Mesh over-segmentation: the `segs.json` that every producer above starts from, made from the mesh itself -- a
 * graph-based segmenter in the style of ScanNet's Segmentator (Felzenszwalb-Huttenlocher merging over the mesh edges, weighted by
 * the difference of the vertex normals, with kThresh and segMinVerts).  The contract is the specification in DESIGN.md 8d, NOT byte
 * equality with the files ScanNet ships (that tool leaves the order of equal weights open).
 *
 * sg_overseg_edges (device): d_xyz [V,3] f32 finite and d_faces [F,3] in 0..V-1, both checked on the device (SG_EINVAL) ->
 *   d_face_normals [F,3] (may be NULL), d_normals [V,3] (sum of the face normals in ascending face index, normalised; zeros where the
 *   sum has no length), and the unique undirected edges a < b (sg_mesh_adjacency's raw list, with its limits and its errors) in
 *   ascending (w, a, b): d_edges [*h_E,2] int32 and d_w [*h_E]; both need room for 3F rows.  Synchronises the stream.
 * sg_overseg_merge (host, no GPU needed): the two ordered passes over those edges and the ids -- h_seg_indices[v] = the lowest vertex
 *   of v's component.  The arrays are untrusted: a vertex outside 0..V-1, a >= b, or weights that do not ascend are SG_EINVAL.
 * sg_overseg_scan: both for one scan, ids on the host.
 * sg_write_segs_json: {"params": {"kThresh": "%f", "segMinVerts": "%d"}, "sceneId": ..., "segIndices": [...]} as json.dump lays
 *   it out, under a temporary name and renamed. */
size_t sg_overseg_ws_bytes(int V, int F);
int sg_overseg_edges(const float* d_xyz, int V, const int32_t* d_faces, int F, float* d_face_normals, float* d_normals, int32_t* d_edges,
                     float* d_w, int* h_E, void* d_ws, size_t ws_bytes, void* stream);
int sg_overseg_merge(const int32_t* h_edges, const float* h_w, int E, int V, float k_thresh, int seg_min_verts, int32_t* h_seg_indices);
int sg_overseg_scan(const float* d_xyz, int V, const int32_t* d_faces, int F, float k_thresh, int seg_min_verts, int32_t* h_seg_indices,
                    void* d_ws, size_t ws_bytes, void* stream);
/* Stage times of sg_overseg_edges by events (tools/time_overseg.py): after sg_overseg_set_timing(1) the calling thread's calls record
 * them; sg_overseg_stage_times copies the last call's microseconds (room for 8 floats) and returns the number of stages. */
int sg_overseg_set_timing(int on);
int sg_overseg_stage_times(float* h_us, int cap);
const char* sg_overseg_stage_name(int i);
int sg_write_segs_json(const char* path, const char* scene_id, const int32_t* h_seg_indices, int V, float k_thresh, int seg_min_verts);

/* Point-cloud over-segmentation: the same segs.json for a scan that has no faces.  The graph is the kNN graph of the
 * cloud, the normals come from the covariance of every point's neighbourhood, the edge order and the host chain are 8d's.
 *
 * sg_pointcloud_knn: d_knn [N,k+1] int32 = the complete top-(k+1) list of every point against the whole cloud, in the scores and the tie
 *   rule of sg_pointcloud_adjacency (descending score, the lower index first among equals); entry 0, normally the point itself, is kept.
 *   d_points rows of `stride` floats, xyz first; k in {5, 10, 20}; N <= k is SG_EINVAL, N > SG_MAX_POINTS is SG_EUNSUP.
 * sg_pointcloud_normals: d_normals [N,3] from d_xyz [N,3] and such a table (entries are checked on the device): the eigenvector of the
 *   smallest eigenvalue of the list points' covariance by a cyclic Jacobi iteration with a fixed number of sweeps, not re-normalised,
 *   turned towards h_viewpoint (3 floats on the host; NULL: the centre of the cloud's bounding box).  Its workspace is
 *   sg_pointcloud_knn_ws_bytes(N).
 * sg_pcseg_edges: d_xyz [N,3] finite (checked on the device, SG_EINVAL) -> d_knn [N,k+1] (may be NULL), d_normals [N,3] and the unique
 *   undirected pairs a < b over (i, list[i][t]), t = 1..k, in ascending (w, a, b): d_edges [*h_E,2] int32 and d_w [*h_E]; both need room
 *   for N*k rows.  Synchronises the stream.
 * sg_pcseg_scan: those stages and sg_overseg_merge for one cloud, ids on the host.
 * Stage times of sg_pcseg_edges by events, as sg_overseg_set_timing: room for 7 floats (tools/time_pcseg.py). */
size_t sg_pointcloud_knn_ws_bytes(int N);
int sg_pointcloud_knn(const float* d_points, int stride, int N, int k, int32_t* d_knn, void* d_ws, size_t ws_bytes, void* stream);
int sg_pointcloud_normals(const float* d_xyz, int N, const int32_t* d_knn, int k, const float* h_viewpoint, float* d_normals, void* d_ws,
                          size_t ws_bytes, void* stream);
size_t sg_pcseg_ws_bytes(int N, int k);
int sg_pcseg_edges(const float* d_xyz, int N, int k, const float* h_viewpoint, int32_t* d_knn, float* d_normals, int32_t* d_edges, float* d_w,
                   int* h_E, void* d_ws, size_t ws_bytes, void* stream);
int sg_pcseg_scan(const float* d_xyz, int N, int k, const float* h_viewpoint, float k_thresh, int seg_min_verts, int32_t* h_seg_indices,
                  void* d_ws, size_t ws_bytes, void* stream);
int sg_pcseg_set_timing(int on);
int sg_pcseg_stage_times(float* h_us, int cap);
const char* sg_pcseg_stage_name(int i);

/* Voxel thinning of a large cloud: one input point per occupied voxel of edge `voxel`, and every point's thinned point.
 * The cell of a point is floor((p - lo) / voxel) per axis, lo = the cloud's minimum; a voxel's representative is its point nearest the
 * cell centre (fp32, op by op as 8g writes it), the lowest index among equals.  d_points rows of `stride` floats, xyz first.
 *   *h_M = occupied voxels; d_rep[0..M) = the representatives' indices, ASCENDING (not in voxel order); d_thin_of_point[i] = j where
 *   d_rep[j] stands for i's voxel.  Both need room for N entries.  h_lo3 (may be NULL) receives lo.  Integers only: the same bytes on
 *   every run.  1 <= N <= SG_MAX_CLOUD_POINTS (above: SG_EUNSUP; the kNN's SG_MAX_POINTS does not apply here).
 * SG_EINVAL: a null pointer, stride < 3, N < 1, voxel not finite or <= 0, a workspace below sg_cloud_thin_ws_bytes(N) (all before the
 *   first HIP call), a coordinate that is not finite (checked on the device before anything else).  SG_EUNSUP: an axis with 2^21 cells
 *   or more ("voxel too small for the cloud's extent").
 * Synchronises the stream twice (check and box, voxel count); the outputs are ordered on the stream.
 * Stage times by events, as sg_overseg_set_timing: room for 6 floats (tools/time_thin.py). */
#define SG_MAX_CLOUD_POINTS (1 << 27)
size_t sg_cloud_thin_ws_bytes(int N);          /* 0 when N < 1 or N > SG_MAX_CLOUD_POINTS */
int sg_cloud_thin(const float* d_points, int stride, int N, float voxel, int32_t* d_rep, int32_t* d_thin_of_point, int* h_M,
                  float* h_lo3, void* d_ws, size_t ws_bytes, void* stream);
int sg_cloud_thin_set_timing(int on);
int sg_cloud_thin_stage_times(float* h_us, int cap);
const char* sg_cloud_thin_stage_name(int i);

/* Exact grid-indexed kNN: sg_pointcloud_knn's table, bit for bit, from a uniform grid over the bounding box.  A query walks
 * the cells round its own in rings and stops once  Lb > delta - s_kth : Lb a true lower bound of the squared distance to every point it
 * has not seen, delta = 2^-19 * max|p|^2 a bound of the pair score's distance from -d^2.  Queries that are not settled within the ring
 * limit are finished against the whole cloud, so neither the cell edge nor the ring limit can change a result; both only cost time.
 *   cell = 0: the library picks the edge from the data (a first guess, the occupied cells counted, one correction); cell > 0 forces it.
 *   k in {5, 10, 20} (else SG_EUNSUP); N <= k is SG_EINVAL; N > SG_MAX_GRID_POINTS is SG_EUNSUP (checked before anything is touched).
 *   SG_EINVAL: a coordinate that is not finite.  SG_EUNSUP: 4 * max|p|^2 or delta not finite (the message names sg_pointcloud_knn, which
 *   decides such a cloud); a forced cell that gives an axis 2^21 cells or more, or more cells than the dense table's max(2^22, 4 N).
 *   SG_ENOMEM: a workspace below sg_pointcloud_knn_grid_ws_bytes(N, k) (0 when N or k is outside the envelope).
 * A cloud whose points crowd into one cell (a million coincident points) stays exact and costs what brute force costs.
 * Synchronises the stream (box; the occupied cells when the library picks the edge; the queue's length).
 * Stage times by events, as sg_overseg_set_timing: room for 7 floats.  sg_pointcloud_knn_grid_stats: the calling thread's last call ->
 *   h[0..2] cells per axis, h[3] occupied cells, h[4] the largest cell, h[5] the bits of the fp32 cell edge, h[6] the largest ring count of
 *   a query the rings settled, h[7] queries finished against the whole cloud, h[8] pair scores evaluated (counted in timed calls only).
 * sg_pointcloud_knn_grid_set_tuning: the calling thread's target occupancy (points per occupied cell) and ring limit; 0 = the default
 *   (tools/time_knn_grid.py sweeps them).
 * The indexed twins of the point-cloud segmenter take index = SG_KNN_BRUTE (exactly the functions above, SG_MAX_POINTS included) or
 *   SG_KNN_GRID (lists from sg_pointcloud_knn_grid with `cell`, up to SG_MAX_GRID_POINTS); every later stage is the same code. */
#define SG_MAX_GRID_POINTS (1 << 24)
#define SG_KNN_BRUTE 0
#define SG_KNN_GRID 1
size_t sg_pointcloud_knn_grid_ws_bytes(int N, int k);
int sg_pointcloud_knn_grid(const float* d_points, int stride, int N, int k, float cell, int32_t* d_knn, void* d_ws, size_t ws_bytes,
                           void* stream);
int sg_pointcloud_knn_grid_set_timing(int on);
int sg_pointcloud_knn_grid_stage_times(float* h_us, int cap);
const char* sg_pointcloud_knn_grid_stage_name(int i);
int sg_pointcloud_knn_grid_stats(int64_t* h, int cap);
int sg_pointcloud_knn_grid_set_tuning(int target_occupancy, int ring_limit);
size_t sg_pcseg_ws_bytes_indexed(int N, int k, int index);
int sg_pcseg_edges_indexed(const float* d_xyz, int N, int k, const float* h_viewpoint, int index, float cell, int32_t* d_knn, float* d_normals,
                           int32_t* d_edges, float* d_w, int* h_E, void* d_ws, size_t ws_bytes, void* stream);
int sg_pcseg_scan_indexed(const float* d_xyz, int N, int k, const float* h_viewpoint, int index, float cell, float k_thresh, int seg_min_verts,
                          int32_t* h_seg_indices, void* d_ws, size_t ws_bytes, void* stream);

/* Exact grid-indexed nearest point between two clouds: sg_nearest_point's d_idx, bit for bit, without scoring every pair.
 * For every query row u of d_x [U, x_stride >= 3] the candidate row of d_y [N, y_stride >= 3] with the largest pair score (|q|^2 formed as
 * (x*x + y*y) + z*z), the lowest candidate index among equal scores, int64.  d_d2 (may be NULL) receives (dx*dx + dy*dy) + dz*dz of
 * d = x[u] - y[idx[u]], each operation rounded once.  The search is sg_pointcloud_knn_grid's with a list of one entry: the index holds the
 * candidates, the box, the largest extent and max|p|^2 are taken over the union of both clouds, the queries are binned by the same cell
 * formula and sorted by cell, and a query is settled when  Lb > delta - s_best .  Queries unsettled at the ring limit (a query far from
 * every candidate, a block without candidates) are finished by sg_nearest_point's kernel, so neither the cell edge nor the ring limit nor
 * the stream can change a result.
 *   0 <= U <= SG_MAX_CLOUD_POINTS, 1 <= N <= SG_MAX_GRID_POINTS (above: SG_EUNSUP, checked before anything is touched); U = 0 is SG_OK
 *   and touches nothing.  SG_EINVAL: null pointers, a stride below 3, N < 1, U < 0, a cell edge that is negative or not finite, a workspace
 *   below sg_nearest_point_grid_ws_bytes(U, N) (0 outside the envelope) -- all before the first device call --, a coordinate of either
 *   cloud that is not finite (checked on the device before anything reads through it).  SG_EUNSUP: 4 * max|p|^2 or delta not finite (the
 *   message names sg_nearest_point), a forced cell that gives an axis 2^21 cells or more or more cells than max(2^22, 4 N).
 * Synchronises the stream like sg_pointcloud_knn_grid.  Stage times, statistics (the same nine words; the `search` stage holds the
 * queries' binning and sort, the `fallback` stage the queue and d2) and tuning per calling thread, as above. */
size_t sg_nearest_point_grid_ws_bytes(int U, int N);
int sg_nearest_point_grid(const float* d_x, int x_stride, int U, const float* d_y, int y_stride, int N, float cell, int64_t* d_idx, float* d_d2,
                          void* d_ws, size_t ws_bytes, void* stream);
int sg_nearest_point_grid_set_timing(int on);
int sg_nearest_point_grid_stage_times(float* h_us, int cap);
const char* sg_nearest_point_grid_stage_name(int i);
int sg_nearest_point_grid_stats(int64_t* h, int cap);
int sg_nearest_point_grid_set_tuning(int target_occupancy, int ring_limit);

/* Exact k nearest candidates of every query between two clouds: row u of d_knn [U, k] holds the k rows of d_y
 * [N, y_stride >= 3] with the largest pair score against the query row u of d_x [U, x_stride >= 3] (|q|^2 formed as (x*x + y*y) + z*z), in
 * descending score, the lower candidate index first among equal scores, original indices, int32: the first k columns of a stable descending
 * sort of the query's full score row, so column 0 is sg_nearest_point_grid's d_idx.  d_d2 [U, k] (may be NULL) receives
 * (dx*dx + dy*dy) + dz*dz of d = x[u] - y[knn[u][t]], each operation rounded once.  The search is sg_nearest_point_grid's with a list of k
 * entries: the same index over the candidates, the box, the largest extent and max|p|^2 over the union of both clouds, the queries sorted by
 * cell, and a query is settled when its list is full and  Lb > delta - s_kth .  Queries unsettled at the ring limit are finished against
 * every candidate in original order, so neither the cell edge nor the ring limit nor the stream can change a result.
 *   k in {5, 10, 20} (else SG_EUNSUP); 0 <= U <= SG_MAX_CLOUD_POINTS and U * k below 2^31 (above: SG_EUNSUP); k <= N <= SG_MAX_GRID_POINTS
 *   (N < k: SG_EINVAL, above: SG_EUNSUP); U = 0 is SG_OK and touches nothing.  SG_EINVAL: null pointers, a stride below 3, U < 0, a cell
 *   edge that is negative or not finite, a workspace below sg_cloud_knn_cross_grid_ws_bytes(U, N, k) (0 outside the envelope) -- all before
 *   the first device call --, a coordinate of either cloud that is not finite (found on the device by the box stage).  SG_EUNSUP:
 *   4 * max|p|^2 or delta not finite, a forced cell outside the table, as sg_nearest_point_grid.
 * Synchronises the stream like sg_nearest_point_grid.  Stage times, statistics (the same seven stages and nine words) and tuning per calling
 * thread, as above. */
size_t sg_cloud_knn_cross_grid_ws_bytes(int U, int N, int k);
int sg_cloud_knn_cross_grid(const float* d_x, int x_stride, int U, const float* d_y, int y_stride, int N, int k, float cell, int32_t* d_knn,
                            float* d_d2, void* d_ws, size_t ws_bytes, void* stream);
int sg_cloud_knn_cross_grid_set_timing(int on);
int sg_cloud_knn_cross_grid_stage_times(float* h_us, int cap);
const char* sg_cloud_knn_cross_grid_stage_name(int i);
int sg_cloud_knn_cross_grid_stats(int64_t* h, int cap);
int sg_cloud_knn_cross_grid_set_tuning(int target_occupancy, int ring_limit);

/* The most frequent value among each row's neighbours.  Row u of d_knn [U, k] is j_0 .. j_{k-1}, indices into d_label [N];
 * c(t) = the number of s with label[j_s] == label[j_t], t* = the smallest t that maximises c.  d_winner[u] = label[j_t*]; d_rep[u] = j_t*,
 * the nearest neighbour that holds the winner (among equally frequent values the one met first in the list wins); d_count[u] = c(t*);
 * d_tied[u] = 1 when some t has c(t) == c(t*) and another label, else 0.  d_count and d_tied may be NULL.  Any int32 is a label; labels are
 * compared by equality only; integers throughout, so every run writes the same bytes.
 *   1 <= k <= 32, U >= 0 (0: SG_OK, nothing touched), N >= 1, else SG_EINVAL.  An entry of d_knn outside 0..N-1: SG_EINVAL after the
 *   call's one stream synchronisation (that row's outputs are not written). */
int sg_knn_vote(const int32_t* d_knn, int U, int k, const int32_t* d_label, int N, int32_t* d_winner, int32_t* d_rep, int32_t* d_count,
                int32_t* d_tied, void* stream);

/* Rigid alignment of two clouds: the three pieces around the nearest-point search that a point-to-point ICP needs.
 *
 * sg_rigid_apply: h_T is a row-major 3x4 matrix of doubles [R|t] (any finite matrix, not only a rotation).  For every row u of d_x
 *   [U, x_stride >= 3]:  d_out[u][r] = (float)(((R[r][0]*x + R[r][1]*y) + R[r][2]*z) + t[r]),  the coordinates widened to double, every
 *   operation rounded once in that order, one final rounding to fp32, no contraction: the bytes of the same statement written element-wise
 *   in NumPy.  d_out is [U,3], dense.  0 <= U <= SG_MAX_CLOUD_POINTS (above: SG_EUNSUP); U = 0 is SG_OK and touches nothing.  SG_EINVAL:
 *   null pointers, a stride below 3, U < 0, an entry of h_T that is not finite -- all before the first device call.  The launch is left on
 *   the stream; the call does not synchronise.
 *
 * sg_align_moments: the 17 sums of a closed-form rigid fit over the pairs (x[u], y[idx[u]]) that have d2[u] <= max_d2 (fp32 compare;
 *   max_d2 may be +inf; a NaN in d2 is never an inlier).  With a = (double)x[u] - h_origin_x and b = (double)y[idx[u]] - h_origin_y, h_out
 *   receives  n (exact) | sum a [3] | sum b [3] | sum a b^T [9, row-major] | sum (double)d2[u],  accumulated in double.  Deterministic: no
 *   floating-point atomics; a workgroup of 256 threads folds 1,024 consecutive pairs (thread t takes pairs t, t + 256, t + 512, t + 768 of
 *   its block in that order, the wave sums run on wave_ops.h's network, the four waves are added in order) into one partial in the
 *   workspace, and one workgroup adds the partials (thread t takes partials t, t + 256, .. in order, then the same wave network): the
 *   launch shape and the summation tree depend on U alone, so two calls on the same input write the same 17 x 8 bytes on any device and
 *   stream.  0 <= U <= SG_MAX_CLOUD_POINTS, 1 <= N <= SG_MAX_CLOUD_POINTS (above: SG_EUNSUP); U = 0 writes 17 zeros and touches no device
 *   memory.  SG_EINVAL: null pointers, a stride below 3, U < 0, N < 1, max_d2 NaN, an origin that is not finite, a workspace below
 *   sg_align_moments_ws_bytes(U) (0 outside the envelope) -- all before the first device call --, an entry of d_idx outside 0..N-1, inlier
 *   or not (checked on the device before anything reads through it; h_out is then not written).  Synchronises the stream.
 *
 * sg_align_solve: host only, no device call.  h_m is sg_align_moments' h_out for the same origins.  h_T receives the row-major 3x4 [R|t]
 *   of the proper rigid transform (det R = +1) that minimises sum |R x + t - y|^2 over the pairs (Kabsch from the moments:
 *   H = sum a b^T - (sum a)(sum b)^T / n, a one-sided Jacobi SVD of H; R is built from the two leading singular pairs and their cross
 *   products, which flips the smallest singular direction exactly when the unconstrained optimum is a reflection).  t is expressed for
 *   un-shifted coordinates (t = ybar - R xbar with the origins added back), so h_T goes straight into sg_rigid_apply.  SG_EINVAL: null
 *   pointers, a moment or an origin that is not finite, n negative.  SG_EUNSUP with a message that says "degenerate": n < 3, or a second
 *   singular value at or below 2^-40 of the first (the pairs lie on a line or in a point: the rotation about it is free). */
int sg_rigid_apply(const float* d_x, int x_stride, int U, const double* h_T, float* d_out, void* stream);
size_t sg_align_moments_ws_bytes(int U);
int sg_align_moments(const float* d_x, int x_stride, int U, const float* d_y, int y_stride, int N, const int64_t* d_idx, const float* d_d2,
                     float max_d2, const double* h_origin_x, const double* h_origin_y, double* h_out, void* d_ws, size_t ws_bytes, void* stream);
int sg_align_solve(const double* h_m, const double* h_origin_x, const double* h_origin_y, double* h_T);

/* Point-to-plane ICP: the two pieces that replace sg_align_moments / sg_align_solve when the fixed cloud has normals.
 *
 * sg_align_plane_moments: the 31 sums of one Gauss-Newton step on the point-to-plane residual.  d_x [U, x_stride >= 3] is the ORIGINAL
 *   moving cloud, h_T the row-major 3x4 [R|t] of the current pose, d_y [N, y_stride >= 3] the fixed cloud, d_n [N, n_stride >= 3] its fp32
 *   normals, d_idx / d_d2 the search's answer for the moved cloud.  A pair u is a candidate when d2[u] <= max_d2 (fp32 compare; max_d2 may
 *   be +inf; a NaN in d2 is never a candidate).  For a candidate, in double, every operation rounded once in the order written, no
 *   contraction:
 *     p[r] = ((R[r][0]*x + R[r][1]*y) + R[r][2]*z) + t[r]        (sg_rigid_apply's statement without its final rounding to fp32)
 *     a = p - h_origin;  b = (double)y[idx[u]] - h_origin;  n = (double)d_n[idx[u]]
 *     usable: 0.25 <= (n0*n0 + n1*n1) + n2*n2 <= 4, which a NaN or an infinite component fails; a normal is not re-normalised
 *     e = a - b;  r = (e0*n0 + e1*n1) + e2*n2
 *     J = [ a1*n2 - a2*n1,  a2*n0 - a0*n2,  a0*n1 - a1*n0,  n0, n1, n2 ]
 *   h_out:  [0] usable candidates (exact) | [1] candidates whose normal is not usable (exact) | [2..22] upper triangle of sum J J^T,
 *   row-major | [23..28] sum J r | [29] sum r r | [30] sum (double)d2 over the usable candidates.  Deterministic exactly as sg_align_moments
 *   is: no floating-point atomics, cdiv(U, 1024) workgroups of 256 threads, thread t takes pairs t, t + 256, t + 512, t + 768 of its block
 *   in that order, wave_ops.h's network, the four waves added in order into one partial row, one folding workgroup over the rows (thread t
 *   takes rows t, t + 256, .. in order): launch shape and both trees depend on U alone, so two calls on the same input write the same
 *   31 x 8 bytes on any device and stream.  0 <= U <= SG_MAX_CLOUD_POINTS, 1 <= N <= SG_MAX_CLOUD_POINTS (above: SG_EUNSUP); U = 0 writes 31
 *   zeros and touches no device memory.  SG_EINVAL: null pointers, a stride below 3, U < 0, N < 1, max_d2 NaN, an entry of h_T or of
 *   h_origin that is not finite, a workspace below sg_align_plane_moments_ws_bytes(U) (0 outside the envelope) -- all before the first
 *   device call --, an entry of d_idx outside 0..N-1, candidate or not, usable or not (checked on the device before anything reads through
 *   it; h_out is then not written).  Synchronises the stream once; the sums and the flag come back in one copy.
 *
 * sg_align_plane_solve: host only, no device call.  h_m is sg_align_plane_moments' h_out for the same h_origin and the same h_T (row-major
 *   3x4; the first three rows of a 4x4 serve).  With M = sum J J^T, g = sum J r and D = diag(1/length, 1/length, 1/length, 1, 1, 1) --
 *   `length` > 0 puts the rotational columns into length units -- D M D = V diag(lambda) V^T by cyclic Jacobi, and the step is
 *   s = -D V diag(1/lambda) V^T D g = (w, v).  Rw is Rodrigues' rotation of angle |w| about w (sin and cos from their series below 1e-8
 *   rad); the step acts about the origin: R_new = Rw R, t_new = Rw (t - origin) + origin + v; R_new is re-orthonormalised (Gram-Schmidt
 *   on rows 0 and 1, row 2 their cross product).  h_T_new receives the row-major 4x4 (last row 0 0 0 1), h_step -- may be null -- the six
 *   values (w, v).  SG_EINVAL: null pointers, a moment, origin, `length` or entry of h_T that is not finite, length <= 0, n negative.
 *   SG_EUNSUP with a message that says "degenerate": n < 6, lambda_max <= 0, or lambda_min <= 2^-40 lambda_max (one plane, parallel
 *   planes, two plane directions: some motion leaves every residual unchanged). */
size_t sg_align_plane_moments_ws_bytes(int U);
int sg_align_plane_moments(const float* d_x, int x_stride, int U, const double* h_T, const float* d_y, int y_stride, int N, const float* d_n,
                           int n_stride, const int64_t* d_idx, const float* d_d2, float max_d2, const double* h_origin, double* h_out, void* d_ws,
                           size_t ws_bytes, void* stream);
int sg_align_plane_solve(const double* h_m, const double* h_origin, double length, const double* h_T, double* h_T_new, double* h_step);

/* Global (init-free) registration: a local descriptor, its nearest neighbour and a hypothesise-and-count RANSAC.  No
 * floating-point atomics in any of them: two calls on the same input write the same bytes.
 *
 * sg_fpfh: d_xyz [N, stride >= 3] fp32, d_normals [N,3] fp32, rows d_off int64 [N+1] / d_idx int32 [off[N]] as sg_radius_neighbours_grid
 *   writes them (the point itself not in its row; d_idx may be NULL when every row is empty).  d_spfh int32 [N,34]: 3 x 11 bin counts
 *   (theta | alpha | phi) and the number of counted pairs; d_fpfh float [N,33].  Per pair (i, j in row i), in double on the widened fp32
 *   inputs, dot(a, b) = (a0*b0 + a1*b1) + a2*b2, nothing contracted:
 *     d = p_j - p_i; len = sqrt(d.d), the pair is skipped when len == 0; dh = d / len; a1 = n_i.dh; a2 = n_j.dh;
 *     |a1| < |a2|: u = n_j, t = n_i, dh = -dh; else u = n_i, t = n_j;  phi = u.dh;  v = dh x u, skipped when |v| == 0, v /= |v|;
 *     w = u x v;  alpha = v.t;  theta = atan2(w.t, u.t);
 *     bins floor(11 * x) clamped to 0..10 for x = (theta + pi) / (2 pi), (alpha + 1) / 2, (phi + 1) / 2.
 *   FPFH of i, per sub-histogram: S[b] = sum over the row in stored order, over neighbours with d2_ij = d.d > 0 and pairs_j > 0, of
 *   ((100 * spfh_j[b]) / pairs_j) / d2_ij in double; fpfh[b] = (float)((100 * S[b]) / sum_b S[b]), the sum over the sub-histogram's 11
 *   bins in ascending order; an empty row or an all-zero S gives zeros.  0 <= N <= SG_MAX_GRID_POINTS (above: SG_EUNSUP); N = 0 is SG_OK
 *   and touches nothing.  SG_EINVAL: null pointers, a stride below 3, a workspace below sg_fpfh_ws_bytes(N) -- before the first device call
 *   --, offsets that do not ascend from 0 to off[N] or a row entry outside 0..N-1 (checked on the device; nothing is read through
 *   either).  Synchronises the stream.
 *
 * sg_feature_nearest: d_a [U,C], d_b [N,C] fp32 dense rows, 1 <= C <= 64.  d2(u, n) = sum over c ascending of (a_c - b_c) * (a_c - b_c),
 *   every operation rounded once in fp32; d_idx[u] (int64) is the n of the smallest d2, the lowest n among equals, d_d2[u] that d2: the
 *   bytes of the NumPy float32 statement written channel by channel.  Inputs are finite by contract.  U, N <= 2^18 (above: SG_EUNSUP,
 *   the message names thinning); N < 1, U < 0 or C outside 1..64: SG_EINVAL; U = 0: SG_OK.  The launch is left on the stream.
 *
 * sg_ransac_count: correspondences (d_ci[c], d_cj[c]), c < C, index d_m [U, m_stride >= 3] and d_f [N, f_stride >= 3]; with
 *   a_c = m[ci[c]] and b_c = f[cj[c]] widened to double.  Triple h = (t0, t1, t2): row h of d_triples int32 [H,3], or, when d_triples is
 *   NULL, t_e = ((z >> 32) * C) >> 32 with z = splitmix64(seed + (3h + e + 1) * 0x9E3779B97F4A7C15) (z = (z ^ z >> 30) *
 *   0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^= z >> 31; all modulo 2^64).  d_count[h] = -1 for a rejected
 *   hypothesis: a repeated t; any edge (0,1), (1,2), (2,0) with la < min_edge or lb < min_edge, la < similarity * lb or
 *   lb < similarity * la (la, lb its lengths in the two clouds); a height |e1 x (x2 - x0)| below min_edge / 8 in either cloud (e1 the
 *   UNIT first edge).  Otherwise d_count[h] = the number of c with |R a_c + t - b_c|^2 <= max_dist * max_dist, p[r] = ((R[r][0]*x +
 *   R[r][1]*y) + R[r][2]*z) + t[r], all in double, [R|t] = sg_triangle_pose of the two triangles.  h_survivors (may be NULL) receives the
 *   number of hypotheses that were counted.  3 <= C <= 2^18, 0 <= H <= 2^24 (above: SG_EUNSUP); H = 0 is SG_OK.  SG_EINVAL: null
 *   pointers, strides below 3, U or N < 1, C < 3, max_dist or min_edge not a finite length > 0, similarity outside (0, 1], a workspace
 *   below sg_ransac_ws_bytes(C, H) -- before the first device call --, a correspondence outside its cloud or an entry of d_triples outside
 *   0..C-1 (raised on the device before anything is read through it).  Synchronises the stream.  sg_ransac_set_tuning(lanes), per calling
 *   thread: lanes = 1 | 64 | 0 (the default, 64) share a survivor in the counting kernel, which cannot change a result.  Stage times by
 *   events, as sg_overseg_set_timing: room for 3 floats (gather, filter, count of the last call; tools/time_register.py).
 *
 * sg_triangle_pose: host only, no device call; the function the counting kernel runs (csrc/triangle_pose.h).  h_a, h_b: two triangles,
 *   x0 | x1 | x2.  Frame of a triangle: e1 = (x1 - x0) / |x1 - x0|, e3 = c / |c| with c = e1 x (x2 - x0), e2 = e3 x e1; R = F_b F_a^T
 *   with F = [e1 e2 e3] as columns, t = mean(b) - R mean(a), mean[r] = ((x0[r] + x1[r]) + x2[r]) / 3.  h_T receives the row-major 3x4
 *   [R|t].  SG_EINVAL: null pointers, a coordinate that is not finite.  SG_EUNSUP ("degenerate"): a zero first edge or corners on a line. */
size_t sg_fpfh_ws_bytes(int N);
int sg_fpfh(const float* d_xyz, int stride, int N, const float* d_normals, const int64_t* d_off, const int32_t* d_idx, int32_t* d_spfh,
            float* d_fpfh, void* d_ws, size_t ws_bytes, void* stream);
int sg_feature_nearest(const float* d_a, int U, const float* d_b, int N, int C, int64_t* d_idx, float* d_d2, void* stream);
size_t sg_ransac_ws_bytes(int C, int H);
int sg_ransac_count(const float* d_m, int m_stride, int U, const float* d_f, int f_stride, int N, const int32_t* d_ci, const int32_t* d_cj, int C,
                    int H, uint64_t seed, const int32_t* d_triples, double max_dist, double similarity, double min_edge, int32_t* d_count,
                    int* h_survivors, void* d_ws, size_t ws_bytes, void* stream);
int sg_ransac_set_tuning(int lanes_per_survivor);
int sg_ransac_set_timing(int on);
int sg_ransac_stage_times(float* h_us, int cap);
const char* sg_ransac_stage_name(int i);
int sg_triangle_pose(const double* h_a, const double* h_b, double* h_T);

/* Plane extraction: the dominant planes of a cloud by hypothesise-and-count RANSAC, a least-squares refit and the
 * labelling of a plane's points.  Arithmetic is double on the widened fp32 inputs, dot(a, b) = (a0*b0 + a1*b1) + a2*b2, a x b =
 * (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0), nothing contracted.  No floating-point atomics: two calls on the same input write
 * the same bytes.  Points are d_xyz [N, stride >= 3] fp32, 0 <= N <= 2^24 (above: SG_EUNSUP).
 *
 * The inlier test of a plane (n, d), one function for all three device entries: |n.p + d| <= dist, and, when d_normals float [N,3] is not
 * NULL, also min_cos <= |n.nrm_i| < inf -- a normal with a component that is not finite fails it.  A point i is FREE when d_label is NULL
 * or d_label[i] < 0.
 *
 * sg_plane_ransac: the free points, in ASCENDING index, form a dense list of M entries (*h_free = M); triples hold POSITIONS in that
 *   list.  Triple h = (t0, t1, t2): row h of d_triples int32 [H,3], or, when d_triples is NULL, sg_ransac_count's generator with C := M.
 *   With p_e the point at position t_e, u = p1 - p0, v = p2 - p0, w = p2 - p1, c = u x v and |x| = sqrt(x.x), hypothesis h is REJECTED
 *   (d_count[h] = -1, d_plane[h] = 0 0 0 0) unless  t0, t1, t2 are distinct  and  |u| >= min_edge, |v| >= min_edge, |w| >= min_edge  and
 *   |c| >= (min_sine * |u|) * |v|  -- written so that a NaN rejects.  A kept hypothesis has n = c / |c| (component by component),
 *   d = -(n.p0), d_plane[h] = (n, d) as double [H,4], and d_count[h] = the number of free points that pass the inlier test.  *h_best = the
 *   h of the highest count, the lowest h among equals, -1 when every hypothesis was rejected (or H = 0).  M < 3: SG_OK, every hypothesis
 *   rejected, *h_best = -1, d_triples is not read.  0 <= H <= 2^20 (above: SG_EUNSUP).  SG_EINVAL: null pointers, a stride below 3, dist
 *   not a finite length >= 0, min_edge not a finite length > 0, min_sine outside (0, 1], min_cos outside 0..1 (read only with d_normals), a
 *   workspace below sg_plane_ransac_ws_bytes(N, H, d_normals != NULL) -- before the first device call --, an entry of d_triples outside
 *   0..M-1 (raised on the device before anything is read through it).  Synchronises the stream.
 *
 * sg_plane_moments: over the free points that pass the inlier test of h_plane (n, d: four doubles), with q = p - h_origin and
 *   r = n.p + d, h_out[11] = count | sum q [3] | sum q q^T as xx xy xz yy yz zz | sum r*r.  The reduction trees are sg_align_moments': a
 *   function of N alone.  N = 0: zeros.  SG_EINVAL: null pointers, a plane or an origin that is not finite, dist, min_cos as above, a
 *   workspace below sg_plane_moments_ws_bytes(N).  Synchronises the stream.
 *
 * sg_plane_fit: host only, no device call.  h_m is sg_plane_moments' h_out for the same h_origin.  C = sum q q^T - (sum q)(sum q)^T / count,
 *   diagonalised by cyclic Jacobi (no LAPACK, as sg_align_plane_solve); n = the eigenvector of the smallest eigenvalue, unit length, its
 *   largest-magnitude component positive (the lowest axis among equals); h_plane = (n, -(n.centroid)), h_centroid [3] (may be NULL) =
 *   h_origin + sum q / count, *h_rms (may be NULL) = sqrt(max(smallest eigenvalue, 0) / count), the inliers' rms distance to the fitted
 *   plane.  SG_EUNSUP ("degenerate"): count < 3, or a middle eigenvalue that is not above 2^-40 of the largest (points on a line or in one
 *   place: zero up to the rounding Jacobi leaves).  SG_EINVAL: null pointers, a moment or an origin that is not finite.
 *
 * sg_plane_assign: d_label[i] = id at every free point that passes the inlier test of h_plane; *h_labelled = how many.  id >= 0.  SG_EINVAL
 *   as sg_plane_moments, a negative id, a NULL d_label.  Synchronises the stream.
 *
 * sg_plane_set_tuning(compact), per calling thread: compact = 0 lets the counting kernel walk all H hypotheses and skip the rejected
 *   ones in place instead of walking the compacted kept ones (the default; it cannot change a result).  Stage times by events, as
 *   sg_overseg_set_timing: room for 5 floats -- compact, generate, count (the last sg_plane_ransac), moments and assign (the last call of
 *   each; tools/time_planes.py). */
size_t sg_plane_ransac_ws_bytes(int N, int H, int with_normals);
int sg_plane_ransac(const float* d_xyz, int stride, int N, const int32_t* d_label, const float* d_normals, double min_cos, int H, uint64_t seed,
                    const int32_t* d_triples, double dist, double min_edge, double min_sine, int32_t* d_count, double* d_plane, int* h_free,
                    int* h_best, void* d_ws, size_t ws_bytes, void* stream);
size_t sg_plane_moments_ws_bytes(int N);
int sg_plane_moments(const float* d_xyz, int stride, int N, const int32_t* d_label, const float* d_normals, double min_cos, const double* h_plane,
                     double dist, const double* h_origin, double* h_out, void* d_ws, size_t ws_bytes, void* stream);
int sg_plane_fit(const double* h_m, const double* h_origin, double* h_plane, double* h_centroid, double* h_rms);
size_t sg_plane_assign_ws_bytes(int N);
int sg_plane_assign(const float* d_xyz, int stride, int N, const float* d_normals, double min_cos, const double* h_plane, double dist, int id,
                    int32_t* d_label, int* h_labelled, void* d_ws, size_t ws_bytes, void* stream);
int sg_plane_set_tuning(int compact);
int sg_plane_set_timing(int on);
int sg_plane_stage_times(float* h_us, int cap);
const char* sg_plane_stage_name(int i);

/* Oriented boxes of labelled points: a label index -- a segmented view of a cloud by a per-point int32 vector -- and the
 * per-label reductions a box needs.  A point is LABELLED when d_label[i] >= 0; negative labels are ignored; every non-negative int32 is a
 * legal value and values need not be dense.  Points are rows of `stride` >= 3 floats, 0 <= N <= 2^24.  Arithmetic is double on the
 * widened fp32 inputs, dot(a, b) = (a0*b0 + a1*b1) + a2*b2, every operation rounded once, nothing contracted, no floating-point atomics.
 * Every device entry synchronises the stream once; a _ws_bytes function returns 0 for a size the entry does not take.
 *
 * sg_label_index: d_order[0..M-1] = the labelled points sorted by label, in ascending index within a label (M = N - *h_ignored);
 *   d_value[0..L-1] = the distinct labels, ascending; d_start[0..L] = their offsets in d_order, d_start[L] = M.  Integers only: it is
 *   np.argsort(labels[labels >= 0], kind="stable") mapped back to raw indices, with np.unique.  d_order, d_value and d_start hold N, N and
 *   N + 1 entries (L can equal N; d_order and d_value are scratch behind M and L).  N = 0 or no labelled point: SG_OK with *h_L = 0.
 *
 * sg_label_moments: d_m [L,10] = count | sum q [3] | sum q q^T (xx xy xz yy yz zz) with q = p - p_first, p_first the label's lowest-index
 *   point (d_order[d_start[l]]): every label is conditioned on itself, and the sums are the same wherever the cloud lies.  A label's list
 *   is cut into chunks of 1,024 consecutive entries; a chunk is summed on the first tree of sg_align_moments (thread t of 256 adds entries
 *   t, t + 256, .. in order, a wave sums on its fixed network, the four waves in order); the chunks of a label are added in ascending
 *   order.  A function of the label's count alone: repeated calls give the same bytes.  d_lo / d_hi [L,3] = the float32 minima and maxima
 *   per axis, exact bits of the inputs.
 *
 * sg_label_yaw_boxes: for every angle a < A with (c, s) = h_cs[a] (host doubles; the caller takes cos / sin, no device transcendental
 *   enters): u = c*x + s*y, v = c*y - s*x, each two rounded products and one rounded sum or difference; the extents umin, umax, vmin,
 *   vmax over the label.  d_best[l] = the a with the smallest (umax - umin) * (vmax - vmin), the lowest a among equals; d_ext [L,4] its
 *   extents; d_all (NULL, or [L,A,4]) all of them.  1 <= A <= 1024.  Exact: minima are order-free.
 *
 * sg_label_frame_extents: d_frame [L,9] doubles, a row-major 3 x 3 frame per label; d_ext [L,6] = min, max of dot(row_k, p), k = 0, 1, 2.
 *
 * sg_box_axes: host only, no device call.  h_m = one row of d_m.  C = (sum q q^T - (sum q)(sum q)^T / count) / count, cyclic Jacobi; the
 *   rows of h_R [9] are the eigenvectors by descending eigenvalue (the lower axis first among equals), rows 0 and 1 with their
 *   largest-magnitude component positive (the lowest axis among equals), row 2 = row 0 x row 1; h_eig [3] (may be NULL) the eigenvalues
 *   in that order.  When the largest eigenvalue is not positive -- one point, or points that coincide -- no direction is singled out and
 *   h_R is the identity.  Points on a line fix row 0 only; row 1 is then whatever Jacobi leaves, the same on every run.
 *
 * SG_EINVAL: a null pointer, stride < 3, L > N, A outside 1..1024, an entry of h_cs that is not finite, a workspace below the _ws_bytes
 *   function (all before the first device call); count < 1 or a moment that is not finite (sg_box_axes); a labelled point with a
 *   coordinate that is not finite, or a d_start / d_order that is not an index of this cloud (one flag word on the device, read with the
 *   call's synchronisation; the outputs are then undefined).  Ignored points may hold anything.  SG_EUNSUP: N above 2^24; d_all with
 *   L * A > 2^24.  Stage times by events, as sg_overseg_set_timing: room for 4 floats -- index, moments, yaw and frame, the last call
 *   of each (tools/time_boxes.py). */
size_t sg_label_index_ws_bytes(int N);
int sg_label_index(const int32_t* d_label, int N, int32_t* d_order, int32_t* d_value, int32_t* d_start, int* h_L, int* h_ignored, void* d_ws,
                   size_t ws_bytes, void* stream);
size_t sg_label_moments_ws_bytes(int N, int L);
int sg_label_moments(const float* d_xyz, int stride, int N, const int32_t* d_order, const int32_t* d_start, int L, double* d_m, float* d_lo,
                     float* d_hi, void* d_ws, size_t ws_bytes, void* stream);
size_t sg_label_yaw_boxes_ws_bytes(int N, int L, int A);
int sg_label_yaw_boxes(const float* d_xyz, int stride, int N, const int32_t* d_order, const int32_t* d_start, int L, const double* h_cs, int A,
                       int32_t* d_best, double* d_ext, double* d_all, void* d_ws, size_t ws_bytes, void* stream);
size_t sg_label_frame_extents_ws_bytes(int N, int L);
int sg_label_frame_extents(const float* d_xyz, int stride, int N, const int32_t* d_order, const int32_t* d_start, int L, const double* d_frame,
                           double* d_ext, void* d_ws, size_t ws_bytes, void* stream);
int sg_box_axes(const double* h_m, double* h_R, double* h_eig);
int sg_label_set_timing(int on);
int sg_label_stage_times(float* h_us, int cap);
const char* sg_label_stage_name(int i);

/* IoU of upright boxes: the consumer of the boxes above.  A BOX is 8 doubles, cx cy cz sx sy sz c s: the centre, the FULL
 * size, and the footprint axes u = (c, s), v = (-s, c) about z, the convention of sg_label_yaw_boxes (u = c*x + s*y, v = c*y - s*x); c and
 * s are host doubles -- the caller takes cos / sin, no device transcendental enters; an axis-aligned box has c = 1, s = 0.  z is up.
 * Sets A [Ka,8] and B [Kb,8] are flat over `B` scenes; the host tables h_off_a [B+1] and h_off_b [B+1] delimit the scenes (ascending
 * from 0 to Ka / Kb; a scene may be empty on either side) and only boxes of the same scene pair.  Double arithmetic, every operation
 * rounded once, nothing contracted, no floating-point atomics, the caller's stream, one synchronisation per call; a _ws_bytes function
 * returns 0 for a size the entry does not take.  At most 2^20 boxes a side and 2^16 scenes.
 *
 * IoU(a, b), THE OPERATION SEQUENCE (tests/boxap_ref.py restates it statement by statement; the device has one function for it):
 *   dx = ax - bx, dy = ay - by;  hax = 0.5*asx, hay = 0.5*asy, hbx = 0.5*bsx, hby = 0.5*bsy
 *   ex = hax*ac, ey = hax*as, fx = hay*as, fy = hay*ac
 *   the corners of a about b's centre, k = 0..3 = (-,-), (+,-), (+,+), (-,+) along a's (u, v), counter-clockwise:
 *     wx = (dx - ex) + fx, (dx + ex) + fx, (dx + ex) - fx, (dx - ex) - fx;   wy = (dy - ey) - fy, (dy + ey) - fy, (dy + ey) + fy, (dy - ey) + fy
 *   into b's frame: u_k = bc*wx_k + bs*wy_k, v_k = bc*wy_k - bs*wx_k (two rounded products, one rounded sum or difference)
 *   the polygon (n = 4) is clipped by b's sides in the order d = hbx - u, d = u + hbx, d = hby - v, d = v + hby; a vertex is inside when
 *   d >= 0.  One side (Sutherland-Hodgman): for i = 0..n-1 with q = vertex i and p = the vertex before it (vertex n-1 for i = 0), in order:
 *     if (dp >= 0) != (dq >= 0):  t = dp / (dp - dq)  -- taken only where the signs differ -- and the crossing is appended: on sides 0 / 1
 *       (+hbx / -hbx, pv + t*(qv - pv)), on sides 2 / 3 (pu + t*(qu - pu), +hby / -hby): the clipped coordinate is the side itself, exactly;
 *     if dq >= 0: q is appended.
 *   The result has at most 8 vertices; an append past the eighth is dropped (rounding alone could ask for one).
 *   area: the fan about vertex 0, acc = 0, for i = 1..n-2 in order: e = vertex i - vertex 0, g = vertex i+1 - vertex 0,
 *     acc = acc + (e.u*g.v - e.v*g.u);  area = 0.5*acc, and 0 unless area > 0 (fewer than three vertices: 0)
 *   h = min(az + 0.5*asz, bz + 0.5*bsz) - max(az - 0.5*asz, bz - 0.5*bsz), and 0 unless h > 0
 *   inter = area*h;  va = (asx*asy)*asz, vb = (bsx*bsy)*bsz;  uni = (va + vb) - inter;  IoU = inter / uni if uni > 0, else 0
 *   So touching boxes (a shared face: every vertex left lies on one side) give exactly 0, two single-point boxes give 0 (the union is
 *   not positive), and an axis-aligned box inside another gives va / vb.  The sequence is NOT symmetric -- a's corners are carried into
 *   b's frame --, so IoU(a, b) and IoU(b, a) agree to rounding (a few 1e-15: tests/test_boxap_ref.py measures it), not to the last bit.
 *
 * sg_box_iou: d_iou is flat; scene b holds a row-major [Ka_b, Kb_b] block and the blocks are stored in scene order; `pairs` is the
 *   number of doubles d_iou holds and must be the sum of Ka_b * Kb_b, at most 2^24.
 * sg_box_best: per box of A the best partner among the boxes of B of its scene: d_best [Ka] = the index WITHIN the scene's B boxes of
 *   the highest IoU, the lowest index among equals, d_best_iou [Ka] that IoU -- the bits sg_box_iou writes for the pair; an IoU of 0 is
 *   not a partner: -1 and 0.0.  d_cls_a [Ka] / d_cls_b [Kb] (int32; both or neither) restrict partners to the same class.  No Ka x Kb
 *   table and no limit on the pairs.
 *
 * SG_EINVAL: offsets that do not start at 0, do not ascend or do not end at Ka / Kb (checked on the host, they are host tables, before
 *   anything is read through them), one class vector without the other, `pairs` that is not the scenes' sum, a workspace below the
 *   _ws_bytes function; and, through one flag word on the device that is read with the call's synchronisation (the outputs are then
 *   undefined): a box with a value that is not finite, a negative size (0 is valid), |c*c + s*s - 1| > 1e-6.  Every message names its
 *   entry and the set.  SG_EUNSUP: more than 2^20 boxes a side, 2^16 scenes or (sg_box_iou) 2^24 pairs.  These entries have no stage
 *   timer: tools/time_boxap.py brackets them with events on the caller's stream. */
size_t sg_box_iou_ws_bytes(int Ka, int Kb, int B);
int sg_box_iou(const double* d_a, int Ka, const double* d_b, int Kb, const int32_t* h_off_a, const int32_t* h_off_b, int B, double* d_iou,
               long long pairs, void* d_ws, size_t ws_bytes, void* stream);
size_t sg_box_best_ws_bytes(int Ka, int Kb, int B);
int sg_box_best(const double* d_a, int Ka, const double* d_b, int Kb, const int32_t* d_cls_a, const int32_t* d_cls_b, const int32_t* h_off_a,
                const int32_t* h_off_b, int B, int32_t* d_best, double* d_best_iou, void* d_ws, size_t ws_bytes, void* stream);

/* Non-maximum suppression of upright boxes: the duplicates of a box set removed, greedily by score.  A BOX is the 8
 * doubles of the IoU entries above, cx cy cz sx sy sz c s; d_box [K,8], d_score [K] (doubles) and d_cls [K] (int32, or NULL for
 * class-agnostic suppression) are flat over `B` scenes; the host table h_off [B+1] delimits the scenes (ascending from 0 to K; a scene may
 * be empty) and only boxes of one scene meet.  Double arithmetic, every operation rounded once, nothing contracted, no floating-point
 * atomics, the caller's stream, one synchronisation per call; the _ws_bytes function returns 0 for a size the entry does not take.
 *
 * THE RULE (tests/boxnms_ref.py restates it in plain loops):
 *   ORDER: within a scene i comes BEFORE j iff s_i > s_j, or s_i == s_j and i < j -- a comparison of doubles, so -0.0 ties with 0.0.
 *   The scene is visited in that order.  Box j is SUPPRESSED iff some box i before it is KEPT, has the class of j (when classes are
 *   given) and IoU(a = box i, b = box j) > thresh, strictly (sg_box_best's partners and boxap's rule): the IoU is the operation sequence
 *   above with the EARLIER box as a -- the sequence is not symmetric, so the argument order is part of the contract.  Otherwise j is KEPT.
 *   The REPRESENTATIVE of a suppressed box is the FIRST such i in the order; a kept box represents itself.  So a box that only a
 *   suppressed box overlaps is kept: that is the whole difference from "overlaps anything better".
 * Outputs, int32 [K] each, addressed by the box's ORIGINAL position, indices counted WITHIN the scene (as sg_box_best's are):
 *   d_rank  the box's place in its scene's order, 0 first
 *   d_keep  1 or 0
 *   d_rep   a kept box's own index; for a suppressed box the index of the box that suppressed it
 * All are integers: equality with the restatement is the gate, and the same bytes come back on every run.
 * `words` is the sum over the scenes of n_s * ceil(n_s / 64), the 64-bit words of the suppression bit matrix (row i of a scene in rank
 * order holds the bits of the boxes after it); the caller passes it as sg_box_iou takes `pairs`, and sg_box_nms_ws_bytes(K, B, words)
 * sizes the workspace from it.  K = 0 is SG_OK.
 *
 * SG_EINVAL: a null pointer, offsets that do not start at 0, do not ascend or do not end at K (a host table, checked on the host before
 *   the first launch), thresh that is not finite or outside [0, 1), `words` that is not the scenes' sum, a workspace below the _ws_bytes
 *   function; and, through one flag word on the device that is read with the call's synchronisation (the outputs are then undefined): a
 *   box value or a score that is not finite, a negative size (0 is valid), |c*c + s*s - 1| > 1e-6.  Every message names the entry.
 *   SG_EUNSUP: K > 2^20, B > 2^16, a scene of more than 2^14 boxes, words > 2^24 (128 MB of bits).  No stage timer: tools/time_boxnms.py
 *   brackets the entry with events on the caller's stream. */
size_t sg_box_nms_ws_bytes(int K, int B, long long words);
int sg_box_nms(const double* d_box, const double* d_score, const int32_t* d_cls, int K, const int32_t* h_off, int B, double thresh,
               int32_t* d_rank, int32_t* d_keep, int32_t* d_rep, long long words, void* d_ws, size_t ws_bytes, void* stream);

/* Which boxes hold a point: the way back from boxes to points.  A BOX is 15 doubles, cx cy cz sx sy sz r00 r01 .. r22: the
 * centre, the FULL size along the rows of R, and R row-major; the rows of R are the box axes (Boxes.center, Boxes.size, Boxes.R as they
 * stand).  The test does not need an upright box: any orthonormal frame is taken.  Points are d_xyz rows of `stride` >= 3 floats.  Points
 * [N] and boxes [K,15] are flat over `B` scenes; the host tables h_off_p [B+1] and h_off_b [B+1] delimit the scenes (ascending from 0 to
 * N / K; a scene may be empty on either side) and only points and boxes of the same scene meet.  Double arithmetic on the widened fp32
 * inputs, every operation rounded once, nothing contracted, no floating-point atomics, the caller's stream, one synchronisation per call;
 * the _ws_bytes function returns 0 for a size the entry does not take.  At most 2^24 points, 2^20 boxes and 2^16 scenes.
 *
 * Point p against box b, THE OPERATION SEQUENCE (tests/boxlabels_ref.py restates it one statement per operation):
 *   d_i = double(p_i) - c_i,                          i = 0, 1, 2
 *   l_k = (r_k0*d_0 + r_k1*d_1) + r_k2*d_2,           k = 0, 1, 2
 *   h_k = 0.5*s_k + margin
 *   b holds p iff fabs(l_k) <= h_k for all three k: a face is inside.  vol = (s_0*s_1)*s_2; the margin does not enter it.
 * Outputs, int32 [N] each, with indices counted WITHIN the scene's boxes:
 *   d_count  the number of boxes of the point's scene that hold it
 *   d_first  the lowest index of a box that holds it, -1 if none
 *   d_inner  the box of smallest vol among those that hold it, the lowest index among equal volumes, -1 if none: the boxes are visited
 *            in ascending index and a box replaces the one kept only when its vol is smaller (vol < kept)
 *   d_held   (may be NULL) int32 [K]: per box the number of points it holds; integer sums, so the same on every run
 * All are order-free (a sum of 0/1, a minimum index, a minimum of (vol, index)): no tiling shows, and equality with the restatement is
 * the gate.  N = 0 or K = 0 is SG_OK; a point of a scene without boxes gets 0 / -1 / -1 whatever its coordinates are.
 *
 * SG_EINVAL: a null pointer, stride < 3, negative sizes, a margin that is negative or not finite, offsets that do not start at 0, do not
 *   ascend or do not end at N / K (host tables, checked on the host before the first launch), a workspace below the _ws_bytes function;
 *   and, through one flag word on the device that is read with the call's synchronisation (the outputs are then undefined): a point of a
 *   scene that has boxes with a coordinate that is not finite, a box value that is not finite, a negative size (0 is valid: a sheet or a
 *   point box holds what lies exactly on it), a row of R with |r.r - 1| > 1e-6 or two rows with |r_i.r_j| > 1e-6, the dot product taken
 *   as l_k above.  Every message names the entry.  SG_EUNSUP: N > 2^24, K > 2^20, B > 2^16.  No stage timer: tools/time_boxlabels.py
 *   brackets the entry with events on the caller's stream. */
size_t sg_points_in_boxes_ws_bytes(int N, int K, int B);
int sg_points_in_boxes(const float* d_xyz, int stride, int N, const double* d_box, int K, const int32_t* h_off_p, const int32_t* h_off_b, int B,
                       double margin, int32_t* d_count, int32_t* d_first, int32_t* d_inner, int32_t* d_held, void* d_ws, size_t ws_bytes,
                       void* stream);

/* Connected components of a scan's graph.  Vertices 0..V-1, 1 <= V <= SG_MAX_CLOUD_POINTS; the undirected graph comes from
 * one of three sources:
 *   sg_components_edges  d_edges int32 [E,2], 0 <= E < 2^30: a row (a, a) is a no-op, duplicates and both orientations are allowed, no order
 *                        is assumed (the ascending-weight lists of sg_overseg_edges / sg_pcseg_edges and lexicographic ones alike).
 *   sg_components_faces  d_faces int32 [F,3]: the three sides of every face; a degenerate face contributes what is left of it.
 *   sg_components_knn    d_knn int32 [N,row] as sg_pointcloud_knn / sg_pointcloud_knn_grid write it (row = k + 1 >= 2), V = N: the pairs
 *                        (i, L[i][t]), t = 1..row-1 (entry 0 is skipped whatever it holds), that have j != i and d2 <= r2, where
 *                        d = p_j - p_i, d2 = (d0*d0 + d1*d1) + d2*d2 and r2 = max_edge * max_edge, fp32, each operation rounded once.
 *                        max_edge = +inf admits every pair.  Points are rows of `stride` >= 3 floats.  This is the kNN graph cut at a
 *                        length, not a radius graph (that one is sg_components_radius below).
 * d_label (may be NULL) int32 [V]: a pair counts only when both ends hold the same value (any value).
 *   d_comp [V] = the lowest vertex index of the vertex's component; d_size [V] (may be NULL) = the component's vertex count, at every
 *   vertex; *h_C = the number of components = #{v : d_comp[v] == v}.  Integers only: the same bytes on every run.  E = 0 and F = 0 are
 *   valid: every vertex is its own component.
 * SG_EINVAL: a null pointer, V < 1, E or F < 0, stride < 3, row < 2, max_edge that is 0, negative or NaN, a workspace below
 *   sg_components_ws_bytes(V) (all before the first HIP call); a vertex index outside 0..V-1, in the kNN form a coordinate that is not
 *   finite (one flag word on the device, read with the call's single synchronisation; the outputs are then undefined).  SG_EUNSUP: V above
 *   SG_MAX_CLOUD_POINTS, E >= 2^30.  SG_EINTERNAL: a chase ran out of its 2 V + 4 steps, which no input can cause.
 * Synchronises the stream once.  Stage times by events, as sg_overseg_set_timing: room for 4 floats (tools/time_components.py). */
size_t sg_components_ws_bytes(int V);          /* 0 when V < 1 or V > SG_MAX_CLOUD_POINTS */
int sg_components_edges(const int32_t* d_edges, long long E, int V, const int32_t* d_label, int32_t* d_comp, int32_t* d_size, int* h_C,
                        void* d_ws, size_t ws_bytes, void* stream);
int sg_components_faces(const int32_t* d_faces, int F, int V, const int32_t* d_label, int32_t* d_comp, int32_t* d_size, int* h_C,
                        void* d_ws, size_t ws_bytes, void* stream);
int sg_components_knn(const float* d_points, int stride, const int32_t* d_knn, int N, int row, float max_edge, const int32_t* d_label,
                      int32_t* d_comp, int32_t* d_size, int* h_C, void* d_ws, size_t ws_bytes, void* stream);
int sg_components_set_timing(int on);
int sg_components_stage_times(float* h_us, int cap);
const char* sg_components_stage_name(int i);

/* Geodesic distances over a scan's graph: multi-source shortest paths along the edges, and which seed owns a vertex.
 * Vertices 0..V-1, 1 <= V <= SG_MAX_CLOUD_POINTS.  d_edges int32 [E,2], 0 <= E <= 2^26, with sg_components_edges' rules: any order,
 * duplicates and both orientations allowed, a row (a, a) is a no-op -- the rows of adj.pth.  The graph is undirected: a row gives two arcs.
 * WEIGHTS, at most one of the two:
 *   d_xyz     rows of `stride` >= 3 floats: the length of a row (a, b) in double, d = (double)p_a - (double)p_b,
 *             w = sqrt((d0*d0 + d1*d1) + d2*d2), each operation rounded once, nothing contracted; symmetric by construction.
 *   d_weight  double [E]: finite and >= 0; duplicate rows may carry different weights and all of them count.
 *   neither   every arc weighs 1.0: distances are hop counts, exact integers.
 * SEEDS: d_seed int32 [V]; v is a seed iff d_seed[v] >= 0 (a weak-label `ins` vector passes as it is).
 *
 * THE RULE for d_dist (double [V]): the unique greatest solution of D(s) = 0 for seeds and D(v) = min over arcs (u, v) of D(u) + w(u, v),
 *   every addition rounded once -- what Dijkstra in double gives (tests/geodesic_ref.py).  A vertex no seed reaches has +inf.  fl(d + w) is
 *   monotone in d and never below d, so the relaxation's fixed point from +inf is unique: the minimum over walks of the left-to-right
 *   rounded sum, whatever the order of the updates.  max_dist is +inf for none, else finite and >= 0: a candidate ABOVE it is not taken,
 *   and the result is the unlimited one with every D > max_dist replaced by +inf (prefixes of a best walk are never longer than it).
 * THE RULE for d_owner (int32 [V]): an arc (u, v) is TIGHT iff D(v) is finite and D(u) + w(u, v) == D(v), the same double addition;
 *   owner(v) is the lowest seed (its vertex index) from which v is reached over tight arcs: the least solution of O(s) <= s for seeds and
 *   O(v) = min over tight arcs (u, v) of O(u).  An unreached vertex has -1.  Two phases on purpose: a pair (D, owner) relaxed together
 *   depends on the order when two sums round to one value; integers and a minimum do not.  Zero weights and absorbed weights
 *   (1.0 + 1e-20 == 1.0) make tight cycles; the rule covers them.
 * The same bytes on every run and every stream.  E = 0 and "no seed" are SG_OK: with E = 0 a seed owns itself, all else is +inf / -1.
 *
 * sg_graph_geodesic_stats: the calling thread's last call, int64: h[0] arcs kept (two a row that is no self loop), h[1] distance launches,
 *   h[2] owner launches, h[3] tight arcs, h[4] reached vertices; returns 5.  The launch counts are launches ENQUEUED: whole batches, so up to
 *   a batch less one more than the launch that first changed nothing.  They are informative: they may differ from run
 *   to run, the outputs may not.
 * SG_EINVAL, on the host before the first HIP call: a null pointer where one is needed, V < 1, E < 0, stride < 3 with d_xyz, both d_xyz
 *   and d_weight, max_dist that is NaN or negative, a workspace below the _ws_bytes function; through one flag word on the device, read
 *   with the call's last synchronisation (the outputs are then undefined; such a row is dropped, never used): a vertex index outside
 *   0..V-1, a weight that is negative or not finite, a coordinate of an edge's end that is not finite.  SG_EUNSUP: V above
 *   SG_MAX_CLOUD_POINTS, E > 2^26.  SG_EINTERNAL: more than V + 1 launches of either phase, which no input can cause.  Every message names
 *   the entry.  The stream is synchronised once per batch of relaxation launches.  No stage timer: tools/time_geodesic.py brackets the
 *   entry with events on the caller's stream. */
/* The workspace function does not know the metric, so it always holds room for one double weight per arc (16 E bytes, 1 GB at the limit),
 * which a call by hops leaves unused. */
size_t sg_graph_geodesic_ws_bytes(int V, long long E);      /* 0 outside the envelope */
int sg_graph_geodesic(const int32_t* d_edges, long long E, int V, const float* d_xyz, int stride, const double* d_weight, const int32_t* d_seed,
                      double max_dist, double* d_dist, int32_t* d_owner, void* d_ws, size_t ws_bytes, void* stream);
int sg_graph_geodesic_stats(int64_t* h, int cap);           /* the calling thread's last call */

/* A scan and its labels as images: a z-buffer rasteriser of the scan's triangles, or of its points as square splats, into
 * B views of W x H pixels in one call.  d_xyz rows of `stride` >= 3 floats, vertices 0..V-1; d_faces int32 [F,3] with F > 0 draws triangles,
 * d_faces NULL with F == 0 draws every point as a splat of side `point_size` (odd, 1..15; ignored for triangles).  h_cam HOST double [B,16]:
 * T, a row-major 3 x 4 world->camera matrix, then fx fy cx cy.  The camera looks along +z, x to the right, y down.  Outputs [B,H,W]:
 * d_prim int32 (the winning face or point, -1 where empty), d_depth float (+inf where empty; may be NULL), d_vert int32 (a vertex index,
 * -1 where empty; may be NULL), and d_hits int32 [V] or NULL: the pixels of all B views whose d_vert is v.
 *
 * THE RULE (tests/render_ref.py restates it).  Everything is in double unless said otherwise, each operation rounded once, nothing
 * contracted; all integer work is int64.
 *   CAMERA SPACE   c_k = ((T[k][0]*x + T[k][1]*y) + T[k][2]*z) + T[k][3], k = 0, 1, 2.
 *   REJECTION      checked in this order.  A vertex with a coordinate that is not finite, with a c_k that is not finite, or with
 *                  c_2 <= near (a NaN counts as such) is BEHIND.  Otherwise u, v are formed, and a vertex with |u| or |v| above 16384 (or
 *                  NaN) is FAR.  A primitive with a behind or far vertex is dropped whole and counted once: as behind if any of its
 *                  vertices is behind, otherwise as far.  Nothing is clipped.  Both projections count alike, and `near` applies to both.
 *   SCREEN         perspective u = fx*(c_0/c_2) + cx, v = fy*(c_1/c_2) + cy; orthographic u = fx*c_0 + cx, v = fy*c_1 + cy.  Fixed point:
 *                  X = (int)floor(u*256.0 + 0.5), Y likewise.  |X|, |Y| <= 2^22, so every edge function stays below 2^47 and converts to
 *                  double exactly.
 *   COVERAGE       the centre of pixel (px, py) is C = (256*px + 128, 256*py + 128).  With corners P_0, P_1, P_2 in the face's order,
 *                  w_i = (X_k - X_j)*(C_y - Y_j) - (Y_k - Y_j)*(C_x - X_j) for (i, j, k) = (0, 1, 2), (1, 2, 0), (2, 0, 1): the edge
 *                  function opposite corner i.  A = w_0 + w_1 + w_2, the same for every pixel.  A == 0 is DEGENERATE: dropped.  A < 0:
 *                  all four are negated (two-sided).  The pixel is covered iff every w_i >= 0: a centre on an edge is inside, and since
 *                  nothing is blended no fill rule is needed.
 *   DEPTH          perspective s = ((double)w_0*(1.0/z_0) + (double)w_1*(1.0/z_1)) + (double)w_2*(1.0/z_2), zp = 1.0 / (s / (double)A);
 *                  orthographic s over z_i in the same order, zp = s / (double)A.  z_i is c_2 of corner i.  depth = (float)zp: not
 *                  negative, so its bits order as uint32.
 *   WINNER         key = (bits(depth) << 32) | primitive index; a pixel keeps the least key of the primitives that cover it: the nearest,
 *                  and at equal float depth the lower index.  An empty pixel has d_prim -1, d_depth +inf, d_vert -1.
 *   d_vert         the corner of the winning face with the largest w_i at that pixel, a tie to the lower corner position, as its vertex index.
 *   SPLATS         point i covers the square of side point_size centred on pixel (X >> 8, Y >> 8) (arithmetic shifts), clipped to the
 *                  image; depth = (float)c_2; d_prim = d_vert = i.
 *   d_hits[v]      the number of pixels over all B views whose d_vert is v: integer adds.
 * The same bytes on every run and every stream.  No primitive in view is SG_OK and an empty image.
 *
 * sg_render_stats: the calling thread's last call, int64, summed over the views: h[0] primitives kept, h[1] behind, h[2] far,
 *   h[3] degenerate, h[4] LARGE -- kept triangles whose clipped box (the pixels whose centres lie inside the corners' bounding box, clipped
 *   to the image) is wider or higher than the small-primitive threshold, 8 --, h[5] covered pixels; returns 6.  None depends on the
 *   schedule.  sg_render_set_tuning(1..32) sets that threshold for the whole PROCESS, 0 restores the build's: a knob of
 *   tools/time_render.py, not part of the interface.  h[4] (LARGE) is counted against the threshold in force, so it depends on the knob;
 *   the images and the other five counts do not.
 * SG_EINVAL, on the host before the first HIP call: a null pointer where one is needed, V, B, W or H < 1, F < 0, stride < 3, faces without
 *   F or F without faces, a point_size that is even or outside 1..15 (splats), near that is not finite or <= 0, a camera number that is
 *   not finite, fx or fy == 0, a workspace below the _ws_bytes function; through one flag word on the device, read at the call's one
 *   synchronisation (the outputs are then undefined): a face index outside 0..V-1; such a face is dropped and never dereferenced.
 *   SG_EUNSUP: V above SG_MAX_CLOUD_POINTS, F > 2^26, B > 64, W or H > 4096, B*H*W > 2^26.  Every message names the entry.
 * The workspace holds 16 bytes per (view, vertex), 8 per pixel and 4 per (view, face): sg_render_ws_bytes(V, F, B, W, H), F = 0 for splats. */
size_t sg_render_ws_bytes(int V, long long P, int B, int W, int H);     /* 0 outside the envelope */
int sg_render(const float* d_xyz, int stride, int V, const int32_t* d_faces, long long F, int point_size, int B, const double* h_cam, int ortho,
              double near, int W, int H, int32_t* d_prim, float* d_depth, int32_t* d_vert, int32_t* d_hits, void* d_ws, size_t ws_bytes, void* stream);
int sg_render_stats(int64_t* h, int cap);                   /* the calling thread's last call */
int sg_render_set_tuning(int small);
/* d_img uint8 [n,3]: pixel i takes h_background (3 bytes, host) where d_vert[i] is outside 0..V-1 (an empty pixel's -1), else the colour of
 * its vertex: exactly one of d_cidx (uint8 [V], a palette index 0..40 as sg_colour_vector_apply leaves it) and d_rgb (uint8 [V,3]).
 * 0 <= n <= 2^26.  No synchronisation. */
int sg_render_colour(const int32_t* d_vert, long long n, const uint8_t* d_cidx, const uint8_t* d_rgb, int V, const uint8_t* h_background,
                     uint8_t* d_img, void* stream);

/* 2D label images onto a scan's vertices: the way back from sg_render's images.  Every vertex is projected into every view,
 * the view's depth image decides whether the view sees it, the label under it is a vote.  d_xyz rows of `stride` >= 3 floats, vertices
 * 0..V-1; h_cam HOST double [B,16], `ortho` and `near` as sg_render takes them; d_label int32 [B,H,W] (negative: no label; every other value
 * is below C); d_depth float [B,H,W], z-depth in the unit of the coordinates: what sg_render writes (+inf where empty) or what a sensor
 * gives (0 or NaN where invalid); d_counts uint32 [V,C] and d_seen int32 [V].  The call ACCUMULATES into d_counts and d_seen -- the caller
 * clears them --, so any number of views goes through in calls of at most 64.
 *
 * THE RULE (tests/lift_ref.py restates it).  For every (view b, vertex v), decided in this order:
 *   PROJECTION     sg_render's CAMERA SPACE, REJECTION and SCREEN, the same function (csrc/render_project_device.h): the vertex is BEHIND, or
 *                  FAR, or has X, Y in 1/256 pixel and its depth c_2, all in double.
 *   PIXEL          px = X >> 8, py = Y >> 8 (arithmetic shifts): the pixel a splat of size 1 lands on.  Outside 0..W-1 x 0..H-1 the pair is
 *                  OUTSIDE.
 *   DEPTH          d = d_depth[b,py,px].  NODEPTH unless d is finite and d > 0.
 *   OCCLUSION      OCCLUDED iff fabs(c_2 - (double)d) > tol, in double.  Equality is visible.
 *   VISIBLE        otherwise.  l = d_label[b,py,px].  l >= C raises the flag word: the pair adds NOTHING (not to d_seen, not to d_counts),
 *                  nothing is indexed by l, and the call returns SG_EINVAL.  Else d_seen[v] += 1, and l < 0 is UNLABELLED (seen, no vote),
 *                  l >= 0 is LABELLED: d_counts[v*C + l] += 1.
 * All additions are integer atomics, so the result is the same bytes under any schedule and on any stream.
 * sg_lift_stats: the calling thread's last call, int64, summed over the views: h[0] behind, h[1] far, h[2] outside, h[3] nodepth,
 *   h[4] occluded, h[5] visible WITHOUT a label (seen, no vote), h[6] labelled (seen, one vote); returns 7.  The seven are disjoint and sum
 *   to B*V; h[5] + h[6] is what the call added to d_seen, h[6] what it added to d_counts.  After a refused call all are 0.
 * SG_EINVAL, on the host before the first HIP call: a null pointer, V, B, W, H or C < 1, stride < 3, near that is not finite or <= 0, tol
 *   that is not finite or < 0, a camera number that is not finite, fx or fy == 0, a workspace below sg_lift_ws_bytes(V, B); through the flag
 *   word, read at the call's ONE stream synchronisation: a visible pixel's label >= C (the other pairs have been added as the rule says).
 *   SG_EUNSUP: V above SG_MAX_CLOUD_POINTS, B > 64, W or H > 4096, B*H*W > 2^26, C > 4096, V*C > 2^31.  Every message names the entry.
 *
 * sg_lift_vote: per vertex, int32 [V] each: d_winner the class with the most votes, a tie to the LOWEST class, -1 where the row is all
 *   zero; d_votes the winner's votes (0 with no winner); d_total the row's sum; d_tied 1 iff another class holds as many votes as the
 *   winner, else 0.  The same limits on V and C.  No synchronisation. */
size_t sg_lift_ws_bytes(int V, int B);                      /* 0 outside the envelope */
int sg_lift(const float* d_xyz, int stride, int V, int B, const double* h_cam, int ortho, double near, int W, int H, const int32_t* d_label,
            const float* d_depth, double tol, int C, uint32_t* d_counts, int32_t* d_seen, void* d_ws, size_t ws_bytes, void* stream);
int sg_lift_stats(int64_t* h, int cap);                     /* the calling thread's last call */
int sg_lift_vote(const uint32_t* d_counts, int V, int C, int32_t* d_winner, int32_t* d_votes, int32_t* d_total, int32_t* d_tied, void* stream);

/* The radius graph on the exact grid index: every pair of points i != j with d2 <= r2, where d = p_j - p_i,
 * d2 = (d0*d0 + d1*d1) + d2*d2 and r2 = radius * radius, fp32, each operation rounded once -- sg_components_knn's pair predicate over ALL
 * pairs of the cloud, not over a kNN table.  Coincident points are neighbours.  Points are rows of `stride` >= 3 floats,
 * 1 <= N <= SG_MAX_GRID_POINTS.  No adjacency is written; two results are computed inside the search:
 *   sg_radius_count_grid   d_count int32 [N]: the number of j that pass for i (the radius outlier filter's figure; below 2^24).
 *   sg_components_radius   the connected components of that graph: d_comp, d_size (may be NULL) and *h_C exactly as sg_components_edges
 *                          leaves them; d_label (may be NULL) int32 [N] keeps only the pairs whose ends hold the same value.
 * The index is sg_pointcloud_knn_grid's (box, cells, sort, dense table).  A query reads the block of Chebyshev radius R round its cell,
 * R the smallest block that no passing point can lie outside of for the cell edge in use, computed on the host and the same for every
 * query: no queue, no fallback.  cell = 0: the library picks the edge just large enough for R = 1 and enlarges it only until the grid
 * fits the table; cell > 0 forces it and may give R > 1.  Integers only: the same bytes on every run, for every cell edge and stream.
 * SG_EINVAL (before the first HIP call): a null pointer, stride < 3, N < 1, a radius that is not finite and positive or whose fp32 square
 *   is not finite or below 2^-100, a cell edge that is negative or not finite; (on the device, one flag word, the library stays usable) a
 *   coordinate that is not finite.  SG_ENOMEM: a workspace below sg_radius_grid_ws_bytes(N) (0 outside the envelope; one size serves both
 *   entry points).  SG_EUNSUP: N above SG_MAX_GRID_POINTS; an extent of the cloud that is not finite; a forced cell that needs R > 16, that
 *   gives an axis 2^21 cells or more, or more cells than the dense table's max(2^22, 4 N) -- the message says which.  SG_EINTERNAL: a chase
 *   ran out of its 2 N + 4 steps, which no input can cause.
 * Synchronises the stream twice (the box; the end).  Stage times by events, as sg_overseg_set_timing: room for 7 floats (box, cells, sort,
 * table, init, search, finish).  sg_radius_grid_stats: the calling thread's last call of either entry point -> h[0..2] cells per axis,
 *   h[3] occupied cells, h[4] the largest cell, h[5] the bits of the fp32 cell edge, h[6] R, h[7] pair tests evaluated, h[8] pairs passed
 *   (ordered pairs: the sum of the counts; h[7] and h[8] are counted in timed calls only). */
size_t sg_radius_grid_ws_bytes(int N);         /* 0 when N < 1 or N > SG_MAX_GRID_POINTS */
int sg_radius_count_grid(const float* d_points, int stride, int N, float radius, float cell, int32_t* d_count, void* d_ws, size_t ws_bytes,
                         void* stream);
int sg_components_radius(const float* d_points, int stride, int N, float radius, float cell, const int32_t* d_label, int32_t* d_comp,
                         int32_t* d_size, int* h_C, void* d_ws, size_t ws_bytes, void* stream);
int sg_radius_grid_set_timing(int on);
int sg_radius_grid_stage_times(float* h_us, int cap);
const char* sg_radius_grid_stage_name(int i);
int sg_radius_grid_stats(int64_t* h, int cap);

/* The radius graph written down, and the point-cloud over-segmenter over it.
 * sg_radius_neighbours_grid: the pairs of sg_radius_count_grid as lists in CSR form.  d_off int64 [N + 1] = the exclusive sum of the counts,
 *   T = off[N]; d_idx int32 [T]: the row of i holds its neighbours in ASCENDING INDEX whatever the cell edge.  d_off and *h_T are always
 *   written.  With T > capacity (capacity = 0 and d_idx = NULL is the query form) nothing is written to d_idx and the call returns SG_ENOMEM
 *   with T in *h_T.  Order of a call: index, count, a 64-bit scan, T read back (one synchronisation), fill in search order, every row
 *   ordered by rank (one wave per row; the work of a row is its length squared / 64).
 *   Refusals before the first HIP call: sg_radius_count_grid's, a negative capacity, room at a null d_idx, a workspace below
 *   sg_radius_neighbours_ws_bytes(N, capacity) (SG_ENOMEM), a capacity above SG_MAX_RADIUS_PAIRS (SG_EUNSUP).  T above SG_MAX_RADIUS_PAIRS is
 *   SG_EUNSUP once T is known; the message names the two ways out: a smaller radius, or thinning the cloud first (sg_thin_*).  The cap keeps
 *   E = T / 2, 2 E and every int the weight sort and sg_overseg_merge form from E below 2^31.
 * sg_pointcloud_normals_csr: d_normals [N,3] from d_xyz [N,3] and such lists: the neighbourhood of i is i itself, then its row in stored
 *   order; mean, covariance and eigenvector as sg_pointcloud_normals.  A caller's lists are checked on the device: an entry outside 0..N-1
 *   or offsets that do not ascend from 0 to off[N] are SG_EINVAL, and nothing is read through them.  d_ws: sg_pointcloud_knn_ws_bytes(N).
 * sg_pcseg_edges_radius / sg_pcseg_scan_radius: sg_pcseg_edges_indexed / sg_pcseg_scan_indexed over the radius graph: `radius`, `cell` and a
 *   pair capacity (d_edges and d_w hold capacity / 2 edges) in place of k and index; d_off / d_idx may both be NULL.  *h_T as above; SG_ENOMEM
 *   with T > capacity.  d_ws: sg_pcseg_ws_bytes_radius(N, capacity) (0 outside the envelope).
 * Stage times by events, as sg_pcseg_set_timing: room for 13 floats (box, cells, sort, table, count, scan, fill, rows, normals, edges,
 *   weights, weight_sort, gather; tools/time_pcseg_radius.py). */
#define SG_MAX_RADIUS_PAIRS (1ll << 30)
size_t sg_radius_neighbours_ws_bytes(int N, int64_t capacity);
int sg_radius_neighbours_grid(const float* d_points, int stride, int N, float radius, float cell, int64_t capacity, int64_t* d_off,
                              int32_t* d_idx, int64_t* h_T, void* d_ws, size_t ws_bytes, void* stream);
int sg_pointcloud_normals_csr(const float* d_xyz, int N, const int64_t* d_off, const int32_t* d_idx, const float* h_viewpoint, float* d_normals,
                              void* d_ws, size_t ws_bytes, void* stream);
size_t sg_pcseg_ws_bytes_radius(int N, int64_t T);
int sg_pcseg_edges_radius(const float* d_xyz, int N, float radius, float cell, int64_t capacity, const float* h_viewpoint, int64_t* d_off,
                          int32_t* d_idx, float* d_normals, int32_t* d_edges, float* d_w, int* h_E, int64_t* h_T, void* d_ws, size_t ws_bytes,
                          void* stream);
int sg_pcseg_scan_radius(const float* d_xyz, int N, float radius, float cell, int64_t capacity, const float* h_viewpoint, float k_thresh,
                         int seg_min_verts, int32_t* h_seg_indices, int64_t* h_T, void* d_ws, size_t ws_bytes, void* stream);
int sg_pcseg_radius_set_timing(int on);
int sg_pcseg_radius_stage_times(float* h_us, int cap);
const char* sg_pcseg_radius_stage_name(int i);

/* Segment vote: what re-keying a scan's annotations onto another over-segmentation needs on the device.  Every vertex has a
 * row id d_ids[v] (any non-negative int32: not contiguous, may exceed V) and a column d_cols[v] in 0..n_cols-1; both are checked on the
 * device (SG_EINVAL).  Rows come out in ascending id order, *h_R of them; every output needs room for V entries.
 *   per vertex  d_rank = the position of its id among the sorted distinct ids, d_vertex_winner = the winner of its row
 *   per row     d_row_ids, d_row_count = its vertices, d_winner = the column most of its vertices hold (ties: the lowest column),
 *               d_winner_count, d_distinct = how many columns it holds, d_tied = 1 when another column is as frequent as the winner,
 *               d_first_vertex = the lowest vertex of the row that holds the winner
 * Integers only, the same bytes on every run, O(V) memory (no rows x columns table).  Synchronises the stream twice (check, row count); the
 * outputs are ordered on the stream.  sg_segment_rank is the first half alone: ranks, ids and counts.
 * sg_rekey_clicks (host, no GPU needed): click i was made on source segment h_click_seg[i] at raw vertex h_click_point[i].  A point
 *   inside 0..V-1 whose source segment is that one keeps the point and lands on h_new_seg[point] (how = 0); otherwise the click lands on
 *   the new segment that holds most of the source segment -- row tables of the vote with rows = source segments, columns = ranks of the new
 *   ones: h_row_ids ascending, h_row_winner in 0..S-1 indexing h_new_ids, h_row_first -- at that intersection's lowest vertex (how = 1); a
 *   source segment without a row is dropped (how = 2, outputs -1).  The arrays are untrusted (SG_EINVAL). */
size_t sg_segment_vote_ws_bytes(int V);
int sg_segment_rank(const int32_t* d_ids, int V, int32_t* d_rank, int32_t* d_row_ids, int32_t* d_row_count, int* h_R, void* d_ws,
                    size_t ws_bytes, void* stream);
int sg_segment_vote(const int32_t* d_ids, const int32_t* d_cols, int V, int n_cols, int32_t* d_rank, int32_t* d_vertex_winner,
                    int32_t* d_row_ids, int32_t* d_row_count, int32_t* d_winner, int32_t* d_winner_count, int32_t* d_distinct, int32_t* d_tied,
                    int32_t* d_first_vertex, int* h_R, void* d_ws, size_t ws_bytes, void* stream);
/* Stage times of sg_segment_vote by events (tools/time_rekey.py), as sg_overseg_set_timing: room for 7 floats. */
int sg_segment_vote_set_timing(int on);
int sg_segment_vote_stage_times(float* h_us, int cap);
const char* sg_segment_vote_stage_name(int i);
int sg_rekey_clicks(const int32_t* h_src_seg, const int32_t* h_new_seg, int V, const int32_t* h_row_ids, const int32_t* h_row_winner,
                    const int32_t* h_row_first, int R, const int32_t* h_new_ids, int S, const int64_t* h_click_seg,
                    const int64_t* h_click_point, int n, int32_t* h_out_seg, int32_t* h_out_point, int32_t* h_out_how);

/* Segment graph of a scan: the scan's edge list contracted through the per-vertex segment number, with counts.  d_adj holds
 * the rows of <scene>.adj.pth (int64 [E,2], 16-byte aligned), d_seg the segment number of every vertex: 0..S-1, negative = no segment.  For
 * every row (u, v) let a = d_seg[u], b = d_seg[v]; the row counts when a >= 0, b >= 0 and a != b.  d_pairs = the distinct
 * (min(a,b), max(a,b)) in ascending lexicographic order, d_cross[i] = the number of rows behind pair i (duplicate rows and both
 * orientations each count), *h_P = the number of pairs.  Rows (u, u) and rows inside one segment are dropped; E = 0 gives P = 0.  d_pairs
 * needs room for E rows of 2, d_cross for E words.  Integers only: the same bytes on every run and every stream.
 * Refused before the first HIP call: SG_EINVAL for null pointers, E < 0, S < 1, V < 1; SG_EUNSUP for S > 2^20 or E >= 2^31 (and later
 * for more than 2^30 crossing rows); SG_ENOMEM for a workspace below sg_segment_graph_ws_bytes(E, S) (0 outside those limits).
 * Refused from the device (one flag word): SG_EINVAL for a vertex index outside 0..V-1 or a segment number >= S; nothing is read
 * through either.  Sort-based (csrc/kernels_seggraph.hip): O(E) memory, where sg_contract_point_edges keeps S * S bits and no counts.
 * Synchronises the stream twice: after the key pass (flag word, crossing rows) and at the end (pairs).
 * sg_click_clusters (host, no GPU needed): the clusters of every instance's segments over that graph, in the list order and member order of
 *   the reference's group_adjacency_segs.  h_pairs: P rows (a, b), a < b, strictly ascending; h_seg_ins[s] = the instance of segment s,
 *   <= 0 = in no cluster.  Instances are visited in ascending value, inside one its segments in ascending number; segment s opens the
 *   list [s], and every list that holds a neighbour t < s of the same instance (ascending t) is appended to it whole.  -> *h_C clusters in
 *   the order their first (= highest) segments were visited: members h_cl_members[h_cl_off[c] .. h_cl_off[c+1]), instance h_cl_ins[c].
 *   Room: h_cl_off [S+1], h_cl_members [S], h_cl_ins [S].  The arrays are untrusted (SG_EINVAL). */
size_t sg_segment_graph_ws_bytes(long long E, int S);
int sg_segment_graph(const int64_t* d_adj, long long E, const int32_t* d_seg, int V, int S, int32_t* d_pairs, int32_t* d_cross, long long* h_P,
                     void* d_ws, size_t ws_bytes, void* stream);
/* Stage times of sg_segment_graph by events (tools/time_clicks.py), as sg_overseg_set_timing: room for 4 floats. */
int sg_segment_graph_set_timing(int on);
int sg_segment_graph_stage_times(float* h_us, int cap);
const char* sg_segment_graph_stage_name(int i);
int sg_click_clusters(const int32_t* h_pairs, long long P, const int32_t* h_seg_ins, int S, int32_t* h_cl_off, int32_t* h_cl_members,
                      int32_t* h_cl_ins, int* h_C);

/* =============================================================================================
 * Training step, operator level: the train-mode tail of SegModel.forward + its backward, and the backward
 * of every operator in front of it (group max, point->cluster max, GCN, EdgeConv MLP2 / MLP3, MLP1); further down the whole step
 * as one object (sg_trainer_*) and the optimizers.  The DDP gradient all-reduce (train.py:88) is the host side's: one
 * torch.distributed all-reduce of the flat gradient vector over RCCL (seggroup_amd/trainer.py).
 * ============================================================================================= */
typedef struct sg_classifier {    /* DEVICE pointers, float32, row-major (model.py:154-166)                         */
    const float* w1;                /* linear1.weight [128,256] (no bias)                                          */
    const float* gamma;             /* bn1.weight [128]                                                            */
    const float* beta;              /* bn1.bias   [128]                                                            */
    const float* w2;                /* linear2.weight [40,128]                                                     */
    const float* b2;                /* linear2.bias   [40]                                                         */
} sg_classifier;

/* model.py:900-932 with Classifier.forward (154-166) and cross_entropy_loss(smoothing=True) (util.py:12-29):
 *   d_feat5 [C,256]   Feat_5, the final clusters' features
 *   d_group [C]       instance slot of every final cluster: rank of its weak instance label among the sorted unique labels
 *                     (np.unique(ins_list), model.py:909; an unlabeled cluster's -1 is a label like any other)
 *   d_gold  [K]       semantic class of every slot (the first cluster's, model.py:913-914)
 *   d_keep  [K,128]   dropout keep mask ALREADY scaled by 1 / (1 - p) (0 or 2 for p = 0.5); NULL = no dropout.  The reference
 *                     draws it from torch's RNG stream; parity is stated with the same mask on both sides.
 * BatchNorm1d uses batch statistics over the K instances (K < 2: SG_EUNSUP, torch raises ValueError there).
 * Writes d_loss[2] = {loss_sum, K} (the reference's `loss [1,2]`), optionally d_logits [K,40]; keeps the activations the
 * backward needs in d_ws (sg_train_tail_ws_bytes). */
size_t sg_train_tail_ws_bytes(int C, int K);
int sg_train_tail_forward(const float* d_feat5, int C, const int32_t* d_group, int K, const int32_t* d_gold, const float* d_keep,
                          const sg_classifier* cls, float* d_logits, float* d_loss, void* d_ws, size_t ws_bytes, void* stream);
/* gradients of loss = scale * loss_sum (train.py:166: scale = 1 / loss_num) w.r.t. the five classifier tensors and Feat_5
 * [C,256]; d_ws as left by the forward call of the same scene */
int sg_train_tail_backward(int C, int K, const int32_t* d_gold, const float* d_keep, const sg_classifier* cls, float scale,
                           float* d_gw1, float* d_ggamma, float* d_gbeta, float* d_gw2, float* d_gb2, float* d_gfeat5,
                           void* d_ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The reference's module-level functions with arguments its own forward never passes (the Python
 * surface keeps the reference's signatures: seggroup_amd/functional.py).  Plain kernels, off every
 * timed path (csrc/kernels_general.hip).
 *   sg_group_mean_rows : aggregate_cluster_feature(use_avg=True), model.py:282-284 -- the mean of each
 *       group's rows (arguments as sg_group_max_rows); the caller concatenates [max | mean].
 *   sg_fps_general     : farthest_point_sampling(pts, k, initial_idx, skip_initial), model.py:329-395 for one
 *       cloud d_pts [n,dim]: d_indices [k]; d_distances [k,n] or NULL (the reference's second return value);
 *       l2_norm in NumPy's order, np.argmax's first-index ties.  d_ws needs sg_fps_general_ws_bytes(n).
 *   sg_knn_general     : knn(x, k), model.py:30-36 for x [B,C,n] of any channel count: d_idx [B,n,k] int64, scores
 *       (-|a|^2 - (-2 a.b)) - |b|^2 descending, lower index first among equal scores (torch.topk leaves that open);
 *       1 <= k <= min(n, 128), otherwise SG_EUNSUP.
 * ------------------------------------------------------------------------------------------- */
int sg_group_mean_rows(const float* d_rows, int row_stride, int D, const int32_t* d_goff, const int32_t* d_gidx, int G,
                       float* d_out, int out_stride, void* stream);
size_t sg_fps_general_ws_bytes(int n);
int sg_fps_general(const float* d_pts, int n, int dim, int k, int initial_idx, int skip_initial, int32_t* d_indices,
                   float* d_distances, void* d_ws, size_t ws_bytes, void* stream);
int sg_knn_general(const float* d_x, int B, int C, int n, int k, int64_t* d_idx, void* stream);

/* backward of sg_group_max_rows (aggregate_cluster_feature, model.py:278-288): the gradient of a group's maximum goes to its
 * first maximal row (torch.max), every other row of the group gets 0; d_grows rows of `grow_stride` floats.
 * Both backward maxima (this one and sg_segment_max_backward) compare BY VALUE, as torch.max does: -0.0 == +0.0, so of a
 * {-0.0, +0.0} pair the FIRST row wins, as among any equal values (duplicates, rows that are all -inf).  A row id may be listed
 * more than once in a group (sg_group_max_rows allows it): the row receives the gradient iff one of its positions is the first
 * maximal position of the list, and a later position of the same row does not clear it (autograd of x[ids].max(0)).  The groups
 * of one call share no row.  An empty group writes nothing, and a row in no group is NOT written: the caller zeroes d_grows
 * where that matters. */
int sg_group_max_rows_backward(const float* d_rows, int row_stride, int D, const int32_t* d_goff, const int32_t* d_gidx, int G,
                               const float* d_gout, int out_stride, float* d_grows, int grow_stride, void* stream);
/* backward of sg_segment_max (model.py:793,834): rows [N,D] in member order, cluster c = rows [d_cl_off[c], d_cl_off[c+1]) with
 * d_cl_off[0] = 0 and d_cl_off[C] = N; the gradient of a cluster's maximum goes to its first maximal row, by value (above), whatever
 * the order in which the blocks' atomics arrive.  Every other entry of d_grows [N,D] is set to 0, an empty cluster sends nothing;
 * with C == 0 or N == 0 nothing is written.  d_ws needs sg_segment_max_backward_ws_bytes(C, D). */
size_t sg_segment_max_backward_ws_bytes(int C, int D);
int sg_segment_max_backward(const float* d_rows, int N, int D, const int32_t* d_cl_off, int C, const float* d_gout, int out_stride,
                            float* d_grows, void* d_ws, size_t ws_bytes, void* stream);
/* backward of sg_gcn_forward, INCLUDING the path through the similarity weights exp(-alpha ||x_a - x_b + 1e-6||) and their
 * row normalisation (autograd differentiates them in the reference: model.py:262-265,305-309): d_gx [S,D], d_gw [D,D] */
size_t sg_gcn_backward_ws_bytes(int S, int D, int E);
int sg_gcn_backward(const float* d_x, int S, int D, const int32_t* d_adj, int E, const int32_t* d_rowptr, const int32_t* d_col,
                    const int32_t* d_eid, const float* d_w, float alpha, const float* d_gout, float* d_gx, float* d_gw,
                    void* d_ws, size_t ws_bytes, void* stream);

/* backward of sg_mlp1_forward w.r.t. its parameters (MLP1, model.py:39-80; batch-statistics BatchNorm2d over all C*64*10 rows):
 *   d_gfeat rows of g_stride floats: gradient w.r.t. Feat_1 [C,128] ([max | mean] over the 64 samples)
 *   d_gw [64,6], d_gg [64], d_gb [64];  d_bn_stats [128] or NULL = batch mean | biased variance of the conv output
 * d_ws needs sg_mlp1_backward_ws_bytes(C). */
size_t sg_mlp1_backward_ws_bytes(int C);
int sg_mlp1_backward(const float* d_samples, int C, const float* d_w, const float* d_gamma, const float* d_beta, const float* d_gfeat,
                     int g_stride, float* d_gw, float* d_gg, float* d_gb, float* d_bn_stats, void* d_ws, size_t ws_bytes, void* stream);

/* backward of sg_edgeconv_forward (get_graph_feature2 + MLP2 / MLP3, model.py:83-138; autograd differentiates it in the reference's
 * training step, train.py:167).  The inputs carry no gradient: parameter gradients only.
 *   d_x9m [N,12], d_knn [N,k]   as for the forward call
 *   d_gout [N,64]               gradient w.r.t. the op's OUTPUT (the post-activation max over k), e.g. from sg_segment_max_backward
 *   d_gw1 [64,18] d_gg1 d_gb1 [64]; layers == 2: d_gw2 [64,64] d_gg2 d_gb2 [64]
 *   d_bn2_in [128] or NULL      layers == 2: batch mean | biased variance of the SECOND BatchNorm's input as the forward computed
 *                               them (sg_trainer's tape); given, the dense forward pass that would recompute them is skipped
 *   d_bn_stats [256] or NULL    batch mean1 | biased var1 | mean2 | var2 (for the running-statistics update, momentum 0.1)
 * BatchNorm2d is differentiated WITH its batch statistics over all N*k rows (training mode).  Deterministic (ordered fp64
 * reductions).  d_ws needs sg_edgeconv_backward_ws_bytes(N). */
size_t sg_edgeconv_backward_ws_bytes(int N);
int sg_edgeconv_backward(const float* d_x9m, const int32_t* d_knn, int N, int k, int layers, const float* d_w1, const float* d_g1,
                         const float* d_b1, const float* d_w2, const float* d_g2, const float* d_b2, const float* d_gout, float* d_gw1,
                         float* d_gg1, float* d_gb1, float* d_gw2, float* d_gg2, float* d_gb2, const float* d_bn2_in, float* d_bn_stats,
                         void* d_ws, size_t ws_bytes, void* stream);

/* cross_entropy_loss (util.py:12-29) on its own: sum over the K rows of -sum_c t_c log softmax(logits)_c with the smoothed target
 * (0.8 on the gold class, 0.2 / (C - 1) elsewhere) or, smoothing == 0, the one-hot target.  d_prob [K,C] receives the softmax
 * (what the backward needs); backward: d_glogits = scale * (softmax - target). */
int sg_cross_entropy_forward(const float* d_logits, int K, int C, const int32_t* d_gold, int smoothing, float* d_prob, float* d_loss, void* stream);
int sg_cross_entropy_backward(const float* d_prob, int K, int C, const int32_t* d_gold, int smoothing, float scale, float* d_glogits, void* stream);

/* batch mean | biased variance [128 | 128] of classifier.bn1 as left in d_ws by sg_train_tail_forward (running-statistics update) */
int sg_train_tail_bn_stats(void* d_ws, size_t ws_bytes, int K, float* d_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * One training step (train.py:160-168 around SegModel.forward in train mode).  Parameters and gradients are flat DEVICE
 * vectors of SG_NUM_PARAMS floats in the reference's `named_parameters()` order (sg_param_slot), owned by the caller: the
 * host side all-reduces the gradient vector over RCCL (train.py:88 DistributedDataParallel averages it over the ranks) and
 * applies the optimizer to the same vectors.
 * ------------------------------------------------------------------------------------------- */
#define SG_NUM_PARAM_TENSORS 19
#define SG_NUM_PARAMS 147880
#define SG_NUM_BN_STATS 768
typedef struct sg_trainer sg_trainer;
int sg_param_slot(int index, const char** name, int* offset, int* count);
sg_trainer* sg_trainer_create(int max_points, int max_segments, int max_edges, int max_vertices, float* d_params, float* d_grads, void* stream);
void sg_trainer_destroy(sg_trainer* tr);
size_t sg_trainer_device_bytes(const sg_trainer* tr);
/* SegModel.forward in train mode up to the classifier (model.py:684-914) with the CURRENT parameter vector: pseudo labels and
 * metrics as in ins_infer (`out`), the record the backward needs, *final_clusters = rows of Feat_5, *instances = K rows of Feat_6 */
int sg_trainer_forward(sg_trainer* tr, const sg_scene* scene, sg_result* out, int* final_clusters, int* instances);
/* Classifier + label-smoothed cross entropy (model.py:916-930) of the last sg_trainer_forward: h_loss[2] = {loss_sum, K} (the
 * reference's `loss [1,2]`); d_keep: DEVICE dropout keep mask [K,128] already scaled by 1 / (1 - p), or NULL (no dropout);
 * d_logits_out [K,40] may be NULL.  K < 2: SG_EUNSUP (BatchNorm1d in training mode raises in the reference). */
int sg_trainer_loss(sg_trainer* tr, const float* d_keep, float* h_loss, float* d_logits_out);
/* loss.backward() for loss = scale * loss_sum (scale <= 0: 1 / K, train.py:164-166), after sg_trainer_loss with the same mask:
 * fills the whole gradient vector. */
int sg_trainer_backward(sg_trainer* tr, const float* d_keep, float scale);
/* HOST h_out[SG_NUM_BN_STATS]: batch mean | biased variance of mlp_1.bn1 [64|64], mlp_2.bn1, mlp_3.bn1, mlp_3.bn2, classifier.bn1
 * [128|128] of the last step (after sg_trainer_backward); h_rows[5] = rows each statistic ran over (running_var is unbiased) */
int sg_trainer_bn_stats(const sg_trainer* tr, float* h_out, double* h_rows);

/* torch.optim.SGD (train.py:96: lr * 100, momentum, weight_decay 1e-4; dampening 0, no Nesterov) on flat vectors */
int sg_optimizer_sgd(float* d_params, const float* d_grads, float* d_momentum_buf, int n, float lr, float momentum, float weight_decay,
                     int first_step, void* stream);
/* torch.optim.Adam (train.py:98: betas 0.9 / 0.999, eps 1e-8, weight_decay added to the gradient); step counts from 1 */
int sg_optimizer_adam(float* d_params, const float* d_grads, float* d_m, float* d_v, int n, float lr, float weight_decay, int step, void* stream);

/* =============================================================================================
 * Readers for the reference's on-disk inputs.  Host only.
 * ============================================================================================= */

/* `<scene>.seg.json` (model.py:713-714; written by dataset/scannet/util.py:205-220): one JSON list per sampled point,
 * non-empty iff the point is the first member of an over-segment.  Fills h_seg_of_point[N] with segment numbers (rank
 * of the segment's first point) and returns the number of segments, or a negative error (malformed JSON, a list that
 * does not start at its own index, a member out of range / claimed twice, an uncovered point). */
int sg_parse_seg_json(const char* path, int N, int32_t* h_seg_of_point);

/* Segment number per point (ranks of the segments' first points) -> CSR of the over-segmentation (h_seg_points [N] ascending
 * inside every segment, h_seg_off [S+1]) + h_seg_first [S], h_seg_size [S]: the host side of DisjointSet's initial state
 * (model.py:712-721) in one counting pass. */
int sg_stage_segments(const int32_t* h_seg_of_point, int N, int S, int32_t* h_seg_points, int32_t* h_seg_off,
                      int32_t* h_seg_first, int32_t* h_seg_size);

/* One scene pack (`<scene>.sgpack`, seggroup_amd/cache.py: magic | header | the staged arrays, 64-byte aligned) from the reference's six per-scene
 * files, natively: src_paths6 = {<s>.pcl.pth, <s>.unmap.pth, weak <s>.label.pth, <s>.seg.json, raw <s>.label.pth, <s>.adj.pth} (data.py:28-38,
 * model.py:696-724 read the same files).  The `.pth` containers are torch.save's STORED zip + a protocol-2 pickle of one tensor; anything
 * else (compressed members, other pickles, float index tensors, names that need JSON escaping) is SG_EINVAL and the caller builds that pack in
 * Python.  Written atomically (temporary file + rename); byte-identical to cache.write_pack's output.
 * sg_pack_build_many: n scenes (src_paths = n x 6 paths) on `threads` plain threads; h_status[i] = SG_OK or the scene's error; returns the number built. */
int sg_pack_build(const char* const* src_paths6, const char* name, const char* out_path);
int sg_pack_build_many(const char* const* src_paths, const char* const* names, const char* const* out_paths, int n, int threads,
                       int32_t* h_status);

#ifdef __cplusplus
}
#endif
#endif /* SEGGROUP_HIP_H */
