// IoU of upright boxes, device side: the box consumer beside kernels_boxes.hip's producer.  A box is 8 doubles,
// cx cy cz sx sy sz c s; include/seggroup_hip.h spells the operation sequence of one pair out, and pair_iou below follows it statement
// by statement -- it is the ONE device function for a pair (box_iou_device.h, shared with kernels_boxnms.hip), so sg_box_iou and
// sg_box_best return the same bits for the same pair.
//
//   k_bi_check         one thread a box: a value that is not finite, a negative size, |c*c + s*s - 1| > 1e-6 -> a bit of the flag word
//   k_bi_pairs         one thread a pair.  The pair's scene is bisected in the pair offsets (at most 16 steps of a table that sits in
//                      L2), then (i, j) = divmod(pair - first pair of the scene, Kb of the scene).
//   k_bb_best          one wave a box of A, lanes over the boxes of B of its scene in steps of 64; a lane keeps its best (iou, j) --
//                      strictly greater only, so the lowest j among equals and never an IoU of 0 -- and a butterfly over the wave takes
//                      the highest IoU, the lowest j among equals.  No Ka x Kb table.
// Double arithmetic, nothing contracted (-ffp-contract=off), no floating-point atomics; the only integer atomic is the OR into the flag
// word.
#include <cmath>
#include <vector>

#include "sg_common.h"
#include "box_iou_device.h"

namespace {

using namespace sg_box;                       // put, side_dist, clip_side, pair_iou, scene_of: the one pair function; upright_flags

constexpr int kBlock = 256;
constexpr int kWave = 64;
constexpr int kWaves = kBlock / kWave;
constexpr long long kMaxPairs = 1ll << 24;    // sg_box_iou's d_iou
constexpr int kSetB = 3;                      // the flag word: upright_flags' three bits for set A, the same three shifted for B

struct Landing { int flag, pad[3]; };

__global__ __launch_bounds__(kBlock) void k_bi_check(const double* __restrict__ box, int K, int shift, int* __restrict__ flag) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= K) return;
    const int bad = upright_flags(box + (size_t)i * 8);
    if (bad) atomicOr(flag, bad << shift);
}

__global__ __launch_bounds__(kBlock) void k_bi_pairs(const double* __restrict__ a, const double* __restrict__ b, const int32_t* __restrict__ off_a,
                                                     const int32_t* __restrict__ off_b, const int32_t* __restrict__ poff, int B, int total,
                                                     double* __restrict__ iou) {
    const int p = blockIdx.x * kBlock + threadIdx.x;         // total <= 2^24
    if (p >= total) return;
    const int s = scene_of(poff, B, p);
    const int kb = off_b[s + 1] - off_b[s];                   // > 0: the scene has a pair
    const int r = p - poff[s];
    const int i = off_a[s] + r / kb, j = off_b[s] + r % kb;   // inside the sets: the host checked the offsets
    iou[p] = pair_iou(a + (size_t)i * 8, b + (size_t)j * 8);
}

__global__ __launch_bounds__(kBlock) void k_bb_best(const double* __restrict__ a, const double* __restrict__ b, const int32_t* __restrict__ cls_a,
                                                    const int32_t* __restrict__ cls_b, const int32_t* __restrict__ off_a,
                                                    const int32_t* __restrict__ off_b, int B, int Ka, int32_t* __restrict__ best,
                                                    double* __restrict__ best_iou) {
    const int lane = threadIdx.x % kWave;
    const int i = blockIdx.x * kWaves + threadIdx.x / kWave;  // uniform over the wave
    if (i >= Ka) return;
    const int s = scene_of(off_a, B, i);
    const int j0 = off_b[s], j1 = off_b[s + 1];
    const int ca = cls_a ? cls_a[i] : 0;
    double top = 0.0;                                         // an IoU of 0 is not a partner
    int at = 0x7fffffff;
    for (int j = j0 + lane; j < j1; j += kWave) {
        if (cls_a && cls_b[j] != ca) continue;
        const double v = pair_iou(a + (size_t)i * 8, b + (size_t)j * 8);
        if (v > top) { top = v; at = j; }                     // ascending j: the lowest among a lane's equals stays
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double other = __shfl_xor(top, o);
        const int other_at = __shfl_xor(at, o);
        if (other > top || (other == top && other_at < at)) { top = other; at = other_at; }
    }
    if (lane == 0) {
        best[i] = at == 0x7fffffff ? -1 : at - j0;
        best_iou[i] = at == 0x7fffffff ? 0.0 : top;
    }
}

bool sizes_ok(int Ka, int Kb, int B) { return Ka >= 0 && Ka <= sg::kMaxBoxes && Kb >= 0 && Kb <= sg::kMaxBoxes && B >= 0 && B <= sg::kMaxScenes; }

size_t table_bytes(int B) { return sg::align_up(sizeof(Landing)) + 3 * sg::align_up((size_t)(B + 1) * sizeof(int32_t)); }

struct Tables {
    Landing* land;
    int32_t *off_a, *off_b, *poff;
    std::vector<int32_t> host;            // off_a | off_b | poff as they were uploaded: alive until the call has synchronised
    long long pairs;
};

// what both entries do first: the sizes, the offsets (host), the tables on the device, the check of every box
int prepare(const char* who, const double* d_a, int Ka, const double* d_b, int Kb, const int32_t* h_off_a, const int32_t* h_off_b, int B,
            void* d_ws, size_t ws_bytes, hipStream_t st, Tables* t) {
    SG_REQUIRE(Ka >= 0 && Kb >= 0 && B >= 0 && h_off_a && h_off_b, "%s: bad arguments (%d and %d boxes, %d scenes)", who, Ka, Kb, B);
    if (!sizes_ok(Ka, Kb, B))
        return sg::fail(SG_EUNSUP, "%s: %d and %d boxes in %d scenes; a call takes at most 2^20 boxes a side and 2^16 scenes", who, Ka, Kb, B);
    if (int rc = sg::check_offsets(who, "set A", h_off_a, B, Ka)) return rc;
    if (int rc = sg::check_offsets(who, "set B", h_off_b, B, Kb)) return rc;
    SG_REQUIRE((d_a || !Ka) && (d_b || !Kb) && d_ws, "%s: bad arguments", who);
    const size_t need = table_bytes(B);
    SG_REQUIRE(ws_bytes >= need, "%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
    sg::Carver cv(d_ws, ws_bytes);
    t->land = cv.take<Landing>(1);
    t->off_a = cv.take<int32_t>((size_t)B + 1);
    t->off_b = cv.take<int32_t>((size_t)B + 1);
    t->poff = cv.take<int32_t>((size_t)B + 1);
    SG_REQUIRE(cv.ok, "%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
    const size_t n = (size_t)B + 1;
    t->host.resize(3 * n);
    t->pairs = 0;
    for (int s = 0; s <= B; ++s) {
        t->host[s] = h_off_a[s];
        t->host[n + s] = h_off_b[s];
        t->host[2 * n + s] = (int32_t)std::min(t->pairs, kMaxPairs + 1);        // used by sg_box_iou alone, which refuses more
        if (s < B) t->pairs += (long long)(h_off_a[s + 1] - h_off_a[s]) * (h_off_b[s + 1] - h_off_b[s]);
    }
    SG_HIP(hipMemsetAsync(t->land, 0, sizeof(Landing), st));
    SG_HIP(hipMemcpyAsync(t->off_a, t->host.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    SG_HIP(hipMemcpyAsync(t->off_b, t->host.data() + n, n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    SG_HIP(hipMemcpyAsync(t->poff, t->host.data() + 2 * n, n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (Ka) k_bi_check<<<sg::cdiv(Ka, kBlock), kBlock, 0, st>>>(d_a, Ka, 0, &t->land->flag);
    if (Kb) k_bi_check<<<sg::cdiv(Kb, kBlock), kBlock, 0, st>>>(d_b, Kb, kSetB, &t->land->flag);
    return SG_OK;
}

int land_flag(const char* who, const Tables& t, hipStream_t st) {
    Landing land{};
    SG_HIP(hipMemcpyAsync(&land, t.land, sizeof(Landing), hipMemcpyDeviceToHost, st));
    SG_HIP(hipStreamSynchronize(st));
    SG_LAUNCH_CHECK();
    if (int rc = upright_refusal(who, "A", land.flag & 7)) return rc;     // every refusal of set A before any of set B
    return upright_refusal(who, "B", land.flag >> kSetB & 7);
}

}  // namespace

extern "C" {

size_t sg_box_iou_ws_bytes(int Ka, int Kb, int B) { return sizes_ok(Ka, Kb, B) ? table_bytes(B) : 0; }

int sg_box_iou(const double* d_a, int Ka, const double* d_b, int Kb, const int32_t* h_off_a, const int32_t* h_off_b, int B, double* d_iou,
               long long pairs, void* d_ws, size_t ws_bytes, void* stream) {
    const char* who = "sg_box_iou";
    hipStream_t st = sg::as_stream(stream);
    Tables t;
    if (int rc = prepare(who, d_a, Ka, d_b, Kb, h_off_a, h_off_b, B, d_ws, ws_bytes, st, &t)) return rc;
    if (t.pairs > kMaxPairs) {
        (void)hipStreamSynchronize(st);                                        // the uploads out of t.host end here
        return sg::fail(SG_EUNSUP, "%s: %lld pairs; d_iou holds at most 2^24 (sg_box_best has no such limit)", who, t.pairs);
    }
    if (pairs != t.pairs || (t.pairs && !d_iou)) {
        (void)hipStreamSynchronize(st);
        return sg::fail(SG_EINVAL, "%s: d_iou holds %lld values and the scenes have %lld pairs", who, pairs, t.pairs);
    }
    if (t.pairs)
        k_bi_pairs<<<sg::cdiv(t.pairs, kBlock), kBlock, 0, st>>>(d_a, d_b, t.off_a, t.off_b, t.poff, B, (int)t.pairs, d_iou);
    return land_flag(who, t, st);
}

size_t sg_box_best_ws_bytes(int Ka, int Kb, int B) { return sizes_ok(Ka, Kb, B) ? table_bytes(B) : 0; }

int sg_box_best(const double* d_a, int Ka, const double* d_b, int Kb, const int32_t* d_cls_a, const int32_t* d_cls_b, const int32_t* h_off_a,
                const int32_t* h_off_b, int B, int32_t* d_best, double* d_best_iou, void* d_ws, size_t ws_bytes, void* stream) {
    const char* who = "sg_box_best";
    SG_REQUIRE((d_cls_a == nullptr) == (d_cls_b == nullptr), "%s: classes are given for both sets or for neither", who);
    SG_REQUIRE((d_best && d_best_iou) || Ka <= 0, "%s: bad arguments", who);
    hipStream_t st = sg::as_stream(stream);
    Tables t;
    if (int rc = prepare(who, d_a, Ka, d_b, Kb, h_off_a, h_off_b, B, d_ws, ws_bytes, st, &t)) return rc;
    if (Ka)
        k_bb_best<<<sg::cdiv(Ka, kWaves), kBlock, 0, st>>>(d_a, d_b, d_cls_a, d_cls_b, t.off_a, t.off_b, B, Ka, d_best, d_best_iou);
    return land_flag(who, t, st);
}

}  // extern "C"
