// The S-sized part of the ScanNet instance AP evaluation, host only; also built under ASan/UBSan (`make asan`).
//   sg_ap_fold   a scene's contingency triples (csrc/kernels_ap.hip, or any source with the same layout) + one layer's (ins, sem) rows
//                -> that layer's match record: the kept predicted instances with their intersections, the ground-truth instances
//   sg_ap_match  greedy matching of a record at every overlap threshold -> the (y_true, y_score) pairs per (class, overlap)
// Everything up to the confidences is integer arithmetic.  Every input is checked: a bad index is SG_EINVAL, never a wild access.
#include <cmath>
#include <utility>

#include "sg_common.h"

namespace {

constexpr int kClasses = 18;
constexpr int kMinRegion = 100;          // vertices: smaller predictions are dropped, smaller ground-truth instances are ignored
constexpr int kClassIds[kClasses] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39};

int class_index(long long label) {       // 0..17, or -1 (void: unannotated, wall, floor, every other NYU40 id)
    for (int c = 0; c < kClasses; ++c)
        if (kClassIds[c] == label) return c;
    return -1;
}

}  // namespace

extern "C" {

int sg_ap_fold(const int32_t* h_triples, long long T, const int32_t* h_first_vertex, int n_slots, const int32_t* h_gt, int G,
               const int32_t* h_ins_row, const int32_t* h_sem_row, int n_row, int32_t* h_pred, long long pred_cap, int32_t* h_match,
               long long match_cap, int32_t* h_gtrec, long long gtrec_cap, long long* h_n) {
    SG_REQUIRE(T >= 0 && (T == 0 || h_triples) && h_first_vertex && n_slots >= 1 && h_gt && G >= 1 && h_ins_row && h_sem_row && n_row >= 0 &&
               h_pred && h_match && h_gtrec && h_n && pred_cap >= 0 && match_cap >= 0 && gtrec_cap >= 0, "sg_ap_fold: bad arguments");
    SG_REQUIRE(n_slots == n_row || n_slots == n_row + 1, "sg_ap_fold: %d slots for table rows of %d entries (S or S + 1 expected)", n_slots, n_row);
    SG_REQUIRE(h_gt[0] == 0, "sg_ap_fold: entry 0 of the ground-truth list must be id 0");
    // ground truth: ascending ids; the instances of the 18 classes get a record
    std::vector<int> rec_of_g(G, -1), class_of_g(G, -1);
    long long n_rec = 0;
    for (int g = 1; g < G; ++g) {
        const int id = h_gt[2 * g], cnt = h_gt[2 * g + 1];
        SG_REQUIRE(id > h_gt[2 * (g - 1)] && id < 41000 && id % 1000 != 0 && cnt > 0, "sg_ap_fold: bad ground-truth list at entry %d (id %d, count %d)", g, id, cnt);
        const int c = class_index(id / 1000);
        class_of_g[g] = c;
        if (c < 0) continue;
        SG_REQUIRE(n_rec < gtrec_cap, "sg_ap_fold: room for %lld ground-truth records", gtrec_cap);
        h_gtrec[3 * n_rec] = id; h_gtrec[3 * n_rec + 1] = id / 1000; h_gtrec[3 * n_rec + 2] = cnt;
        rec_of_g[g] = (int)n_rec++;
    }
    // the triples of every slot (ordered by (slot, g))
    std::vector<long long> row(n_slots + 1, 0);
    for (long long t = 0; t < T; ++t) {
        const int s = h_triples[3 * t], g = h_triples[3 * t + 1], c = h_triples[3 * t + 2];
        SG_REQUIRE(s >= 0 && s < n_slots && g >= 0 && g < G && c > 0, "sg_ap_fold: triple %lld (%d, %d, %d) out of range", t, s, g, c);
        if (t) {
            const int ps = h_triples[3 * t - 3], pg = h_triples[3 * t - 2];
            SG_REQUIRE(ps < s || (ps == s && pg < g), "sg_ap_fold: triples not in (slot, g) order at %lld", t);
        }
        row[s + 1] += 1;
    }
    for (int s = 0; s < n_slots; ++s) row[s + 1] += row[s];
    // predicted instances: distinct values > 0 of the slots that hold vertices, ascending = mask order
    std::vector<std::pair<int, int>> vs;     // (value, slot)
    for (int s = 0; s < std::min(n_slots, n_row); ++s) {
        if (row[s + 1] == row[s] || h_ins_row[s] <= 0) continue;
        SG_REQUIRE(h_first_vertex[s] >= 0, "sg_ap_fold: slot %d has vertices but no first vertex", s);
        vs.emplace_back(h_ins_row[s], s);
    }
    std::sort(vs.begin(), vs.end());
    std::vector<long long> acc(G, 0);
    std::vector<int> touched;
    long long n_pred = 0, n_match = 0;
    int mask = 0;
    for (size_t i = 0; i < vs.size(); ++mask) {
        size_t j = i;
        int first = INT32_MAX, first_slot = -1;
        long long count = 0;
        touched.clear();
        for (; j < vs.size() && vs[j].first == vs[i].first; ++j) {
            const int s = vs[j].second;
            if (h_first_vertex[s] < first) { first = h_first_vertex[s]; first_slot = s; }
            for (long long t = row[s]; t < row[s + 1]; ++t) {
                const int g = h_triples[3 * t + 1];
                if (!acc[g]) touched.push_back(g);
                acc[g] += h_triples[3 * t + 2];
                count += h_triples[3 * t + 2];
            }
        }
        const int value = vs[i].first;
        i = j;
        const int label = h_sem_row[first_slot], c = class_index(label);
        if (c >= 0 && count >= kMinRegion) {
            SG_REQUIRE(n_pred < pred_cap && count <= INT32_MAX, "sg_ap_fold: room for %lld predictions", pred_cap);
            std::sort(touched.begin(), touched.end());
            long long void_n = 0;
            int nm = 0;
            for (int g : touched) {
                if (class_of_g[g] < 0) void_n += acc[g];
                else if (class_of_g[g] == c) {
                    SG_REQUIRE(n_match < match_cap, "sg_ap_fold: room for %lld matches", match_cap);
                    h_match[2 * n_match] = rec_of_g[g]; h_match[2 * n_match + 1] = (int32_t)acc[g];
                    ++n_match; ++nm;
                }
            }
            int32_t* p = h_pred + 6 * n_pred++;
            p[0] = mask; p[1] = value; p[2] = label; p[3] = (int32_t)count; p[4] = (int32_t)void_n; p[5] = nm;
        }
        for (int g : touched) acc[g] = 0;
    }
    h_n[0] = n_pred; h_n[1] = n_match; h_n[2] = n_rec;
    return SG_OK;
}

int sg_ap_match(const int32_t* h_pred, long long P, const int32_t* h_match, long long M, const int32_t* h_gtrec, long long Gv,
                const double* h_conf, const double* h_overlaps, int n_overlaps, double* h_y_score, uint8_t* h_y_true, long long y_cap,
                long long* h_y_off, int32_t* h_info) {
    SG_REQUIRE(P >= 0 && M >= 0 && Gv >= 0 && (P == 0 || h_pred) && (M == 0 || h_match) && (Gv == 0 || h_gtrec) && h_overlaps && n_overlaps >= 1 &&
               n_overlaps <= 64 && h_y_score && h_y_true && y_cap >= 0 && h_y_off && h_info, "sg_ap_match: bad arguments");
    struct Pair { int other; int inter; };
    std::vector<long long> moff(P + 1, 0);
    std::vector<int> pclass(P), gclass(Gv);
    std::vector<std::vector<Pair>> gt_preds(Gv);             // per ground-truth instance: (prediction, intersection) in mask order
    for (long long g = 0; g < Gv; ++g) {
        gclass[g] = class_index(h_gtrec[3 * g + 1]);
        SG_REQUIRE(gclass[g] >= 0 && h_gtrec[3 * g + 2] > 0, "sg_ap_match: ground-truth record %lld is not of a benchmark class", g);
    }
    for (long long p = 0; p < P; ++p) {
        pclass[p] = class_index(h_pred[6 * p + 2]);
        SG_REQUIRE(pclass[p] >= 0 && h_pred[6 * p + 3] > 0 && h_pred[6 * p + 5] >= 0, "sg_ap_match: prediction %lld is malformed", p);
        moff[p + 1] = moff[p] + h_pred[6 * p + 5];
    }
    SG_REQUIRE(moff[P] == M, "sg_ap_match: the predictions list %lld matches, %lld given", moff[P], M);
    for (long long p = 0; p < P; ++p)
        for (long long m = moff[p]; m < moff[p + 1]; ++m) {
            const int g = h_match[2 * m], inter = h_match[2 * m + 1];
            SG_REQUIRE(g >= 0 && g < Gv && inter > 0 && gclass[g] == pclass[p], "sg_ap_match: match %lld is out of range", m);
            gt_preds[g].push_back({(int)p, inter});
        }
    auto conf = [&](long long p) { return h_conf ? h_conf[p] : 1.0; };
    auto iou = [&](int g, long long p, int inter) {
        return (double)inter / (double)((long long)h_gtrec[3 * g + 2] + h_pred[6 * p + 3] - inter);
    };
    std::vector<std::vector<int>> gts_of(kClasses), preds_of(kClasses);
    for (long long g = 0; g < Gv; ++g)
        if (h_gtrec[3 * g + 2] >= kMinRegion) gts_of[gclass[g]].push_back((int)g);
    for (long long p = 0; p < P; ++p) preds_of[pclass[p]].push_back((int)p);

    long long n_y = 0;
    std::vector<std::vector<std::pair<uint8_t, double>>> out((size_t)kClasses * n_overlaps);
    std::vector<char> visited(P);
    std::vector<double> score;
    std::vector<char> matched;
    for (int o = 0; o < n_overlaps; ++o) {
        const double th = h_overlaps[o];
        std::fill(visited.begin(), visited.end(), 0);
        for (int c = 0; c < kClasses; ++c) {
            auto& y = out[(size_t)c * n_overlaps + o];
            int32_t* info = h_info + 3 * ((size_t)c * n_overlaps + o);
            const auto& gts = gts_of[c];
            info[0] = 0; info[1] = !gts.empty(); info[2] = !preds_of[c].empty();
            score.assign(gts.size(), -INFINITY);
            matched.assign(gts.size(), 0);
            std::vector<double> extra;                         // the lower score of a second match on one ground truth: a false positive
            for (size_t gi = 0; gi < gts.size(); ++gi) {
                bool found = false;
                for (const Pair& pr : gt_preds[gts[gi]]) {
                    if (visited[pr.other]) continue;
                    if (!(iou(gts[gi], pr.other, pr.inter) > th)) continue;
                    const double cf = conf(pr.other);
                    if (matched[gi]) {                         // (such a prediction is not marked visited)
                        extra.push_back(std::min(score[gi], cf));
                        score[gi] = std::max(score[gi], cf);
                    } else {
                        found = true;
                        matched[gi] = 1;
                        score[gi] = cf;
                        visited[pr.other] = 1;
                    }
                }
                if (!found) info[0] += 1;                      // hard false negative
            }
            for (size_t gi = 0; gi < gts.size(); ++gi)
                if (matched[gi]) y.emplace_back((uint8_t)1, score[gi]);
            for (double s : extra) y.emplace_back((uint8_t)0, s);
            // predictions without a ground truth above the threshold: false positives unless mostly void / small instances
            for (int p : preds_of[c]) {
                bool found_gt = false;
                long long ignore = h_pred[6 * (long long)p + 4];
                for (long long m = moff[p]; m < moff[p + 1]; ++m) {
                    const int g = h_match[2 * m], inter = h_match[2 * m + 1];
                    if (iou(g, p, inter) > th) { found_gt = true; break; }
                    if (h_gtrec[3 * g + 2] < kMinRegion) ignore += inter;
                }
                if (found_gt) continue;
                if ((double)ignore / (double)h_pred[6 * (long long)p + 3] <= th) y.emplace_back((uint8_t)0, conf(p));
            }
            n_y += (long long)y.size();
        }
    }
    SG_REQUIRE(n_y <= y_cap, "sg_ap_match: %lld pairs, room for %lld", n_y, y_cap);
    long long k = 0;
    for (size_t i = 0; i < out.size(); ++i) {
        h_y_off[i] = k;
        for (const auto& e : out[i]) { h_y_true[k] = e.first; h_y_score[k] = e.second; ++k; }
    }
    h_y_off[out.size()] = k;
    return SG_OK;
}

}  // extern "C"
