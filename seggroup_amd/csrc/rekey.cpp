// Re-keying annotations, host side: where a click made on ScanNet's segmentation lands on another one.  The device has
// voted (kernels_rekey.hip); what is left per click is a look-up in the rows of that vote.  No HIP call in this file: it is part of the
// host-only sanitizer build, and its arrays are treated as untrusted.
#include "sg_common.h"

extern "C" {

int sg_rekey_clicks(const int32_t* h_src_seg, const int32_t* h_new_seg, int V, const int32_t* h_row_ids, const int32_t* h_row_winner,
                    const int32_t* h_row_first, int R, const int32_t* h_new_ids, int S, const int64_t* h_click_seg,
                    const int64_t* h_click_point, int n, int32_t* h_out_seg, int32_t* h_out_point, int32_t* h_out_how) {
    SG_REQUIRE(V > 0 && R > 0 && S > 0 && n >= 0 && h_src_seg && h_new_seg && h_row_ids && h_row_winner && h_row_first && h_new_ids,
               "sg_rekey_clicks: bad arguments");
    SG_REQUIRE(n == 0 || (h_click_seg && h_click_point && h_out_seg && h_out_point && h_out_how), "sg_rekey_clicks: bad arguments");
    for (int r = 1; r < R; ++r)
        if (h_row_ids[r - 1] >= h_row_ids[r]) return sg::fail(SG_EINVAL, "sg_rekey_clicks: the row ids do not ascend at row %d", r);
    for (int r = 0; r < R; ++r) {
        if (h_row_winner[r] < 0 || h_row_winner[r] >= S) return sg::fail(SG_EINVAL, "sg_rekey_clicks: row %d names a new segment outside 0..%d", r, S - 1);
        const int32_t f = h_row_first[r];
        if (f < 0 || f >= V) return sg::fail(SG_EINVAL, "sg_rekey_clicks: row %d names a vertex outside 0..%d", r, V - 1);
        if (h_src_seg[f] != h_row_ids[r] || h_new_seg[f] != h_new_ids[h_row_winner[r]])
            return sg::fail(SG_EINVAL, "sg_rekey_clicks: row %d's vertex is not in the intersection the row names", r);
    }
    for (int i = 0; i < n; ++i) {
        const int64_t seg = h_click_seg[i], pt = h_click_point[i];
        if (pt >= 0 && pt < V && (int64_t)h_src_seg[pt] == seg) {
            h_out_seg[i] = h_new_seg[pt];
            h_out_point[i] = (int32_t)pt;
            h_out_how[i] = 0;
            continue;
        }
        const int32_t* end = h_row_ids + R;
        const int32_t* it = seg < 0 || seg > 0x7fffffffll ? end : std::lower_bound(h_row_ids, end, (int32_t)seg);
        if (it == end || *it != (int32_t)seg) {
            h_out_seg[i] = -1;
            h_out_point[i] = -1;
            h_out_how[i] = 2;
            continue;
        }
        const size_t r = (size_t)(it - h_row_ids);
        h_out_seg[i] = h_new_ids[h_row_winner[r]];
        h_out_point[i] = h_row_first[r];
        h_out_how[i] = 1;
    }
    return SG_OK;
}

}  // extern "C"
