"""The NumPy statement of DESIGN.md 8e: the segment vote and the re-keying of a scan's annotations onto another over-segmentation.
Test infrastructure (like overseg_ref.py): written from the specification with np.unique, np.add.at and argmax and with plain loops
over groups and clicks -- the library is not loaded."""
import copy
import hashlib

import numpy as np

DENSE_LIMIT = 1 << 24          # cells of the rows x columns table the literal statement may build; above it the same vote over the pairs


def vote(row_ids, cols, n_cols):
    """-> dict of int32 arrays: per row (ascending ids) row_ids, row_count, winner, winner_count, distinct, tied, first_vertex; per vertex
    rank, vertex_winner."""
    row_ids = np.asarray(row_ids, dtype=np.int64).reshape(-1)
    cols = np.asarray(cols, dtype=np.int64).reshape(-1)
    assert row_ids.shape == cols.shape and row_ids.size and row_ids.min() >= 0 and cols.min() >= 0 and cols.max() < n_cols
    ids, rank, count = np.unique(row_ids, return_inverse=True, return_counts=True)
    rank = rank.reshape(-1)
    r = ids.shape[0]
    if r * n_cols <= DENSE_LIMIT:
        table = np.zeros((r, n_cols), dtype=np.int64)
        np.add.at(table, (rank, cols), 1)
        winner = table.argmax(axis=1)                                   # the first maximum: ties go to the lowest column
        wcount = table[np.arange(r), winner]
        distinct = (table > 0).sum(axis=1)
        tied = ((table == wcount[:, None]).sum(axis=1) > 1).astype(np.int64)
    else:
        winner, wcount, distinct, tied = _vote_pairs(rank, cols, n_cols, r)
    hit = np.nonzero(cols == winner[rank])[0]                           # ascending vertices that hold their row's winner
    first = np.full(r, -1, dtype=np.int64)
    first[rank[hit][::-1]] = hit[::-1]                                  # the last write per row is the lowest vertex
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    return dict(row_ids=i32(ids), row_count=i32(count), winner=i32(winner), winner_count=i32(wcount), distinct=i32(distinct), tied=i32(tied),
                first_vertex=i32(first), rank=i32(rank), vertex_winner=i32(winner[rank]))


def _vote_pairs(rank, cols, n_cols, r):
    pk, plen = np.unique(rank * np.int64(n_cols) + cols, return_counts=True)
    prow, pcol = pk // n_cols, pk % n_cols
    order = np.lexsort((pcol, -plen, prow))                             # per row: the longest run first, the lowest column among equals
    head = np.ones(order.shape[0], dtype=bool)
    head[1:] = prow[order][1:] != prow[order][:-1]
    winner, wcount = pcol[order][head], plen[order][head]
    distinct = np.bincount(prow, minlength=r)
    tied = (np.bincount(prow, weights=(plen == wcount[prow]), minlength=r) > 1).astype(np.int64)
    return winner, wcount, distinct, tied


def reached(aggregation, scene_name):
    groups = aggregation["segGroups"]
    if scene_name[:12] == "scene0217_00":
        for i, g in enumerate(groups):
            if g["objectId"] == 31:
                return i
    return len(groups)


def vertex_groups(src_seg, aggregation, scene_name):
    """grp[v] = 1 + the file position of the group that owns src_seg[v] (the last one listing it), 0 = none"""
    src_seg = np.asarray(src_seg, dtype=np.int64)
    grp = np.zeros(src_seg.shape[0], dtype=np.int64)
    for i, g in enumerate(aggregation["segGroups"][:reached(aggregation, scene_name)]):
        grp[np.isin(src_seg, np.asarray(g["segments"], dtype=np.int64))] = i + 1
    return grp


def clicks_of(manual):
    out = []
    for ins in manual:
        segs = manual[ins]
        for s in segs:
            out.append((ins, int(s), int(segs[s]) if isinstance(segs, dict) else -1))
    return out


def rekey(src_seg, new_seg, aggregation, manual=None, scene_name=""):
    src_seg = np.asarray(src_seg, dtype=np.int64).reshape(-1)
    new_seg = np.asarray(new_seg, dtype=np.int64).reshape(-1)
    v = src_seg.shape[0]
    n_reached = reached(aggregation, scene_name)
    grp = vertex_groups(src_seg, aggregation, scene_name)
    nv = vote(new_seg, grp, n_reached + 1)
    agg = copy.deepcopy(aggregation)
    for i, g in enumerate(agg["segGroups"]):
        g["segments"] = [int(s) for s in nv["row_ids"][nv["winner"] == i + 1]] if i < n_reached else []
    after = nv["vertex_winner"].astype(np.int64)
    groups = aggregation["segGroups"]
    report = dict(scene=scene_name, V=v, src_segments=int(np.unique(src_seg).shape[0]), new_segments=int(nv["row_ids"].shape[0]),
                  groups=len(groups), annotated_before=int((grp != 0).sum()), annotated_after=int((after != 0).sum()),
                  unchanged=int((after == grp).sum()), unchanged_share=float((after == grp).sum()) / v,
                  impure_segments=int((nv["distinct"] > 1).sum()), tied_segments=int(nv["tied"].sum()),
                  lost_groups=[groups[i].get("id", i) for i in range(n_reached) if not (nv["winner"] == i + 1).any()])
    out = dict(grp=grp, vote=nv, aggregation=agg, report=report, manual=None, clicks=None)
    if manual is None:
        return out
    win_of = dict(zip(nv["row_ids"].tolist(), nv["winner"].tolist()))
    new_manual = {ins: {} for ins in manual}
    records, taken = [], set()
    c = dict(total=0, by_point=0, by_overlap=0, dropped=0, on_taken=0, off_group=0)
    for ins, seg, pt in clicks_of(manual):
        c["total"] += 1
        members = np.nonzero(src_seg == seg)[0]
        if 0 <= pt < v and src_seg[pt] == seg:
            how, ns, npt = "point", int(new_seg[pt]), pt
            c["by_point"] += 1
        elif members.size == 0:
            c["dropped"] += 1
            records.append(dict(instance=ins, seg=seg, point=pt, how="dropped", new_seg=-1, new_point=-1, taken=False))
            continue
        else:
            ids, counts = np.unique(new_seg[members], return_counts=True)
            ns = int(ids[np.argmax(counts)])                           # the first maximum: the lowest new id among equals
            how, npt = "overlap", int(members[new_seg[members] == ns][0])
            c["by_overlap"] += 1
        own = int(grp[members[0]]) if members.size else 0
        c["on_taken"] += ns in taken
        c["off_group"] += win_of[ns] != own
        records.append(dict(instance=ins, seg=seg, point=pt, how=how, new_seg=ns, new_point=npt, taken=ns in taken))
        taken.add(ns)
        new_manual[ins].setdefault(str(ns), npt)
    report["clicks"] = c
    out.update(manual=new_manual, clicks=records)
    return out


def labels_of(result, aggregation, mapper):
    """(ins, sem) per vertex as generate_real_labels writes them for the re-keyed tree"""
    groups = aggregation["segGroups"]
    ins = np.array([0] + [g["objectId"] + 1 for g in groups], dtype=np.int64)
    sem = np.array([0] + [mapper[g["label"]] for g in groups], dtype=np.int64)
    w = result["vote"]["vertex_winner"]
    return ins[w], sem[w]


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<i4").tobytes()).hexdigest()


# ---- the synthetic scan of the whole-scan tests and of tools/capture_rekey.py -----------------------------------------------------------
SCAN = dict(w=96, h=80, seed=5, cell=7, ann_seed=11, blocks_per_row=14, name="scene0005_00")
SEGMENTATIONS = ("identity", "refine", "cell14", "cell5", "cell21")


def source_scan():
    from seggroup_amd import synthetic
    scan = synthetic.make_raw_scan(SCAN["w"], SCAN["h"], SCAN["seed"], name=SCAN["name"], cell=SCAN["cell"])
    ann = synthetic.make_annotations(scan, SCAN["ann_seed"], blocks_per_row=SCAN["blocks_per_row"])
    return scan, ann


def clicks_with_points(scan, ann):
    """make_annotations writes the bare-list form; the shipped click files carry the raw vertex of every click.  Every second instance
    gets the dict form: a vertex inside the segment (string keys), one click with a point outside its segment, one out of range."""
    seg = np.asarray(scan.seg_indices, dtype=np.int64)
    out = {}
    for k, (ins, segs) in enumerate(ann["manual"].items()):
        if k % 2:
            out[ins] = segs
            continue
        d = {}
        for j, s in enumerate(segs):
            members = np.nonzero(seg == int(s))[0]
            pt = int(members[(7 * k + 3) % members.size])
            if k % 8 == 2 and j == 0:
                pt = int(np.nonzero(seg != int(s))[0][k])               # a point outside its segment
            if k % 8 == 6 and j == 0:
                pt = seg.shape[0] + 17                                  # out of range
            d[str(s)] = pt
        out[ins] = d
    out["9999"] = [int(seg.max()) + 7]                                  # a source segment that is not in the scan: dropped
    return out


def new_segmentation(scan, which):
    from seggroup_amd import synthetic
    src = np.asarray(scan.seg_indices, dtype=np.int64)
    if which == "identity":
        return src.copy()
    if which == "refine":
        return 2 * src + (np.arange(src.shape[0]) & 1)
    cell = int(which[4:])
    other = synthetic.make_raw_scan(SCAN["w"], SCAN["h"], SCAN["seed"], name=SCAN["name"], cell=cell)
    assert np.array_equal(other.xyz, scan.xyz) and np.array_equal(other.faces, scan.faces)
    return np.asarray(other.seg_indices, dtype=np.int64)


def write_tree(root, scan, tsv, new_seg, result):
    """The re-keyed scan as files, from the statement's result alone (no library): what rekey_scan must write -> the scene path"""
    import json
    import os
    sp = os.path.join(root, "scans", scan.name)
    os.makedirs(sp, exist_ok=True)
    with open(os.path.join(sp, scan.name + "_vh_clean_2.0.010000.segs.json"), "w") as f:
        json.dump({"params": {}, "sceneId": scan.name, "segIndices": [int(s) for s in new_seg]}, f)
    with open(os.path.join(sp, scan.name + ".aggregation.json"), "w") as f:
        json.dump(result["aggregation"], f)
    with open(os.path.join(root, "scannetv2-labels.combined.tsv"), "w") as f:
        f.write(tsv)
    if result["manual"] is not None:
        os.makedirs(os.path.join(root, "manual_label"), exist_ok=True)
        with open(os.path.join(root, "manual_label", scan.name + ".json"), "w") as f:
            json.dump(result["manual"], f)
    return sp
