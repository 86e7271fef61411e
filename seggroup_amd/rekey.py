"""Carry a scan's annotations over to another over-segmentation.

`<scene>.aggregation.json` and the manual click files are keyed by the segment ids of the segmentation ScanNet shipped.  A segmentation
made here (oversegment.py at any kThresh / segMinVerts) or taken from another segmenter gets its ground truth and its weak labels from the
same annotation: a vertex's annotation is `aggregation[src_seg[v]]`, every new segment takes the group most of its vertices hold (ties:
the group that comes first in the file; "no group" votes too), and a click moves to the new segment under the raw vertex it was made at.
The output is a tree that `prepare_scene`, every label style of `labels.py` and the reference's own scripts read unchanged.

The V-sized work -- ranks of the ids, the two votes -- runs on the GPU (`sg_segment_vote`, csrc/kernels_rekey.hip); there is no other
path.  The group table, the aggregation writer, the click resolver and the report are host code that takes vote results as arrays.

    python -m seggroup_amd.rekey --scans DIR --out DIR [--scenes LIST] [--k-thresh K --seg-min-verts M | --new-segs-from DIR]
                                 [--manual_label_path DIR] [--force] [--copy-mesh] [--workers N] [--report FILE]
"""
from __future__ import annotations

import argparse
import copy
import ctypes as C
import dataclasses
import glob
import json
import os
import shutil
import sys
from typing import Optional

import numpy as np

from . import hip, scans
from .device import device_tensor, on_stream, stream_ptr, sync, torch_device, workspace
from .oversegment import segment_mesh, write_segs_json
from .prepare import load_seg_labels, mesh_arrays, read_ply

SEGS_SUFFIX = "_vh_clean_2.0.010000.segs.json"        # the one name every reader opens, whatever the parameters inside
ROW_FIELDS = ("row_ids", "row_count", "winner", "winner_count", "distinct", "tied", "first_vertex")


@dataclasses.dataclass
class Vote:
    """One `sg_segment_vote`: int32 arrays, rows in ascending id order (device tensors from `vote`, NumPy arrays after `host()`)."""
    row_ids: object
    row_count: object
    winner: object
    winner_count: object
    distinct: object
    tied: object
    first_vertex: object
    rank: object
    vertex_winner: object

    def host(self) -> "Vote":
        return Vote(**{f.name: (getattr(self, f.name).cpu().numpy() if hasattr(getattr(self, f.name), "cpu") else np.asarray(getattr(self, f.name)))
                       for f in dataclasses.fields(self)})


# ---- device side ----------------------------------------------------------------------------------------------------------------------
def _ids(a, dev, what):
    import torch
    if not isinstance(a, torch.Tensor):
        a = np.asarray(a)
        if a.dtype.kind not in "iu" or (a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31)):
            raise ValueError(f"rekey: {what} must be integers that fit int32")
    t = device_tensor(a, torch.int32, dev).reshape(-1)
    if t.shape[0] < 1:
        raise ValueError(f"rekey: {what} is empty")
    return t


def rank_ids(ids, device=None, stream=None):
    """-> (rank [V], row_ids [R], row_count [R]) int32 device tensors: the distinct ids ascending and every vertex's position among them."""
    import torch
    dev = torch_device(device)
    lib = hip.lib()
    with torch.cuda.device(dev), on_stream(stream):
        d_ids = _ids(ids, dev, "the ids")
        v = int(d_ids.shape[0])
        out = torch.empty((3, v), dtype=torch.int32, device=dev)
        ws = workspace(lib.sg_segment_vote_ws_bytes(v), dev)
        n_r = C.c_int(0)
        hip.check(lib.sg_segment_rank(d_ids.data_ptr(), v, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), C.byref(n_r), ws.data_ptr(),
                                      ws.numel(), stream_ptr(stream)))
        sync(stream)
    return out[0], out[1, :n_r.value], out[2, :n_r.value]


def vote(row_ids, cols, n_cols: int, device=None, stream=None) -> Vote:
    """Per distinct row id the column most of its vertices hold (ties: the lowest column) -> `Vote` of device tensors.  `row_ids` are any
    non-negative int32 values, `cols` lie in 0..n_cols-1; both are checked on the device (`hip.SgError`, SG_EINVAL)."""
    import torch
    dev = torch_device(device)
    lib = hip.lib()
    with torch.cuda.device(dev), on_stream(stream):
        d_ids, d_cols = _ids(row_ids, dev, "the row ids"), _ids(cols, dev, "the columns")
        v = int(d_ids.shape[0])
        if d_cols.shape[0] != v:
            raise ValueError("rekey.vote: one column per row id")
        if not 1 <= int(n_cols) < 2 ** 31:
            raise ValueError("rekey.vote: n_cols must be in 1..2^31-1")
        out = torch.empty((9, v), dtype=torch.int32, device=dev)
        ws = workspace(lib.sg_segment_vote_ws_bytes(v), dev)
        n_r = C.c_int(0)
        # rank, vertex_winner, then the row fields in ROW_FIELDS order
        hip.check(lib.sg_segment_vote(d_ids.data_ptr(), d_cols.data_ptr(), v, int(n_cols), *[out[i].data_ptr() for i in range(9)], C.byref(n_r),
                                      ws.data_ptr(), ws.numel(), stream_ptr(stream)))
        sync(stream)
    r = n_r.value
    return Vote(rank=out[0], vertex_winner=out[1], **{f: out[2 + i, :r] for i, f in enumerate(ROW_FIELDS)})


# ---- host side: everything below takes vote results as NumPy arrays and needs no GPU -----------------------------------------------------
def reached_groups(aggregation: dict, scene_name: str) -> int:
    """How many of the file's groups `labels.load_aggregation` reads: all, or those in front of scene0217_00's objectId 31."""
    groups = aggregation["segGroups"]
    if scene_name[:12] == "scene0217_00":
        for i, g in enumerate(groups):
            if g["objectId"] == 31:
                return i
    return len(groups)


def group_table(aggregation: dict, scene_name: str, src_ids) -> np.ndarray:
    """-> int32 [len(src_ids)]: per source segment id 1 + the file position of the group that owns it (the last one listing it), 0 = none."""
    owner = {}
    for i, g in enumerate(aggregation["segGroups"][:reached_groups(aggregation, scene_name)]):
        for s in g["segments"]:
            owner[int(s)] = i + 1
    return np.array([owner.get(int(s), 0) for s in np.asarray(src_ids).reshape(-1)], dtype=np.int32)


def rekeyed_aggregation(aggregation: dict, scene_name: str, new_ids, winner) -> dict:
    """The source file with every key kept and only `segments` replaced: the ascending new ids the group won ([] for a group the reader
    never reaches or that won nothing)."""
    new_ids, winner = np.asarray(new_ids).reshape(-1), np.asarray(winner).reshape(-1)
    out = copy.deepcopy(aggregation)
    reached = reached_groups(aggregation, scene_name)
    for i, g in enumerate(out["segGroups"]):
        g["segments"] = [int(s) for s in np.sort(new_ids[winner == i + 1])] if i < reached else []
    return out


def click_list(manual: dict):
    """Either form the readers accept -- {instance: {segment: point}} or {instance: [segment, ...]}, keys possibly strings ->
    [(instance key, segment, point or -1)] in file order."""
    out = []
    for ins, segs in manual.items():
        if isinstance(segs, dict):
            out.extend((ins, int(s), int(p)) for s, p in segs.items())
        else:
            out.extend((ins, int(s), -1) for s in segs)
    return out


def resolve_clicks(manual: dict, src_seg, new_seg, src_vote: Vote, new_ids):
    """`src_vote`: rows = source segments, columns = ranks of the new ones (host arrays).  -> (the click file of the new segmentation
    {instance: {new segment: point}}, one record per click: dict(instance, seg, point, how, new_seg, new_point, taken))."""
    src_seg = np.ascontiguousarray(src_seg, dtype=np.int32).reshape(-1)
    new_seg = np.ascontiguousarray(new_seg, dtype=np.int32).reshape(-1)
    new_ids = np.ascontiguousarray(new_ids, dtype=np.int32).reshape(-1)
    clicks = click_list(manual)
    n = len(clicks)
    c_seg = np.array([c[1] for c in clicks], dtype=np.int64)
    c_pt = np.array([c[2] for c in clicks], dtype=np.int64)
    o_seg, o_pt, o_how = (np.full(n, -1, dtype=np.int32) for _ in range(3))
    rows = [np.ascontiguousarray(getattr(src_vote, f), dtype=np.int32) for f in ("row_ids", "winner", "first_vertex")]
    p = lambda a: a.ctypes.data if a.size else None
    hip.check(hip.lib().sg_rekey_clicks(p(src_seg), p(new_seg), src_seg.shape[0], p(rows[0]), p(rows[1]), p(rows[2]), rows[0].shape[0],
                                        p(new_ids), new_ids.shape[0], p(c_seg), p(c_pt), n, p(o_seg), p(o_pt), p(o_how)))
    out = {ins: {} for ins in manual}
    records, taken = [], set()
    for (ins, seg, pt), ns, npt, how in zip(clicks, o_seg.tolist(), o_pt.tolist(), o_how.tolist()):
        rec = dict(instance=ins, seg=seg, point=pt, how=("point", "overlap", "dropped")[how], new_seg=ns, new_point=npt, taken=False)
        if how != 2:
            rec["taken"] = ns in taken
            taken.add(ns)
            out[ins].setdefault(str(ns), npt)              # a second click of the instance on the same new segment keeps the first point
        records.append(rec)
    return out, records


def assemble_report(scene_name: str, aggregation: dict, table, new_vote: Vote, n_src: int, before: int, after: int, unchanged: int,
                    clicks=None, src_ids=None) -> dict:
    """`table` = group_table over the ascending source ids `src_ids`; `new_vote`: rows = new segments, columns = groups."""
    v = int(np.asarray(new_vote.rank).shape[0])
    winner = np.asarray(new_vote.winner)
    reached = reached_groups(aggregation, scene_name)
    groups = aggregation["segGroups"]
    won = np.zeros(reached + 1, dtype=bool)
    won[winner] = True
    rep = dict(scene=scene_name, V=v, src_segments=int(n_src), new_segments=int(winner.shape[0]), groups=len(groups),
               annotated_before=int(before), annotated_after=int(after), unchanged=int(unchanged), unchanged_share=float(unchanged) / v,
               impure_segments=int((np.asarray(new_vote.distinct) > 1).sum()), tied_segments=int(np.asarray(new_vote.tied).sum()),
               lost_groups=[groups[i].get("id", i) for i in range(reached) if not won[i + 1]])
    if clicks is not None:
        owner = dict(zip(np.asarray(src_ids).tolist(), np.asarray(table).tolist()))
        win_of = dict(zip(np.asarray(new_vote.row_ids).tolist(), winner.tolist()))
        live = [c for c in clicks if c["how"] != "dropped"]
        rep["clicks"] = dict(total=len(clicks), by_point=sum(c["how"] == "point" for c in clicks),
                             by_overlap=sum(c["how"] == "overlap" for c in clicks), dropped=len(clicks) - len(live),
                             on_taken=sum(c["taken"] for c in live),
                             off_group=sum(win_of[c["new_seg"]] != owner.get(c["seg"], 0) for c in live))
    return rep


REPORT_SUMS = ("V", "src_segments", "new_segments", "groups", "annotated_before", "annotated_after", "unchanged", "impure_segments",
               "tied_segments")


def total_report(reports) -> dict:
    tot = {k: sum(r[k] for r in reports) for k in REPORT_SUMS}
    tot["scenes"] = len(reports)
    tot["unchanged_share"] = tot["unchanged"] / tot["V"] if tot["V"] else 0.0
    tot["lost_groups"] = sum(len(r["lost_groups"]) for r in reports)
    with_clicks = [r["clicks"] for r in reports if "clicks" in r]
    if with_clicks:
        tot["clicks"] = {k: sum(c[k] for c in with_clicks) for k in with_clicks[0]}
    return tot


@dataclasses.dataclass
class Rekeyed:
    scene_name: str
    new_vote: Vote                   # rows = new segments, columns = groups (host arrays); vertex_winner = every vertex's group afterwards
    src_vote: Optional[Vote]         # rows = source segments, columns = ranks of the new ones; only when there are clicks
    table: np.ndarray                # group per ascending source id
    src_ids: np.ndarray
    aggregation: dict                # the re-keyed file content
    manual: Optional[dict]
    clicks: Optional[list]
    report: dict


def rekey_arrays(src_seg, new_seg, aggregation: dict, manual: Optional[dict] = None, scene_name: str = "", device=None, stream=None) -> Rekeyed:
    """The whole re-keying of one scan from arrays: three device calls (ranks of the source ids, the vote of the new segments over the
    groups, and -- with clicks -- the vote of the source segments over the new ones), everything else on the host."""
    import torch
    dev = torch_device(device)
    with torch.cuda.device(dev):
        d_src, d_new = _ids(src_seg, dev, "src_seg"), _ids(new_seg, dev, "new_seg")
        if d_src.shape != d_new.shape:
            raise ValueError("rekey: src_seg and new_seg must name the same vertices")
        src_rank, src_ids, _ = rank_ids(d_src, device=dev, stream=stream)
        h_src_ids = src_ids.cpu().numpy()
        table = group_table(aggregation, scene_name, h_src_ids)
        with on_stream(stream):
            grp = torch.from_numpy(table).to(dev)[src_rank.long()].contiguous()         # the gather through the per-rank table
        nv = vote(d_new, grp, reached_groups(aggregation, scene_name) + 1, device=dev, stream=stream)
        with on_stream(stream):
            before = int((grp != 0).sum())
            after = int((nv.vertex_winner != 0).sum())
            unchanged = int((nv.vertex_winner == grp).sum())
        new_vote = nv.host()
        src_vote = out_manual = clicks = None
        if manual is not None:
            src_vote = vote(d_src, nv.rank, int(nv.row_ids.shape[0]), device=dev, stream=stream).host()
            out_manual, clicks = resolve_clicks(manual, d_src.cpu().numpy(), d_new.cpu().numpy(), src_vote, new_vote.row_ids)
    agg = rekeyed_aggregation(aggregation, scene_name, new_vote.row_ids, new_vote.winner)
    report = assemble_report(scene_name, aggregation, table, new_vote, h_src_ids.shape[0], before, after, unchanged, clicks, h_src_ids)
    return Rekeyed(scene_name, new_vote, src_vote, table, h_src_ids, agg, out_manual, clicks, report)


def vertex_labels(result: Rekeyed, mapper: dict, aggregation: Optional[dict] = None):
    """-> (ins, sem) int64 [V]: per vertex the winner's (objectId + 1, mapper[label]), 0 = unlabeled -- what `generate_real_labels` writes
    for the re-keyed tree."""
    groups = (aggregation or result.aggregation)["segGroups"]
    ins = np.array([0] + [g["objectId"] + 1 for g in groups], dtype=np.int64)
    sem = np.array([0] + [mapper[g["label"]] for g in groups], dtype=np.int64)
    w = np.asarray(result.new_vote.vertex_winner)
    return ins[w], sem[w]


# ---- files ------------------------------------------------------------------------------------------------------------------------------
def _tmp(path: str) -> str:
    import threading
    return "%s.tmp.%d.%d" % (path, os.getpid(), threading.get_ident())


def _write_bytes(path: str, data: bytes) -> None:
    tmp = _tmp(path)
    with open(tmp, "wb") as f:
        f.write(data)
    os.replace(tmp, path)


def _json_bytes(doc) -> bytes:
    return json.dumps(doc).encode()


def rekey_scan(scene_path: str, out_root: str, new_seg=None, k_thresh: float = 0.01, seg_min_verts: int = 20,
               manual_label_path: Optional[str] = None, force: bool = False, copy_mesh: bool = False, device=None, stream=None) -> dict:
    """One scan directory -> the same scan under `out_root` keyed by another segmentation; -> the scene's report.

    `new_seg`: None = segment the mesh here with `k_thresh` / `seg_min_verts` (oversegment.py); a path = somebody's segs.json, copied byte
    for byte; an array = ids per vertex.  Written: out_root/scans/<s>/<s>_vh_clean_2.ply (a link, or a copy with `copy_mesh`), the
    segs.json under the name every reader opens, <s>.aggregation.json, out_root/scannetv2-labels.combined.tsv and -- with
    `manual_label_path` -- out_root/manual_label/<s>.json.  Every file is written under a temporary name and renamed; nothing that
    exists is overwritten without `force`; an `out_root` whose scans directory is the source's is refused."""
    scene_path = scene_path[:-1] if scene_path.endswith("/") else scene_path
    name = scans.scene_name(scene_path)
    src_scans = os.path.dirname(os.path.abspath(scene_path))
    out_scans = os.path.join(out_root, "scans")
    if os.path.realpath(out_scans) == os.path.realpath(src_scans):
        raise ValueError(f"rekey_scan: {out_root} holds the source scans; the re-keyed tree must be another one")
    out_dir = os.path.join(out_scans, name)
    mesh = os.path.join(scene_path, name + "_vh_clean_2.ply")
    targets = dict(mesh=os.path.join(out_dir, name + "_vh_clean_2.ply"), segs=os.path.join(out_dir, name + SEGS_SUFFIX),
                   agg=os.path.join(out_dir, name + ".aggregation.json"))
    if manual_label_path is not None:
        targets["manual"] = os.path.join(out_root, "manual_label", name + ".json")
    if not force:
        for p in targets.values():
            if os.path.lexists(p):
                raise FileExistsError(f"rekey_scan: {p} exists (force=True overwrites)")
    src_seg = np.asarray(load_seg_labels(os.path.join(scene_path, name + SEGS_SUFFIX)), dtype=np.int64)
    with open(os.path.join(scene_path, name + ".aggregation.json")) as f:
        aggregation = json.load(f)
    manual = None
    if manual_label_path is not None:
        with open(os.path.join(manual_label_path, name + ".json")) as f:
            manual = json.load(f)
    with open(os.path.join(os.path.dirname(src_scans), "scannetv2-labels.combined.tsv"), "rb") as f:
        tsv = f.read()
    segs_bytes = None
    if new_seg is None:
        xyz, _, faces = mesh_arrays(read_ply(mesh))
        new_arr = segment_mesh(xyz, faces, k_thresh, seg_min_verts, device=device, stream=stream)
    elif isinstance(new_seg, (str, os.PathLike)):
        with open(new_seg, "rb") as f:
            segs_bytes = f.read()
        new_arr = np.asarray(json.loads(segs_bytes)["segIndices"], dtype=np.int64)
    else:
        new_arr = np.asarray(new_seg).reshape(-1)
    if new_arr.shape[0] != src_seg.shape[0]:
        raise ValueError(f"rekey_scan: {name}: the new segmentation has {new_arr.shape[0]} vertices, the scan {src_seg.shape[0]}")
    res = rekey_arrays(src_seg, new_arr, aggregation, manual, scene_name=name, device=device, stream=stream)

    os.makedirs(out_dir, exist_ok=True)
    tmp = _tmp(targets["mesh"])
    if os.path.lexists(tmp):
        os.remove(tmp)
    (shutil.copyfile(mesh, tmp) if copy_mesh else os.symlink(os.path.abspath(mesh), tmp))
    os.replace(tmp, targets["mesh"])
    if segs_bytes is not None:
        _write_bytes(targets["segs"], segs_bytes)
    elif new_seg is None:
        write_segs_json(targets["segs"], new_arr, name, k_thresh, seg_min_verts)
    else:
        _write_bytes(targets["segs"], _json_bytes({"params": {}, "sceneId": name, "segIndices": [int(s) for s in new_arr]}))
    _write_bytes(targets["agg"], _json_bytes(res.aggregation))
    tsv_out = os.path.join(out_root, "scannetv2-labels.combined.tsv")
    have = None                                                           # looked at once: another worker may write the same file meanwhile
    if os.path.exists(tsv_out):
        with open(tsv_out, "rb") as f:
            have = f.read()
    if have != tsv:
        if have is not None and not force:
            raise FileExistsError(f"rekey_scan: {tsv_out} exists and differs from the source's (force=True overwrites)")
        _write_bytes(tsv_out, tsv)
    if manual is not None:
        os.makedirs(os.path.dirname(targets["manual"]), exist_ok=True)
        _write_bytes(targets["manual"], _json_bytes(res.manual))
    return res.report


def _new_segs_file(new_segs_from: str, scene: str) -> str:
    found = sorted(glob.glob(os.path.join(new_segs_from, scene, "*.segs.json")))
    if len(found) != 1:
        raise ValueError(f"--new-segs-from: {os.path.join(new_segs_from, scene)} must hold exactly one *.segs.json, found {len(found)}")
    return found[0]


def rekey_scans(scans_dir: str, out_root: str, scenes=None, new_segs_from: Optional[str] = None, k_thresh: float = 0.01,
                seg_min_verts: int = 20, manual_label_path: Optional[str] = None, force: bool = False, copy_mesh: bool = False,
                workers: int = 4, device=None):
    """Every annotated scan directory under `scans_dir` (or the named ones) -> (reports in scene order, their totals).  Workers are threads,
    each with its own stream, as in `oversegment_scans`."""
    dev = torch_device(device)
    if scenes is None:
        scenes = scans.scan_names(scans_dir, ".aggregation.json")

    def one(scene, stream):
        new_seg = _new_segs_file(new_segs_from, scene) if new_segs_from else None
        return rekey_scan(os.path.join(scans_dir, scene), out_root, new_seg, k_thresh, seg_min_verts, manual_label_path, force, copy_mesh,
                          device=dev, stream=stream)

    reports = [report for _, report in scans.map_scans(scenes, workers, dev, one)]
    return reports, total_report(reports)


def report_line(r: dict) -> str:
    s = (f"{r.get('scene', 'total')}: V {r['V']}, segments {r['src_segments']} -> {r['new_segments']}, annotated {r['annotated_before']} -> "
         f"{r['annotated_after']}, unchanged {100.0 * r['unchanged_share']:.1f} %, impure {r['impure_segments']}, tied {r['tied_segments']}, "
         f"groups lost {r['lost_groups'] if isinstance(r['lost_groups'], int) else len(r['lost_groups'])}")
    if "clicks" in r:
        c = r["clicks"]
        s += (f", clicks {c['total']} (point {c['by_point']}, overlap {c['by_overlap']}, dropped {c['dropped']}, on a taken segment "
              f"{c['on_taken']}, off their group {c['off_group']})")
    return s


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m seggroup_amd.rekey", description=__doc__.split("\n\n")[0])
    ap.add_argument("--scans", required=True, help="directory of annotated scan directories; scannetv2-labels.combined.tsv lies beside it")
    ap.add_argument("--out", required=True, help="root of the re-keyed tree (scans/, scannetv2-labels.combined.tsv, manual_label/)")
    ap.add_argument("--scenes", default=None, help="text file with one scene name per line (default: every scan with an aggregation file)")
    ap.add_argument("--k-thresh", type=float, default=None)
    ap.add_argument("--seg-min-verts", type=int, default=None)
    ap.add_argument("--new-segs-from", default=None, help="directory of scan directories holding exactly one *.segs.json each")
    ap.add_argument("--manual_label_path", default=None, help="directory of the click files (<scene>.json)")
    ap.add_argument("--force", action="store_true", help="overwrite existing files")
    ap.add_argument("--copy-mesh", action="store_true", help="copy the meshes instead of linking them")
    scans.add_workers_argument(ap)
    ap.add_argument("--report", default=None, help="where the report goes (default: <out>/rekey_report.json)")
    ap.add_argument("--device", default=None)
    a = ap.parse_args(argv)
    if a.new_segs_from is not None and (a.k_thresh is not None or a.seg_min_verts is not None):
        ap.error("--new-segs-from takes the segmentation as it is: --k-thresh / --seg-min-verts do not go with it")
    for d in (a.scans, a.new_segs_from, a.manual_label_path):
        if d is not None and not os.path.isdir(d):
            ap.error(f"{d} is not a directory")
    reports, total = rekey_scans(a.scans, a.out, scans.scene_list(a.scenes), a.new_segs_from, 0.01 if a.k_thresh is None else a.k_thresh,
                                 20 if a.seg_min_verts is None else a.seg_min_verts, a.manual_label_path, a.force, a.copy_mesh, a.workers,
                                 a.device)
    for r in reports:
        print(report_line(r))
    print(report_line(dict(total, scene=f"total of {total['scenes']} scenes")))
    os.makedirs(a.out, exist_ok=True)
    _write_bytes(a.report or os.path.join(a.out, "rekey_report.json"), json.dumps(dict(scenes=reports, total=total), indent=1).encode())
    return 0


if __name__ == "__main__":
    sys.exit(main())
