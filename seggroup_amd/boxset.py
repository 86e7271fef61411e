"""What a set of boxes is, below the box tools `boxap`, `boxlabels` and `boxnms`: the limits of one call, the two row
layouts, scene offsets, class vectors, the two kinds of box file, the scenes of a tree of them, and the packing of scenes into calls.
Imports nothing from the package but `hip` (for SgError) and never `torch`.  A Boxes (seggroup_amd/boxes.py) is recognised by its
attributes `center`, `size` and `R`, so what read_boxes returns is one too.

    rows  = box_rows(x, who)                    -- float64 [K,8]  = cx cy cz sx sy sz c s: the centre, the full size, c = R[:,0,0],
                                                   s = R[:,0,1] (the bits that made the box); an UPRIGHT box, kind aabb or yaw
    rows  = box_frames(x)                       -- float64 [K,15] = cx cy cz sx sy sz r00 .. r22: a box of any kind
    f     = read_boxes(path)                    -- BoxFile: <scene>.boxes.npz as `boxes` writes it (center, size, R, kind; `sem` on its
                                                   experiment route; `values`, `count`, ... ) or <scene>_bbox.npy, float64 [K,7] = centre,
                                                   full size, class id, with its scores in <scene>_score.npy beside it
    for first, end in pack(costs, caps, max_scenes): ...
"""
from __future__ import annotations

import os
from typing import NamedTuple

import numpy as np

from . import hip

MAX_BOXES = 1 << 20                     # boxes of one set in one call
MAX_SCENES = 1 << 16                    # scenes of one call
KINDS = ("aabb", "yaw")                 # the upright kinds: z is the box's axis
NPZ_SUFFIX = ".boxes.npz"
NPY_SUFFIX = "_bbox.npy"
SUFFIXES = (NPZ_SUFFIX, NPY_SUFFIX)
SCORE_SUFFIX = "_score.npy"


def is_boxes(x) -> bool:
    return hasattr(x, "R") and hasattr(x, "center") and hasattr(x, "size")


def _numbers(r) -> bool:
    return np.issubdtype(r.dtype, np.floating) or np.issubdtype(r.dtype, np.integer)


def check_upright(kind, who: str) -> None:
    """kind pca, and any kind but aabb and yaw, is a ValueError under the name `who` (an entry, an option, a file)"""
    if kind == "pca":
        raise ValueError("%s: a box of kind pca is not upright (its axes are the label's principal frame), and the IoU here is of upright "
                         "boxes: make the boxes with kind aabb or yaw" % who)
    if kind not in KINDS:
        raise ValueError("%s: boxes of kind %s are needed, not %r" % (who, " or ".join(KINDS), kind))


def box_rows(x, who: str = "box_rows") -> np.ndarray:
    """A Boxes of kind aabb or yaw, or [K,8] numbers -> float64 [K,8] = centre, full size, c = R[:,0,0], s = R[:,0,1].  Any other kind is
    a ValueError, more than 2^20 rows an SgError(SG_EUNSUP)."""
    if is_boxes(x):
        check_upright(getattr(x, "kind", None), who)
        R = np.asarray(x.R, np.float64).reshape(-1, 3, 3)
        r = np.concatenate([np.asarray(x.center, np.float64).reshape(-1, 3), np.asarray(x.size, np.float64).reshape(-1, 3), R[:, 0, 0:1],
                            R[:, 0, 1:2]], 1)
    else:
        r = np.asarray(x)
        if r.ndim != 2 or r.shape[1] != 8 or not _numbers(r):
            raise ValueError("%s: boxes are [K,8] rows cx cy cz sx sy sz c s (or Boxes), not %s %r" % (who, r.dtype, r.shape))
    if r.shape[0] > MAX_BOXES:
        raise hip.SgError(hip.SG_EUNSUP, "%s: %d boxes; a call takes at most 2^20 in a set" % (who, r.shape[0]))
    return np.ascontiguousarray(r, dtype=np.float64)


def box_frames(x, classes: bool = False):
    """-> float64 [K,15] = centre, full size, R row-major.  `x`: a Boxes of any kind (center, size, R as they stand); [K,15] rows, taken
    as they are; [K,8] rows (R = [[c,s,0],[-s,c,0],[0,0,1]]); [K,7] detector rows (identity frame).  With `classes` -> (rows, the class
    column of [K,7] rows as int64 [K], None for every other input)."""
    cls = None
    if is_boxes(x):
        c, s = np.asarray(x.center, np.float64).reshape(-1, 3), np.asarray(x.size, np.float64).reshape(-1, 3)
        R = np.asarray(x.R, np.float64).reshape(-1, 9)
        if not c.shape[0] == s.shape[0] == R.shape[0]:
            raise ValueError("box_frames: center, size and R of the Boxes hold %d, %d and %d boxes" % (c.shape[0], s.shape[0], R.shape[0]))
        rows = np.concatenate([c, s, R], 1)
    else:
        r = np.asarray(x)
        if r.ndim != 2 or r.shape[1] not in (7, 8, 15) or not _numbers(r):
            raise ValueError("box_frames: boxes are a Boxes, or [K,15] (centre, size, R), [K,8] (centre, size, c, s) or [K,7] (centre, "
                             "size, class) rows of numbers, not %s %r" % (r.dtype, r.shape))
        r = r.astype(np.float64)
        k = r.shape[0]
        if r.shape[1] == 15:
            rows = r
        else:
            R = np.zeros((k, 3, 3))
            if r.shape[1] == 8:
                R[:, 0, 0], R[:, 0, 1], R[:, 1, 0], R[:, 1, 1], R[:, 2, 2] = r[:, 6], r[:, 7], -r[:, 7], r[:, 6], 1.0
            else:
                R[:, 0, 0] = R[:, 1, 1] = R[:, 2, 2] = 1.0
                cls = r[:, 6].astype(np.int64)
                if not np.array_equal(cls.astype(np.float64), r[:, 6]):
                    raise ValueError("box_frames: the class column of [K,7] rows holds whole numbers")
            rows = np.concatenate([r[:, :6], R.reshape(k, 9)], 1)
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    return (rows, cls) if classes else rows


# ---- scenes of one call -------------------------------------------------------------------------------------------------------------------------
def offsets(off, total: int, who: str, name: str, what: str) -> np.ndarray:
    """The argument `name` of the entry `who`, [B+1] whole numbers that ascend from 0 to the `total` `what` ("boxes", "points") -> int32
    [B+1].  More than 2^16 scenes are an SgError(SG_EUNSUP)."""
    o = np.asarray(off)
    if o.ndim != 1 or o.shape[0] < 1 or not np.issubdtype(o.dtype, np.integer):
        raise ValueError("%s: %s is [B+1] whole numbers" % (who, name))
    o = o.astype(np.int64)
    if o[0] != 0 or o[-1] != total or (np.diff(o) < 0).any():
        raise ValueError("%s: %s must ascend from 0 to the %d %s" % (who, name, total, what))
    if o.shape[0] - 1 > MAX_SCENES:
        raise hip.SgError(hip.SG_EUNSUP, "%s: %d scenes; a call takes at most 2^16" % (who, o.shape[0] - 1))
    return np.ascontiguousarray(o, dtype=np.int32)


def paired_offsets(who: str, a: tuple, b: tuple) -> tuple:
    """`a` and `b` are (off, total, name, what) of two sets that are split into the same scenes -> their two int32 [B+1]: both vectors
    or neither (then each set is one scene), and as many scenes in one as in the other."""
    if (a[0] is None) != (b[0] is None):
        raise ValueError("%s: %s and %s delimit the same scenes: both or neither" % (who, a[2], b[2]))
    oa, ob = (offsets([0, total] if off is None else off, total, who, name, what) for off, total, name, what in (a, b))
    if oa.shape != ob.shape:
        raise ValueError("%s: %s and %s name %d and %d scenes" % (who, a[2], b[2], oa.shape[0] - 1, ob.shape[0] - 1))
    return oa, ob


def class_vector(cls, k: int, who: str, name: str) -> np.ndarray:
    """`name`, one whole number per box -> [K+1], a 0 appended: the upload is never empty, so a pointer always says "classes given" """
    c = np.asarray(cls)
    if c.shape != (k,) or not np.issubdtype(c.dtype, np.integer):
        raise ValueError("%s: %s is one whole number per box, [%d]" % (who, name, k))
    return np.concatenate([c, [0]])


def pack(costs, caps, max_scenes: int):
    """Scenes into calls.  `costs`: per scene one number for every cap (say boxes of A and boxes of B, or boxes and bit-matrix words);
    `caps`: what the sums of one call may reach.  Yields (first, end) in order: a call takes the next scene while it holds fewer than
    `max_scenes` and every sum stays within its cap.  The first scene of a call is always taken, so a scene that alone exceeds a cap
    forms its own call, for the entry to refuse."""
    at = 0
    while at < len(costs):
        end, used = at, [0] * len(caps)
        while end < len(costs) and end - at < max_scenes and (end == at or all(u + c <= cap for u, c, cap in zip(used, costs[end], caps))):
            used = [u + c for u, c in zip(used, costs[end])]
            end += 1
        yield at, end
        at = end


# ---- files --------------------------------------------------------------------------------------------------------------------------------------
class BoxFile(NamedTuple):
    """What a box file held: `arrays` {name: array} as they were stored (a _bbox.npy: {"rows": [K,7]}), `kind` (None when the file names
    none; a _bbox.npy is aabb), `center` and `size` float64 [K,3], `R` float64 [K,3,3], `sem` and `values` as stored, None where the
    file has none (a _bbox.npy: sem is column 6).  It has a Boxes' attributes, so box_rows and box_frames take it."""
    path: str
    arrays: dict
    kind: object
    center: np.ndarray
    size: np.ndarray
    R: np.ndarray
    sem: object
    values: object


def read_boxes(path: str) -> BoxFile:
    """<scene>.boxes.npz or <scene>_bbox.npy -> BoxFile.  What a command needs beyond the boxes (`sem`, scores, a kind) it asks for itself."""
    if path.endswith(NPY_SUFFIX):
        r = np.load(path)
        if r.ndim != 2 or r.shape[1] != 7:
            raise ValueError("%s holds %r, not the [K,7] rows (centre, size, class) of `boxes --detector-files`: there is no class" % (path, r.shape))
        if (r[:, 6] != np.round(r[:, 6])).any():
            raise ValueError("%s: column 6 is the class, a whole number" % path)
        return BoxFile(path, {"rows": r}, "aabb", r[:, :3].astype(np.float64), r[:, 3:6].astype(np.float64), np.tile(np.eye(3), (r.shape[0], 1, 1)),
                       r[:, 6].astype(np.int64), None)
    with np.load(path) as z:
        arrays = {name: z[name] for name in z.files}
    return BoxFile(path, arrays, str(arrays["kind"]) if "kind" in arrays else None, np.asarray(arrays["center"], np.float64).reshape(-1, 3),
                   np.asarray(arrays["size"], np.float64).reshape(-1, 3), np.asarray(arrays["R"], np.float64).reshape(-1, 3, 3),
                   arrays.get("sem"), arrays.get("values"))


def file_classes(f: BoxFile, advice: str = "") -> np.ndarray:
    """the class of every box of the file, [K] as stored; a file without `sem` is refused, with `advice` on what else the command takes"""
    if f.sem is None:
        raise ValueError("%s holds no `sem` (the class of every box): `boxes` writes it on its experiment route%s" % (f.path, advice))
    sem = np.asarray(f.sem)
    if sem.shape != (f.center.shape[0],):
        raise ValueError("%s: %d classes for %d boxes" % (f.path, sem.size, f.center.shape[0]))
    return sem


def file_scores(f: BoxFile, score_key=None) -> np.ndarray:
    """one number per box, as stored: the array `score_key` of a .boxes.npz, <scene>_score.npy beside a _bbox.npy"""
    k = f.center.shape[0]
    if f.path.endswith(NPY_SUFFIX):
        spath = f.path[:-len(NPY_SUFFIX)] + SCORE_SUFFIX
        if not os.path.exists(spath):
            raise ValueError("%s has no scores: %s must hold one per box" % (f.path, spath))
        score = np.load(spath)
        if score.shape != (k,):
            raise ValueError("%s holds %r values for the %d boxes of %s" % (spath, score.shape, k, f.path))
        return score
    if score_key not in f.arrays:
        raise ValueError("%s has no array %r (it has %s)" % (f.path, score_key, ", ".join(sorted(f.arrays))))
    score = np.asarray(f.arrays[score_key])
    if score.shape != (k,) or not _numbers(score):
        raise ValueError("%s: %r holds %s %r, not one number for each of the %d boxes" % (f.path, score_key, score.dtype, score.shape, k))
    return score


def scene_files(directory: str, suffix: str) -> set:
    """the scenes that have a file <scene><suffix> in the directory"""
    return {f[:-len(suffix)] for f in os.listdir(directory) if f.endswith(suffix)}


def listed_scenes(sides: list, scenes=None) -> list:
    """`sides`: (what, names) pairs -- the scenes a side of the command has, and what a scene lacks without it, "{}" for its name:
    ("{}.boxes.npz under --pred", names).  -> `scenes` as listed, or the sorted names of all sides; a scene that a side lacks is a
    ValueError that names it."""
    names = sorted(set().union(*(have for _, have in sides))) if scenes is None else list(scenes)
    for s in names:
        for what, have in sides:
            if s not in have:
                raise ValueError("scene %s has no %s%s" % (s, what.format(s), ": every scene needs both sides" if len(sides) > 1 else ""))
    return names
