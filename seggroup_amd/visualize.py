"""Label visualisation: coloured PLY meshes (reference seggroup/visualize.py and dataset/scannet/util.py:431-527).

`visualize_labels` / `visualize_grouping_process` keep the reference's names, positional order and defaults.  A vertex takes one of 41
palette colours chosen by its label (`colors`: entry 0 white, 1..40 ScanNet's class colours); the output is the SOURCE mesh file's bytes
with the red / green / blue byte of every vertex record replaced, written to ``<dir of label file>/visualize/<label file name without its
last suffix>.ply``.  The colours are computed on the GPU (csrc/kernels_visualize.hip: np.unique as a radix sort, the per-vertex records
by one streaming kernel); there is no CPU path.  Shuffles draw from the generators the reference uses, the same number of draws in the
same order: the global `random.shuffle` over a sequence as long as the number of distinct labels ('segment' with shuffle=True), and
`np.random.seed(seed)` + one `np.random.randint(1, 10)` (grouping process) -- a caller that seeds the generator gets the reference's colours.

    python -m seggroup_amd.visualize --mesh_path <scene>_vh_clean_2.ply --label_path <dir>/layer_2.seg.txt --label_type segment [--shuffle]

Deviations: a label count different from the vertex count raises ValueError (the reference prints and exits); `label_file` may also be a
`.npy` file or ``(<pseudo_labels.sgl>, <vector name>)`` -- the colours then come straight from the label tables.
"""
from __future__ import annotations

import ctypes as C
import os
import random
from typing import List, Optional, Sequence

import numpy as np

from . import hip

num_colors = 40
colors = [
    (255, 255, 255),
    (174, 199, 232), (152, 223, 138), (31, 119, 180), (255, 187, 120), (188, 189, 34), (140, 86, 75), (255, 152, 150), (214, 39, 40),
    (197, 176, 213), (148, 103, 189), (196, 156, 148), (23, 190, 207), (178, 76, 76), (247, 182, 210), (66, 188, 102), (219, 219, 141),
    (140, 57, 197), (202, 185, 52), (51, 176, 203), (200, 54, 131), (92, 193, 61), (78, 71, 183), (172, 114, 82), (255, 127, 14),
    (91, 163, 138), (153, 98, 156), (140, 153, 101), (158, 218, 229), (100, 125, 154), (178, 127, 135), (120, 185, 128), (146, 111, 194),
    (44, 160, 44), (112, 128, 144), (96, 207, 209), (227, 119, 194), (213, 92, 176), (94, 106, 211), (82, 84, 163), (100, 85, 144),
]

TYPES = {"semantic": hip.COLOUR_SEMANTIC, "instance": hip.COLOUR_INSTANCE, "segment": hip.COLOUR_SEGMENT}
# SegModel.forward's calls (model.py:739-742, 776-779, 821-824, 862-865, 889-891): the type of every exported vector, and which are shuffled
VECTOR_TYPES = [TYPES[{"seg": "segment", "ins": "instance", "sem": "semantic"}[n.split(".")[1]]] for n in hip.LABEL_NAMES]
VECTOR_SHUFFLED = [n in ("layer_2.seg", "layer_3.seg", "layer_4.seg") for n in hip.LABEL_NAMES]


def _device(device=None):
    import torch
    hip.require_device()
    return torch.device(device if device is not None else "cuda")


def _stream_ptr():
    import torch
    return torch.cuda.current_stream().cuda_stream


# ---- the source mesh ----------------------------------------------------------------------------------------------------------------
class PlySource:
    """A mesh as the three pieces of its file: everything in front of the vertex block, the vertex block [V * stride] uint8, the rest."""

    def __init__(self, head: bytes, block: np.ndarray, tail: bytes, stride: int, offsets: Sequence[int]):
        self.head, self.block, self.tail = head, np.ascontiguousarray(block, dtype=np.uint8).reshape(-1), tail
        self.stride, self.offsets = int(stride), tuple(int(o) for o in offsets)
        self.V = self.block.size // self.stride if self.stride else 0
        self._dev = {}

    def on_device(self, dev):
        import torch
        key = str(dev)
        if key not in self._dev:
            self._dev = {key: torch.from_numpy(self.block).to(dev)}     # (torch's allocations are 512-byte aligned: the 16-byte path applies)
        return self._dev[key]


def ply_plan(path: str) -> dict:
    """sg_ply_plan: where the vertex block of a binary little-endian PLY file sits and which bytes of a vertex are its colour."""
    plan = (C.c_longlong * 10)()
    hip.check_arg(hip.lib().sg_ply_plan(os.fsencode(path), plan))
    keys = ("vertex_offset", "V", "stride", "red", "green", "blue", "tail_offset", "tail_bytes", "file_bytes", "header_bytes")
    return dict(zip(keys, [int(x) for x in plan]))


def read_source(mesh_file: str) -> PlySource:
    if not os.path.isfile(mesh_file):
        raise FileNotFoundError(mesh_file)
    p = ply_plan(mesh_file)
    raw = np.fromfile(mesh_file, dtype=np.uint8)
    if raw.size != p["file_bytes"]:
        raise ValueError(f"{mesh_file}: the file changed while it was read")
    return PlySource(raw[:p["vertex_offset"]].tobytes(), raw[p["vertex_offset"]:p["tail_offset"]], raw[p["tail_offset"]:].tobytes(), p["stride"],
                     (p["red"], p["green"], p["blue"]))


def source_from_plydata(plydata) -> PlySource:
    """A `prepare.PlyMesh` (or anything `prepare.mesh_arrays` reads) re-serialised in ScanNet's layout: float xyz + uchar rgba, triangles."""
    from . import prepare
    xyz, rgb, faces = prepare.mesh_arrays(plydata)
    v = np.zeros(xyz.shape[0], dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1")])
    v["x"], v["y"], v["z"], v["red"], v["green"], v["blue"], v["alpha"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], rgb[:, 0], rgb[:, 1], rgb[:, 2], 255
    try:
        v["alpha"] = np.asarray(plydata["vertex"]["alpha"], dtype=np.uint8)
    except (KeyError, ValueError, IndexError):
        pass
    fc = np.zeros(faces.shape[0], dtype=[("n", "u1"), ("v", "<i4", (3,))])
    fc["n"], fc["v"] = 3, faces
    hdr = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
           "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\nelement face %d\n"
           "property list uchar int vertex_indices\nend_header\n" % (xyz.shape[0], faces.shape[0]))
    return PlySource(hdr.encode(), np.frombuffer(v.tobytes(), dtype=np.uint8), fc.tobytes(), 16, (12, 13, 14))


def _source(mesh_file, plydata) -> PlySource:
    if isinstance(plydata, PlySource):
        return plydata
    if plydata is not None:
        return source_from_plydata(plydata)
    return read_source(mesh_file)


# ---- labels -------------------------------------------------------------------------------------------------------------------------
def load_label_vector(label_file: str) -> np.ndarray:
    """One integer per line (`.txt`, as the reference's load_labels) or a `.npy` vector -> int32 [V]."""
    if label_file.endswith(".npy"):
        a = np.load(label_file)
    elif label_file.endswith(".txt"):
        with open(label_file, "rb") as f:
            a = np.array(f.read().split(), dtype=np.int64)
    else:
        raise ValueError(f"{label_file}: label files are .txt or .npy (or a .sgl file with a vector name)")
    if a.ndim != 1 or (a.size and (a.min() < -2**31 or a.max() >= 2**31)):
        raise ValueError(f"{label_file}: not a vector of 32-bit labels")
    return np.ascontiguousarray(a, dtype=np.int32)


def _split_sgl(label_file):
    """(path, vector name) of the table form, or None: a tuple / list, or '<path>.sgl#<name>'."""
    if isinstance(label_file, (tuple, list)) and len(label_file) == 2:
        return str(label_file[0]), str(label_file[1])
    if isinstance(label_file, str) and "#" in label_file and label_file.rsplit("#", 1)[0].endswith(".sgl"):
        return tuple(label_file.rsplit("#", 1))
    return None


def output_path(label_file: str) -> str:
    """<dir of the label file>/visualize/<its name without the last suffix>.ply (util.py:480-484)."""
    d, base = os.path.split(label_file)
    stem = base.rsplit(".", 1)[0] if "." in base else base
    return os.path.join(d, "visualize", stem + ".ply")


def dilate_labels(labels: np.ndarray, adj: np.ndarray) -> np.ndarray:
    """visualize_labels' adj_path step (util.py:445-454) over a CSR instead of a dense [V,V] matrix: sg_dilate_labels.  adj [E,2]."""
    lab = np.array(labels, dtype=np.int32, copy=True)
    V = lab.shape[0]
    adj = np.asarray(adj, dtype=np.int64).reshape(-1, 2)
    if adj.size and (adj.min() < 0 or adj.max() >= V):
        raise ValueError("adjacency names a vertex outside the mesh")
    src = np.concatenate([adj[:, 0], adj[:, 1]])
    dst = np.concatenate([adj[:, 1], adj[:, 0]])
    order = np.argsort(src, kind="stable")
    indptr = np.zeros(V + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=V), out=indptr[1:])
    indices = np.ascontiguousarray(dst[order], dtype=np.int32)
    hip.check_arg(hip.lib().sg_dilate_labels(lab.ctypes.data, V, indptr.ctypes.data, indices.ctypes.data if indices.size else None))
    return lab


def draw_positions(count: int, rng=random) -> np.ndarray:
    """The reference's `random.shuffle(labels_dict)` (util.py:459) as positions: pos[rank] = where the rank-th distinct label sits after the
    shuffle.  One shuffle of a `count`-long sequence: the same draws from `rng` as the reference makes."""
    order = list(range(count))
    rng.shuffle(order)
    pos = np.empty(count, dtype=np.int32)
    pos[np.asarray(order, dtype=np.int64)] = np.arange(count, dtype=np.int32)
    return pos


# ---- colours on the device ------------------------------------------------------------------------------------------------------------
def _labels_on_device(x, dev):
    import torch
    t = x if hasattr(x, "data_ptr") else torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32))
    return t.to(dev, torch.int32).contiguous()


def colour_vector(labels, label_type, shuffle: bool = False, second=None, mult: int = 1, rng=random, device=None):
    """Vector form: palette indices uint8 [V] (a device tensor) of one label vector.  `labels` / `second`: int32 device tensors or arrays.
    label_type: 'semantic' | 'instance' | 'segment' | hip.COLOUR_GROUPING."""
    import torch
    dev = _device(device)
    lib = hip.lib()
    t = TYPES[label_type] if isinstance(label_type, str) else int(label_type)
    lab = _labels_on_device(labels, dev)
    sec = None if second is None else _labels_on_device(second, dev)
    if sec is not None and sec.shape != lab.shape:
        raise ValueError("the two label vectors differ in length")
    V = int(lab.shape[0])
    ws_bytes = int(lib.sg_colour_vector_ws_bytes(V))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty(max(V, 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        st = _stream_ptr()
        count = C.c_int(0)
        hip.check_arg(lib.sg_colour_vector_unique(lab.data_ptr(), V, t, C.byref(count), ws.data_ptr(), ws_bytes, st))
        pos = draw_positions(count.value, rng) if (shuffle and t == hip.COLOUR_SEGMENT) else None
        hip.check_arg(lib.sg_colour_vector_apply(lab.data_ptr(), V, t, None if sec is None else sec.data_ptr(), count.value,
                                          None if pos is None else pos.ctypes.data, int(mult), out.data_ptr(), ws.data_ptr(), ws_bytes, st))
    return out[:V]


def colour_tables(tables, seg_of_vertex, types: Sequence[int], shuffled: Optional[Sequence[bool]] = None, sem_rows: Optional[Sequence[int]] = None,
                  rngs=None, sov_width: int = 4):
    """Table form: palette indices uint8 [nvec, S+1] (slot S: a vertex without a segment) from device tensors tables [nvec,S] int32 and
    seg_of_vertex [V] (int32, or int16 holding uint16 bits with sov_width=2).  rngs: one generator for every shuffled row in row order
    (default: the global `random`, drawn in row order)."""
    import torch
    lib = hip.lib()
    dev = tables.device
    nvec, S = int(tables.shape[0]), int(tables.shape[1])
    V = int(seg_of_vertex.shape[0])
    ty = (C.c_int * nvec)(*[int(t) for t in types])
    counts = (C.c_int * nvec)()
    ws_bytes = int(lib.sg_colour_tables_ws_bytes(S))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty((nvec, S + 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        st = _stream_ptr()
        hip.check_arg(lib.sg_colour_tables_unique(tables.data_ptr(), nvec, S, seg_of_vertex.data_ptr(), sov_width, V, ty, counts, ws.data_ptr(), ws_bytes, st))
        perm_off = np.full(nvec, -1, dtype=np.int64)
        perms: List[np.ndarray] = []
        at = 0
        for r in range(nvec):
            if shuffled is not None and shuffled[r] and ty[r] == hip.COLOUR_SEGMENT:
                rng = random if rngs is None else (rngs if hasattr(rngs, "shuffle") else rngs[r])
                perms.append(draw_positions(counts[r], rng))
                perm_off[r] = at
                at += counts[r]
        perm = np.concatenate(perms) if perms else np.zeros(1, np.int32)
        sr = None if sem_rows is None else (C.c_int * nvec)(*[int(x) for x in sem_rows])
        hip.check_arg(lib.sg_colour_tables_apply(tables.data_ptr(), nvec, S, ty, sr, counts, perm.ctypes.data, perm_off.ctypes.data, out.data_ptr(),
                                          ws.data_ptr(), ws_bytes, st))
    return out


def vertex_records(src_dev, V: int, stride: int, offsets: Sequence[int], cidx, rows: Sequence[int], seg_of_vertex=None, S: int = 0, sov_width: int = 4):
    """sg_ply_vertex_records_device: uint8 [len(rows), V * stride] on the device, the source block with every vertex's colour bytes replaced.
    Table form: cidx [*, S+1] + seg_of_vertex; vector form (seg_of_vertex None): cidx [*, V]."""
    import torch
    lib = hip.lib()
    dev = src_dev.device
    rows = [int(r) for r in rows]
    out = torch.empty((len(rows), max(V * stride, 1)), dtype=torch.uint8, device=dev)
    if cidx.dim() == 1:
        cidx = cidx.reshape(1, -1)
    ld = int(cidx.stride(0)) if cidx.shape[0] > 1 else int(cidx.shape[1])
    if max(rows) >= cidx.shape[0] or min(rows) < 0:
        raise ValueError("a requested row is outside the colour table")
    if cidx.shape[1] < (S + 1 if seg_of_vertex is not None else V):
        raise ValueError("the colour table is narrower than the scene")
    with torch.cuda.device(dev):
        hip.check_arg(lib.sg_ply_vertex_records_device(src_dev.data_ptr(), V, stride, offsets[0], offsets[1], offsets[2],
                                                None if seg_of_vertex is None else seg_of_vertex.data_ptr(), sov_width, S, cidx.data_ptr(), ld,
                                                len(rows), (C.c_int * len(rows))(*rows), out.data_ptr(), _stream_ptr()))
    return out[:, :V * stride]


# ---- writing --------------------------------------------------------------------------------------------------------------------------
_pool = None


def _writer():
    global _pool
    if _pool is None:
        h = hip.lib().sg_writer_create(2, 64)
        if not h:
            raise hip.SgError(hip.SG_EINVAL, hip.lib().sg_last_error().decode())
        _pool = h
    return _pool


def write_plys(src: PlySource, blocks: np.ndarray, paths: Sequence[str], writer=None, tag: int = -1, flush: bool = True) -> None:
    """One writer job per file (sg_writer_submit_ply: head | block | tail by reference, temporary name + rename, creates visualize/).
    With flush=False the caller keeps `src`, `blocks` alive until it flushed the writer itself."""
    lib = hip.lib()
    w = writer if writer is not None else _writer()
    blocks = np.ascontiguousarray(blocks)
    for i, p in enumerate(paths):
        os.makedirs(os.path.dirname(os.path.dirname(os.path.abspath(p))), exist_ok=True)
        b = blocks[i]
        hip.check_arg(lib.sg_writer_submit_ply(w, os.fsencode(p), src.head, len(src.head), b.ctypes.data, b.size, src.tail, len(src.tail), tag))
    if flush:
        hip.check_arg(lib.sg_writer_flush(w))


# ---- the reference's two functions ----------------------------------------------------------------------------------------------------
def visualize_labels(mesh_file, label_file, label_type, plydata=None, shuffle=False, adj_path=None, sem_labels=None):
    """util.py:431-485.  Writes <dir of label_file>/visualize/<name>.ply and returns its path."""
    import torch
    if label_type not in TYPES:
        raise ValueError(f"label_type must be one of {sorted(TYPES)}")
    dev = _device()
    src = _source(mesh_file, plydata)
    sgl = _split_sgl(label_file)
    sem = None if sem_labels is None else load_label_vector(sem_labels)
    if sgl is not None and adj_path is None and sem is None:
        from . import pseudo_labels
        pl = pseudo_labels.load(sgl[0])
        row = pl._rows([sgl[1]])[0]
        if pl.V != src.V:
            raise ValueError('Loaded labels = ' + str(pl.V) + 'vs mesh vertices = ' + str(src.V))
        tab = torch.from_numpy(pl.tables[row:row + 1].copy()).to(dev)
        sov = torch.from_numpy(pl.seg_of_vertex).to(dev)
        cidx = colour_tables(tab, sov, [TYPES[label_type]], [bool(shuffle)])
        out = vertex_records(src.on_device(dev), src.V, src.stride, src.offsets, cidx, [0], seg_of_vertex=sov, S=pl.S)
        path = os.path.join(os.path.dirname(sgl[0]), "visualize", sgl[1] + ".ply")
    else:
        if sgl is not None:
            from . import pseudo_labels
            labels = pseudo_labels.load(sgl[0]).vector(sgl[1])
            path = os.path.join(os.path.dirname(sgl[0]), "visualize", sgl[1] + ".ply")
        else:
            labels = load_label_vector(label_file)
            path = output_path(label_file)
        if labels.shape[0] != src.V:
            raise ValueError('Loaded labels = ' + str(labels.shape[0]) + 'vs mesh vertices = ' + str(src.V))
        if sem is not None and sem.shape[0] != src.V:
            raise ValueError("sem_labels: " + str(sem.shape[0]) + " labels vs mesh vertices = " + str(src.V))
        if adj_path is not None:
            labels = dilate_labels(labels, np.asarray(torch.load(adj_path)))
        cidx = colour_vector(labels, label_type, shuffle=bool(shuffle), second=sem if label_type == "instance" else None, device=dev)
        out = vertex_records(src.on_device(dev), src.V, src.stride, src.offsets, cidx, [0])
    write_plys(src, out.cpu().numpy(), [path])
    return path


def visualize_grouping_process(mesh_file, ins_label_file, seg_label_file, plydata=None, shuffle=True, seed=0):
    """util.py:489-527.  A vertex with an instance label takes the colour of that label's rank, every other one a colour from its segment
    label (times one number drawn after np.random.seed(seed) when `shuffle`).  Output under visualize/, named after the seg file."""
    dev = _device()
    src = _source(mesh_file, plydata)
    ins, seg = load_label_vector(ins_label_file), load_label_vector(seg_label_file)
    if ins.shape[0] != src.V or seg.shape[0] != src.V:
        raise ValueError('Loaded labels = ' + str(ins.shape[0]) + ', ' + str(seg.shape[0]) + 'vs mesh vertices = ' + str(src.V))
    mult = 1
    if shuffle:
        # the reference shuffles a copy of the segment ids it never reads, then re-seeds and draws the same number for every vertex
        # (util.py:505-515): the global NumPy generator is left where the reference leaves it -- seeded, one randint drawn
        np.random.seed(seed)
        mult = int(np.random.randint(1, 10))
    cidx = colour_vector(ins, hip.COLOUR_GROUPING, second=seg, mult=mult, device=dev)
    out = vertex_records(src.on_device(dev), src.V, src.stride, src.offsets, cidx, [0])
    path = output_path(seg_label_file)
    write_plys(src, out.cpu().numpy(), [path])
    return path


# ---- a whole export directory at once (SegModel(visualize=True), the batch driver) ------------------------------------------------------
def scene_mesh_path(mesh_root: str, scene_name: str) -> str:
    return os.path.join(mesh_root, "scans", scene_name, scene_name + "_vh_clean_2.ply")


def scene_generators(seed: int, scene_name: str):
    """The batch driver's per-layer generators: seeded by (seed, scene, layer), so a scene's files do not depend on the engine's shape,
    the batch order or the number of ranks.  Indexed by table row."""
    return [random.Random(f"{seed}/{scene_name}/{n}") if VECTOR_SHUFFLED[i] else None for i, n in enumerate(hip.LABEL_NAMES)]


def visualize_scene(src: PlySource, tables: np.ndarray, seg_of_vertex: np.ndarray, output_root: str, rngs=None, device=None, writer=None,
                    tag: int = -1, flush: bool = True):
    """The reference's set of files for one export directory: every vector of `tables` ([14,S] ins mode, [6,S] sem mode) coloured by its
    type (seg: 'segment', shuffled for layers 2-4 in row order from `rngs` / the global `random`; ins: 'instance'; sem: 'semantic') ->
    <output_root>/visualize/<vector>.ply.  One upload of the vertex block, one colour-table call, one record launch, one D2H, one writer
    job per file.  Returns (paths, the host blocks the jobs reference)."""
    import torch
    dev = _device(device)
    tables = np.ascontiguousarray(tables, dtype=np.int32)
    sov = np.ascontiguousarray(seg_of_vertex, dtype=np.int32)
    nvec, S = tables.shape
    if sov.shape[0] != src.V:
        raise ValueError('Loaded labels = ' + str(sov.shape[0]) + 'vs mesh vertices = ' + str(src.V))
    d_tab, d_sov = torch.from_numpy(tables).to(dev), torch.from_numpy(sov).to(dev)
    cidx = colour_tables(d_tab, d_sov, VECTOR_TYPES[:nvec], VECTOR_SHUFFLED[:nvec], rngs=rngs)
    out = vertex_records(src.on_device(dev), src.V, src.stride, src.offsets, cidx, list(range(nvec)), seg_of_vertex=d_sov, S=S)
    host = torch.empty(out.shape, dtype=torch.uint8, pin_memory=True)
    host.copy_(out)
    blocks = host.numpy()
    paths = [os.path.join(output_root, "visualize", n + ".ply") for n in hip.LABEL_NAMES[:nvec]]
    write_plys(src, blocks, paths, writer=writer, tag=tag, flush=flush)
    return paths, host


def main(argv=None):
    import argparse
    parser = argparse.ArgumentParser(description="Colour a ScanNet mesh by a label file (output: <label dir>/visualize/<name>.ply)")
    parser.add_argument('--mesh_path', type=str, required=True,
                        help='Path for mesh. The format is `<scannet path>/scans/<scene name>/<scene name>_vh_clean_2.ply`.')
    parser.add_argument('--label_path', type=str, required=True,
                        help='Path for labels: `<result path>/<scene name>/epoch_<epoch>/<file name>.txt` (or .npy, or '
                             '`<dir>/pseudo_labels.sgl#<vector name>`).')
    parser.add_argument('--label_type', type=str, required=True, choices=['instance', 'semantic', 'segment'],
                        help='Type of labels. The type determines visualization colors.')
    parser.add_argument('--shuffle', action='store_true', help='Whether to randomly shuffle colors in visualization.')
    parser.add_argument('--seed', type=int, default=None, help='Seed of the shuffle (default: unseeded, like the reference)')
    parser.add_argument('--sem_label_path', type=str, default=None,
                        help='Semantic labels of the same mesh: instance colours are white on wall and floor (classes 1 and 2)')
    args = parser.parse_args(argv)
    if args.seed is not None:
        random.seed(args.seed)
    path = visualize_labels(args.mesh_path, args.label_path, label_type=args.label_type, shuffle=args.shuffle, sem_labels=args.sem_label_path)
    print(path)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
