"""Compact pseudo-label files (`pseudo_labels.sgl`, one per export directory ``results/<exp>/<scene>/<stage>/``).

Every label vector the reference writes (model.py:525-605) is a look-up through the scene's over-segmentation:
``vec[t][v] = tables[t][seg_of_vertex[v]]``, -1 where ``seg_of_vertex[v] < 0``.  A `.sgl` file holds the [nvec,S] tables and the one
seg_of_vertex array the vectors share (~0.38 MB per 150k-vertex / 1.5k-segment scene against 8.4 MB of `.npy`); the format is defined
in include/seggroup_hip.h and INTEGRATION.md.  This module reads it (every size and the CRC checked by the native reader: a bad file is
a ValueError, never a crash) and expands it on the host (`sg_expand_labels`) or on the device (`sg_expand_labels_device[_batch]`).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import hip

SGL_NAME = "pseudo_labels.sgl"
INS_NVEC, SEM_NVEC = hip.NUM_LABEL_VECTORS, 6


def sgl_path(path_or_dir: str) -> str:
    return os.path.join(path_or_dir, SGL_NAME) if os.path.isdir(path_or_dir) else path_or_dir


def write(path_or_dir: str, tables: np.ndarray, seg_of_vertex: np.ndarray) -> str:
    """Write tables [nvec,S] + seg_of_vertex [V] as a `.sgl` file (atomically); a directory gets `pseudo_labels.sgl`.  -> the path."""
    path = sgl_path(path_or_dir)
    tab = np.ascontiguousarray(tables, dtype=np.int32)
    sov = np.ascontiguousarray(seg_of_vertex, dtype=np.int32)
    if tab.ndim != 2:
        raise ValueError("tables must be [nvec, S]")
    hip.check_arg(hip.lib().sg_write_sgl(path.encode(), tab.ctypes.data, tab.shape[0], tab.shape[1], sov.ctypes.data, sov.shape[0]))
    return path


def read_header(path_or_dir: str) -> Dict[str, int]:
    """{version, nvec, S, V, sov_width} of a `.sgl` file (sizes checked against the file's length; the CRC is checked by `load`)."""
    info = (C.c_int * 5)()
    hip.check_arg(hip.lib().sg_read_sgl_header(sgl_path(path_or_dir).encode(), info))
    return dict(zip(("version", "nvec", "S", "V", "sov_width"), list(info)))


class PseudoLabels:
    """One export directory's label vectors in compact form."""

    def __init__(self, tables: np.ndarray, seg_of_vertex: np.ndarray, path: Optional[str] = None):
        self.tables = np.ascontiguousarray(tables, dtype=np.int32)
        self.seg_of_vertex = np.ascontiguousarray(seg_of_vertex, dtype=np.int32)
        self.path = path
        nvec = self.tables.shape[0]
        self.names: List[str] = hip.LABEL_NAMES[:nvec]
        self.mode = "ins" if nvec == INS_NVEC else "sem" if nvec == SEM_NVEC else "partial"
        self.S = int(self.tables.shape[1])
        self.V = int(self.seg_of_vertex.shape[0])

    def _rows(self, names: Optional[Sequence[str]]) -> List[int]:
        if names is None:
            return list(range(len(self.names)))
        if isinstance(names, str):
            names = [names]
        missing = [n for n in names if n not in self.names]
        if missing:
            raise KeyError(f"{missing} not in this file ({self.mode} mode: {self.names})")
        return [self.names.index(n) for n in names]

    def vectors(self, names: Optional[Sequence[str]] = None) -> np.ndarray:
        """[k, V] int32 on the host (sg_expand_labels), rows in `names` order (default: every vector of the file)."""
        tab = np.ascontiguousarray(self.tables[self._rows(names)])
        out = np.empty((tab.shape[0], self.V), dtype=np.int32)
        hip.check(hip.lib().sg_expand_labels(tab.ctypes.data, tab.shape[0], self.S, self.seg_of_vertex.ctypes.data, self.V, out.ctypes.data))
        return out

    def vector(self, name: str) -> np.ndarray:
        return self.vectors([name])[0]

    def to_device(self, names: Optional[Sequence[str]] = None, device=None, dtype=None):
        """[k, V] torch tensor on the GPU, expanded there by sg_expand_labels_device (~0.4 MB crosses PCIe instead of k * V * 4 bytes)."""
        return expand_on_device([self], names, device=device, dtype=dtype)[0]


def load(path_or_dir: str) -> PseudoLabels:
    """Read a `.sgl` file (or the one in a directory).  A truncated, corrupt or inconsistent file raises ValueError."""
    path = sgl_path(path_or_dir)
    h = read_header(path)
    tab = np.empty((h["nvec"], h["S"]), dtype=np.int32)
    sov = np.empty(h["V"], dtype=np.int32)
    hip.check_arg(hip.lib().sg_read_sgl(path.encode(), tab.ctypes.data, tab.size, sov.ctypes.data if h["V"] else None, sov.size))
    return PseudoLabels(tab, sov, path=path)


def pack_for_device(items: Sequence[PseudoLabels], rows: Optional[Sequence[Sequence[int]]] = None):
    """Host staging of many scenes for one launch: (tables int32 flat, seg_of_vertex flat as uint16 (0xFFFF = -1) when every S < 65535
    else int32, sov_width, [(table offset, S, sov offset, V)] per scene).  `rows[i]` selects table rows of scene i (default: all)."""
    width = 2 if all(p.S < 65535 for p in items) else 4
    tabs, sovs, desc = [], [], []
    t_off = s_off = 0
    for i, p in enumerate(items):
        tab = p.tables if rows is None else p.tables[list(rows[i])]
        tabs.append(np.ascontiguousarray(tab, dtype=np.int32).reshape(-1))
        sov = p.seg_of_vertex
        sovs.append(np.where(sov < 0, 0xFFFF, sov).astype(np.uint16) if width == 2 else sov)
        desc.append((t_off, p.S, s_off, p.V))
        t_off += tabs[-1].size
        s_off += p.V
    tab_all = np.concatenate(tabs) if tabs else np.zeros(0, np.int32)
    sov_all = np.concatenate(sovs) if sovs else np.zeros(0, np.uint16 if width == 2 else np.int32)
    return tab_all, sov_all, width, desc


def upload(arr: np.ndarray, device):
    """A host array on the device as raw bytes' worth of a torch dtype (uint16 travels as int16: the kernels read the bits)."""
    import torch
    a = np.ascontiguousarray(arr)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).to(device, non_blocking=False)


def expand_on_device(items: Sequence[PseudoLabels], names: Optional[Sequence[str]] = None, device=None, dtype=None):
    """The label vectors of many scenes in ONE launch (scene index = grid.y, sg_expand_labels_device_batch).  -> a list of [k, V_i]
    tensors (views of one buffer; every scene's block starts 16-byte aligned), rows in `names` order (default: every vector of each
    file; every file must then hold the same number).  dtype torch.int32 (default) or torch.int64."""
    import torch
    hip.require_device()
    dtype = torch.int32 if dtype is None else dtype
    if dtype not in (torch.int32, torch.int64):
        raise ValueError("dtype: torch.int32 or torch.int64")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    items = list(items)
    if not items:
        return []
    rows = [p._rows(names) for p in items]
    k = len(rows[0])
    if any(len(r) != k for r in rows):
        raise ValueError("expand_on_device: the files hold different numbers of vectors; name the ones wanted")
    tab_all, sov_all, width, desc = pack_for_device(items, rows)
    ebytes = 4 if dtype == torch.int32 else 8
    per16 = 16 // ebytes
    out_off, off = [], 0
    for (_, _, _, V) in desc:
        out_off.append(off)
        off += -(-k * V // per16) * per16
    d_desc = np.array([(t, (S), s, V, o) for (t, S, s, V), o in zip(desc, out_off)], dtype=np.int64).reshape(-1, 5)
    with torch.cuda.device(dev):
        out = torch.empty(max(off, 1), dtype=dtype, device=dev)
        g_tab = upload(tab_all, dev)
        g_sov = upload(sov_all if sov_all.size else np.zeros(1, sov_all.dtype), dev)
        g_desc = upload(d_desc, dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        if len(items) == 1:
            p = items[0]
            hip.check(hip.lib().sg_expand_labels_device(g_tab.data_ptr(), k, p.S, g_sov.data_ptr(), width, p.V, out.data_ptr(), ebytes, st))
        else:
            hip.check(hip.lib().sg_expand_labels_device_batch(len(items), g_desc.data_ptr(), max(p.V for p in items), max(p.S for p in items),
                                                              g_tab.data_ptr(), k, g_sov.data_ptr(), width, out.data_ptr(), ebytes, st))
    return [out[o:o + k * p.V].view(k, p.V) for o, p in zip(out_off, items)]
