"""The segment graph of a scan: the scan's edge list contracted through the per-vertex segment number, and the clusters of
an instance's segments over it.

    pairs, cross = segment_graph(adj, seg)            # device: sg_segment_graph (csrc/kernels_seggraph.hip), sized by edges
    off, members, ins = click_clusters(pairs, seg_ins, S)   # host: sg_click_clusters (csrc/clicks.cpp), sized by segments

`labels.generate_weak_labels(seg_graph="scan")` draws its simulated clicks from these two instead of a dense [S,S] matrix.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import hip
from .device import device_tensor, on_stream, stream_ptr, sync, torch_device, workspace


def segment_graph(adj, seg, S=None, device=None, stream=None):
    """adj: the rows of <scene>.adj.pth ([E,2] integers, any order, duplicates and both orientations allowed), seg: the segment number of
    every vertex (0..S-1, negative = none; S defaults to max + 1) -> (pairs int32 [P,2], cross int32 [P]) NumPy arrays: the distinct
    (lower, higher) segment pairs an edge joins, ascending, and the number of rows behind each.  A vertex index outside the scan or a
    segment number >= S is refused on the device (`hip.SgError`, SG_EINVAL)."""
    import torch
    dev = torch_device(device)
    lib = hip.lib()
    with torch.cuda.device(dev), on_stream(stream):
        d_adj = device_tensor(adj, torch.int64, dev)
        if d_adj.dim() != 2 or d_adj.shape[1] != 2:
            raise ValueError("segment_graph: adj must be [E,2]")
        d_seg = device_tensor(seg, torch.int32, dev).reshape(-1)
        e, v = int(d_adj.shape[0]), int(d_seg.shape[0])
        if v < 1:
            raise ValueError("segment_graph: a scan needs at least one vertex")
        if S is None:
            S = max(int(d_seg.max().item()) + 1, 1)
        need = lib.sg_segment_graph_ws_bytes(e, int(S))
        if e == 0:                                                  # room for one row: the library takes no null pointer
            d_adj = torch.zeros((1, 2), dtype=torch.int64, device=dev)
        d_pairs = torch.empty((max(e, 1), 2), dtype=torch.int32, device=dev)
        d_cross = torch.empty(max(e, 1), dtype=torch.int32, device=dev)
        ws = workspace(need, dev)
        n_p = C.c_longlong(0)
        # outside the envelope `need` is 0 and the call below is refused on its arguments, before anything is launched
        hip.check(lib.sg_segment_graph(d_adj.data_ptr(), e, d_seg.data_ptr(), v, int(S), d_pairs.data_ptr(), d_cross.data_ptr(), C.byref(n_p),
                                       ws.data_ptr(), ws.numel() if need else 0, stream_ptr(stream)))
        p = int(n_p.value)
        pairs, cross = d_pairs[:p].cpu().numpy(), d_cross[:p].cpu().numpy()
        sync(stream)
    return pairs, cross


def click_clusters(pairs, seg_ins, S=None):
    """pairs: int32 [P,2] as `segment_graph` gives them, seg_ins[s]: the instance of segment s (<= 0: in no cluster) ->
    (off int32 [C+1], members int32 [off[C]], ins int32 [C]): the clusters of every instance's segments, in the list order and member order of
    `labels.group_adjacency_segs` (instances ascending).  Host code; needs no GPU.  Bad arrays are a ValueError."""
    h_ins = np.ascontiguousarray(np.asarray(seg_ins).reshape(-1), dtype=np.int32)
    S = int(h_ins.shape[0]) if S is None else int(S)
    if S < 1 or h_ins.shape[0] != S:
        raise ValueError("click_clusters: seg_ins holds one instance per segment, S >= 1 of them")
    h_pairs = np.ascontiguousarray(np.asarray(pairs).reshape(-1, 2), dtype=np.int32)
    off, members, ins = np.zeros(S + 1, np.int32), np.zeros(S, np.int32), np.zeros(S, np.int32)
    n_c = C.c_int(0)
    hip.check_arg(hip.lib().sg_click_clusters(h_pairs.ctypes.data, h_pairs.shape[0], h_ins.ctypes.data, S, off.ctypes.data, members.ctypes.data,
                                              ins.ctypes.data, C.byref(n_c)))
    c = n_c.value
    return off[:c + 1], members[:int(off[c])], ins[:c]
