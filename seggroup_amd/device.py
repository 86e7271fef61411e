"""The plumbing of one device call, below every module that makes one: the device, the workspace, uploads, the caller's
stream and the sync that ends the call.  Imports nothing from the package but `hip`; `torch` is imported on use, so a module that
imports this one still loads without it.

    dev = torch_device(device)
    with torch.cuda.device(dev), on_stream(stream):
        d_xyz, n = device_cloud(xyz, dev, "who")
        ws = workspace(lib.sg_..._ws_bytes(n), dev)
        hip.check(lib.sg_...(d_xyz.data_ptr(), n, ..., ws.data_ptr(), ws.numel(), stream_ptr(stream)))
        sync(stream)
"""
from __future__ import annotations

import numpy as np

from . import hip


def torch_device(device=None):
    """-> torch.device (default "cuda"); raises without a HIP device: there is no CPU path"""
    import torch
    hip.require_device()
    return torch.device(device if device is not None else "cuda")


def workspace(nbytes, dev):
    """-> uint8 device tensor of at least 256 bytes: what a library call takes as (ws, ws_bytes)"""
    import torch
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)


def device_tensor(a, dtype, dev):
    """NumPy array or tensor -> contiguous tensor of `dtype` on `dev`"""
    import torch
    if isinstance(a, torch.Tensor):
        return a.to(device=dev, dtype=dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dtype)


def stream_ptr(stream):
    """-> what the library takes as hipStream_t; None is the default stream"""
    return None if stream is None else stream.cuda_stream


def on_stream(stream):
    """The caller's stream as torch's current one (uploads, allocations and the library's launches share it), behind whatever the
    current stream has queued."""
    import torch
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    return torch.cuda.stream(stream)


def sync(stream) -> None:
    """The end of a call: the caller's stream when one was given, the whole (current) device otherwise"""
    import torch
    (stream.synchronize() if stream is not None else torch.cuda.synchronize())


def device_cloud(xyz, dev, who: str, exact: bool = False):
    """-> (float32 device tensor, N) of a cloud of at least one point: [N, >= 3] rows with xyz first, or with `exact` [N, 3]"""
    import torch
    d_xyz = device_tensor(xyz, torch.float32, dev)
    if d_xyz.dim() != 2 or (d_xyz.shape[1] != 3 if exact else d_xyz.shape[1] < 3):
        raise ValueError("%s: xyz must be %s" % (who, "[N,3]" if exact else "[N, >= 3]"))
    if d_xyz.shape[0] < 1:
        raise ValueError(f"{who}: a cloud needs at least one point")
    return d_xyz, int(d_xyz.shape[0])


def device_rows(xyz, dev, who: str, limit=None):
    """-> float32 device tensor of a cloud that may be empty: [N, >= 3] rows with xyz first, N at most `limit` (a power of two) if given"""
    import torch
    d = device_tensor(xyz, torch.float32, dev)
    if d.dim() != 2 or d.shape[1] < 3:
        raise ValueError(f"{who}: a cloud is [N, >= 3] rows with xyz first")
    if limit is not None and d.shape[0] > limit:
        raise hip.SgError(hip.SG_EUNSUP, "%s: %d points; a call takes at most 2^%d" % (who, d.shape[0], limit.bit_length() - 1))
    return d


def vec3(v, who: str) -> np.ndarray:
    """an origin for a library call -> contiguous float64 [3]; None is the zero vector"""
    v = np.ascontiguousarray(np.zeros(3) if v is None else v, dtype=np.float64)
    if v.shape != (3,):
        raise ValueError(f"{who}: an origin is 3 numbers")
    return v


def cloud_box(d_xyz, who: str):
    """the box of a device cloud of at least one point -> (lo, hi) float64 [3] on the host; a coordinate that is not finite is a ValueError"""
    lo, hi = (m(0).values.double().cpu().numpy() for m in (d_xyz[:, :3].min, d_xyz[:, :3].max))
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError(f"{who}: a coordinate that is not finite")
    return lo, hi
