#!/usr/bin/env python3
"""Label visualisation, measured ("Label visualisation"): the record kernel against its HBM byte count, the colour tables against
NumPy on the host, and assembling the records on the GPU against patching host copies.

    python tools/time_visualize.py [--vertices 150000] [--segments 1500] [--scenes 8] [--rows 14] [--iters 20] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_visualize.py --only-kernel      (k_ply_records16_b in the kernel stats)

Prints one JSON object (and writes it to --out).  Bytes per scene and launch of the record kernel: 16 V read + the seg_of_vertex entry of
every vertex (2 or 4 bytes) + rows x 16 V written.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vertices", type=int, default=150000)
    ap.add_argument("--segments", type=int, default=1500)
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--rows", type=int, default=14)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only-kernel", action="store_true", help="only the batched record launches (for a profiler run)")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import torch
    from seggroup_amd import hip, visualize
    lib = hip.lib()
    hip.require_device()
    V, S, B, R = a.vertices, a.segments, a.scenes, a.rows
    rng = np.random.default_rng(0)
    al = lambda x: (x + 255) // 256 * 256                                       # noqa: E731
    rows = list(range(R))
    c_rows = (C.c_int * R)(*rows)
    tables = [np.stack([rng.integers(0, S, S) if t == hip.COLOUR_SEGMENT else rng.integers(-1, 41, S) for t in visualize.VECTOR_TYPES[:R]]).astype(np.int32)
              for _ in range(B)]
    sovs = [rng.integers(-1, S, V).astype(np.int32) for _ in range(B)]
    res = dict(vertices=V, segments=S, scenes=B, rows=R, device=torch.cuda.get_device_name(0))
    for width in (2, 4):
        desc, so, vo, co, oo = [], 0, 0, 0, 0
        for _ in range(B):
            desc.append([so, V, vo, S, co, S + 1, oo])
            so += al(V * 16); vo += V; co += R * (S + 1); oo += al(R * V * 16)
        d_src = torch.randint(0, 255, (so,), dtype=torch.uint8, device="cuda")
        sov_all = np.concatenate(sovs)
        d_sov = torch.from_numpy(np.where(sov_all < 0, 0xFFFF, sov_all).astype(np.uint16).view(np.int16) if width == 2 else sov_all).cuda()
        d_cidx = torch.randint(0, 41, (co,), dtype=torch.uint8, device="cuda")
        d_desc = torch.tensor(desc, dtype=torch.int64, device="cuda")
        d_out = torch.empty(oo, dtype=torch.uint8, device="cuda")
        st = torch.cuda.current_stream().cuda_stream

        def launch():
            hip.check(lib.sg_ply_vertex_records_device_batch(B, d_desc.data_ptr(), V, S, d_src.data_ptr(), 16, 12, 13, 14, d_sov.data_ptr(), width,
                                                             d_cidx.data_ptr(), R, c_rows, d_out.data_ptr(), st))
        for _ in range(3):
            launch()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = []
        for _ in range(a.iters):
            e0.record(); launch(); e1.record(); e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3)
        us = float(np.median(times))
        nbytes = B * (16 * V + width * V + R * 16 * V)
        res["records_batched_sov%d" % (width * 8)] = dict(us_per_launch=round(us, 1), us_per_scene=round(us / B, 2), bytes_per_launch=nbytes,
                                                          tb_per_s=round(nbytes / us / 1e6, 3), us_min=round(float(np.min(times)), 1))
    if not a.only_kernel:
        # one scene as SegModel / the driver do it: upload of tables + seg_of_vertex, colour tables (two calls, both synchronise), one record
        # launch, one copy to pinned host memory -- beside NumPy for the colours and for patching host copies of the vertex block
        block = rng.integers(0, 256, V * 16).astype(np.uint8)
        d_block = torch.from_numpy(block).cuda()
        host = torch.empty((R, V * 16), dtype=torch.uint8, pin_memory=True)
        palette = np.asarray(visualize.colors, dtype=np.uint8)
        t_tab, t_rec, t_d2h, t_np_col, t_np_patch = [], [], [], [], []
        for it in range(max(a.iters // 2, 3)):
            tab, sov = tables[it % B], sovs[it % B]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d_tab, d_sv = torch.from_numpy(tab).cuda(), torch.from_numpy(sov).cuda()
            cidx = visualize.colour_tables(d_tab, d_sv, visualize.VECTOR_TYPES[:R], None)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            out = visualize.vertex_records(d_block, V, 16, (12, 13, 14), cidx, rows, seg_of_vertex=d_sv, S=S)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            host.copy_(out)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            # NumPy: the colours of the R vectors (np.unique + rank look-up for the segment rows), then R patched copies of the block
            exp = np.where(sov[None, :] >= 0, tab[:, np.clip(sov, 0, S - 1)], -1)
            idx = np.empty((R, V), dtype=np.uint8)
            for r in range(R):
                t = visualize.VECTOR_TYPES[r]
                if t == hip.COLOUR_SEGMENT:
                    d = np.unique(exp[r])
                    idx[r] = np.where(exp[r] == -1, 0, np.searchsorted(d, exp[r]) % 40 + 1)
                elif t == hip.COLOUR_INSTANCE:
                    idx[r] = np.where(exp[r] <= 0, 0, (exp[r] - 1) % 40 + 1)
                else:
                    idx[r] = np.where(exp[r] <= 0, 0, exp[r])
            t4 = time.perf_counter()
            cpu = np.empty((R, V, 16), dtype=np.uint8)
            for r in range(R):
                cpu[r] = block.reshape(V, 16)
                cpu[r, :, 12:15] = palette[idx[r]]
            t5 = time.perf_counter()
            if it == 0:
                assert np.array_equal(cpu.reshape(R, -1), host.numpy()), "GPU and NumPy records differ"
            t_tab.append(t1 - t0); t_rec.append(t2 - t1); t_d2h.append(t3 - t2); t_np_col.append(t4 - t3); t_np_patch.append(t5 - t4)
        med = lambda x: round(float(np.median(x)) * 1e3, 3)                      # noqa: E731
        res["one_scene_ms"] = dict(gpu_upload_and_colour_tables=med(t_tab), gpu_record_launch=med(t_rec), d2h_to_pinned=med(t_d2h),
                                   numpy_colours=med(t_np_col), numpy_patch_host_copies=med(t_np_patch),
                                   d2h_bytes=R * V * 16)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
