#!/usr/bin/env python3
"""Expand compact pseudo-label files into the reference's per-vector files, for the trainers that read those.

    python -m seggroup_amd.expand -n EXP --stage S [--only final.ins,final.sem] [--out-format txt,npy] [--root .] [--scenes LIST]

For every scene with `results/<exp>/<scene>/<stage>/pseudo_labels.sgl`, writes `<name>.txt` / `<name>.npy` next to it through the native
writer pool -- the same formatter the inference driver uses, so the files are byte-identical to what a run with `--out-format txt,npy`
writes.  `--only` writes just the named vectors (the downstream readers need two files per scene: INTEGRATION.md).
"""
from __future__ import annotations

import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional

from . import hip, pseudo_labels


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Expand pseudo_labels.sgl files into per-vector label files")
    p.add_argument("-n", "--exp_name", required=True, type=str)
    p.add_argument("--stage", required=True, type=str, help="epoch_N | epoch_last | ins_infer | sem_infer")
    p.add_argument("--only", type=str, default=None, help="comma list of vector names (e.g. final.ins,final.sem); default: every vector of the file")
    p.add_argument("--out-format", type=str, default="txt,npy", help="comma list of txt,npy")
    p.add_argument("--root", type=str, default=".", help="directory holding results/ (default: CWD)")
    p.add_argument("--scenes", type=str, default=None, help="scene list (default: every scene directory under results/<exp>/ with a .sgl file)")
    p.add_argument("-j", "--threads", type=int, default=8, help="writer threads")
    return p


def scene_dirs(root: str, exp: str, stage: str, scenes: Optional[str]) -> List[str]:
    base = os.path.join(root, "results", exp)
    if scenes:
        with open(scenes) as f:
            names = [ln.strip() for ln in f if ln.strip()]
        dirs = [os.path.join(base, s, stage) for s in names]
        missing = [d for d in dirs if not os.path.isfile(os.path.join(d, pseudo_labels.SGL_NAME))]
        if missing:
            raise SystemExit("no %s in %d scene directories, e.g. %s" % (pseudo_labels.SGL_NAME, len(missing), missing[0]))
        return dirs
    names = sorted(os.listdir(base)) if os.path.isdir(base) else []
    return [os.path.join(base, s, stage) for s in names if os.path.isfile(os.path.join(base, s, stage, pseudo_labels.SGL_NAME))]


def expand_dirs(dirs: List[str], only: Optional[List[str]] = None, formats=("txt", "npy"), threads: int = 8) -> int:
    """Write the per-vector files of every directory's `.sgl`; -> files written."""
    from .model import AsyncLabelWriter
    fm = (1 if "txt" in formats else 0) | (2 if "npy" in formats else 0)
    if not fm:
        raise ValueError("--out-format: txt and / or npy")
    lib = hip.lib()
    writer = AsyncLabelWriter(threads=max(1, threads))
    n = 0
    try:
        with ThreadPoolExecutor(max_workers=4) as pool:                    # files are read ahead of the submissions
            for d, p in zip(dirs, pool.map(pseudo_labels.load, dirs)):
                if only is None:
                    # tables + seg_of_vertex (copied): a worker expands each vector while it formats -- the driver's own job kind
                    hip.check(lib.sg_writer_submit_scene_tables(writer.handle, d.encode(), p.tables.ctypes.data, p.S, p.seg_of_vertex.ctypes.data,
                                                                p.V, p.tables.shape[0], fm, -1))
                    n += p.tables.shape[0] * bin(fm).count("1")
                else:
                    vecs = p.vectors(only)
                    for name, vec in zip(only, vecs):
                        hip.check(lib.sg_writer_submit(writer.handle, os.path.join(d, name).encode(), vec.ctypes.data, p.V, fm))
                        n += bin(fm).count("1")
        writer.flush()
    finally:
        writer.close()
    return n


def main(argv=None):
    a = build_parser().parse_args(argv)
    formats = tuple(x for x in a.out_format.split(",") if x)
    bad = [f for f in formats if f not in ("txt", "npy")]
    if bad or not formats:
        raise SystemExit("--out-format: a comma list of txt,npy (got %r)" % a.out_format)
    only = [x for x in a.only.split(",") if x] if a.only else None
    if only:
        unknown = [x for x in only if x not in hip.LABEL_NAMES]
        if unknown:
            raise SystemExit("--only: unknown vector name(s) %s (names: %s)" % (", ".join(unknown), ", ".join(hip.LABEL_NAMES)))
    dirs = scene_dirs(a.root, a.exp_name, a.stage, a.scenes)
    if not dirs:
        raise SystemExit("no %s under %s" % (pseudo_labels.SGL_NAME, os.path.join(a.root, "results", a.exp_name, "*", a.stage)))
    t0 = time.time()
    n = expand_dirs(dirs, only, formats, a.threads)
    print("expanded %d scenes: %d files in %.3f s" % (len(dirs), n, time.time() - t0))


if __name__ == "__main__":
    main(sys.argv[1:])
