"""A tree of scan directories, and one function over its scans on threads: the names of a scan's files, the listing, the
scene-list file, the `--workers` option, the report file and the runner every batch command uses.  Imports nothing from the package;
`torch` is imported on use.
"""
from __future__ import annotations

import json
import os

import numpy as np

MAX_WORKERS = 16                       # threads with a stream each; one limit for every batch command
PLY_SUFFIX = "_vh_clean_2.ply"


def scene_name(scene_path: str) -> str:
    return os.path.split(scene_path[:-1] if scene_path.endswith("/") else scene_path)[-1]


def segs_json_name(scene_name: str, k_thresh: float = 0.01) -> str:
    return "%s_vh_clean_2.%f.segs.json" % (scene_name, float(np.float32(k_thresh)))


def scan_names(scans_dir: str, marker: str = PLY_SUFFIX):
    """the scan directories <d> under `scans_dir` that hold <d><marker>, sorted"""
    return sorted(d for d in os.listdir(scans_dir) if os.path.exists(os.path.join(scans_dir, d, d + marker)))


def declared_count(ply_path: str, element: bytes) -> int:
    """the count a PLY's header declares for `element` (0 without that element); the body is not read"""
    with open(ply_path, "rb") as f:
        for _ in range(256):
            tok = f.readline().split()
            if not tok or tok[0] == b"end_header":
                break
            if len(tok) == 3 and tok[0] == b"element" and tok[1] == element:
                return int(tok[2])
    return 0


def declared_faces(ply_path: str) -> int:
    """the face count a PLY's header declares (0 without a face element); the body is not read"""
    return declared_count(ply_path, b"face")


def scene_list(path):
    """a text file with one scene name per line -> the names; no file -> None"""
    if not path:
        return None
    with open(path) as f:
        return [ln.strip() for ln in f if ln.strip()]


def add_workers_argument(ap) -> None:
    ap.add_argument("--workers", type=int, default=4, help=f"threads, each with its own stream (at most {MAX_WORKERS})")


def add_batch_arguments(ap, force_help: str) -> None:
    """the options every batch command that writes per-scan results has: --scenes, --force, --workers, --device"""
    ap.add_argument("--scenes", default=None, help="text file with one scene name per line")
    ap.add_argument("--force", action="store_true", help=force_help)
    add_workers_argument(ap)
    ap.add_argument("--device", default=None)


def check_workers(ap, workers: int) -> None:
    if not 1 <= workers <= MAX_WORKERS:
        ap.error(f"--workers must be in 1..{MAX_WORKERS}")


def write_report(path: str, doc) -> None:
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


def worker_count(workers, scenes: int) -> int:
    return max(1, min(int(workers), MAX_WORKERS, scenes or 1))


def map_scans(scenes, workers, dev, fn):
    """fn(scene, stream) over the scenes on threads with a stream each -> [(scene, result)] in the scenes' order.  A thread makes its
    stream on `dev` when it takes its first scene; the host work of one scan overlaps the device work of the next."""
    import concurrent.futures
    import threading

    import torch
    local = threading.local()

    def one(scene):
        if not hasattr(local, "stream"):
            with torch.cuda.device(dev):
                local.stream = torch.cuda.Stream(device=dev)
        return scene, fn(scene, local.stream)

    with concurrent.futures.ThreadPoolExecutor(max_workers=worker_count(workers, len(scenes))) as pool:
        return list(pool.map(one, scenes))


def run_scans(scans_dir: str, scenes, workers, dev, out_dir: str, report_name: str, head: dict, one):
    """A batch command: one(scene_path, stream) -> the scan's entry, or None for a scan whose result was there already, over the named
    scans (None: every scan directory under `scans_dir`) -> (report {scene: entry}, skipped scene names); writes <out_dir>/<report_name>,
    `head` with the report and the skipped names."""
    if scenes is None:
        scenes = scan_names(scans_dir)
    done = map_scans(scenes, workers, dev, lambda scene, stream: one(os.path.join(scans_dir, scene), stream))
    report = {scene: entry for scene, entry in done if entry is not None}
    skipped = [scene for scene, entry in done if entry is None]
    os.makedirs(out_dir, exist_ok=True)
    write_report(os.path.join(out_dir, report_name), dict(head, scenes=report, skipped=skipped))
    return report, skipped


def print_outcome(report, skipped, line, skipped_note: str, verb: str = "written") -> None:
    """what a batch command prints: line(scene, entry) -> the words of a scene's line, a line per skipped scene, the tail"""
    for scene, entry in report.items():
        print(*line(scene, entry))
    for s in skipped:
        print("skipped", s, skipped_note)
    print(f"{len(report)} {verb}, {len(skipped)} skipped")
