"""The pose tools' outputs, to the byte, across a change of the layers above their kernels: align.icp under both
metrics, register.global_registration, planes.detect_planes, boxes.label_boxes of every kind, and one batch run each of the thin,
components, planes and boxes commands on a one-scene tree.

Every call here is documented as deterministic, and the modules' own tests hold each to its reference; a change of the call layer, of
the ICP loop or of the batch runner that moves a result inside those bounds passes them.  tests/golden/tool_bytes.npz holds what the build
BEFORE the shared timer contract, call layer and batch runner returned on an MI355X (tools/capture_tool_bytes.py wrote it from that
build; only outputs are stored, the inputs are the fixtures the modules' own GPU tests build from fixed seeds)."""
import contextlib
import io
import os

import numpy as np
import pytest

import align_ref as A
import pcseg_ref as R
import planes_ref as PR
import register_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tool_bytes.npz")
SCENE = "scene0042_00"
KINDS = ("aabb", "yaw", "pca")
COMMANDS = ("thin", "components", "planes", "boxes")

_golden = {}


def golden():
    if not _golden:
        with np.load(GOLDEN) as f:
            _golden.update({k: f[k] for k in f.files})
    return _golden


def icps():
    """test_gpu_align's and test_gpu_align_plane's two cases at the first pose by name: every second fixed point under the inverse of the pose
    (point: "fixed point"; plane: "min_delta"), and another sampling of the room"""
    from seggroup_amd import align
    fixed = A.room(1, 4096).copy()
    back = A.inverse(A.pose(*A.POSES[sorted(A.POSES)[0]]))
    out = {}
    for case, moving in (("exact", A.apply(fixed[::2], back)), ("resampled", A.apply(A.room(2, 3000), back))):
        for metric in align.METRICS:
            al = align.icp(moving, fixed, 0.25, device=DEV, metric=metric)
            pre = "icp.%s.%s." % (case, metric)
            out[pre + "T"] = al.T
            out[pre + "counts"] = np.array([al.iterations, al.inliers, -1 if al.skipped is None else al.skipped], np.int64)
            out[pre + "converged"] = np.array(str(al.converged))
            out[pre + "rms"] = np.array([np.nan if v is None else v for v in (al.rms_before, al.rms_after, al.plane_rms_before, al.plane_rms_after)],
                                        np.float64)
            out[pre + "translation"] = np.array([al.rotation_deg] + al.translation, np.float64)
    return out


def registration():
    """test_gpu_register's first fixture, as its pipeline test calls it"""
    from seggroup_amd import register
    moving, fixed, _ = G.fixture(sorted(G.FIXTURES)[0])
    c = register.global_registration(moving, fixed, voxel=None, hypotheses=2 ** 20, verify=16, device=DEV, **G.RADII)
    return {"register.T": c.T, "register.counts": np.array([c.h, c.count, c.verified_inliers, c.survivors], np.int64),
            "register.ranked": np.array(c.ranked, np.int64)}


def planes_found():
    from seggroup_amd import planes
    return {"planes." + k: np.asarray(v) for k, v in planes.detect_planes(PR.fixture()[0], device=DEV, **PR.PARAMS).arrays().items()}


def boxes_found():
    """the planes of the rotated room as labels (0..5, nothing ignored but the few points no plane took)"""
    from seggroup_amd import boxes, planes
    xyz = PR.fixture()[0]
    labels = planes.detect_planes(xyz, device=DEV, **PR.PARAMS).labels
    return {"boxes.%s.%s" % (kind, k): np.asarray(v) for kind in KINDS for k, v in boxes.label_boxes(xyz, labels, kind, device=DEV).arrays().items()}


def _npz(path):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def commands(root):
    """the four batch commands' main() on a tree that holds the rotated room as its one scan, run with `root` as the working directory so
    that no path of this machine enters a report -> per command the report's bytes, what it printed and the arrays of the .npz it wrote"""
    from seggroup_amd import boxes, components, planes, thin
    here = os.getcwd()
    os.chdir(root)
    try:
        os.makedirs(os.path.join("scans", SCENE))
        xyz = PR.fixture()[0]
        R.write_vertex_only_ply(os.path.join("scans", SCENE, SCENE + "_vh_clean_2.ply"), xyz, np.zeros(xyz.shape, np.uint8))
        runs = (("thin", thin, ["--voxel", "0.1"], thin.REPORT_NAME, os.path.join(SCENE, SCENE + thin.MAP_SUFFIX)),
                ("components", components, ["--radius", "0.2", "--min-verts", "20"], components.REPORT_NAME,
                 os.path.join(SCENE, SCENE + components.MAP_SUFFIX)),
                ("planes", planes, ["--dist", "0.005", "--min-points", "40", "--hypotheses", "1024", "--level"], planes.REPORT_NAME,
                 SCENE + planes.NPZ_SUFFIX),
                ("boxes", boxes, ["--labels-from", "planes", "--suffix", planes.NPZ_SUFFIX, "--key", "labels", "--min-points", "40"],
                 boxes.REPORT_NAME, SCENE + boxes.NPZ_SUFFIX))
        out = {}
        for name, module, args, report, npz in runs:
            said = io.StringIO()
            with contextlib.redirect_stdout(said):
                assert module.main(["--scans", "scans", "--out", name, "--workers", "1", "--device", DEV] + args) == 0
            with open(os.path.join(name, report), "rb") as f:
                out[name + ".report"] = np.frombuffer(f.read(), np.uint8)
            out[name + ".stdout"] = np.array(said.getvalue())
            out.update({"%s.npz.%s" % (name, k): v for k, v in _npz(os.path.join(name, npz)).items()})
        return out
    finally:
        os.chdir(here)


def _same(got):
    want = golden()
    assert got, "nothing was recorded"
    for key, v in got.items():
        v, w = np.asarray(v), want[key]
        assert v.dtype == w.dtype and v.shape == w.shape, (key, v.dtype, w.dtype, v.shape, w.shape)
        assert v.tobytes() == w.tobytes(), (key, v, w)


def test_icp_under_both_metrics():
    got = icps()
    assert str(got["icp.exact.point.converged"]) == "fixed point" and str(got["icp.exact.plane.converged"]) == "min_delta"
    _same(got)


def test_global_registration():
    _same(registration())


def test_detect_planes():
    got = planes_found()
    assert got["planes.planes"].shape == (6, 4)
    _same(got)


def test_label_boxes_of_every_kind():
    got = boxes_found()
    assert got["boxes.pca.values"].shape == (6,)
    _same(got)


def test_the_batch_commands(tmp_path):
    got = commands(str(tmp_path))
    for name in COMMANDS:
        assert "1 written, 0 skipped" in str(got[name + ".stdout"]), name
    _same(got)
