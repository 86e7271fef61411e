"""Mesh over-segmentation, host side (needs no GPU): sg_overseg_merge -- the two ordered passes over the sorted edges
and the ids -- against the NumPy statement of the specification (tests/overseg_ref.py) on that reference's own sorted edges, the
consequences the specification promises, the committed digests, the refusal of hostile arrays, and the segs.json writer."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import overseg_ref as R
from conftest import GOLDEN, ROOT

CASES = ["room_j0", "room_j5e-4", "room_j2e-3", "raw_scan", "isolated", "one_vertex", "no_edges"]
_cache = {}


def _case(name):
    if not _cache:
        for n, (xyz, faces) in R.case_meshes().items():
            nrm, edges, w = R.sorted_edges(xyz, faces)
            _cache[n] = dict(xyz=xyz, faces=faces, normals=nrm, edges=edges, w=w)
    return _cache[name]


def _expected():
    with open(os.path.join(GOLDEN, "overseg_expected.json")) as f:
        return json.load(f)


def test_the_cases_are_the_ones_the_digests_were_captured_for():
    assert sorted(R.case_meshes()) == sorted(CASES)
    exp = _expected()
    for n in CASES:
        c = _case(n)
        assert (c["xyz"].shape[0], c["faces"].shape[0], c["edges"].shape[0]) == (exp[n]["V"], exp[n]["F"], exp[n]["edges"]), n
        if c["w"].shape[0] > 1:
            assert int((np.diff(c["w"]) == 0).sum()) == exp[n]["ties"], n
    assert exp["room_j0"]["ties"] > 30000 and exp["room_j0"]["negative_weights"] > 0       # the tie order and the sign-aware key are exercised
    assert _case("one_vertex")["xyz"].shape[0] == 1 and _case("no_edges")["edges"].shape[0] == 0


@pytest.mark.parametrize("name", CASES)
def test_host_merge_equals_the_reference_and_the_digest(sg_lib, name):
    from seggroup_amd import oversegment
    c, exp = _case(name), _expected()[name]
    v = c["xyz"].shape[0]
    ref = R.merge(c["edges"], c["w"], v)
    got = oversegment.merge_edges(c["edges"], c["w"], v)
    assert got.dtype == np.int32 and np.array_equal(got, ref)
    assert R.digest(ref) == exp["sha256"], "the reference moved away from the committed digest"
    assert R.digest(got) == exp["sha256"] and np.unique(got).shape[0] == exp["segments"]
    assert np.array_equal(oversegment.merge_edges(c["edges"], c["w"], v), got)               # twice: the same bytes


@pytest.mark.parametrize("k_thresh,seg_min_verts", R.PARAM_SWEEP)
def test_parameter_sweep(sg_lib, k_thresh, seg_min_verts):
    from seggroup_amd import oversegment
    c = _case("room_j5e-4")
    v = c["xyz"].shape[0]
    ref = R.merge(c["edges"], c["w"], v, k_thresh, seg_min_verts)
    got = oversegment.merge_edges(c["edges"], c["w"], v, k_thresh, seg_min_verts)
    assert np.array_equal(got, ref)
    assert R.digest(got) == _expected()["room_j5e-4"]["sweep"][f"{k_thresh:g}/{seg_min_verts}"]


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("seg_min_verts", [1, 20, 200])
def test_consequences_of_the_specification(sg_lib, name, seg_min_verts):
    from seggroup_amd import oversegment
    c = _case(name)
    v = c["xyz"].shape[0]
    seg = oversegment.merge_edges(c["edges"], c["w"], v, 0.01, seg_min_verts)
    ids, first, counts = np.unique(seg, return_index=True, return_counts=True)
    assert np.array_equal(ids, first), "a segment's id is its lowest vertex"
    # a component smaller than seg_min_verts has no edge leaving it
    size_of = np.zeros(v, np.int64)
    size_of[ids] = counts
    a, b = c["edges"][:, 0], c["edges"][:, 1]
    leaving = seg[a] != seg[b]
    assert not ((size_of[seg[a]][leaving] < seg_min_verts) | (size_of[seg[b]][leaving] < seg_min_verts)).any()
    # a vertex in no face is a segment of its own
    named = np.zeros(v, bool)
    named[c["faces"].reshape(-1)] = True
    lonely = np.nonzero(~named)[0]
    assert np.array_equal(seg[lonely], lonely) and (size_of[lonely] == 1).all()
    if name == "isolated":
        assert lonely.tolist() == [600, 601, 602]
    if name == "no_edges":
        assert np.array_equal(seg, np.arange(v))


def test_hostile_arrays_are_refused(sg_lib):
    from seggroup_amd import hip, oversegment
    edges = np.array([[0, 1], [1, 2], [2, 3]], np.int32)
    w = np.array([0.0, 0.001, 0.002], np.float32)
    assert oversegment.merge_edges(edges, w, 4).tolist() == [0, 0, 0, 0]

    def refused(e, ww, v, needle, **kw):
        with pytest.raises(hip.SgError) as ei:
            oversegment.merge_edges(e, ww, v, **kw)
        assert ei.value.code == hip.SG_EINVAL and needle in str(ei.value), str(ei.value)

    for bad in ([1, 4], [-1, 2], [1, 1 << 30]):
        e = edges.copy()
        e[1] = bad
        refused(e, w, 4, "outside 0..3")
    for bad in ([2, 1], [2, 2]):
        e = edges.copy()
        e[1] = bad
        refused(e, w, 4, "not a < b")
    refused(edges, np.array([0.0, 0.002, 0.001], np.float32), 4, "not ascending")
    refused(edges, np.array([0.0, np.nan, 0.001], np.float32), 4, "not ascending")
    refused(edges, np.array([np.nan, 0.0, 0.001], np.float32), 4, "not ascending")
    refused(edges, w, 0, "bad arguments")
    refused(edges, w, 4, "k_thresh", k_thresh=float("nan"))
    refused(edges, w, 4, "seg_min_verts", seg_min_verts=-1)
    # slightly negative weights are legal and sort first
    assert oversegment.merge_edges(edges, np.array([-1e-7, 0.0, 0.5], np.float32), 4, 0.01, 1).tolist() == [0, 0, 0, 3]


def test_segs_json_writer_bytes_and_round_trip(sg_lib, tmp_path):
    from seggroup_amd import hip, oversegment, prepare
    p = str(tmp_path / oversegment.segs_json_name("scene0000_00"))
    assert p.endswith("scene0000_00_vh_clean_2.0.010000.segs.json")
    seg = np.array([0, 0, 2, 0, 2, 5, 123456, 2147483647], np.int32)
    oversegment.write_segs_json(p, seg, "scene0000_00", 0.01, 20)
    want = ('{"params": {"kThresh": "0.010000", "segMinVerts": "20"}, "sceneId": "scene0000_00", '
            '"segIndices": [0, 0, 2, 0, 2, 5, 123456, 2147483647]}')
    assert open(p, "rb").read() == want.encode()
    doc = json.load(open(p))
    assert want == json.dumps(doc) and doc["params"] == {"kThresh": "0.010000", "segMinVerts": "20"}
    assert prepare.load_seg_labels(p) == seg.tolist()
    assert os.listdir(tmp_path) == [os.path.basename(p)], "the temporary name is gone"
    # a larger vector, an empty one, and the refusals
    big = (np.arange(70000, dtype=np.int64) * 7 % 65521).astype(np.int32)
    oversegment.write_segs_json(p, big, "s", 0.1, 1)
    assert prepare.load_seg_labels(p) == big.tolist() and json.load(open(p))["params"]["kThresh"] == "0.100000"
    oversegment.write_segs_json(p, np.zeros(0, np.int32), "s")
    assert json.load(open(p))["segIndices"] == []
    for args, needle in (((np.array([1, -1], np.int32), "s"), "negative"), ((seg, 'a"b'), "escaping"),
                         ((seg, "a\\b"), "escaping")):
        with pytest.raises(hip.SgError) as ei:
            oversegment.write_segs_json(p, *args)
        assert ei.value.code == hip.SG_EINVAL and needle in str(ei.value)
    with pytest.raises(hip.SgError):
        oversegment.write_segs_json(str(tmp_path / "missing_dir" / "x.segs.json"), seg, "s")


def test_prepare_scene_keeps_its_error_for_a_missing_segs_file(sg_lib):
    """oversegment defaults to False, and the False path does not look at the new module"""
    import inspect
    from seggroup_amd import prepare
    sig = inspect.signature(prepare.prepare_scene)
    assert sig.parameters["oversegment"].default is False


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_asan_host_build_holds_the_merge_and_runs_it(sg_lib):
    """overseg.cpp is part of the host-only AddressSanitizer + UBSan build; the merge and the writer run clean under it on the
    hostile arrays and on a tie-heavy case (a child process with the sanitizer runtimes preloaded)."""
    if os.environ.get("SEGGROUP_HIP_HOST_LIB"):
        pytest.skip("already running inside the sanitizer child")
    csrc = os.path.join(ROOT, "seggroup_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    host_srcs = [ln for ln in mk.splitlines() if ln.startswith("HOST_SRCS")][0]
    assert "overseg.cpp" in host_srcs.split()
    r = subprocess.run(["make", "-C", csrc, "asan"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    so = os.path.join(csrc, "build_asan", "libseggroup_host_asan.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True).stdout
    assert " sg_overseg_merge" in syms and " sg_write_segs_json" in syms
    gxx = lambda n: subprocess.run(["g++", "-print-file-name=" + n], capture_output=True, text=True).stdout.strip()
    env = dict(os.environ, SEGGROUP_HIP_HOST_LIB=so, LD_PRELOAD=gxx("libasan.so") + ":" + gxx("libubsan.so"),
               ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0:exitcode=66", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    me = os.path.abspath(__file__)
    r = subprocess.run(["python3", "-m", "pytest", me, "-x", "-q", "-p", "no:cacheprovider", "-k",
                        "hostile or writer or (equals and (room_j0 or no_edges or one_vertex or isolated))"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "AddressSanitizer" not in tail and "runtime error" not in tail, tail
    assert " passed" in r.stdout


def test_design_table_is_generated_from_the_committed_profile():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import time_overseg
    doc = json.load(open(os.path.join(ROOT, "profiles", "overseg_time.json")))
    assert [m["V"] for m in doc["meshes"]] == [150000, 500000]
    assert time_overseg.table(doc) in open(os.path.join(ROOT, "DESIGN.md")).read()
