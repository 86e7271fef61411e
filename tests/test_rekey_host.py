"""Re-keying annotations, host side (needs no GPU): the group table, the aggregation writer, the click resolver
(sg_rekey_clicks) and the report of seggroup_amd/rekey.py, driven from vote results of the NumPy statement (tests/rekey_ref.py) -- on
hand-made cases for every rule, and on the synthetic scan against that statement and against what the reference's own label scripts
made of the written tree (tests/golden/rekey_expected.json, tools/capture_rekey.py); rekey_scan's refusals; the command line's."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import rekey_ref as R
from conftest import GOLDEN, ROOT

os.environ.setdefault("SEGGROUP_HOST_ONLY", "1")


def _vote(d):
    from seggroup_amd import rekey
    return rekey.Vote(**d)


def _host_rekey(src, new, agg, manual, name):
    """rekey_arrays with the device calls replaced by the statement's votes: only the host functions of the module run"""
    from seggroup_amd import rekey
    src, new = np.asarray(src, dtype=np.int64), np.asarray(new, dtype=np.int64)
    src_ids, src_rank = np.unique(src, return_inverse=True)
    table = rekey.group_table(agg, name, src_ids)
    grp = table[src_rank.reshape(-1)]
    nv = _vote(R.vote(new, grp, rekey.reached_groups(agg, name) + 1))
    out_manual = clicks = None
    if manual is not None:
        sv = _vote(R.vote(src, nv.rank, nv.row_ids.shape[0]))
        out_manual, clicks = rekey.resolve_clicks(manual, src, new, sv, nv.row_ids)
    report = rekey.assemble_report(name, agg, table, nv, src_ids.shape[0], int((grp != 0).sum()), int((nv.vertex_winner != 0).sum()),
                                   int((nv.vertex_winner == grp).sum()), clicks, src_ids)
    return dict(grp=grp, vote=nv, aggregation=rekey.rekeyed_aggregation(agg, name, nv.row_ids, nv.winner), manual=out_manual, clicks=clicks,
                report=report)


def _agg(*groups):
    return {"sceneId": "s", "segGroups": [dict(id=i, objectId=o, segments=list(s), label=l) for i, (o, s, l) in enumerate(groups)]}


def test_the_statement_votes_the_same_with_and_without_the_table(monkeypatch):
    rng = np.random.default_rng(3)
    for _ in range(30):
        v, nc = int(rng.integers(1, 500)), int(rng.integers(1, 7))
        ids, cols = rng.integers(0, 40, v) * 9 + 2, rng.integers(0, nc, v)
        a = R.vote(ids, cols, nc)
        monkeypatch.setattr(R, "DENSE_LIMIT", 0)
        b = R.vote(ids, cols, nc)
        monkeypatch.undo()
        assert all(np.array_equal(a[k], b[k]) for k in a)
    a = R.vote([5, 5, 5, 5, 9], [2, 1, 2, 1, 0], 3)
    assert a["row_ids"].tolist() == [5, 9] and a["winner"].tolist() == [1, 0] and a["tied"].tolist() == [1, 0]
    assert a["first_vertex"].tolist() == [1, 4] and a["distinct"].tolist() == [2, 1] and a["winner_count"].tolist() == [2, 1]
    assert a["rank"].tolist() == [0, 0, 0, 0, 1] and a["vertex_winner"].tolist() == [1, 1, 1, 1, 0]


def test_tie_goes_to_the_lowest_value_and_no_group_votes_too(sg_lib):
    from seggroup_amd import rekey
    agg = _agg((0, [10], "wall"), (1, [20], "floor"), (2, [30], "chair"))
    #      new segment 100: two of group 2, two of group 1 -> group 1; 200: two unlabeled, two of group 3 -> nobody; 300: group 3
    src = [20, 20, 10, 10, 40, 30, 40, 30, 30]
    new = [100, 100, 100, 100, 200, 200, 200, 200, 300]
    r = _host_rekey(src, new, agg, None, "s")
    assert r["vote"].winner.tolist() == [1, 0, 3] and r["vote"].tied.tolist() == [1, 1, 0]
    assert [g["segments"] for g in r["aggregation"]["segGroups"]] == [[100], [], [300]]
    assert r["report"]["tied_segments"] == 2 and r["report"]["impure_segments"] == 2 and r["report"]["lost_groups"] == [1]
    assert (r["report"]["annotated_before"], r["report"]["annotated_after"], r["report"]["unchanged"]) == (7, 5, 5)
    ins, sem = rekey.vertex_labels(rekey.Rekeyed("s", r["vote"], None, None, None, r["aggregation"], None, None, r["report"]),
                                   {"wall": 1, "floor": 2, "chair": 5})
    assert ins.tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 3] and sem.tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 5]
    assert r["report"] == R.rekey(src, new, agg, None, "s")["report"]


def test_the_last_group_listing_a_segment_owns_it(sg_lib):
    from seggroup_amd import rekey
    agg = _agg((0, [10, 20], "wall"), (1, [20, 30], "floor"))
    assert rekey.group_table(agg, "s", [10, 20, 30, 40]).tolist() == [1, 2, 2, 0]
    r = _host_rekey([10, 20, 20, 30], [7, 7, 7, 8], agg, None, "s")
    assert [g["segments"] for g in r["aggregation"]["segGroups"]] == [[], [7, 8]]


def test_two_groups_sharing_an_object_id_vote_apart(sg_lib):
    """by objectId the two halves of object 4 would outvote group 2 (5 > 4); the vote is on the file position"""
    agg = _agg((4, [10], "chair"), (4, [20], "chair"), (6, [30], "table"))
    src = [10] * 3 + [20] * 2 + [30] * 4
    r = _host_rekey(src, [50] * 9, agg, None, "s")
    assert r["vote"].winner.tolist() == [3] and r["vote"].winner_count.tolist() == [4] and r["vote"].distinct.tolist() == [3]
    assert [g["segments"] for g in r["aggregation"]["segGroups"]] == [[], [], [50]]
    assert r["report"]["lost_groups"] == [0, 1]


def test_scene0217_00_is_cut_at_object_31(sg_lib, tmp_path):
    from seggroup_amd import labels, rekey
    agg = _agg((30, [10], "wall"), (31, [20], "floor"), (32, [30], "chair"))
    agg["segGroups"][2]["extra"] = {"kept": True}
    name = "scene0217_00"
    assert rekey.reached_groups(agg, name) == 1 and rekey.reached_groups(agg, "scene0217_01") == 3
    assert rekey.group_table(agg, name, [10, 20, 30]).tolist() == [1, 0, 0]
    r = _host_rekey([10, 20, 30, 30], [1, 2, 3, 3], agg, None, name)
    assert [g["segments"] for g in r["aggregation"]["segGroups"]] == [[1], [], []]
    assert r["aggregation"]["segGroups"][2]["extra"] == {"kept": True} and r["report"]["lost_groups"] == []
    # the project's reader makes the same of the written file as of the source
    mapper = {"wall": 1, "floor": 2, "chair": 5}
    for doc, segs in ((agg, [10, 20, 30, 30]), (r["aggregation"], [1, 2, 3, 3])):
        p = str(tmp_path / (name + ".aggregation.json"))
        json.dump(doc, open(p, "w"))
        s2i, s2s = labels.load_aggregation(p, mapper)
        assert [s2i.get(s, 0) for s in segs] == [31, 0, 0, 0] and [s2s.get(s, 0) for s in segs] == [1, 0, 0, 0]
    other = _host_rekey([10, 20, 30, 30], [1, 2, 3, 3], agg, None, "scene0217_01")
    assert [g["segments"] for g in other["aggregation"]["segGroups"]] == [[1], [2], [3]]


def test_every_key_of_the_source_file_is_copied(sg_lib):
    agg = {"sceneId": "scannet.scene0000_00", "appId": "Aggregator.v2", "segmentsFile": "x.segs.json", "nested": {"a": [1, {"b": 2}]},
           "segGroups": [{"id": 7, "objectId": 0, "segments": [10, 11], "label": "wall", "obb": {"centroid": [0.5, 1, 2]}, "dominantNormal": [0, 0, 1],
                          "partId": 1, "index": 3}]}
    before = json.dumps(agg)
    r = _host_rekey([10, 11, 12], [3, 3, 4], agg, None, "scene0000_00")
    assert json.dumps(agg) == before, "the source content is not touched"
    out = r["aggregation"]
    assert list(out) == list(agg) and list(out["segGroups"][0]) == list(agg["segGroups"][0])
    want = json.loads(before)
    want["segGroups"][0]["segments"] = [3]
    assert out == want


def test_clicks_both_forms_and_every_way_a_click_can_go(sg_lib):
    agg = _agg((0, [10], "wall"), (1, [20], "floor"), (2, [30], "chair"))
    #        v:  0   1   2   3   4   5   6   7   8
    src = [10, 10, 10, 20, 20, 20, 30, 30, 30]
    new = [5, 6, 6, 6, 9, 9, 9, 9, 4]
    manual = {"1": {"10": 0, "20": 3},              # by point, string keys: v0 -> 5; v3 -> 6
              "2": [20, "30"],                      # bare list: overlap -> 9 at v4; 30 -> 9 at v6 (taken)
              "3": {"30": 99, 10: 7},               # out of range -> overlap 9 at v6; a point outside its segment -> most of 10 is 6, at v1
              "4": {"77": 2},                       # a source segment that is not in the scan
              "5": {"10": 1, "20": 3}}              # two clicks of one instance on new segment 6: the first point stays
    r = _host_rekey(src, new, agg, manual, "s")
    assert r["manual"] == {"1": {"5": 0, "6": 3}, "2": {"9": 4}, "3": {"9": 6, "6": 1}, "4": {}, "5": {"6": 1}}
    assert [c["how"] for c in r["clicks"]] == ["point", "point", "overlap", "overlap", "overlap", "overlap", "dropped", "point", "point"]
    assert [c["new_point"] for c in r["clicks"]] == [0, 3, 4, 6, 6, 1, -1, 1, 3]
    # winners: 4 -> group 3, 5 -> 1, 6 -> 1 (two of group 1, one of group 2), 9 -> tie of groups 2 and 3 -> 2
    assert r["vote"].row_ids.tolist() == [4, 5, 6, 9] and r["vote"].winner.tolist() == [3, 1, 1, 2]
    assert r["report"]["clicks"] == dict(total=9, by_point=4, by_overlap=4, dropped=1, on_taken=5, off_group=4)
    ref = R.rekey(src, new, agg, manual, "s")
    assert ref["manual"] == r["manual"] and ref["clicks"] == r["clicks"] and ref["report"] == r["report"]
    # what the project's manual reader picks from either file names the same kind of thing: segment ids of the file's own segmentation
    assert sorted(int(s) for ins in r["manual"] for s in r["manual"][ins]) == [5, 6, 6, 6, 9, 9]


def test_click_tables_are_untrusted(sg_lib):
    from seggroup_amd import hip, rekey
    src, new = np.array([10, 10, 20], np.int32), np.array([5, 6, 6], np.int32)
    good = R.vote(src, R.vote(new, [0, 0, 0], 1)["rank"], 2)
    rekey.resolve_clicks({"1": [10]}, src, new, _vote(good), [5, 6])

    def refused(needle, **change):
        d = dict(good)
        d.update({k: np.asarray(v, np.int32) for k, v in change.items()})
        with pytest.raises(hip.SgError) as ei:
            rekey.resolve_clicks({"1": [10]}, src, new, _vote(d), [5, 6])
        assert ei.value.code == hip.SG_EINVAL and needle in str(ei.value), str(ei.value)

    refused("do not ascend", row_ids=[20, 10])
    refused("new segment outside", winner=[0, 2])
    refused("new segment outside", winner=[-1, 1])
    refused("vertex outside", first_vertex=[0, 3])
    refused("vertex outside", first_vertex=[-1, 2])
    refused("not in the intersection", first_vertex=[2, 2])
    refused("not in the intersection", winner=[1, 1], first_vertex=[0, 2])


@pytest.fixture(scope="module")
def scan_case():
    scan, ann = R.source_scan()
    return scan, ann, R.clicks_with_points(scan, ann), json.load(open(os.path.join(GOLDEN, "rekey_expected.json")))


def test_the_synthetic_scan_is_the_one_the_golden_was_captured_for(scan_case):
    scan, ann, manual, exp = scan_case
    e = exp["scan"]
    assert (scan.xyz.shape[0], np.unique(scan.seg_indices).shape[0], len(ann["aggregation"]["segGroups"])) == (7833, 168, 30)
    assert (e["V"], e["src_segments"], e["groups"], e["clicks"]) == (7833, 168, 30, len(R.clicks_of(manual)))
    plain = R.rekey(scan.seg_indices, R.new_segmentation(scan, "cell14"), ann["aggregation"], ann["manual"], scan.name)["report"]
    # every rule is exercised on this input
    assert plain["new_segments"] == 42 and plain["impure_segments"] > 0 and plain["tied_segments"] > 0 and plain["lost_groups"]
    assert plain["clicks"]["total"] == 40 and plain["clicks"]["off_group"] > 0 and plain["clicks"]["on_taken"] > 0
    c = exp["cell14"]["report"]["clicks"]
    assert c["by_point"] > 0 and c["by_overlap"] > 0 and c["dropped"] == 1


@pytest.mark.parametrize("which", R.SEGMENTATIONS)
def test_host_functions_equal_the_statement_and_the_reference_scripts(sg_lib, scan_case, which, tmp_path):
    """the tree written from the module's host functions, read by the project's label producers, against what the reference's scripts
    wrote and returned for the statement's tree"""
    from oracle import prep_ref
    from seggroup_amd import labels, prepare
    scan, ann, manual, exp = scan_case
    new = R.new_segmentation(scan, which)
    ref = R.rekey(scan.seg_indices, new, ann["aggregation"], manual, scan.name)
    got = _host_rekey(scan.seg_indices, new, ann["aggregation"], manual, scan.name)
    assert got["aggregation"] == ref["aggregation"] and got["manual"] == ref["manual"] and got["clicks"] == ref["clicks"]
    assert got["report"] == ref["report"] == exp[which]["report"]
    assert np.array_equal(got["grp"], ref["grp"])
    td = str(tmp_path)
    sp = R.write_tree(td, scan, ann["tsv"], new, got)
    labels.generate_real_labels(sp, root=td)
    raw = os.path.join(td, "label", "real", "raw", scan.name)
    real = {k: open(os.path.join(raw, f"{scan.name}.{k}.txt"), "rb").read() for k in ("ins", "sem")}
    for k in ("ins", "sem"):
        assert R.digest(np.array(real[k].split(), dtype=np.int64)) == exp[which][f"real.{k}"], k
    if which in ("identity", "refine"):                            # the same bytes as from the source tree
        src_root = str(tmp_path / "src")
        src_res = dict(aggregation=ann["aggregation"], manual=None)
        ssp = R.write_tree(src_root, scan, ann["tsv"], scan.seg_indices, src_res)
        labels.generate_real_labels(ssp, root=src_root)
        for k in ("ins", "sem"):
            assert open(os.path.join(src_root, "label", "real", "raw", scan.name, f"{scan.name}.{k}.txt"), "rb").read() == real[k], k
    # weak labels: manual from the re-keyed click file; maxseg needs the mesh and the .seg.txt the GPU producers leave behind (here the oracle's)
    prepare.write_ply(os.path.join(sp, scan.name + "_vh_clean_2.ply"), scan.xyz, scan.rgb, scan.faces)
    mapper = prep_ref.make_mapper(scan.xyz.shape[0], 2000, scan.perm)
    raw_lab, _ = prep_ref.segment_lists(np.asarray(new, dtype=np.int32), mapper)
    with open(os.path.join(raw, scan.name + ".seg.txt"), "w") as f:
        f.write("".join("%d\n" % v for v in raw_lab))
    for style in ("manual", "maxseg"):
        ret = labels.generate_weak_labels(sp, None, label_style=style, manual_label_path=os.path.join(td, "manual_label"), root=td)
        assert list(ret) == exp[which][f"{style}.ret"], style
        for k in ("ins", "sem"):
            got_l = np.array(labels.load_labels(os.path.join(td, "label", "seg", style, "raw", scan.name, f"{scan.name}.{k}.txt")))
            assert R.digest(got_l) == exp[which][f"{style}.{k}"], (style, k)


def _source_tree(root, scan, ann, manual):
    from seggroup_amd import prepare
    sp = R.write_tree(root, scan, ann["tsv"], scan.seg_indices, dict(aggregation=ann["aggregation"], manual=manual))
    prepare.write_ply(os.path.join(sp, scan.name + "_vh_clean_2.ply"), scan.xyz, scan.rgb, scan.faces)
    return sp


def test_rekey_scan_refuses_the_source_tree_and_existing_files(sg_lib, scan_case, tmp_path):
    from seggroup_amd import rekey
    scan, ann, manual, _ = scan_case
    root = str(tmp_path / "src")
    sp = _source_tree(root, scan, ann, manual)
    new = R.new_segmentation(scan, "cell14")
    before = {f: open(os.path.join(sp, f), "rb").read() for f in os.listdir(sp)}
    with pytest.raises(ValueError, match="source scans"):
        rekey.rekey_scan(sp, root, new)
    os.symlink(root, str(tmp_path / "alias"))
    with pytest.raises(ValueError, match="source scans"):
        rekey.rekey_scan(sp + "/", str(tmp_path / "alias"), new)
    out = str(tmp_path / "out")
    for rel in (os.path.join("scans", scan.name, scan.name + ".aggregation.json"), os.path.join("scans", scan.name, scan.name + rekey.SEGS_SUFFIX),
                os.path.join("scans", scan.name, scan.name + "_vh_clean_2.ply"), os.path.join("manual_label", scan.name + ".json")):
        shutil.rmtree(out, ignore_errors=True)
        os.makedirs(os.path.dirname(os.path.join(out, rel)))
        open(os.path.join(out, rel), "w").write("mine")
        with pytest.raises(FileExistsError, match="force=True"):
            rekey.rekey_scan(sp, out, new, manual_label_path=os.path.join(root, "manual_label"))
        assert open(os.path.join(out, rel)).read() == "mine"
        assert sum(len(fs) for _, _, fs in os.walk(out)) == 1, "nothing was written beside it"
    assert {f: open(os.path.join(sp, f), "rb").read() for f in os.listdir(sp)} == before


def test_command_line_errors(sg_lib, tmp_path, capsys):
    from seggroup_amd import rekey
    scans = str(tmp_path / "scans")
    os.makedirs(scans)
    cases = ((["--scans", scans], "--out"),
             (["--out", str(tmp_path / "o")], "--scans"),
             (["--scans", scans, "--out", str(tmp_path / "o"), "--new-segs-from", scans, "--k-thresh", "0.05"], "do not go with it"),
             (["--scans", scans, "--out", str(tmp_path / "o"), "--new-segs-from", scans, "--seg-min-verts", "5"], "do not go with it"),
             (["--scans", str(tmp_path / "missing"), "--out", str(tmp_path / "o")], "is not a directory"),
             (["--scans", scans, "--out", str(tmp_path / "o"), "--new-segs-from", str(tmp_path / "missing")], "is not a directory"),
             (["--scans", scans, "--out", str(tmp_path / "o"), "--manual_label_path", str(tmp_path / "missing")], "is not a directory"),
             (["--scans", scans, "--out", str(tmp_path / "o"), "--workers", "many"], "invalid int value"))
    for argv, needle in cases:
        with pytest.raises(SystemExit) as ei:
            rekey.main(argv)
        assert ei.value.code == 2 and needle in capsys.readouterr().err, argv
    assert not os.path.exists(str(tmp_path / "o"))
    os.makedirs(os.path.join(scans, "a"))
    for n in ("x.segs.json", "y.segs.json"):
        open(os.path.join(scans, "a", n), "w").write("{}")
    with pytest.raises(ValueError, match="exactly one"):
        rekey._new_segs_file(scans, "a")
    os.remove(os.path.join(scans, "a", "y.segs.json"))
    assert rekey._new_segs_file(scans, "a").endswith("x.segs.json")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_asan_host_build_holds_the_click_resolver_and_runs_it(sg_lib):
    """rekey.cpp is part of the host-only AddressSanitizer + UBSan build; the resolver runs clean under it on the hand-made clicks and
    on the hostile tables (a child process with the sanitizer runtimes preloaded)."""
    if os.environ.get("SEGGROUP_HIP_HOST_LIB"):
        pytest.skip("already running inside the sanitizer child")
    csrc = os.path.join(ROOT, "seggroup_amd", "csrc")
    r = subprocess.run(["make", "-C", csrc, "asan"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    so = os.path.join(csrc, "build_asan", "libseggroup_host_asan.so")
    assert " sg_rekey_clicks" in subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True).stdout
    gxx = lambda n: subprocess.run(["g++", "-print-file-name=" + n], capture_output=True, text=True).stdout.strip()
    env = dict(os.environ, SEGGROUP_HIP_HOST_LIB=so, LD_PRELOAD=gxx("libasan.so") + ":" + gxx("libubsan.so"),
               ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0:exitcode=66", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-p", "no:cacheprovider", "-k", "click"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "AddressSanitizer" not in tail and "runtime error" not in tail, tail
    assert " passed" in r.stdout
