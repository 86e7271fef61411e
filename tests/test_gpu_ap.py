"""Instance AP on the GPU.  Kernel level: the triples, first vertices, ground-truth list and counts of `sg_ap_contingency`
(both seg_of_vertex widths, B = 1 and a ragged batch of 8, with and without the in-wave merge, twice for the same bytes) and of
`sg_ap_contingency_vectors` equal NumPy's exactly.  End to end: `evaluate --ap --layer all --json` on a synthetic tree gives the same "ap"
objects in the three label formats, equal to a deliberately naive NumPy evaluation written here from the semantics (masks and
count_nonzero), and without `--ap` the command prints what it printed before.  The new kernels are in the library and use no scratch."""
import io
import json
import os
import re
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_ap_host import LAYER_ROWS, expand, numpy_contingency, table_slots

pytestmark = pytest.mark.gpu

CLASS_IDS = [3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39]
SYNTHETIC = [(150000, 1500, 81001, {}), (500000, 3000, 81002, {}), (12000, 120, 81003, {"raw_vertices": 15000}),
             (30000, 300, 81004, {"seg_profile": "scannet"})]


def _same(a, b):
    return np.array_equal(a.gt, b.gt) and np.array_equal(a.first_vertex, b.first_vertex) and np.array_equal(a.triples, b.triples)


@pytest.fixture(scope="module")
def fixture_scenes(sg_lib):
    from seggroup_amd.pseudo_labels import PseudoLabels
    z = np.load(os.path.join(GOLDEN, "ap_cases.npz"))
    return [(PseudoLabels(z["tables_%d" % k], z["sov_%d" % k]), z["gt_%d" % k]) for k in range(8)]


@pytest.fixture(scope="module")
def synthetic_scenes(sg_lib):
    from seggroup_amd import synthetic
    from seggroup_amd.pseudo_labels import PseudoLabels
    rng = np.random.default_rng(5)
    out = []
    for n, s, seed, kw in SYNTHETIC:
        sc = synthetic.make_scene(n, s, seed, **kw)
        S = sc.num_segments
        sov = sc.seg[sc.unmap].astype(np.int32)
        sov[rng.random(sov.shape[0]) < 0.01] = -1
        tab = np.stack([rng.integers(-1, max(2, S // 10), S) if t % 3 == 1 or t == 12 else rng.integers(-1, 41, S) for t in range(14)]).astype(np.int32)
        out.append((PseudoLabels(tab, sov), np.ascontiguousarray(sc.gt, dtype=np.int32)))
    assert out[2][0].V == 15000 and out[0][0].V == 150000
    return out


def _want(p, gt):
    return numpy_contingency(table_slots(p.seg_of_vertex, p.S), p.S + 1, gt)


def test_fixture_batch_of_8_both_widths_merge_and_plain_twice(fixture_scenes):
    from seggroup_amd import ap
    items, gts = [p for p, _ in fixture_scenes], [g for _, g in fixture_scenes]
    assert len({p.V for p in items}) > 4                      # ragged
    want = [_want(p, g) for p, g in fixture_scenes]
    runs = [ap.contingency_batch(items, gts, sov_width=w, flags=f) for w in (2, 4) for f in (0, 1)]
    runs.append(ap.contingency_batch(items, gts))
    for r in runs:
        for k in range(8):
            assert _same(r[k], want[k]), k
    for k, (p, g) in enumerate(fixture_scenes):               # B = 1
        assert _same(ap.contingency_batch([p], [g])[0], want[k]), k
        assert _same(ap.contingency_batch([p], [g], sov_width=4, flags=1)[0], want[k]), k


def test_synthetic_scenes_single_and_in_a_ragged_batch(synthetic_scenes, fixture_scenes):
    from seggroup_amd import ap
    want = [_want(p, g) for p, g in synthetic_scenes]
    for k, (p, g) in enumerate(synthetic_scenes):
        for w in (2, 4):
            a = ap.contingency_batch([p], [g], sov_width=w)[0]
            assert _same(a, want[k]), (k, w)
        assert _same(ap.contingency_batch([p], [g], flags=1)[0], want[k]), k
        assert int(want[k].triples[:, 2].sum()) == p.V
    mixed = synthetic_scenes + fixture_scenes[:4]
    got = ap.contingency_batch([p for p, _ in mixed], [g for _, g in mixed])
    assert len(got) == 8
    for k, (p, g) in enumerate(mixed):
        assert _same(got[k], want[k] if k < 4 else _want(p, g)), k


def test_vector_form_equals_numpy_and_the_table_form(fixture_scenes, synthetic_scenes):
    from seggroup_amd import ap
    for p, gt in fixture_scenes[:3] + synthetic_scenes[:1] + synthetic_scenes[2:]:
        for ir, sr in (LAYER_ROWS["1"], LAYER_ROWS["final"]):
            ins, sem = expand(p.tables, p.seg_of_vertex, ir), expand(p.tables, p.seg_of_vertex, sr)
            S = max(int(ins.max()), 0)
            want = numpy_contingency(np.where(ins > 0, ins, 0), S + 1, gt)
            for f in (0, 1):
                assert _same(ap.contingency_vector(ins, gt, flags=f), want)
            a = ap.fold(want, *ap.vector_rows(want, sem))
            b = ap.fold(ap.contingency_batch([p], [gt])[0], p.tables[ir], p.tables[sr])
            assert np.array_equal(a.pred, b.pred) and np.array_equal(a.match, b.match) and np.array_equal(a.gtrec, b.gtrec)


def test_many_ground_truth_ids_and_refusals(fixture_scenes):
    """more ids than the default workspace allows for (a second, larger call), an empty instance vector, labels the id cannot hold"""
    from seggroup_amd import ap
    from seggroup_amd.pseudo_labels import PseudoLabels
    rng = np.random.default_rng(9)
    V, S = 40000, 700
    p = PseudoLabels(rng.integers(-1, 50, (14, S)).astype(np.int32), np.sort(rng.integers(-1, S, V)).astype(np.int32))
    gt = np.stack([rng.integers(0, 41, V), rng.integers(-1, 1000, V)], 1).astype(np.int32)
    want = _want(p, gt)
    assert want.gt.shape[0] > 20000
    assert _same(ap.contingency_batch([p], [gt])[0], want)
    items, gts = [p, fixture_scenes[0][0]], [gt, fixture_scenes[0][1]]
    got = ap.contingency_batch(items, gts, flags=1)
    assert _same(got[0], want) and _same(got[1], _want(*fixture_scenes[0]))
    none = np.full(5000, -1, np.int32)
    assert _same(ap.contingency_vector(none, gt[:5000]), numpy_contingency(np.zeros(5000, np.int64), 1, gt[:5000]))
    for bad in ((3, 1000), (41, 1), (-1, 5)):
        g2 = gt.copy()
        g2[V - 7] = bad
        with pytest.raises(ValueError, match="sem outside 0..40 or ins >= 1000"):
            ap.contingency_batch([p], [g2])
        with pytest.raises(ValueError, match="sem outside 0..40 or ins >= 1000"):
            ap.contingency_vector(expand(p.tables, p.seg_of_vertex, 1), g2)
    with pytest.raises(ValueError, match="vertices in the labels"):
        ap.contingency_batch([p], [gt[:-1]])
    with pytest.raises(ValueError, match="label values for"):
        ap.contingency_vector(none, gt)


def test_fixture_ap_through_the_gpu_equals_the_recorded_reference(fixture_scenes):
    """the whole chain on the fixture scenes: device contingency, fold, match, accumulate -> the recorded ap[18,10] of every layer"""
    from seggroup_amd import ap
    z = np.load(os.path.join(GOLDEN, "ap_cases.npz"))
    exp = json.load(open(os.path.join(GOLDEN, "ap_expected.json")))
    conts = ap.contingency_batch([p for p, _ in fixture_scenes], [g for _, g in fixture_scenes])
    for layer, (ir, sr) in LAYER_ROWS.items():
        acc = ap.APAccumulator()
        for k, ((p, _), c) in enumerate(zip(fixture_scenes, conts)):
            ins = expand(p.tables, p.seg_of_vertex, ir)
            acc.add(ap.match(ap.fold(c, p.tables[ir], p.tables[sr]), z["conf_%d" % k][np.unique(ins[ins > 0])]))
        got, want = acc.ap(), np.array(exp["layers"][layer]["ap"])
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.abs(got[~np.isnan(want)] - want[~np.isnan(want)]).max() <= 1e-9


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------------------
TREE = [(20000, 200, 83001, {}), (4000, 40, 83002, {"dup_frac": 0.05}), (30000, 300, 83003, {"seg_profile": "scannet"}),
        (12000, 120, 83004, {"raw_vertices": 15000}), (9000, 90, 83006, {})]
OVERLAPS = [0.5 + 0.05 * i for i in range(9)] + [0.25]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    import torch
    from seggroup_amd import infer, synthetic, weights
    root = str(tmp_path_factory.mktemp("ap_tree"))
    scenes = [synthetic.make_scene(n, s, seed, name=f"scene{i:04d}_00", **kw) for i, (n, s, seed, kw) in enumerate(TREE)]
    synthetic.write_reference_tree(root, scenes)
    ck = os.path.join(root, "checkpoints", "exp", "models")
    os.makedirs(ck)
    torch.save({"state_dict": weights.to_full_state_dict(weights.load_npz(os.path.join(GOLDEN, "weights_g2.npz")))}, os.path.join(ck, "last.t7"))
    for mode in ("ins_infer", "sem_infer"):
        args = infer.build_parser().parse_args(["-n", "exp", "--" + mode, "--root", root, "--world-size", "1", "--out-format", "txt,npy,sgl",
                                                "--label-transfer", "tables", "--batch", "4", "--inflight", "4", "-j", "2"])
        infer.run_worker(0, 1, args)
    return root, scenes


def naive_ap(scenes):
    """scenes: [(ins [V], sem [V], gt [V,2])] -> ap [18,10].  Written from DESIGN.md 9d, on purpose the slow way."""
    pairs = {(c, o): ([], []) for c in range(18) for o in range(10)}
    hard = np.zeros((18, 10), np.int64)
    has_gt, has_pred = np.zeros(18, bool), np.zeros(18, bool)
    for ins, sem, gt in scenes:
        gid = np.where(gt[:, 1] > 0, gt[:, 0].astype(np.int64) * 1000 + gt[:, 1], 0)
        void = ~np.isin(gid // 1000, CLASS_IDS)
        truths = [(int(i), int(np.count_nonzero(gid == i))) for i in np.unique(gid) if i != 0 and int(i) // 1000 in CLASS_IDS]
        preds = []
        for val in np.unique(ins[ins > 0]):
            mask = ins == val
            label, size = int(sem[np.nonzero(mask)[0][0]]), int(np.count_nonzero(mask))
            if label in CLASS_IDS and size >= 100:
                preds.append((mask, label, size, int(np.count_nonzero(mask & void))))
        inter = np.array([[np.count_nonzero(m & (gid == i)) for i, _ in truths] for m, _, _, _ in preds]).reshape(len(preds), len(truths))

        def iou(p, t):
            return inter[p, t] / (truths[t][1] + preds[p][2] - inter[p, t])
        for c, cid in enumerate(CLASS_IDS):
            mine = [p for p in range(len(preds)) if preds[p][1] == cid]
            same = [t for t in range(len(truths)) if truths[t][0] // 1000 == cid]
            large = [t for t in same if truths[t][1] >= 100]
            has_gt[c] |= bool(large)
            has_pred[c] |= bool(mine)
            for o, th in enumerate(OVERLAPS):
                y_true, y_score = pairs[c, o]
                taken = set()
                for t in large:
                    best = None
                    for p in mine:
                        if p in taken or inter[p, t] == 0 or not iou(p, t) > th:
                            continue
                        if best is None:
                            best = 1.0
                            taken.add(p)
                            y_true.append(1); y_score.append(1.0)
                        else:                                  # a second match of this ground truth: a false positive
                            y_true.append(0); y_score.append(1.0)
                    if best is None:
                        hard[c, o] += 1
                for p in mine:
                    if any(inter[p, t] > 0 and iou(p, t) > th for t in same):
                        continue
                    ignore = preds[p][3] + sum(int(inter[p, t]) for t in same if truths[t][1] < 100)
                    if ignore / preds[p][2] <= th:
                        y_true.append(0); y_score.append(1.0)
    ap = np.full((18, 10), np.nan)
    for c in range(18):
        for o in range(10):
            if has_gt[c] and not has_pred[c]:
                ap[c, o] = 0.0
            if not (has_gt[c] and has_pred[c]):
                continue
            yt, ys = np.array(pairs[c, o][0], float), np.array(pairs[c, o][1], float)
            prec, rec = [], []
            for s in np.unique(ys):
                tp = yt[ys >= s].sum()
                prec.append(tp / np.count_nonzero(ys >= s))
                rec.append(tp / (yt.sum() + hard[c, o]))
            prec.append(1.0); rec.append(0.0)
            r = [rec[0]] + rec + [0.0]
            ap[c, o] = sum(prec[i] * 0.5 * (r[i] - r[i + 2]) for i in range(len(prec)))
    return ap


def _close(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.array_equal(np.isnan(a), np.isnan(b)) and (np.abs(a - b)[~np.isnan(a)] <= 1e-9).all()


def _run_eval(root, stage, extra):
    from seggroup_amd import evaluate
    buf = io.StringIO()
    with redirect_stdout(buf):
        evaluate.main(["-n", "exp", "--stage", stage, "--root", root, "--batch", "2"] + extra)
    return buf.getvalue().splitlines()


def test_evaluate_ap_across_formats_against_the_naive_evaluation(tree):
    from seggroup_amd import ap, evaluate, pseudo_labels
    root, scenes = tree
    got = {}
    for fmt in ("sgl", "npy", "txt"):
        js = os.path.join(root, "ap_%s.json" % fmt)
        out = _run_eval(root, "ins_infer", ["--layer", "all", "--format", fmt, "--ap", "--json", js])
        got[fmt] = json.load(open(js))["layers"]
        assert sum(ln.startswith("Instance AP, layer") for ln in out) == 5
    assert list(got["sgl"]) == ["1", "2", "3", "4", "final"]
    for layer in got["sgl"]:
        a = got["sgl"][layer]["ap"]
        assert set(a) == {"ap", "ap50", "ap25", "classes"} and list(a["classes"]) == ap.CLASS_LABELS
        for fmt in ("npy", "txt"):
            assert json.dumps(got[fmt][layer]["ap"]) == json.dumps(a), (layer, fmt)
            assert got[fmt][layer]["v"] == got["sgl"][layer]["v"]
        ir, sr = evaluate.LAYER_ROWS[layer]
        data = []
        for sc in scenes:
            p = pseudo_labels.load(os.path.join(root, "results", "exp", sc.name, "ins_infer"))
            data.append((expand(p.tables, p.seg_of_vertex, ir), expand(p.tables, p.seg_of_vertex, sr), evaluate.load_gt(root, sc.name)))
        want = ap.compute_averages(naive_ap(data))
        assert _close([a["ap"], a["ap50"], a["ap25"]], [want["all_ap"], want["all_ap_50%"], want["all_ap_25%"]]), layer
        for n in ap.CLASS_LABELS:
            assert _close([a["classes"][n][k] for k in ("ap", "ap50", "ap25")], [want["classes"][n][k] for k in ("ap", "ap50%", "ap25%")]), (layer, n)
    # a single layer gives that layer's object
    js = os.path.join(root, "ap_one.json")
    _run_eval(root, "ins_infer", ["--layer", "3", "--ap", "--json", js])
    assert json.dumps(json.load(open(js))["layers"]["3"]["ap"]) == json.dumps(got["sgl"]["3"]["ap"])


def _without_time(lines):
    return [re.sub(r" in [0-9.]+ s ", " in T s ", ln) if ln.startswith("evaluated ") else ln for ln in lines]


def test_without_the_flag_the_output_is_what_it_was(tree):
    root, _ = tree
    block = 1 + 4 + 18 + 3
    for fmt in ("sgl", "npy"):
        js0, js1 = os.path.join(root, "plain.json"), os.path.join(root, "with_ap.json")
        plain = _run_eval(root, "ins_infer", ["--layer", "all", "--format", fmt, "--json", js0])
        with_ap = _run_eval(root, "ins_infer", ["--layer", "all", "--format", fmt, "--json", js1, "--ap"])
        kept, k = [], 0
        while k < len(with_ap):
            if with_ap[k].startswith("Instance AP, layer"):
                k += block
                continue
            kept.append(with_ap[k])
            k += 1
        assert len(with_ap) == len(plain) + 5 * block
        assert _without_time(kept) == _without_time(plain)
        a, b = json.load(open(js0)), json.load(open(js1))
        assert all("ap" not in v for v in a["layers"].values()) and all("ap" in v for v in b["layers"].values())
        for l in a["layers"]:
            assert a["layers"][l]["v"] == b["layers"][l]["v"]
    assert "seggroup_amd.ap" in sys.modules


def test_sem_infer_directories_allow_layers_1_and_2_only(tree):
    root, _ = tree
    js = os.path.join(root, "sem.json")
    out = _run_eval(root, "sem_infer", ["--layer", "all", "--ap", "--json", js])
    assert sum(ln.startswith("Instance AP, layer") for ln in out) == 2 and any(ln.startswith("note: sem_infer labels") for ln in out)
    assert list(json.load(open(js))["layers"]) == ["1", "2"]
    with pytest.raises(SystemExit, match="--ap is defined for --layer 1, 2 or all"):
        _run_eval(root, "sem_infer", ["--layer", "final", "--ap"])


def test_the_new_kernels_are_in_the_library_and_use_no_scratch(sg_lib):
    from seggroup_amd import hip
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import scratch_report
    ks = [k for k in scratch_report.kernels_of_library(hip.LIB_PATH) if "k_ap_" in k[0]]
    names = " ".join(k[0] for k in ks)
    for needle in ("k_ap_gt_count", "k_ap_gt_index", "k_ap_contingency", "k_ap_chunk_count", "k_ap_chunk_scan", "k_ap_compact"):
        assert needle in names, needle
    assert len([k for k in ks if "k_ap_contingency" in k[0]]) == 6          # three slot sources x merge / plain
    assert not [k for k in ks if k[1]], "kernels with scratch: %r" % [k for k in ks if k[1]]
    pk = scratch_report.packed_fp32_of_library(hip.LIB_PATH)
    assert not [k for k in pk if "k_ap_" in str(k)]
