"""Instance AP on the host: `sg_ap_fold` + `sg_ap_match` + seggroup_amd.ap against the recorded results of the label consumer's
own evaluator on the eight fixture scenes (tools/capture_ap.py -> tests/golden/ap_cases.npz, ap_expected.json).

The contingency of each scene is formed here with np.unique, so no GPU is needed.  Every recorded integer of gt2pred / pred2gt must be
reproduced exactly, the NaN pattern of ap[18,10] must be the same and every finite AP and average must lie within 1e-9 absolute: the
integers are exact, so only the order of float64 additions over at most a few thousand terms in [0,1] can differ (about 1e-13), while the
smallest change one match can cause is far above 1e-9.  Also run in the sanitizer child (tools/run_asan_host_tests.sh).
"""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

LAYER_ROWS = {"1": (1, 2), "2": (4, 5), "3": (7, 8), "4": (10, 11), "final": (12, 13)}
TOL = 1e-9


def numpy_contingency(slot, n_slots, gt):
    """(gt list [G,2], first_vertex [n_slots], triples [T,3]) of one scene with np.unique; slot [V] in [0, n_slots)."""
    from seggroup_amd import ap
    gid = ap.gt_ids(gt)
    ids, cnt = np.unique(np.concatenate([[0], gid]), return_counts=True)
    cnt[0] -= 1
    g = np.searchsorted(ids, gid)
    G = ids.shape[0]
    key, n = np.unique(slot.astype(np.int64) * G + g, return_counts=True)
    first = np.full(n_slots, -1, np.int32)
    s, i = np.unique(slot, return_index=True)
    first[s] = i
    return ap.Contingency(np.stack([ids, cnt], 1), first, np.stack([key // G, key % G, n], 1))


def table_slots(sov, S):
    return np.where((sov >= 0) & (sov < S), sov, S)


def expand(tables, sov, row):
    return np.where(sov >= 0, tables[row][np.maximum(sov, 0)], -1).astype(np.int32)


@pytest.fixture(scope="module")
def cases(sg_lib):
    z = np.load(os.path.join(GOLDEN, "ap_cases.npz"))
    exp = json.load(open(os.path.join(GOLDEN, "ap_expected.json")))
    out = []
    for k in range(exp["num_scenes"]):
        sov, tables, gt, conf = z["sov_%d" % k], z["tables_%d" % k], z["gt_%d" % k], z["conf_%d" % k]
        out.append(dict(sov=sov, tables=tables, gt=gt, conf=conf, cont=numpy_contingency(table_slots(sov, tables.shape[1]), tables.shape[1] + 1, gt)))
    assert len(out) == 8 and all(c["sov"].shape[0] <= 30000 for c in out)
    return out, exp


def mask_conf(c, ir):
    ins = expand(c["tables"], c["sov"], ir)
    return c["conf"][np.unique(ins[ins > 0])]


def check_layer(layer_exp, acc):
    from seggroup_amd import ap
    got = acc.ap()
    want = np.array(layer_exp["ap"], dtype=np.float64)
    assert got.shape == want.shape == (18, 10)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    fin = ~np.isnan(want)
    assert np.abs(got[fin] - want[fin]).max() <= TOL
    avgs = ap.compute_averages(got)
    for k in ("all_ap", "all_ap_50%", "all_ap_25%"):
        assert abs(avgs[k] - layer_exp[k]) <= TOL, k
    for name, c in layer_exp["classes"].items():
        for k, v in c.items():
            g = avgs["classes"][name][k]
            assert (np.isnan(v) and np.isnan(g)) or abs(g - v) <= TOL, (name, k)
    return got


def test_every_recorded_integer_and_every_ap(cases):
    from seggroup_amd import ap
    scenes, exp = cases
    n_pred = 0
    for layer, (ir, sr) in LAYER_ROWS.items():
        acc = ap.APAccumulator()
        for k, c in enumerate(scenes):
            rec = ap.fold(c["cont"], c["tables"][ir], c["tables"][sr])
            g2p, p2g = rec.dicts()
            want = exp["layers"][layer]["scenes"][k]
            assert g2p == want["gt2pred"], (layer, k)
            assert p2g == want["pred2gt"], (layer, k)
            n_pred += rec.pred.shape[0]
            acc.add(ap.match(rec, mask_conf(c, ir)))
        got = check_layer(exp["layers"][layer], acc)
        assert np.isnan(got).all(axis=1).any() and (got == 0).all(axis=1).any() and (got > 0).any()
    assert n_pred > 500


def test_vector_form_gives_the_same_record(cases):
    """slot = the instance value (values <= 0 -> slot 0), rows from vector_rows: the same predictions, matches and pairs as the table form"""
    from seggroup_amd import ap
    scenes, _ = cases
    for c in scenes[:4]:
        for ir, sr in (LAYER_ROWS["1"], LAYER_ROWS["final"]):
            ins, sem = expand(c["tables"], c["sov"], ir), expand(c["tables"], c["sov"], sr)
            S = max(int(ins.max()), 0)
            cont = numpy_contingency(np.where(ins > 0, ins, 0), S + 1, c["gt"])
            a = ap.fold(cont, *ap.vector_rows(cont, sem))
            b = ap.fold(c["cont"], c["tables"][ir], c["tables"][sr])
            for x, y in ((a.pred, b.pred), (a.match, b.match), (a.gtrec, b.gtrec)):
                assert np.array_equal(x, y)
            conf = mask_conf(c, ir)
            ma, mb = ap.match(a, conf), ap.match(b, conf)
            assert np.array_equal(ma.y_true, mb.y_true) and np.array_equal(ma.y_score, mb.y_score) and np.array_equal(ma.info, mb.info)


def test_default_confidence_is_one(cases):
    from seggroup_amd import ap
    scenes, _ = cases
    c = scenes[0]
    rec = ap.fold(c["cont"], c["tables"][12], c["tables"][13])
    a, b = ap.match(rec), ap.match(rec, np.ones(10000))
    assert np.array_equal(a.y_score, b.y_score) and np.array_equal(a.y_true, b.y_true) and a.y_score.size and (a.y_score == 1.0).all()


def test_refusals(cases):
    from seggroup_amd import ap
    scenes, _ = cases
    c = scenes[2]
    S = c["tables"].shape[1]
    gt = c["gt"].copy()
    gt[5] = (3, 1000)
    with pytest.raises(ValueError, match="ins >= 1000"):
        ap.gt_ids(gt)
    gt[5] = (41, 2)
    with pytest.raises(ValueError, match="sem outside"):
        ap.gt_ids(gt)
    with pytest.raises(ValueError):
        ap.gt_ids(c["gt"][:, :1])
    cont = c["cont"]
    with pytest.raises(ValueError, match="differ in length"):
        ap.fold(cont, c["tables"][12], c["tables"][13][:-1])
    with pytest.raises(ValueError, match="slots for table rows"):
        ap.fold(cont, c["tables"][12][:-3], c["tables"][13][:-3])
    bad = ap.Contingency(cont.gt, cont.first_vertex, cont.triples.copy())
    bad.triples[3, 1] = cont.gt.shape[0]
    with pytest.raises(ValueError, match="out of range"):
        ap.fold(bad, c["tables"][12], c["tables"][13])
    bad = ap.Contingency(cont.gt, cont.first_vertex, cont.triples[::-1].copy())
    with pytest.raises(ValueError, match="order"):
        ap.fold(bad, c["tables"][12], c["tables"][13])
    bad = ap.Contingency(cont.gt[::-1].copy(), cont.first_vertex, cont.triples)
    with pytest.raises(ValueError):
        ap.fold(bad, c["tables"][12], c["tables"][13])
    rec = ap.fold(cont, c["tables"][12], c["tables"][13])
    with pytest.raises(ValueError, match="confidences"):
        ap.match(rec, np.ones(3))
    with pytest.raises(ValueError):
        ap.match(ap.Record(rec.pred, rec.match[:-1].copy(), rec.gtrec))
    with pytest.raises(ValueError, match="beyond the sem vector"):
        ap.vector_rows(cont, np.zeros(10, np.int32))
    assert S + 1 == cont.first_vertex.shape[0]


def test_precision_recall_integration_by_hand():
    """two true positives above one false positive, one hard false negative: thresholds 0.4 / 0.8 / 0.9 give (p, r) = (2/3, 2/3), (1, 2/3),
    (1, 1/3), then the end point (1, 0); recall steps centred on the points"""
    from seggroup_amd import ap
    got = ap.average_precision(np.array([1, 0, 1]), np.array([0.9, 0.4, 0.8]), 1)
    r = [2 / 3, 2 / 3, 2 / 3, 1 / 3, 0.0, 0.0]
    want = sum(p * 0.5 * (r[i] - r[i + 2]) for i, p in enumerate([2 / 3, 1.0, 1.0, 1.0]))
    assert abs(got - want) < 1e-15
    assert ap.average_precision(np.zeros(0), np.zeros(0), 3) == 0.0


def test_report_layout():
    from seggroup_amd import ap
    a = np.full((18, 10), np.nan)
    a[2] = np.linspace(0.1, 1.0, 10)
    lines = ap.report_lines(ap.compute_averages(a))
    assert lines[1] == "#" * 64 and lines[2].split() == ["what", ":", "AP", "AP_50%", "AP_25%"] and len(lines) == 4 + 18 + 3
    assert lines[4 + 2].startswith("chair          :") and lines[4 + 2].split()[-3:] == ["0.500", "0.100", "1.000"]
    assert lines[-2].startswith("average") and lines[-2].split()[-3:] == ["0.500", "0.100", "1.000"]
    js = ap.to_json(ap.compute_averages(a))
    assert set(js) == {"ap", "ap50", "ap25", "classes"} and js["classes"]["chair"]["ap50"] == pytest.approx(0.1)
