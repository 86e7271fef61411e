"""`.sgl` pseudo-label files on the GPU: the drivers write them in every path (engine with both label transfers, the per-scene loop,
the training driver) and every vector expanded from them equals the `.npy` / `.txt` files; device expansion (single and batched) equals
the host's; `seggroup_amd.evaluate` reproduces what infer.py logged, agrees across the three formats and with the NumPy oracle."""
import io
import json
import os
from contextlib import redirect_stdout

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SCENES = [(20000, 200, 73001, {}), (4000, 40, 73002, {"dup_frac": 0.05}), (30000, 300, 73003, {"seg_profile": "scannet"}),
          (12000, 120, 73004, {"raw_vertices": 15000}), (500000, 3000, 73005, {}), (9000, 90, 73006, {})]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    import torch
    from seggroup_amd import synthetic, weights
    root = str(tmp_path_factory.mktemp("sgl_tree"))
    scenes = [synthetic.make_scene(n, s, seed, name=f"scene{i:04d}_00", **kw) for i, (n, s, seed, kw) in enumerate(SCENES)]
    assert any(sc.unmap.shape[0] != sc.data.shape[0] for sc in scenes)
    synthetic.write_reference_tree(root, scenes)
    ck = os.path.join(root, "checkpoints", "exp", "models")
    os.makedirs(ck)
    torch.save({"state_dict": weights.to_full_state_dict(weights.load_npz(os.path.join(GOLDEN, "weights_g2.npz")))}, os.path.join(ck, "last.t7"))
    return root, [sc.name for sc in scenes]


def _check_dir(d, nvec):
    import torch
    from seggroup_amd import hip, pseudo_labels
    p = pseudo_labels.load(d)
    assert p.tables.shape[0] == nvec
    host = p.vectors()
    dev = p.to_device().cpu().numpy()
    dev64 = p.to_device(names=hip.LABEL_NAMES[nvec - 2:nvec], dtype=torch.int64).cpu().numpy()
    for i, n in enumerate(hip.LABEL_NAMES[:nvec]):
        npy = np.load(os.path.join(d, n + ".npy"))
        assert np.array_equal(host[i], npy), n
        assert np.array_equal(dev[i], npy), n
        assert open(os.path.join(d, n + ".txt"), "rb").read() == b"".join(b"%d\n" % x for x in npy.tolist()), n
    assert np.array_equal(dev64, host[nvec - 2:nvec].astype(np.int64))


def _infer(root, mode, transfer, batch, fmt="txt,npy,sgl"):
    import shutil
    from seggroup_amd import infer
    shutil.rmtree(os.path.join(root, "results"), ignore_errors=True)
    args = infer.build_parser().parse_args(["-n", "exp", "--" + mode, "--root", root, "--world-size", "1", "--out-format", fmt,
                                            "--label-transfer", transfer, "--batch", str(batch), "--inflight", "4", "-j", "2"])
    return infer.run_worker(0, 1, args)


def _last_infer_block(root):
    lines = open(os.path.join(root, "checkpoints", "exp", "run_infer.log")).read().splitlines()
    k = max(i for i, ln in enumerate(lines) if ln.startswith("==> Infer"))
    return lines[k:k + 44]


@pytest.mark.parametrize("mode,transfer,batch", [("ins_infer", "tables", 4), ("ins_infer", "full", 4), ("sem_infer", "tables", 4),
                                                 ("sem_infer", "full", 4), ("ins_infer", "tables", 0), ("sem_infer", "tables", 0)])
def test_driver_sgl_equals_vector_files_and_evaluate_reproduces_the_log(tree, mode, transfer, batch, capsys):
    from seggroup_amd import evaluate
    root, names = tree
    r = _infer(root, mode, transfer, batch)
    nvec = 14 if mode == "ins_infer" else 6
    for s in names:
        _check_dir(os.path.join(root, "results", "exp", s, mode), nvec)
    layer = "final" if mode == "ins_infer" else "2"
    js = os.path.join(root, "eval.json")
    capsys.readouterr()
    accs = evaluate.run(evaluate.build_parser().parse_args(["-n", "exp", "--stage", mode, "--root", root, "--layer", layer, "--json", js,
                                                            "--format", "sgl"]))
    out = capsys.readouterr().out.splitlines()
    s = accs[layer].summary()
    for k in ("iou_sem", "iou_ins", "acc_sem", "acc_ins", "acc_sem_sel", "acc_ins_sel", "n"):
        assert np.array_equal(np.asarray(s[k]), np.asarray(r[k]), equal_nan=True), k
    head = next(i for i, ln in enumerate(out) if ln.startswith("Layer %s" % layer))
    assert out[head + 1:head + 45] == _last_infer_block(root)
    assert json.load(open(js))["layers"][layer]["n"] == len(names)


def test_evaluate_all_layers_agree_across_formats(tree):
    from seggroup_amd import evaluate
    root, names = tree
    _infer(root, "ins_infer", "tables", 4)
    got = {}
    for fmt in ("sgl", "npy", "txt"):
        with redirect_stdout(io.StringIO()):
            got[fmt] = evaluate.run(evaluate.build_parser().parse_args(["-n", "exp", "--stage", "ins_infer", "--root", root, "--layer", "all",
                                                                        "--format", fmt, "--batch", "4"]))
    assert list(got["sgl"]) == ["1", "2", "3", "4", "final"]
    for l in got["sgl"]:
        assert np.array_equal(got["sgl"][l].v, got["npy"][l].v, equal_nan=True), l
        assert np.array_equal(got["sgl"][l].v, got["txt"][l].v, equal_nan=True), l


def _oracle_layers(p, gt, layers):
    from oracle import cpu_ref
    from seggroup_amd import evaluate
    vec = p.vectors()
    out = []
    for l in layers:
        ins_r, sem_r = evaluate.LAYER_ROWS[l]
        a, b, c = cpu_ref.evaluate(gt, vec[sem_r], vec[ins_r])
        out.append(np.concatenate([a.reshape(-1), b.reshape(-1), c]))
    return np.stack(out)


def test_eval_tables_equals_the_oracle_on_edge_cases():
    """Hand-made scenes: instance ids far beyond the LDS path's counters, a scene with no valid GT vertex, vertices that map to no point,
    negative semantic slots, 16- and 32-bit seg_of_vertex; every layer's counts exact, the float ratios to the ulp."""
    import torch
    from seggroup_amd import evaluate
    from seggroup_amd.pseudo_labels import PseudoLabels
    rng = np.random.default_rng(11)
    dev = torch.device("cuda", 0)

    def scene(S, V, nvec, max_id, gt_valid=0.8):
        tab = np.empty((nvec, S), np.int32)
        for t in range(nvec):
            kind = t % 3 if t < 12 else t - 11
            tab[t] = rng.integers(-1, max_id, S) if kind == 1 else (rng.integers(-1, 41, S) if kind == 2 else rng.integers(0, S, S))
        sov = rng.integers(-1, S, V).astype(np.int32)
        sov[rng.random(V) < 0.1] = -1
        gt = np.stack([np.where(rng.random(V) < gt_valid, rng.integers(0, 41, V), 0), rng.integers(-1, max_id + 3, V)], 1).astype(np.int32)
        return PseudoLabels(tab, sov), gt

    cases = [scene(500, 20000, 14, 40), scene(3000, 50001, 14, 5000), scene(40, 999, 14, 30, gt_valid=0.0), scene(1200, 7777, 14, 2000),
             scene(10, 3, 14, 5)]
    layers = evaluate.LAYERS_OF_MODE["ins"]
    m = evaluate.eval_tables_batch([c[0] for c in cases], [c[1] for c in cases], layers, dev)
    for k, (p, gt) in enumerate(cases):
        want = _oracle_layers(p, gt, layers)
        assert np.array_equal(m[k][:, :160], want[:, :160]), k
        np.testing.assert_array_max_ulp(np.nan_to_num(m[k][:, 160:], nan=-7.0), np.nan_to_num(want[:, 160:], nan=-7.0), maxulp=1)
        assert np.array_equal(np.isnan(m[k][:, 160:]), np.isnan(want[:, 160:]))
        # the per-vector path of the evaluator gives the same floats
        vec = p.vectors()
        lab = {l: (vec[evaluate.LAYER_ROWS[l][0]], vec[evaluate.LAYER_ROWS[l][1]]) for l in layers}
        assert np.array_equal(evaluate.eval_vectors(gt, lab, layers, dev), m[k], equal_nan=True), k
    # sem mode (6 vectors, layers 1-2) and S >= 65535 (32-bit seg_of_vertex)
    sem = [scene(70000, 30000, 6, 100), scene(300, 4000, 6, 50)]
    m = evaluate.eval_tables_batch([c[0] for c in sem], [c[1] for c in sem], ["1", "2"], dev)
    for k, (p, gt) in enumerate(sem):
        want = _oracle_layers(p, gt, ["1", "2"])
        assert np.array_equal(m[k][:, :160], want[:, :160]), k
        np.testing.assert_array_max_ulp(np.nan_to_num(m[k][:, 160:], nan=-7.0), np.nan_to_num(want[:, 160:], nan=-7.0), maxulp=1)


def test_batched_device_expansion_of_64_mixed_scenes():
    import torch
    from seggroup_amd import hip, pseudo_labels
    from seggroup_amd.pseudo_labels import PseudoLabels
    rng = np.random.default_rng(12)
    items = []
    for i in range(64):
        nvec = 14 if i % 3 else 6
        S = int(rng.choice([1, 7, 300, 1500, 2500, 6000]))
        V = int(rng.integers(0, 60000)) if i % 7 else int(rng.integers(1, 9))
        tab = rng.integers(-1, 100000, (nvec, S)).astype(np.int32)
        sov = rng.integers(-1, S, V).astype(np.int32)
        items.append(PseudoLabels(tab, sov))
    for names in (["layer_1.seg", "layer_2.sem"], ["layer_2.ins"]):
        for dt in (torch.int32, torch.int64):
            outs = pseudo_labels.expand_on_device(items, names, dtype=dt)
            for p, o in zip(items, outs):
                assert o.shape == (len(names), p.V) and o.dtype == dt
                assert np.array_equal(o.cpu().numpy(), p.vectors(names).astype(o.cpu().numpy().dtype))
    ins = [p for p in items if p.mode == "ins"]
    for p, o in zip(ins, pseudo_labels.expand_on_device(ins)):
        assert np.array_equal(o.cpu().numpy(), p.vectors())
    # one S >= 65535 in the batch: 32-bit seg_of_vertex for every scene
    big = PseudoLabels(rng.integers(-1, 9, (14, 70000)).astype(np.int32), rng.integers(-1, 70000, 12345).astype(np.int32))
    mixed = ins[:5] + [big]
    for p, o in zip(mixed, pseudo_labels.expand_on_device(mixed, hip.LABEL_NAMES[:3])):
        assert np.array_equal(o.cpu().numpy(), p.vectors(hip.LABEL_NAMES[:3]))
    assert np.array_equal(big.to_device().cpu().numpy(), big.vectors())


def test_train_driver_writes_sgl(golden_index, tmp_path):
    from seggroup_amd import synthetic, train
    root = str(tmp_path)
    scenes = []
    for i, name in enumerate(("tiny_4k", "tiny_dup_4k")):
        e = golden_index[name]
        scenes.append(synthetic.make_scene(e["n"], e["s"], e["seed"], name=f"scene{i:04d}_00", **e["kw"]))
    synthetic.write_reference_tree(root, scenes)
    for d in ("checkpoints/t/models", "results/t"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    args = train.build_parser().parse_args(["-n", "t", "--root", root, "--epochs", "1", "--out-format", "txt,npy,sgl", "--lr", "0.0002"])
    r = train.run_worker(0, 1, args)
    assert r["epoch"] == 1
    for sc in scenes:
        _check_dir(os.path.join(root, "results", "t", sc.name, "epoch_last"), 14)
