"""The compact pseudo-label file (`pseudo_labels.sgl`) on the host: writer job and readers round trip, the untrusted-input checks, the
expander's byte-identical files, and the evaluator's host side (discovery, format order, refusals, report).  No GPU needed."""
import io
import os
import struct
import zlib
from contextlib import redirect_stdout

import numpy as np
import pytest

from conftest import ROOT  # noqa: F401


def _case(rng, nvec, S, V):
    tab = rng.integers(-1, 3000, (nvec, S)).astype(np.int32)
    sov = rng.integers(-1, S, V).astype(np.int32)
    sov[: min(V, 7)] = -1                                  # vertices that map to no point
    if V > 10:
        sov[8] = S - 1
        sov[9] = 0
    return tab, sov


def _writer_roundtrip(sg_lib, d, tab, sov):
    from seggroup_amd import hip
    w = sg_lib.sg_writer_create(2, 16)
    try:
        hip.check(sg_lib.sg_writer_submit_scene_sgl(w, d.encode(), tab.ctypes.data, tab.shape[1], sov.ctypes.data, sov.shape[0], tab.shape[0], 3))
        hip.check(sg_lib.sg_writer_flush(w))
    finally:
        sg_lib.sg_writer_destroy(w)


@pytest.mark.parametrize("nvec,S,V", [(14, 1500, 20011), (6, 1500, 4096), (14, 70000, 3001), (6, 65535, 999), (14, 65534, 1000), (6, 3, 0)])
def test_writer_job_round_trip(sg_lib, tmp_path, nvec, S, V):
    from seggroup_amd import hip, pseudo_labels
    rng = np.random.default_rng(nvec * 1000 + S)
    tab, sov = _case(rng, nvec, S, V)
    d = str(tmp_path)
    _writer_roundtrip(sg_lib, d, tab, sov)
    path = os.path.join(d, "pseudo_labels.sgl")
    assert sorted(os.listdir(d)) == ["pseudo_labels.sgl"]            # the temporary name is gone
    h = pseudo_labels.read_header(path)
    width = 2 if S < 65535 else 4
    assert h == {"version": 1, "nvec": nvec, "S": S, "V": V, "sov_width": width}
    raw = open(path, "rb").read()
    assert len(raw) == 48 + nvec * S * 4 + V * width
    assert raw[:8] == b"SGLABEL\0"
    assert struct.unpack_from("<I", raw, 40)[0] == zlib.crc32(raw[48:])
    if width == 2:
        stored = np.frombuffer(raw, np.uint16, V, 48 + nvec * S * 4)
        assert np.array_equal(stored, np.where(sov < 0, 0xFFFF, sov).astype(np.uint16))
    p = pseudo_labels.load(d)
    assert np.array_equal(p.tables, tab) and np.array_equal(p.seg_of_vertex, sov)
    assert p.V == V and p.S == S and p.names == hip.LABEL_NAMES[:nvec] and p.mode == ("ins" if nvec == 14 else "sem")
    ref = np.empty((nvec, V), np.int32)
    hip.check(sg_lib.sg_expand_labels(tab.ctypes.data, nvec, S, sov.ctypes.data, V, ref.ctypes.data))
    assert np.array_equal(p.vectors(), ref)
    assert np.array_equal(p.vector(hip.LABEL_NAMES[nvec - 1]), ref[nvec - 1])
    # the synchronous writer gives the same bytes
    p2 = pseudo_labels.write(str(tmp_path / "again.sgl"), tab, sov)
    assert open(p2, "rb").read() == raw


def _good_file(tmp_path):
    from seggroup_amd import pseudo_labels
    rng = np.random.default_rng(5)
    tab, sov = _case(rng, 14, 100, 5000)
    return pseudo_labels.write(str(tmp_path / "good.sgl"), tab, sov)


def _expect_bad(path, what):
    from seggroup_amd import pseudo_labels
    with pytest.raises(ValueError):
        pseudo_labels.load(path)
    assert os.path.exists(path), what


def test_corrupt_files_are_rejected(sg_lib, tmp_path):
    from seggroup_amd import hip
    good = open(_good_file(tmp_path), "rb").read()
    cases = {}
    for n in (0, 10, 47, 48, 100, len(good) - 1):
        cases[f"truncated_{n}"] = good[:n]
    cases["trailing"] = good + b"\0"
    for off in (48, 48 + 14 * 100 * 4 - 1, len(good) - 1, len(good) // 2):
        b = bytearray(good); b[off] ^= 0x40; cases[f"flip_{off}"] = bytes(b)
    b = bytearray(good); b[0:8] = b"SGLABEX\0"; cases["magic"] = bytes(b)
    b = bytearray(good); struct.pack_into("<I", b, 8, 2); cases["version"] = bytes(b)
    b = bytearray(good); struct.pack_into("<I", b, 12, 15); cases["nvec_15"] = bytes(b)
    b = bytearray(good); struct.pack_into("<I", b, 12, 0); cases["nvec_0"] = bytes(b)
    b = bytearray(good); struct.pack_into("<I", b, 28, 0); cases["reserved"] = bytes(b[:28]) + struct.pack("<I", 7) + bytes(b[32:])
    b = bytearray(good); struct.pack_into("<I", b, 24, 4); cases["width_mismatch"] = bytes(b)
    # sizes chosen to overflow nvec*S*4 and V*width in 32 bits, with a payload length that matches the wrapped product
    for name, (nvec, S, V, width) in {"nvecS": (14, 0x7FFFFFFF, 5000, 4), "Vw": (14, 100, 0xFFFFFFFF, 2), "S_huge": (1, 0x40000001, 0, 4)}.items():
        b = bytearray(good)
        struct.pack_into("<IIIII", b, 12, nvec, S, V, width, 0)
        struct.pack_into("<Q", b, 32, (nvec * S * 4 + V * width) & 0xFFFFFFFF)
        cases[f"overflow_{name}"] = bytes(b)
        struct.pack_into("<Q", b, 32, nvec * S * 4 + V * width)
        cases[f"huge_{name}"] = bytes(b)
    # a CRC-correct file whose seg_of_vertex names a segment beyond S
    tab = np.zeros((6, 10), np.int32)
    payload = tab.tobytes() + np.array([0, 10, 0xFFFF], np.uint16).tobytes()
    hdr = b"SGLABEL\0" + struct.pack("<IIIIII", 1, 6, 10, 3, 2, 0) + struct.pack("<Q", len(payload)) + struct.pack("<II", zlib.crc32(payload), 0)
    cases["sov_out_of_range"] = hdr + payload
    for name, data in cases.items():
        p = str(tmp_path / f"{name}.sgl")
        open(p, "wb").write(data)
        _expect_bad(p, name)
    # the C entry points themselves: SG_EINVAL, never a crash
    info = (__import__("ctypes").c_int * 5)()
    assert sg_lib.sg_read_sgl_header(str(tmp_path / "magic.sgl").encode(), info) == hip.SG_EINVAL
    assert sg_lib.sg_read_sgl_header(str(tmp_path / "nope.sgl").encode(), info) == hip.SG_EINVAL
    t = np.zeros(14 * 100, np.int32); s = np.zeros(10, np.int32)
    assert sg_lib.sg_read_sgl(str(tmp_path / "good.sgl").encode(), t.ctypes.data, t.size, s.ctypes.data, s.size) == hip.SG_EINVAL  # capacity


def test_writer_refuses_bad_seg_of_vertex(sg_lib, tmp_path):
    from seggroup_amd import pseudo_labels
    with pytest.raises(ValueError):
        pseudo_labels.write(str(tmp_path), np.zeros((14, 5), np.int32), np.array([0, 5], np.int32))
    with pytest.raises(ValueError):
        pseudo_labels.write(str(tmp_path), np.zeros((15, 5), np.int32), np.array([0, 1], np.int32))
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("nvec", [14, 6])
def test_expand_tool_is_byte_identical_to_the_writer(sg_lib, tmp_path, nvec):
    from seggroup_amd import expand, hip, pseudo_labels
    rng = np.random.default_rng(nvec)
    exp = tmp_path / "results" / "e"
    scenes = {}
    for k, V in enumerate((3001, 150, 20000)):
        S = (300, 70000, 1500)[k]
        tab, sov = _case(rng, nvec, S, V)
        d = exp / f"scene{k:04d}_00" / "ins_infer"
        d.mkdir(parents=True)
        pseudo_labels.write(str(d), tab, sov)
        ref = tmp_path / f"ref{k}"
        ref.mkdir()
        w = sg_lib.sg_writer_create(2, 16)
        hip.check(sg_lib.sg_writer_submit_scene_tables(w, str(ref).encode(), tab.ctypes.data, S, sov.ctypes.data, V, nvec, 3, 0))
        hip.check(sg_lib.sg_writer_flush(w))
        sg_lib.sg_writer_destroy(w)
        scenes[d] = ref
    expand.main(["-n", "e", "--stage", "ins_infer", "--root", str(tmp_path)])
    for d, ref in scenes.items():
        names = sorted(os.listdir(ref))
        assert len(names) == 2 * nvec
        assert sorted(os.listdir(d)) == sorted(names + ["pseudo_labels.sgl"])
        for n in names:
            assert open(d / n, "rb").read() == open(ref / n, "rb").read(), n
    # --only: exactly the named files, same bytes
    for d in scenes:
        for n in os.listdir(d):
            if n != "pseudo_labels.sgl":
                os.remove(d / n)
    only = ["layer_2.sem", "layer_1.ins"] if nvec == 6 else ["final.ins", "final.sem"]
    expand.main(["-n", "e", "--stage", "ins_infer", "--root", str(tmp_path), "--only", ",".join(only), "--out-format", "txt"])
    for d, ref in scenes.items():
        assert sorted(os.listdir(d)) == sorted([n + ".txt" for n in only] + ["pseudo_labels.sgl"])
        for n in only:
            assert open(d / (n + ".txt"), "rb").read() == open(ref / (n + ".txt"), "rb").read()


def _tree(tmp_path, layout):
    """results/e/<scene>/epoch_last with the given per-scene kinds: 'sgl14', 'sgl6', 'npy14', 'txt14', 'npy6', 'all14', None"""
    from seggroup_amd import hip, pseudo_labels
    rng = np.random.default_rng(0)
    names = []
    for k, kind in enumerate(layout):
        s = f"scene{k:04d}_00"
        names.append(s)
        if kind is None:
            continue
        d = tmp_path / "results" / "e" / s / "epoch_last"
        d.mkdir(parents=True)
        nvec = 14 if kind.endswith("14") else 6
        tab, sov = _case(rng, nvec, 50, 200)
        vec = np.where(sov[None] >= 0, tab[:, np.maximum(sov, 0)], -1).astype(np.int32)
        if kind.startswith(("sgl", "all")):
            pseudo_labels.write(str(d), tab, sov)
        for i in range(nvec):
            if kind.startswith(("npy", "all")):
                np.save(d / (hip.LABEL_NAMES[i] + ".npy"), vec[i])
            if kind.startswith(("txt", "all")):
                (d / (hip.LABEL_NAMES[i] + ".txt")).write_text("".join("%d\n" % x for x in vec[i]))
    lst = tmp_path / "list.txt"
    lst.write_text("".join(n + "\n" for n in names))
    return names, str(lst)


def test_evaluate_discovery_and_format_order(sg_lib, tmp_path):
    from seggroup_amd import evaluate
    names, lst = _tree(tmp_path, ["all14", "npy14", "txt14", "sgl14"])
    found, layers = evaluate.discover(str(tmp_path), "e", "epoch_last", names, "auto", "all")
    assert [f[2] for f in found] == ["sgl", "npy", "txt", "sgl"]
    assert all(f[3] == "ins" for f in found) and layers == ["1", "2", "3", "4", "final"]
    d0 = os.path.join(str(tmp_path), "results", "e", names[0], "epoch_last")
    assert evaluate.find_format(d0, "npy") == ("npy", "ins") and evaluate.find_format(d0, "txt") == ("txt", "ins")
    os.remove(os.path.join(d0, "pseudo_labels.sgl"))
    assert evaluate.find_format(d0) == ("npy", "ins")
    for f in os.listdir(d0):
        if f.endswith(".npy"):
            os.remove(os.path.join(d0, f))
    assert evaluate.find_format(d0) == ("txt", "ins")
    # an explicit format the scenes lack: the error lists them
    with pytest.raises(SystemExit, match=r"npy labels .* 3 of 4 scenes: scene0000_00, scene0002_00, scene0003_00"):
        evaluate.discover(str(tmp_path), "e", "epoch_last", names, "npy", "final")
    assert evaluate.scene_names(str(tmp_path), lst) == names


def test_evaluate_lists_missing_scenes_and_refuses_absent_layers(sg_lib, tmp_path):
    from seggroup_amd import evaluate
    names, _ = _tree(tmp_path, ["sgl6", None, "npy6", None])
    with pytest.raises(SystemExit, match=r"2 of 4 scenes: scene0001_00, scene0003_00"):
        evaluate.discover(str(tmp_path), "e", "epoch_last", names, "auto", "2")
    names = [names[0], names[2]]
    found, layers = evaluate.discover(str(tmp_path), "e", "epoch_last", names, "auto", "all")
    assert layers == ["1", "2"] and [f[3] for f in found] == ["sem", "sem"]
    for layer in ("final", "3", "4"):
        with pytest.raises(SystemExit, match="sem_infer labels"):
            evaluate.discover(str(tmp_path), "e", "epoch_last", names, "auto", layer)
    assert evaluate.discover(str(tmp_path), "e", "epoch_last", names, "auto", "2")[1] == ["2"]
    names2, _ = _tree(tmp_path / "mix", ["sgl6", "sgl14"])
    with pytest.raises(SystemExit, match="mixes"):
        evaluate.discover(str(tmp_path / "mix"), "e", "epoch_last", names2, "auto", "1")


def test_evaluate_parser_defaults():
    from seggroup_amd import evaluate
    a = evaluate.build_parser().parse_args(["-n", "x"])
    assert (a.layer, a.stage, a.format, a.root, a.scenes, a.json) == ("final", "epoch_last", "auto", ".", None, None)
    for bad in (["-n", "x", "--layer", "5"], ["-n", "x", "--format", "ply"]):
        with pytest.raises(SystemExit):
            evaluate.build_parser().parse_args(bad)


def test_evaluate_accumulators_and_report_on_hand_made_counts():
    """accumulate() forms infer.py's float64 sums in scene order; report() prints infer.py's block under a per-layer heading."""
    from seggroup_amd import evaluate, infer
    rng = np.random.default_rng(3)
    per_scene = []
    for _ in range(3):
        m = np.zeros((2, 164), np.float32)
        m[:, :160] = rng.integers(0, 50, (2, 160)).astype(np.float32)
        m[:, 160:] = rng.random((2, 4)).astype(np.float32)
        per_scene.append(m)
    per_scene[1][0, 160] = np.nan                                 # an empty set's accuracy
    accs = evaluate.accumulate(per_scene, ["1", "2"])
    for k, l in enumerate(["1", "2"]):
        ref = infer.Accumulator()
        for m in per_scene:
            ref.add(m[k, :80], m[k, 80:160], m[k, 160:])
        assert np.array_equal(accs[l].v, ref.v, equal_nan=True)
    buf = io.StringIO()
    with redirect_stdout(buf):
        evaluate.report(accs, "e", "sem_infer")
    out = buf.getvalue().splitlines()
    assert out[0] == "Layer 1  (results/e/*/sem_infer, 3 scenes)"
    assert out[1].startswith("==> Infer           Instance mIoU: ")
    heads = [i for i, ln in enumerate(out) if ln.startswith("Layer ")]
    assert len(heads) == 2
    ref_buf = io.StringIO()
    with redirect_stdout(ref_buf):
        infer.final_report(accs["2"].summary(), evaluate._Print())
    assert "\n".join(out[heads[1] + 1:]) + "\n" == ref_buf.getvalue()
    js = evaluate.to_json(accs, "e", "sem_infer", {"sgl": 3}, 0.5)
    assert js["layers"]["2"]["n"] == 3 and len(js["layers"]["1"]["v"]) == 165


def test_infer_accepts_sgl_and_rejects_unknown_formats():
    from seggroup_amd import infer
    a = infer.build_parser().parse_args(["-n", "x", "--ins_infer", "--out-format", "sgl"])
    assert a.out_format == "sgl"
    with pytest.raises(SystemExit):
        infer.main(["-n", "x", "--ins_infer", "--out-format", "npy,ply"])


def test_write_label_files_and_async_writer_take_sgl(sg_lib, tmp_path):
    """The Python writers: 'sgl' alone or with txt / npy, from a result that carries its tables."""
    from seggroup_amd import hip, pseudo_labels
    from seggroup_amd.model import AsyncLabelWriter, SceneResult, write_label_files
    rng = np.random.default_rng(9)
    tab, sov = _case(rng, 14, 40, 300)
    res = SceneResult(None, 14, hip.Result(), tables=tab, seg_of_vertex=sov)
    written = write_label_files(str(tmp_path / "a"), res, ("sgl",))
    assert written == [str(tmp_path / "a" / "pseudo_labels.sgl")] and os.listdir(tmp_path / "a") == ["pseudo_labels.sgl"]
    w = AsyncLabelWriter(threads=2)
    w.submit(str(tmp_path / "b"), res, ("npy", "sgl"))
    w.close()
    assert len(os.listdir(tmp_path / "b")) == 15
    p = pseudo_labels.load(str(tmp_path / "b"))
    for i, n in enumerate(hip.LABEL_NAMES):
        assert np.array_equal(np.load(tmp_path / "b" / (n + ".npy")), p.vectors()[i])
    assert open(tmp_path / "a" / "pseudo_labels.sgl", "rb").read() == open(tmp_path / "b" / "pseudo_labels.sgl", "rb").read()
    no_tables = SceneResult(np.zeros((14, 3), np.int32), 14, hip.Result())
    with pytest.raises(ValueError):
        write_label_files(str(tmp_path / "c"), no_tables, ("sgl",))
