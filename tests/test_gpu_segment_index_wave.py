"""The segment index (sg_segment_sort_boxes: segment boxes, Morton order, chunk boxes, coordinate sums) on one wave per segment.

Segments of at most `wave_max` points (sg_segment_sort_set_wave_max: 0 | 64 | 128 | 256) are sorted in registers by
k_segment_sort_boxes_wave, the others by the block kernel in LDS.  Every setting must write the same bytes, and those must be the
NumPy statement of the order (`_morton_sort_oracle` of test_gpu_ops.py); the coordinate sums are compared with a float64 sum taken
in the kernels' own tree (a thread's points in index order, the DPP network over a wave's 64 lanes, the four waves in order)."""
import os

import numpy as np
import pytest

from test_gpu_ops import _morton_sort_oracle

pytestmark = pytest.mark.gpu

SETTINGS = (0, 256, 64, 128)


def _wave_tree(a):
    """sgw::wave_sum over 64 doubles: quads, rows of four quads, row 1 + row 0 and row 3 + row 2, then the two halves (csrc/wave_ops.h)"""
    q = (a[0::4] + a[1::4]) + (a[2::4] + a[3::4])
    r = (q[3::4] + q[2::4]) + (q[1::4] + q[0::4])
    return (r[3] + r[2]) + (r[1] + r[0])


def _sums_oracle(data, seg_points, seg_off):
    S = len(seg_off) - 1
    out = np.zeros((S, 3), np.float64)
    for s in range(S):
        lo, hi = int(seg_off[s]), int(seg_off[s + 1])
        assert hi - lo <= 2048
        xyz = data[seg_points[lo:hi], :3].astype(np.float64)
        for k in range(3):
            t = np.zeros(256, np.float64)
            for i0 in range(0, hi - lo, 256):                      # thread tid holds points tid, tid + 256, ...
                part = xyz[i0:i0 + 256, k]
                t[:len(part)] = t[:len(part)] + part
            d = [_wave_tree(t[64 * w:64 * w + 64]) for w in range(4)]
            out[s, k] = ((d[0] + d[1]) + d[2]) + d[3]
    return out


def _cloud(sizes, rng, fill=None):
    """[N,6] rows and a CSR whose segments have the given sizes; the rows of a segment are scattered over the cloud"""
    seg_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    N = int(seg_off[-1])
    data = rng.uniform(-2.0, 2.0, size=(N, 6)).astype(np.float32)
    seg_points = rng.permutation(N).astype(np.int32)
    if fill:
        for s, f in fill.items():
            rows = seg_points[seg_off[s]:seg_off[s + 1]]
            data[rows, :3] = f(data[rows, :3], len(rows))
    return data, seg_points, seg_off


def _run(torch, hip, lib, data, seg_points, seg_off, wave_max):
    S, N = len(seg_off) - 1, len(seg_points)
    n = np.diff(seg_off)
    chunk_off = np.concatenate([[0], np.cumsum((n + 31) // 32)]).astype(np.int32)
    seg_of_point = np.zeros(N, np.int32)
    seg_of_point[seg_points] = np.repeat(np.arange(S, dtype=np.int32), n)
    dev = [torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0") for x in (data, seg_points, seg_off, seg_of_point, chunk_off)]
    nchunk = int(chunk_off[-1])
    box = torch.full((S, 8), 7.0, device="cuda:0")
    sperm = torch.full((N,), -1, dtype=torch.int32, device="cuda:0")
    cbox = torch.full((nchunk + 1, 8), 5.0, device="cuda:0")
    sums = torch.full((S, 3), 3.0, dtype=torch.float64, device="cuda:0")
    ws = torch.zeros(max(int(lib.sg_segment_sort_ws_bytes(N)), 256), dtype=torch.uint8, device="cuda:0")
    hip.check(lib.sg_segment_sort_set_wave_max(wave_max))
    assert lib.sg_segment_sort_get_wave_max() == wave_max
    hip.check(lib.sg_segment_sort_boxes(dev[0].data_ptr(), N, dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), S, dev[4].data_ptr(),
                                        int(n.max()), box.data_ptr(), sperm.data_ptr(), cbox.data_ptr(), sums.data_ptr(), ws.data_ptr(),
                                        ws.numel(), None))
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in (box, sperm, cbox, sums))


def _check(data, seg_points, seg_off, exact_bits):
    """every setting against the block kernel alone, byte for byte; then against the NumPy statement"""
    import torch
    from seggroup_amd import hip
    hip.require_device()
    lib = hip.lib()
    names = ("segbox", "sperm", "chunk_box", "seg_sums")
    try:
        got = {wm: _run(torch, hip, lib, data, seg_points, seg_off, wm) for wm in SETTINGS}
    finally:
        hip.check(lib.sg_segment_sort_set_wave_max(256))
    n = np.diff(seg_off)
    for wm in SETTINGS[1:]:
        for name, a, b in zip(names, got[0], got[wm]):
            bad = np.nonzero(np.any((a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)), axis=1))[0]
            assert bad.size == 0, f"wave_max {wm}: {name} differs from the block kernel's in {bad.size} rows, first {bad[0]} (segment sizes {n.tolist()})"
    box, sperm, cbox, sums = got[256]
    obox, osperm, ocbox = _morton_sort_oracle(data, seg_points, seg_off)
    nz = n > 0
    same = (lambda a, b: a.tobytes() == b.tobytes()) if exact_bits else np.array_equal      # a box of -0.0 and +0.0: equal values, the oracle's zero has no defined sign
    assert same(box[nz], obox[nz]), np.nonzero(np.any(box != obox, axis=1) & nz)[0]
    assert np.array_equal(sperm, osperm), np.nonzero(sperm != osperm)[0][:8]
    assert same(cbox[:len(ocbox)], ocbox)
    assert np.all(cbox[len(ocbox)] == 5.0)                          # nothing behind the last chunk
    want = _sums_oracle(data, seg_points, seg_off)
    assert sums.tobytes() == want.tobytes() if exact_bits else np.array_equal(sums, want), np.abs(sums - want).max()
    return got


def test_every_size_class_and_boundary_equals_block_kernel_and_oracle():
    """Segments of 1 .. 300 points around every boundary of the one-wave kernel's three classes (64, 128, 256) and of a 32-point chunk, 19
    segments (not a multiple of a block's four), their rows scattered over a cloud of ~3,000 points."""
    rng = np.random.default_rng(20240)
    sizes = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 97, 450, 200, 511]
    assert len(sizes) % 4 != 0
    data, seg_points, seg_off = _cloud(sizes, rng)
    _check(data, seg_points, seg_off, exact_bits=True)


def test_edge_inputs_equal_block_kernel_and_oracle():
    """All points identical (every key ties: the order is the index order), a flat segment, coordinates shifted to 1e3, both zeros in one coordinate,
    an empty segment (the block kernel writes its box as +inf / -inf / 0 and its sums as 0: kept)."""
    rng = np.random.default_rng(20241)

    def identical(x, m):
        return np.tile(np.float32([0.25, -1.5, 0.75]), (m, 1))

    def flat(x, m):
        x[:, 2] = np.float32(0.5)
        return x

    def shifted(x, m):
        return (x * np.float32(0.05) + np.float32(1e3)).astype(np.float32)

    def zeros(x, m):
        x[:, 1] = np.where(np.arange(m) % 2 == 0, np.float32(0.0), np.float32(-0.0))
        return x

    sizes = [40, 100, 150, 70, 0, 130, 90]
    data, seg_points, seg_off = _cloud(sizes, rng, fill={0: identical, 1: flat, 2: shifted, 3: zeros, 5: identical, 6: zeros})
    assert np.signbit(data[seg_points[seg_off[3]:seg_off[4]], 1]).any() and not np.signbit(data[seg_points[seg_off[3]:seg_off[4]], 1]).all()
    got = _check(data, seg_points, seg_off, exact_bits=False)
    box, sperm, cbox, sums = got[256]
    assert np.array_equal(sperm[:40], np.arange(40))                # all keys tie: index order
    assert np.array_equal(box[4], np.float32([np.inf, np.inf, np.inf, -np.inf, -np.inf, -np.inf, 0, 0])) and np.all(sums[4] == 0)


def test_setter_refuses_other_sizes():
    from seggroup_amd import hip
    hip.require_device()
    lib = hip.lib()
    assert lib.sg_segment_sort_get_wave_max() == 256
    for bad in (-1, 1, 32, 96, 512):
        assert lib.sg_segment_sort_set_wave_max(bad) == hip.SG_EINVAL and lib.sg_last_error().decode().startswith("sg_segment_sort_set_wave_max:")
    assert lib.sg_segment_sort_get_wave_max() == 256


def test_engine_labels_equal_with_and_without_the_wave_kernel():
    """The small scenes of test_small_scenes_engine_equals_pipeline_in_every_group_shape (3,000 points / 30 segments, and 150 small segments) through
    one engine shape with every segment in the block kernel and with the one-wave kernel: the same label digests, and the single pipeline's."""
    import torch
    import bench
    from conftest import ROOT
    from seggroup_amd import hip, synthetic, weights
    from seggroup_amd.model import Engine, Pipeline
    from seggroup_amd.scene import DeviceScene
    hip.require_device()
    lib = hip.lib()
    W = weights.load_npz(os.path.join(ROOT, "tests", "golden", "weights_g2.npz"))
    mode = hip.MODE_INS_INFER
    n = 16
    scenes = [DeviceScene.from_synthetic(synthetic.make_scene(3000, 30, 40000 + i) if i % 2 == 0 else synthetic.make_scene(3000, 150, 41000 + i, min_seg=1),
                                         device="cuda:0") for i in range(n)]
    caps = (max(s.N for s in scenes), max(s.S for s in scenes), max(s.E0 for s in scenes), max(s.V for s in scenes))
    got = {}
    try:
        for wm in (0, 256):
            hip.check(lib.sg_segment_sort_set_wave_max(wm))
            eng = Engine(W, caps, groups=2, per_group=4, device="cuda:0", timing=0)
            got[wm] = [bench.label_digest(r) for r in eng.run(scenes, mode)]
            eng.close()
            solo = Pipeline(W, *caps, device="cuda:0")
            got["solo", wm] = [bench.label_digest(solo.forward(s, mode)) for s in scenes]
            solo.close()
    finally:
        hip.check(lib.sg_segment_sort_set_wave_max(256))
    torch.cuda.synchronize()
    assert got[0] == got[256]
    assert got["solo", 0] == got[0] and got["solo", 256] == got[256]
