"""The deterministic sums, to the byte, across a change of the code (csrc/moments_device.h).

The other gates hold the sums to a bound against np.sum and to equality between two calls of one build; a silent change of the summation
order passes both.  tests/golden/moment_bytes.npz holds what the build BEFORE csrc/moments_device.h returned on an MI355X for the inputs
below (tools/capture_moment_bytes.py wrote it from that build; only outputs are stored, the inputs come from fixed seeds): the float64
outputs of align.moments, align.plane_moments and planes.plane_moments at every item count where a part of the two trees changes -- a
wave, a workgroup's 256 threads, a partial row of 1,024 items, more than 256 partial rows (the fold's strided pass runs twice) --,
boxes.label_moments over labels of 1, 1,024, 1,025 and 3 * 1,024 + 5 points, and, for the hypothesis draw of csrc/ransac_draw_device.h, the
count vectors of planes.plane_ransac and register.ransac_count."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "moment_bytes.npz")
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4 * 1024 + 7, 256 * 1024 + 1]
LABEL_SIZES = [1, 1024, 1025, 3 * 1024 + 5]
CANDIDATES = 500
POSE = np.array([[0.96, -0.28, 0.0, 0.125], [0.28, 0.96, 0.0, -0.25], [0.0, 0.0, 1.0, 0.0625]])   # a rotation about z and a shift
ORIGIN_X, ORIGIN_Y = np.array([1.0, 0.5, 0.25]), np.array([0.75, 1.25, 0.5])
PLANE, PLANE_DIST = np.array([0.0, 0.6, 0.8, -1.0]), 0.3

_golden = {}


def golden(key):
    if not _golden:
        with np.load(GOLDEN) as f:
            _golden.update({k: f[k] for k in f.files})
    return _golden[key]


def _rows(xyz, stride):
    return xyz if stride == 3 else np.ascontiguousarray(np.concatenate([xyz, np.full((xyz.shape[0], stride - 3), 7.0, np.float32)], 1))


def sums(u):
    """the three kernels of one launch shape on `u` items -> {key: float64 vector}.  Rows of 3 floats at an even count and of 6 at an odd
    one; every 7th d2 is a NaN, about half of the rest lie inside the radius; every 11th normal is too short to use; a label mask takes every
    third point out of the plane sums; the origins are not 0."""
    from seggroup_amd import align, planes
    rng = np.random.RandomState(4000 + u)
    stride = 6 if u % 2 else 3
    x = _rows((rng.rand(u, 3) * 2.0).astype(np.float32), stride)
    y = _rows((rng.rand(CANDIDATES, 3) * 2.0).astype(np.float32), 9 - stride)
    nrm = rng.randn(CANDIDATES, 3)
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    nrm[::11] *= np.float32(0.25)
    idx = rng.randint(0, CANDIDATES, u).astype(np.int64)
    d2 = (rng.rand(u) * 0.02).astype(np.float32)
    d2[3::7] = np.nan
    labels = np.where(np.arange(u) % 3 == 1, 5, -1).astype(np.int32)
    return {"align_%d" % u: align.moments(x, y, idx, d2, 0.1, ORIGIN_X, ORIGIN_Y, device=DEV),
            "align_plane_%d" % u: align.plane_moments(x, POSE, y, nrm, idx, d2, 0.1, ORIGIN_Y, device=DEV),
            "plane_%d" % u: planes.plane_moments(x, PLANE, PLANE_DIST, ORIGIN_X, labels=labels, device=DEV)}


def label_sums():
    """boxes.label_moments over four labels side by side, their points scattered among one another and among ignored ones"""
    from seggroup_amd import boxes
    rng = np.random.RandomState(77)
    lab = np.concatenate([np.full(n, 3 * l + 2, np.int32) for l, n in enumerate(LABEL_SIZES)] + [np.full(333, -1, np.int32)])
    lab = lab[rng.permutation(lab.size)]
    xyz = _rows((rng.rand(lab.size, 3) * 4.0 - 1.0).astype(np.float32), 6)
    m = boxes.label_moments(xyz, boxes.label_index(lab, device=DEV), device=DEV)
    return {"label_m": m.moments.cpu().numpy(), "label_lo": m.lo.cpu().numpy(), "label_hi": m.hi.cpu().numpy()}


def draws():
    """the count vectors of 1,000 generated hypotheses: 300 free points, half of them near a plane; 250 correspondences, a fifth of them wrong"""
    from seggroup_amd import planes, register
    rng = np.random.RandomState(99)
    p = rng.rand(300, 3) * 2.0
    on = rng.rand(300) < 0.5
    p[on, 2] = 0.5 * p[on, 0] + 0.25 + rng.randn(int(on.sum())) * 0.002
    count = planes.plane_ransac(p.astype(np.float32), 0.02, 1000, seed=12345, min_edge=0.2, device=DEV)[0]
    moving = (rng.rand(250, 3) * 2.0).astype(np.float32)
    fixed = (moving.astype(np.float64) @ POSE[:, :3].T + POSE[:, 3] + rng.randn(250, 3) * 0.002).astype(np.float32)
    ci, cj = np.arange(250, dtype=np.int32), np.arange(250, dtype=np.int32)
    cj[::5] = rng.randint(0, 250, cj[::5].size)
    votes = register.ransac_count(moving, fixed, ci, cj, 1000, 0.05, seed=54321, device=DEV)
    return {"draw_planes": count.cpu().numpy(), "draw_register": votes.cpu().numpy()}


@pytest.mark.parametrize("u", COUNTS)
def test_the_sums_of_one_launch_shape(u):
    got = sums(u)
    for key, m in got.items():
        want = golden(key)
        assert m.dtype == np.float64 and m.shape == want.shape, key
        assert m.tobytes() == want.tobytes(), (key, m, want)
    if u:
        assert got["align_%d" % u][0] > 0 or u < 4, "no pair inside the radius: the case checks nothing"


def test_the_label_sums():
    for key, m in label_sums().items():
        want = golden(key)
        assert m.dtype == want.dtype and m.shape == want.shape, key
        assert m.tobytes() == want.tobytes(), (key, m, want)


def test_the_hypothesis_draw():
    for key, count in draws().items():
        want = golden(key)
        assert count.dtype == np.int32 and (count >= 0).sum() > 100, (key, "too few hypotheses were kept: the case checks little")
        assert np.array_equal(count, want), key
