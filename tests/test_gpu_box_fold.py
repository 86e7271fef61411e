"""The bounding-box reduction that sg_cloud_thin (k_thin_box) and the grid index (k_grid_box) share (overseg_device.h), at the one shape
that is all its own: N = kBoxBlocks * kBlock + 1 points, so the grid-stride loop's second trip has exactly one live thread -- and that
thread holds the extremes of all three axes.  A box that drops it moves `lo`, and with it every cell of both tools."""
import numpy as np
import pytest

import radius_ref as R
import thin_ref as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIDE = 64                                   # 64^3 = 1024 blocks * 256 threads
STEP = 1.0 / SIDE
JITTER = 0.05                               # of a step, per axis and sign
# axis neighbours lie within sqrt(1.1^2 + 2 * 0.1^2) = 1.109 steps, every other pair beyond sqrt(2) * 0.9 = 1.272 steps: the radius
# stands in the gap, far from every pair
RADIUS = 1.19 * STEP
FAR = (-3.0, -2.5, 4.0)
VOXEL = 0.05


def _cloud():
    rng = np.random.RandomState(262145)
    g = (np.stack(np.meshgrid(*[np.arange(SIDE)] * 3, indexing="ij"), -1).reshape(-1, 3) + 0.5) * STEP
    g = g + (rng.rand(*g.shape) - 0.5) * (2 * JITTER * STEP)
    xyz = np.concatenate([g[rng.permutation(g.shape[0])], np.array([FAR])]).astype(np.float32)
    assert xyz.shape[0] == 1024 * 256 + 1
    return xyz


def test_the_last_point_alone_in_the_second_trip_holds_the_extremes():
    from seggroup_amd import components, thin
    xyz = _cloud()
    n = xyz.shape[0]
    # sg_cloud_thin: the box itself, then everything that is derived from it
    rep, top, lo = (t.cpu().numpy() for t in thin.thin_cloud(xyz, VOXEL, device=DEV))
    assert lo.tobytes() == xyz.min(0).tobytes() and lo[0] == FAR[0] and lo[1] == FAR[1]
    want_rep, want_top, want_lo = T.thin(xyz, VOXEL)
    assert lo.tobytes() == want_lo.tobytes()
    assert np.array_equal(rep, want_rep) and np.array_equal(top, want_top)
    # sg_radius_count_grid: a host count in float64 on the fp32 values; no pair is near enough to the radius for the two to differ
    want_cnt, _, _, nearest = R.kdtree(xyz, RADIUS)
    assert nearest > 1e-6, "a pair lies on the radius: the float64 count does not decide the fp32 predicate"
    cnt = components.neighbour_counts(xyz, RADIUS, device=DEV).cpu().numpy()
    assert cnt.dtype == np.int32 and cnt.shape == (n,)
    assert cnt[n - 1] == 0 and want_cnt[n - 1] == 0
    assert 3 <= want_cnt[:n - 1].min() and want_cnt.max() == 6, "the lattice's axis neighbours, and nothing else"
    assert np.array_equal(cnt, want_cnt)
