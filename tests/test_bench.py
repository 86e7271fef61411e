"""bench.py's plain run and `--dump-outputs`: a plain run times the steps and prints the headline only, and what it dumps is what the
timed path returned for its last step -- the same from run to run, and the same as the single pipeline gives for those scenes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, GOLDEN


class _FakeResult:
    def __init__(self, rng, n_vertices):
        self.n_vectors = 14
        self.labels = rng.integers(-1, 1500, (14, n_vertices)).astype(np.int32)
        self.iou_sem = rng.integers(0, 50, (1, 2, 40)).astype(np.float32)
        self.iou_ins = rng.integers(0, 50, (1, 2, 40)).astype(np.float32)
        self.acc = np.array([np.nan, 0.5, 0.25, 1.0], np.float32)
        self.trace = [40, 34, 9, 5, 2]


@pytest.mark.parametrize("batch,n_vertices", [(64, 150000), (128, 150000), (4, 3000)])
def test_dump_outputs_samples_every_vector_at_the_same_seeded_vertices(tmp_path, batch, n_vertices):
    import bench
    rng = np.random.default_rng(7)
    results = [_FakeResult(rng, n_vertices - 13 * b) for b in range(batch)]
    shapes = bench.dump_outputs(str(tmp_path / "a"), results)
    bench.dump_outputs(str(tmp_path / "b"), results)
    total = 0
    for name, shape in shapes.items():
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype in (np.float32, np.float64) and list(a.shape) == shape and a.shape[0] == batch, name
        assert np.array_equal(a, b, equal_nan=True), name                       # the sample is fixed, not drawn per run
        total += os.path.getsize(tmp_path / "a" / f"{name}.npy")
    assert total <= 64 << 20
    sample, index, sums = (np.load(tmp_path / "a" / f"{n}.npy") for n in ("labels_sample", "labels_sample_index", "labels_sum"))
    assert sample.shape[2] == min(bench.DUMP_POINTS, bench.DUMP_BYTES // (batch * (4 * 14 + 8)), n_vertices - 13 * (batch - 1))
    for b, r in enumerate(results):
        idx = index[b].astype(np.int64)
        assert np.all(np.diff(idx) > 0) and idx[-1] < r.labels.shape[1]
        assert np.array_equal(sample[b], r.labels[:, idx].astype(np.float32))
        assert np.array_equal(sums[b], r.labels.sum(axis=1, dtype=np.int64).astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "a" / "iou_sem.npy"), np.stack([r.iou_sem[0] for r in results]))
    assert np.array_equal(np.load(tmp_path / "a" / "trace.npy"), np.array([r.trace for r in results], np.float32))


def test_full_is_off_by_default():
    import bench
    assert not bench.parse_args([]).full and bench.parse_args(["--full"]).full
    assert bench.parse_args(["--dump-outputs", "d"]).dump_outputs == "d"


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step_and_nothing_else_runs(tmp_path):
    from seggroup_amd import hip, synthetic, weights
    from seggroup_amd.model import Pipeline
    from seggroup_amd.scene import DeviceScene
    small = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--points", "3000", "--segments", "30", "--batch", "8", "--groups", "2", "--per-group", "4"]
    lines = []
    for run in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + small + ["--dump-outputs", str(tmp_path / run)],
                           capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append(json.loads([l_ for l_ in r.stdout.splitlines() if l_.startswith("{")][-1]))
    for j in lines:
        assert j["full"] is False and j["steps"] == 3 and j["ms_per_step"] > 0 and j["pseudo_label_mIoU"]["scenes"] == 3 * 8
        assert abs(j["ms_per_step"] * 3 - j["timed_region_s"] * 1e3) <= 0.6                  # both rounded to 3 decimals
        for k in ("repeat_values", "roofline", "cpu_baseline", "parity_check", "with_label_files_scenes_per_s", "extra", "comm"):
            assert k not in j, k
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and "labels_sample.npy" in names
    got = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    for n in names:
        assert np.array_equal(got[n[:-4]], np.load(tmp_path / "b" / n), equal_nan=True), n
    # the dump is what one default-stream pipeline gives for the scenes of the last timed batch (seeds 30000 + i)
    W = weights.load_npz(os.path.join(GOLDEN, "weights_g2.npz"))
    scenes = [DeviceScene.from_synthetic(synthetic.make_scene(3000, 30, 30000 + i), device="cuda:0") for i in range(8)]
    solo = Pipeline(W, max(s.N for s in scenes), max(s.S for s in scenes), max(s.E0 for s in scenes), max(s.V for s in scenes),
                    stream=None, device="cuda:0")
    try:
        for b, sc in enumerate(scenes):
            res = solo.forward(sc, hip.MODE_INS_INFER)
            lab = np.asarray(res.labels[:res.n_vectors])
            idx = got["labels_sample_index"][b].astype(np.int64)
            assert np.array_equal(got["labels_sample"][b], lab[:, idx].astype(np.float32)), b
            assert np.array_equal(got["labels_sum"][b], lab.sum(axis=1, dtype=np.int64).astype(np.float64)), b
            assert np.array_equal(got["iou_sem"][b], res.iou_sem[0]) and np.array_equal(got["iou_ins"][b], res.iou_ins[0]), b
            assert np.array_equal(got["acc"][b], res.acc, equal_nan=True) and list(got["trace"][b]) == list(res.trace), b
    finally:
        solo.close()
