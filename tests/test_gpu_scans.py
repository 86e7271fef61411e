"""scans.map_scans on the GPU: the runner under every batch command.  No kernel is launched: the function handed in
returns the address of the stream it was given.  Five scenes on three workers is the smallest shape that has both a thread that takes
a second scene and, with `workers=99`, threads that must not exist."""
import pytest

pytestmark = pytest.mark.gpu

SCENES = ["scene%04d_00" % i for i in (7, 3, 11, 1, 5)]                 # not sorted: the order that comes back is the order given


def _run(workers, scenes=SCENES):
    import threading

    import torch
    from seggroup_amd import scans
    from seggroup_amd.device import torch_device
    threads = set()

    def fn(scene, stream):
        threads.add(threading.get_ident())
        return stream.cuda_stream

    done = scans.map_scans(scenes, workers, torch_device("cuda:0"), fn)
    return done, threads, torch.cuda.default_stream(torch.device("cuda:0")).cuda_stream


def test_results_in_order_on_a_stream_per_worker():
    done, threads, default = _run(3)
    assert [scene for scene, _ in done] == SCENES
    ptrs = [p for _, p in done]
    assert 1 <= len(set(ptrs)) <= 3 and len(threads) <= 3
    assert len(set(ptrs)) == len(threads), "one stream per worker thread, kept for every scene the thread takes"
    assert all(p not in (0, None, default) for p in ptrs), "a worker never runs on the default stream"


def test_more_workers_than_scenes_are_not_made():
    from seggroup_amd import scans
    assert scans.worker_count(99, len(SCENES)) == 5
    done, threads, default = _run(99)
    assert [scene for scene, _ in done] == SCENES
    assert len(threads) <= 5 and len({p for _, p in done}) == len(threads)
    assert all(p not in (0, None, default) for _, p in done)


def test_no_scene_is_no_work():
    assert _run(4, [])[0] == []
