"""The stage timers of the cloud tools without a GPU: every family exports sg_*_set_timing, sg_*_stage_times and sg_*_stage_name over one
piece of plumbing (overseg_device.h's StageTimes), and each keeps the same contract -- the refusals name the family's own function, the
names are the ones the tools and profiles print, in order, and nothing outside 0 .. stages - 1 has a name.  No device call is made."""
import ctypes as C

import pytest

from seggroup_amd import hip

LIST_STAGES = ("box", "cells", "sort", "table", "count", "scan", "fill", "rows")
FAMILIES = {
    "overseg": ("check", "face_normals", "incidence_sort", "vertex_normals", "edges", "weights", "weight_sort", "gather"),
    "pcseg": ("check", "knn", "normals", "edges", "weights", "weight_sort", "gather"),
    "pcseg_radius": LIST_STAGES + ("normals", "edges", "weights", "weight_sort", "gather"),
    "cloud_thin": ("check_box", "keys", "sort", "representatives", "compact", "map"),
    "pointcloud_knn_grid": ("box", "probe", "cells", "sort", "table", "search", "fallback"),
    "nearest_point_grid": ("box", "probe", "cells", "sort", "table", "search", "fallback"),
    "cloud_knn_cross_grid": ("box", "probe", "cells", "sort", "table", "search", "fallback"),
    "components": ("init", "hook", "flatten", "sizes"),
    "radius_grid": ("box", "cells", "sort", "table", "init", "search", "finish"),
    "segment_vote": ("check", "rank_sort", "rank_unique", "pair_sort", "pair_unique", "arg_max", "vertex_gather"),
    "segment_graph": ("keys", "sort", "unique", "emit"),
    "ransac": ("gather", "filter", "count"),
    "plane": ("compact", "generate", "count", "moments", "assign"),
    "label": ("index", "moments", "yaw", "frame"),
}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_one_contract_for_every_family(sg_lib, family):
    names = FAMILIES[family]
    n = len(names)
    times = getattr(sg_lib, f"sg_{family}_stage_times")
    name = getattr(sg_lib, f"sg_{family}_stage_name")
    who = f"sg_{family}_stage_times".encode()
    buf = (C.c_float * (n + 1))()
    assert times(None, n) == hip.SG_EINVAL
    assert who in sg_lib.sg_last_error()
    assert times(buf, n - 1) == hip.SG_EINVAL
    err = sg_lib.sg_last_error()
    assert who in err and f"room for {n} floats is needed".encode() in err
    assert times(buf, n) == n and times(buf, n + 1) == n
    assert name(-1) is None and name(n) is None
    assert tuple(name(i) for i in range(n)) == tuple(s.encode() for s in names)
    assert getattr(sg_lib, f"sg_{family}_set_timing")(0) == hip.SG_OK


class _Recorded:
    """the library, with every sg_*_set_timing call written down"""

    def __init__(self, lib):
        self._lib, self.switched = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.endswith("_set_timing"):
            return fn
        return lambda on: (self.switched.append((name, on)), fn(on))[1]


def test_the_reader_covers_every_family():
    """the library's set is read off hip.SIGNATURES (the timers a thread switches with one int), so a family without an entry here fails"""
    exported = sorted(n[len("sg_"):-len("_set_timing")] for n, (_, args) in hip.SIGNATURES.items()
                      if n.endswith("_set_timing") and args == [C.c_int])
    assert exported == sorted(FAMILIES)
    assert sorted(hip.STAGE_FAMILIES) == exported
    for family in exported:
        assert all(f"sg_{family}_{f}" in hip.SIGNATURES for f in ("stage_times", "stage_name"))


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_reader_names_values_and_switch(sg_lib, family, monkeypatch):
    rec = _Recorded(sg_lib)
    monkeypatch.setattr(hip, "lib", lambda: rec)
    switch = f"sg_{family}_set_timing"
    with hip.stage_timer(family) as t:
        assert rec.switched == [(switch, 1)]
        assert tuple(t.names) == FAMILIES[family]
        us = t.read()
        assert len(us) == len(FAMILIES[family]) and all(isinstance(u, float) for u in us)
    assert rec.switched == [(switch, 1), (switch, 0)]
    with pytest.raises(KeyError, match="inside the block"):
        with hip.stage_timer(family):
            raise KeyError("inside the block")
    assert rec.switched == [(switch, 1), (switch, 0)] * 2            # off again after the exception, which is passed on
