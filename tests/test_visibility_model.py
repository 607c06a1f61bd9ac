"""CPU-only: what the rule of the map cleaning (include/loamx.h, "map cleaning") does on a drive, by the numpy model of
tests/visibility_common.py alone: 16 scans of 16 x 256 cells of the lot scene with a box of 4.4 x 1.8 x 1.6 m that comes towards
the sensor by 1.5 m per scan, map points = the voxel centroids of all scans at leaf 0.4, default parameters. The bounds were set
before the model first ran on table cells: at most 0.5 % of the static voxels flagged, at least 90 % of the box's; the model gives
16 of 18 809 (0.09 %) and 281 of 295 (95.3 %). With the window closed to the point's own cell the ground at grazing angles is
seen `through`, which is why the default window is one line and one column each way."""
import functools

import numpy as np

import visibility_common as V


@functools.lru_cache(maxsize=None)
def drive():
    d = V.drive()
    d["tables"] = V.analytic_tables(d["H"], d["W"], V.S.FANS["lot"])
    return d


def flagged(params):
    d = drive()
    v, in_range, projected = V.votes(d["points"], d["scans"], d["poses"], d["H"], d["W"], *d["tables"], False, params)
    total = sum(int(v[name].astype(np.uint64).sum()) for name in V.FIELDS)
    assert total == projected <= in_range <= len(d["points"]) * len(d["scans"])
    dyn = V.dynamic(v, params)
    return int((dyn & d["is_static"]).sum()), int(d["is_static"].sum()), int((dyn & d["is_box"]).sum()), int(d["is_box"].sum())


def test_the_default_window_keeps_the_static_map_and_removes_the_moving_box():
    s_flagged, s_all, b_flagged, b_all = flagged(V.Params())
    print("static %d of %d flagged, box %d of %d" % (s_flagged, s_all, b_flagged, b_all))
    assert s_all > 15_000 and b_all > 200
    assert s_flagged <= 0.005 * s_all
    assert b_flagged >= 0.9 * b_all


def test_a_window_of_the_own_cell_alone_flags_the_ground_at_grazing_angles():
    s_flagged, s_all, b_flagged, b_all = flagged(V.Params(window_lines=0, window_cols=0))
    print("static %d of %d flagged, box %d of %d" % (s_flagged, s_all, b_flagged, b_all))
    assert s_flagged > 0.1 * s_all
