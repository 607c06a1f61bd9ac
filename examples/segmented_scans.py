#!/usr/bin/env python3
"""What a scan shows before its features are taken: ground, clusters, outliers, and the scan without the outliers.

    python -m loam_amd.build            # once: libloamx.so
    python examples/segmented_scans.py [canyon|lot]

LeGO-LOAM and LIO-SAM run a range-image segmentation in front of the feature extraction: the ground is labelled, the other
returns are clustered by connected components under an angle criterion, and the components too small to be a surface (leaves,
wires, rain, the edges of moving objects) are thrown away. `Context.segment_scan` does that on the device and returns the class
of every cell, the components, and a filtered scan in which the dropped cells read (0, 0, 0) — a beam without a return for
`extract_features`.

The scan is a canyon or a parking lot of tests/outdoor_scenes.py. The last lines say how many of the features the extraction
takes from the raw scan sat on cells the filter removes, and what it takes from the filtered scan instead. They promise no
accuracy gain: whether a registration is better off without those features depends on the scene."""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for p in (os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)
import outdoor_scenes  # noqa: E402  (only for the stand-in scan)
from loam_amd import capi  # noqa: E402


def main(scene="canyon", scan_lines=64, points_per_line=1024, verbose=True, ctx=None):
    ctx = ctx or capi.Context(0)
    lidar = capi.LidarParams(scan_lines, points_per_line, 1.0, 120.0)
    origin, yaw = outdoor_scenes.sensor_origin(scene, 0)
    scan = outdoor_scenes.scan_at(scene, 0, origin, yaw, H=scan_lines, W=points_per_line)

    params = capi.SegmentParams()  # 10 degrees of ground slope, 60 degrees, 30 cells or 5 cells over 3 lines; outliers dropped
    classes, labels, sizes, filtered, clusters, stats = ctx.segment_scan(scan, lidar, params)
    removed = classes == capi.SEGMENT_OUTLIER  # the returns the filter takes out (out-of-range returns were never features)
    assert not filtered[removed].any() and np.array_equal(filtered[classes == capi.SEGMENT_CLUSTER], scan[classes == capi.SEGMENT_CLUSTER])

    edge_raw, planar_raw = ctx.extract_features(scan, lidar)
    edge_f, planar_f = ctx.extract_features(filtered, lidar)
    counts = dict(invalid=int(stats[0]), ground=int(stats[1]), cluster_cells=int(stats[2]), outlier_cells=int(stats[3]),
                  accepted=int(stats[4]), rejected=int(stats[5]), largest=int(stats[6]), removed=int(removed.sum()),
                  edge_raw=len(edge_raw), planar_raw=len(planar_raw), edge_on_removed=int(removed[edge_raw].sum()),
                  planar_on_removed=int(removed[planar_raw].sum()), edge_filtered=len(edge_f), planar_filtered=len(planar_f))
    if verbose:
        n = len(classes)
        print("%s, %d x %d cells: %.1f %% no return, %.1f %% ground, %.1f %% in %d accepted components (largest %d cells), "
              "%.1f %% in %d rejected ones" % (scene, scan_lines, points_per_line, 100.0 * stats[0] / n, 100.0 * stats[1] / n,
                                              100.0 * stats[2] / n, stats[4], stats[6], 100.0 * stats[3] / n, stats[5]))
        big = clusters[np.argsort(-clusters["size"].astype(np.int64), kind="stable")[:3]]
        print("largest components: " + ", ".join("root %d, %d cells, lines %d-%d" % tuple(int(v) for v in c) for c in big))
        print("the filter removes %d returns of rejected components" % counts["removed"])
        print("raw scan:      %5d edge / %5d planar features, of which %d / %d on removed cells"
              % (counts["edge_raw"], counts["planar_raw"], counts["edge_on_removed"], counts["planar_on_removed"]))
        print("filtered scan: %5d edge / %5d planar features" % (counts["edge_filtered"], counts["planar_filtered"]))
    return counts


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "canyon")
