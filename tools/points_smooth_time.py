#!/usr/bin/env python3
"""What one iteration of the smoothed positions costs against the estimated normals at the same radius on the same cloud:
Points.smoothed_positions(radius, 2) against Points.estimate_normals(radius, 2) -- the same sort into cells, the same walk, the
same solve; the smoothing adds a binary64 division and four multiplications per neighbour and the projection -- and
Points.with_smoothed_positions(radius, 2, 3), three iterations and the copy of the other arrays, on device-resident clouds
(DESIGN.md section 4).  Not part of bench.py; needs a GPU.  Asserts nothing.

  tools/points_smooth_time.py      call times: per cloud 1 warm-up round, then 7 rounds that alternate the calls; the median and
                                   the minimum of the host clock around each call (a call ends in a device synchronise inside
                                   the library) and the ratio of the medians to estimate_normals'

Clouds: those of tools/points_normals_time.py but the 4 * 10^6 points: large_case of the tests (2 * 10^5 points, four to a cell),
the largest real cloud of the tests (mixed_sizes fused by the tat_advanced loop on the device, at the radius the tests choose for
it) and the tilted plane of the tests at 10^6 points, twelve to a unit of area."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def clouds(pkg):
    import numpy as np
    import fusion_cases
    import points_radius_checker as PR
    import tempfile
    from oracle import binding as ob
    from test_gpu_points_average import fused
    from test_points_normals import plane_case
    from test_points_radius import dressed, large_case, real_cloud_radius
    from test_points_voxel import arrays_of, from_cloud, views_of
    c, views = dressed(np.random.default_rng(9), large_case(np.random.default_rng(10)))
    yield "large_case, %d points" % c.count, from_cloud(pkg, c, *views, on_device=True), 1.0
    ob.lib()
    real = fused(pkg, ob, fusion_cases.case("mixed_sizes"), "tat_advanced", True)
    radius = real_cloud_radius(PR.build(tempfile.mkdtemp()), arrays_of(real))
    yield "mixed_sizes tat_advanced, %d points" % real.count, real, radius
    c, _ = plane_case(np.random.default_rng(33), side=289.0)
    yield "plane at 12 per unit of area, %d points" % c.count, from_cloud(pkg, c, *views_of(1), on_device=True), 1.0


def calls(pts, radius):
    yield "estimate_normals(min=2)", lambda: pts.estimate_normals(radius, 2)
    yield "smoothed_positions(min=2)", lambda: pts.smoothed_positions(radius, 2)
    yield "with_smoothed_positions(min=2, 3)", lambda: pts.with_smoothed_positions(radius, 2, 3)[0].close()


def measure():
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    assert pkg.device_count() >= 1, "no HIP device visible"
    for name, pts, radius in clouds(pkg):
        todo = list(calls(pts, radius))
        for what, f in todo:   # warm-up
            f()
        times = {what: [] for what, _ in todo}
        for _ in range(7):
            for what, f in todo:
                torch.cuda.synchronize()
                t = time.perf_counter()
                f()
                torch.cuda.synchronize()
                times[what].append(1e3 * (time.perf_counter() - t))
        base = statistics.median(times[todo[0][0]])
        moved = int(torch.isfinite(pts.smoothed_positions(radius, 2)[1]).sum())
        print("%s, radius %.6g, %d points with an estimate at min_neighbours = 2" % (name, radius, moved))
        for what, _ in todo:
            med = statistics.median(times[what])
            print("    %-34s call ms: median %9.3f  min %9.3f  max %9.3f   ratio to estimate_normals %6.2f" %
                  (what, med, min(times[what]), max(times[what]), med / base))
        sys.stdout.flush()


if __name__ == "__main__":
    measure()
