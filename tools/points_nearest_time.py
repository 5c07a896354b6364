#!/usr/bin/env python3
"""What the nearest point of another cloud costs against the neighbour counts at the same radius on the same cloud:
Points.nearest(p, p) against uncapped Points.neighbour_counts(p) -- the same sort into cells (the same object on both sides is
sorted once), the same walk, the same distance test per candidate; the nearest search adds the compare against the best so far,
the read of the candidate's input index where that passes, and writes two values per point and not one -- then Points.nearest(p, q)
for another cloud q of the same size, which sorts both, and Points.score(p, q), two searches from one pair of sorts and two
reductions, on device-resident clouds.  Not part of bench.py; needs a GPU.  Asserts nothing.

  tools/points_nearest_time.py     call times: per cloud 1 warm-up round, then 7 rounds that alternate the calls; the median and
                                   the minimum of the host clock around each call (a call ends in a device synchronise inside
                                   the library) and the ratio of the medians to neighbour_counts'

Clouds: those of tools/points_smooth_time.py: large_case of the tests (2 * 10^5 points, four to a cell), the largest real cloud of
the tests (mixed_sizes fused by the tat_advanced loop on the device, at the radius the tests choose for it) and the tilted plane of
the tests at 10^6 points, twelve to a unit of area.  q is p with every point moved by a Gaussian of a third of the radius per axis."""
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
    from test_points_voxel import arrays_of, cloud, from_cloud, views_of

    def moved(xyz, radius, seed):
        other = (np.asarray(xyz, np.float64) + np.random.default_rng(seed).normal(size=(len(xyz), 3)) * radius / 3.0).astype(np.float32)
        return from_cloud(pkg, cloud(other), *views_of(1), on_device=True)

    c, views = dressed(np.random.default_rng(9), large_case(np.random.default_rng(10)))
    yield "large_case, %d points" % c.count, from_cloud(pkg, c, *views, on_device=True), moved(c.xyz, 1.0, 1), 1.0
    ob.lib()
    real = fused(pkg, ob, fusion_cases.case("mixed_sizes"), "tat_advanced", True)
    radius = real_cloud_radius(PR.build(tempfile.mkdtemp()), arrays_of(real))
    yield "mixed_sizes tat_advanced, %d points" % real.count, real, moved(real.xyz.cpu().numpy(), radius, 2), radius
    c, _ = plane_case(np.random.default_rng(33), side=289.0)
    yield "plane at 12 per unit of area, %d points" % c.count, from_cloud(pkg, c, *views_of(1), on_device=True), moved(c.xyz, 1.0, 3), 1.0


def calls(p, q, radius):
    yield "neighbour_counts(p)", lambda: p.neighbour_counts(radius)
    yield "nearest(p, p)", lambda: p.nearest(p, radius)
    yield "nearest(p, q)", lambda: p.nearest(q, radius)
    yield "score(p, q)", lambda: p.score(q, radius)


def measure():
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    assert pkg.device_count() >= 1, "no HIP device visible"
    for name, p, q, radius in clouds(pkg):
        todo = list(calls(p, q, radius))
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
        s = p.score(q, radius)
        print("%s, radius %.6g, precision %.4f recall %.4f of p against q" % (name, radius, s.precision, s.recall))
        for what, _ in todo:
            med = statistics.median(times[what])
            print("    %-22s call ms: median %9.3f  min %9.3f  max %9.3f   ratio to neighbour_counts %6.2f" %
                  (what, med, min(times[what]), max(times[what]), med / base))
        sys.stdout.flush()


if __name__ == "__main__":
    measure()
