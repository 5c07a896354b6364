#!/usr/bin/env python3
"""What the moment sums and the eigen-solve of the estimated normals cost on top of the walk they share with the radius filter:
Points.estimate_normals(radius, min_neighbours) with a min_neighbours no point reaches (the walk and the ten binary64 sums, no
solve) and with min_neighbours = 2 (a solve for nearly every point) against Points.neighbour_counts(radius, cap=0) on the same
device-resident cloud at the same radius.  Not part of bench.py; needs a GPU.

  tools/points_normals_time.py                 call times: per cloud 1 warm-up round, then 7 rounds that alternate the three calls;
                                               the median and the minimum of the host clock around each call (a call ends in a
                                               device synchronise inside the library) and the ratio of the medians to the walk's
  tools/points_normals_time.py --once          every call once in a fixed order, nothing printed but the order: the run to put under
                                               rocprofv3 --kernel-trace -d DIR -o NAME --output-format csv -- python3 tools/points_normals_time.py --once
  tools/points_normals_time.py --parse DIR     reads the kernel trace of such a run: kernel time of k_neighbour_count and of both
                                               k_point_normals in dispatch order, and their ratios

Clouds: large_case of the tests (2 * 10^5 points, four to a cell), the largest real cloud of the tests (mixed_sizes fused by the
tat_advanced loop on the device, at the radius the tests choose for it), 4 * 10^6 points of three_per_cell, and the tilted plane of
the tests at 10^6 points, twelve to a unit of area -- a surface, which is what the call is for --, all at radius 1 but the real one."""
import csv
import glob
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
NOBODY = 2 ** 31 - 1     # a min_neighbours no point reaches: the sums without the solve
MINS = (NOBODY, 2)


def clouds(pkg):
    import numpy as np
    import fusion_cases
    import points_radius_checker as PR
    import tempfile
    from oracle import binding as ob
    from test_gpu_points_average import fused
    from test_points_normals import plane_case
    from test_points_radius import dressed, large_case, real_cloud_radius, three_per_cell
    from test_points_voxel import arrays_of, from_cloud, views_of
    c, views = dressed(np.random.default_rng(9), large_case(np.random.default_rng(10)))
    yield "large_case, %d points" % c.count, from_cloud(pkg, c, *views, on_device=True), 1.0
    ob.lib()
    real = fused(pkg, ob, fusion_cases.case("mixed_sizes"), "tat_advanced", True)
    radius = real_cloud_radius(PR.build(tempfile.mkdtemp()), arrays_of(real))
    yield "mixed_sizes tat_advanced, %d points" % real.count, real, radius
    c, views = dressed(np.random.default_rng(31), three_per_cell(np.random.default_rng(32), 4000000))
    yield "three_per_cell, %d points" % c.count, from_cloud(pkg, c, *views, on_device=True), 1.0
    c, _ = plane_case(np.random.default_rng(33), side=289.0)
    yield "plane at 12 per unit of area, %d points" % c.count, from_cloud(pkg, c, *views_of(1), on_device=True), 1.0


def calls(pts, radius):
    yield "neighbour_counts(cap=0)", lambda: pts.neighbour_counts(radius, 0)
    for k in MINS:
        yield "estimate_normals(min=%s)" % ("nobody" if k == NOBODY else k), (lambda k=k: pts.estimate_normals(radius, k))


def measure(once):
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    assert pkg.device_count() >= 1, "no HIP device visible"
    for name, pts, radius in clouds(pkg):
        todo = list(calls(pts, radius))
        if once:
            for what, f in todo:
                f()
                print(name, "|", what, flush=True)
            continue
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
        estimated = int(torch.isfinite(pts.estimate_normals(radius, 2)[1]).sum())
        print("%s, radius %.6g, %d points with an estimate at min_neighbours = 2" % (name, radius, estimated))
        for what, _ in todo:
            med = statistics.median(times[what])
            print("    %-28s call ms: median %9.3f  min %9.3f  max %9.3f   ratio to the walk %6.2f" % (what, med, min(times[what]), max(times[what]), med / base))
        sys.stdout.flush()


def parse(folder):
    rows = []
    for path in glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    mine = [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6) for r in rows
            if "k_neighbour_count" in r["Kernel_Name"] or "k_point_normals" in r["Kernel_Name"]]
    per = 1 + len(MINS)
    assert mine and len(mine) % per == 0, len(mine)
    for g in range(0, len(mine), per):
        group = mine[g:g + per]
        assert "k_neighbour_count" in group[0][0] and all("k_point_normals" in n for n, _ in group[1:]), group
        print("cloud %d: k_neighbour_count %9.3f ms" % (g // per, group[0][1]) +
              "".join("   k_point_normals %s %9.3f ms (x %.2f)" % ("sums" if k == NOBODY else "sums + solve", t, t / group[0][1])
                      for k, (_, t) in zip(MINS, group[1:])))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--parse":
        parse(sys.argv[2])
    else:
        measure("--once" in sys.argv[1:])
