#!/usr/bin/env python3
"""What the k-nearest selection costs on top of the walk it shares with the radius filter: Points.knn_mean_distances(radius, k) at
k = 8, 20 and 64 against Points.neighbour_counts(radius, cap=0) on the same device-resident cloud at the same radius (DESIGN.md
section 6).  Not part of bench.py; needs a GPU.

  tools/points_knn_time.py                 call times: per cloud 1 warm-up round, then 7 rounds that alternate the four calls; the
                                           median and the minimum of the host clock around each call (a call ends in a device
                                           synchronise inside the library) and the ratio of the medians to the walk's
  tools/points_knn_time.py --once          every call once in a fixed order, nothing printed but the order: the run to put under
                                           rocprofv3 --kernel-trace -d DIR -o NAME --output-format csv -- python3 tools/points_knn_time.py --once
  tools/points_knn_time.py --parse DIR     reads the kernel trace of such a run: kernel time of k_neighbour_count and of every
                                           k_knn_mean in dispatch order, and their ratios

Clouds: large_case of the tests (2 * 10^5 points, four to a cell), the largest real cloud of the tests (mixed_sizes fused by the
tat_advanced loop on the device, at the radius the tests choose for it) and 4 * 10^6 points of three_per_cell, all at radius 1 but
the real one."""
import csv
import glob
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
KS = (8, 20, 64)


def clouds(pkg):
    import numpy as np
    import fusion_cases
    import points_radius_checker as PR
    import tempfile
    from oracle import binding as ob
    from test_gpu_points_average import fused
    from test_points_radius import dressed, large_case, real_cloud_radius, three_per_cell
    from test_points_voxel import arrays_of, from_cloud
    c, views = dressed(np.random.default_rng(9), large_case(np.random.default_rng(10)))
    yield "large_case, %d points" % c.count, from_cloud(pkg, c, *views, on_device=True), 1.0
    ob.lib()
    real = fused(pkg, ob, fusion_cases.case("mixed_sizes"), "tat_advanced", True)
    radius = real_cloud_radius(PR.build(tempfile.mkdtemp()), arrays_of(real))
    yield "mixed_sizes tat_advanced, %d points" % real.count, real, radius
    c, views = dressed(np.random.default_rng(31), three_per_cell(np.random.default_rng(32), 4000000))
    yield "three_per_cell, %d points" % c.count, from_cloud(pkg, c, *views, on_device=True), 1.0


def calls(pts, radius):
    yield "neighbour_counts(cap=0)", lambda: pts.neighbour_counts(radius, 0)
    for k in KS:
        yield "knn_mean_distances(k=%d)" % k, (lambda k=k: pts.knn_mean_distances(radius, k))


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
        print("%s, radius %.6g" % (name, radius))
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
            if "k_neighbour_count" in r["Kernel_Name"] or "k_knn_mean" in r["Kernel_Name"]]
    per = 1 + len(KS)
    assert mine and len(mine) % per == 0, len(mine)
    for g in range(0, len(mine), per):
        group = mine[g:g + per]
        assert "k_neighbour_count" in group[0][0] and all("k_knn_mean" in n for n, _ in group[1:]), group
        print("cloud %d: k_neighbour_count %9.3f ms" % (g // per, group[0][1]) +
              "".join("   k_knn_mean k=%d %9.3f ms (x %.2f)" % (k, t, t / group[0][1]) for k, (_, t) in zip(KS, group[1:])))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--parse":
        parse(sys.argv[2])
    else:
        measure("--once" in sys.argv[1:])
