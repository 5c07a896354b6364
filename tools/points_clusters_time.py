#!/usr/bin/env python3
"""What the connected components cost against the walk they share with the radius filter: Points.components(radius) and
Points.remove_small_components(radius, 8) against Points.neighbour_counts(radius, cap=0) on the same device-resident cloud at the
same radius.  k_cluster_link does half the distance tests of k_neighbour_count.  Not part of bench.py; needs
a GPU.

  tools/points_clusters_time.py                 call times: per cloud 1 warm-up round, then 7 rounds that alternate the three calls;
                                                the median, the minimum and the maximum of the host clock around each call (a call
                                                ends in a device synchronise inside the library) and the ratio of the medians to
                                                the walk's
  tools/points_clusters_time.py --once          every call once in a fixed order after one warm-up round, nothing printed but the
                                                order: the run to put under
                                                rocprofv3 --kernel-trace -d DIR -o NAME --output-format csv -- python3 tools/points_clusters_time.py --once
  tools/points_clusters_time.py --parse DIR     reads the kernel trace of such a run: per cloud the kernel time of k_neighbour_count
                                                and of k_cluster_link, _flatten, _reduce and _emit of the components() call, and
                                                the ratio of the link to the walk
  --library PATH                                loads that libapd_mi355x.so in place of the tree's: a lab build of the same sources
                                                with -DAPD_LAB_CLUSTER_REDUCE_NAIVE (one atomic per lane in k_cluster_reduce), to
                                                set its k_cluster_reduce beside the combined one's
  --points N                                    the size of both clouds (default 10^7)

Clouds, both uniform in a cube at radius 1, made once before anything is timed: `giant`, 3 points per cell -- the cloud of
profiles/points_radius/timing.txt, one component but for some thousand stragglers --, and `small`, 0.6 points per cell -- below
the percolation threshold: millions of components from singletons to some hundred points."""
import csv
import glob
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
KERNELS = ("k_neighbour_count", "k_cluster_link", "k_cluster_flatten", "k_cluster_reduce", "k_cluster_emit")
MIN_SIZE = 8


def option(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def clouds(pkg, n):
    import numpy as np
    from test_points_voxel import cloud, from_cloud
    for name, density, seed in (("giant", 3.0, 41), ("small", 0.6, 42)):
        side = (n / density) ** (1.0 / 3.0)
        xyz = (np.random.default_rng(seed).random((n, 3)) * side).astype(np.float32)
        pts = from_cloud(pkg, cloud(xyz), [4], [5], [[]], on_device=True)
        label, size, components = pts.components(1.0)
        size = size.cpu().numpy().view(np.uint32)
        yield "%s: %d points at %.1f per cell, side %.1f: %d components, the largest of %d points" % (name, n, density, side, components, int(size.max())), pts


def calls(pts):
    yield "neighbour_counts(cap=0)", lambda: pts.neighbour_counts(1.0, 0)
    yield "components()", lambda: pts.components(1.0)
    yield "remove_small_components(%d)" % MIN_SIZE, lambda: pts.remove_small_components(1.0, MIN_SIZE)[0].close()


def measure(once, n, library):
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    if library:
        pkg.LIB_PATH = os.path.abspath(library)
    assert pkg.device_count() >= 1, "no HIP device visible"
    print("library: %s" % pkg.LIB_PATH, flush=True)
    for name, pts in clouds(pkg, n):
        todo = list(calls(pts))
        for what, f in todo:   # warm-up
            f()
        if once:
            for what, f in todo:
                f()
                print(name, "|", what, flush=True)
            continue
        times = {what: [] for what, _ in todo}
        for _ in range(7):
            for what, f in todo:
                torch.cuda.synchronize()
                t = time.perf_counter()
                f()
                torch.cuda.synchronize()
                times[what].append(1e3 * (time.perf_counter() - t))
        base = statistics.median(times[todo[0][0]])
        print(name)
        for what, _ in todo:
            med = statistics.median(times[what])
            print("    %-30s call ms: median %9.3f  min %9.3f  max %9.3f   ratio to the walk %6.2f" % (what, med, min(times[what]), max(times[what]), med / base))
        sys.stdout.flush()
        pts.close()


def parse(folder):
    rows = []
    for path in glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    mine = [(k, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6) for r in rows for k in KERNELS if k in r["Kernel_Name"]]
    # per cloud: the set-up's components() call, a warm-up round (walk, components, removal), then the traced round
    per = 4 + 2 * (1 + 4 + 4)
    assert mine and len(mine) % per == 0, (len(mine), per)
    for g in range(0, len(mine), per):
        walk, link, flatten, reduce_, emit = mine[g + per - 9:g + per - 4]
        assert [k for k, _ in (walk, link, flatten, reduce_, emit)] == list(KERNELS), mine[g:g + per]
        print("cloud %d: k_neighbour_count %9.3f ms   k_cluster_link %9.3f ms (x %.2f)   k_cluster_flatten %9.3f ms   k_cluster_reduce %9.3f ms   "
              "k_cluster_emit %9.3f ms" % (g // per, walk[1], link[1], link[1] / walk[1], flatten[1], reduce_[1], emit[1]))


if __name__ == "__main__":
    if "--parse" in sys.argv:
        parse(option("--parse", None))
    else:
        measure("--once" in sys.argv[1:], int(float(option("--points", "1e7"))), option("--library", None))
