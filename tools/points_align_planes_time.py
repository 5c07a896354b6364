#!/usr/bin/env python3
"""What a step of the alignment to another cloud's planes costs next to a step of the point-to-point alignment on the same
clouds: Points.align_planes(p, q) and Points.align(p, q) at 1 and at 9 steps, tolerance 0, so that (9 steps - 1 step) / 8 is a
further step of either -- one sort of the moved positions, one search, the move, pass 1, and then k_align_plane_sums (30 sums, a
gather of the match's normal) and the 6 x 6 solve in the place of k_align_sums2 (10 sums) and the 4 x 4 Jacobi (DESIGN.md section
4).  On device-resident clouds.  Not part of bench.py; needs a GPU.  Asserts nothing.

  tools/points_align_planes_time.py    call times: per cloud 1 warm-up round, then 7 rounds that alternate the calls; the median
                                       and the minimum of the host clock around each call (a call ends in a device synchronise
                                       inside the library), the steps each call took and how it ended

Clouds: those of tools/points_nearest_time.py, q with random unit normals in the place of its stored ones -- every match usable and
every motion constrained, so no call ends early; the answer is near the identity."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]


def measure():
    import numpy as np
    import torch
    import __graft_entry__ as ge
    from points_nearest_time import clouds
    from test_points_voxel import cloud, from_cloud, views_of
    pkg = ge.load_package()
    assert pkg.device_count() >= 1, "no HIP device visible"
    for name, p, q, radius in clouds(pkg):
        normal = np.random.default_rng(5).normal(size=(q.count, 3))
        normal = (normal / np.linalg.norm(normal, axis=1, keepdims=True)).astype(np.float32)
        q = from_cloud(pkg, cloud(q.xyz.cpu().numpy(), normal=normal), *views_of(1), on_device=True)
        todo = []
        for steps in (1, 9):
            todo.append(("align(p, q), %d step(s)" % steps, lambda steps=steps: p.align(q, radius, iterations=steps, tolerance=0.0)))
            todo.append(("align_planes(p, q), %d step(s)" % steps, lambda steps=steps: p.align_planes(q, radius, iterations=steps, tolerance=0.0)))
        taken = {what: f() for what, f in todo}   # warm-up
        times = {what: [] for what, _ in todo}
        for _ in range(7):
            for what, f in todo:
                torch.cuda.synchronize()
                t = time.perf_counter()
                f()
                torch.cuda.synchronize()
                times[what].append(1e3 * (time.perf_counter() - t))
        print("%s, radius %.6g" % (name, radius))
        for what, _ in todo:
            a = taken[what]
            print("    %-32s call ms: median %9.3f  min %9.3f  max %9.3f   steps %2d   stopped %d" %
                  (what, statistics.median(times[what]), min(times[what]), max(times[what]), a.steps, a.stopped))
        for call in ("align", "align_planes"):
            one, nine = (statistics.median(times["%s(p, q), %d step(s)" % (call, steps)]) for steps in (1, 9))
            print("    a further step of %-14s %9.3f ms" % (call + ":", (nine - one) / 8.0))
        sys.stdout.flush()


if __name__ == "__main__":
    measure()
