#!/usr/bin/env python3
"""What the alignment to another cloud costs over the searches it makes: Points.align(p, q) at 1 and at 16 steps next to
(steps + 1) times Points.nearest(p, q) at the same radius -- a call with K steps makes K + 1 searches, each with a sort of p's
positions, and the sort of q once; what it adds per step is the two chunk reductions k_align_sums1 / k_align_sums2 with their
downloads, the solve on the host and the move.  On device-resident clouds.  Not part of bench.py; needs a
GPU.  Asserts nothing.

  tools/points_align_time.py       call times: per cloud 1 warm-up round, then 7 rounds that alternate the calls; the median and
                                   the minimum of the host clock around each call (a call ends in a device synchronise inside
                                   the library), the steps each call took, and the ratio of the medians to (steps + 1) x nearest

Clouds: those of tools/points_nearest_time.py; q is p with every point moved by a Gaussian of a third of the radius per axis, so
the answer is near the identity and no call ends early: the tolerance is 0."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]


def measure():
    import torch
    import __graft_entry__ as ge
    from points_nearest_time import clouds
    pkg = ge.load_package()
    assert pkg.device_count() >= 1, "no HIP device visible"
    for name, p, q, radius in clouds(pkg):
        todo = [("nearest(p, q)", lambda: p.nearest(q, radius))]
        for steps in (1, 16):
            todo.append(("align(p, q), %d step(s)" % steps, lambda steps=steps: p.align(q, radius, iterations=steps, tolerance=0.0)))
        taken = {what: f() for what, f in todo}   # warm-up
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
            a = taken[what]
            searches = a.steps + 1 if hasattr(a, "steps") else 1
            print("    %-26s call ms: median %9.3f  min %9.3f  max %9.3f   searches %2d   ratio to searches x nearest %6.2f" %
                  (what, med, min(times[what]), max(times[what]), searches, med / (searches * base)))
        sys.stdout.flush()


if __name__ == "__main__":
    measure()
