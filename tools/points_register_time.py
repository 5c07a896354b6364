#!/usr/bin/env python3
"""What the global registration costs.  Per phase of Points.register at the default number of trials -- the sort into cells, SPFH,
FPFH, the match, the trials on the host, the inlier count, the refit -- from the library's own phase clock
(apd_points_register_time_phases, an export outside the interface: every phase then ends in a device synchronise, which a call
does not otherwise pay), and by the calls that make it up without that clock: Points.features, Points.match_features (the
descriptors of both clouds and the exhaustive match; the match alone is the difference) and Points.register at 1, 4096 and 65536
trials.  For the match kernel the achieved (query, candidate)
pairs per second, next to the binary32 vector rate of the device as a fraction: a pair is 33 subtractions, 33 multiplications
and 33 additions.  On device-resident clouds thinned by merge_voxels to a few ten thousand points.  Not part of bench.py; needs a
GPU.  Asserts nothing.

  tools/points_register_time.py    per call 1 warm-up, then 5 rounds; the median and the minimum of the host clock around each call;
                                   then 5 calls of register under the phase clock, the mean per call

Clouds: the surface of tests/test_points_register.py at 400000 points, merged at a cell of 0.06, normals estimated at 0.2; P is two
of every three of its points under 130 degrees and a shift of several diameters; descriptors at radius 0.3, inliers within 0.09."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

VECTOR_FP32_FLOPS = 157.3e12     # MI355X peak vector binary32 rate with FMA counted as two; these kernels may not contract
FLOPS_PER_PAIR = 99


def measure():
    import torch
    import __graft_entry__ as ge
    from test_points_register import PLANTED_R, PLANTED_T, surface
    from test_points_voxel import cloud, from_cloud
    pkg = ge.load_package()
    assert pkg.device_count() >= 1, "no HIP device visible"
    voxel, normal_radius, radius, distance = 0.06, 0.2, 0.3, 0.09
    dense = from_cloud(pkg, cloud(surface(400000)), [4], [5], [[]], on_device=True)
    q, _ = dense.merge_voxels(voxel)[0].with_estimated_normals(normal_radius, 5)
    xyz, normal = q.xyz.cpu().numpy(), q.normal.cpu().numpy()
    keep = np.arange(len(xyz)) % 3 != 0
    part = from_cloud(pkg, cloud(xyz[keep], normal=normal[keep]), [4], [5], [[]], on_device=True)
    p = part.transformed(1.0, PLANTED_R.T, -PLANTED_R.T @ PLANTED_T)
    todo = [("features(q)", lambda: q.features(radius)),
            ("features(p)", lambda: p.features(radius)),
            ("match_features(p, q), one way", lambda: p.match_features(q, radius, mutual=False)),
            ("match_features(p, q), mutual", lambda: p.match_features(q, radius, mutual=True)),
            ("register(p, q), 1 trial", lambda: p.register(q, radius, distance, trials=1)),
            ("register(p, q), 4096 trials", lambda: p.register(q, radius, distance)),
            ("register(p, q), 65536 trials", lambda: p.register(q, radius, distance, trials=65536))]
    taken = {what: f() for what, f in todo}   # warm-up
    times = {what: [] for what, _ in todo}
    for _ in range(5):
        for what, f in todo:
            torch.cuda.synchronize()
            t = time.perf_counter()
            f()
            torch.cuda.synchronize()
            times[what].append(1e3 * (time.perf_counter() - t))
    med = {what: statistics.median(v) for what, v in times.items()}
    r = taken["register(p, q), 4096 trials"]
    print("surface: q %d points, p %d points, radius %g, inlier distance %g" % (q.count, p.count, radius, distance))
    for what, _ in todo:
        print("    %-32s call ms: median %9.3f  min %9.3f  max %9.3f" % (what, med[what], min(times[what]), max(times[what])))
    for what in ("register(p, q), 1 trial", "register(p, q), 4096 trials", "register(p, q), 65536 trials"):
        a = taken[what]
        print("    %-32s descriptors %d / %d, matches %d, admitted %d, best trial %d, inliers %d -> %d, rms %.4g, stopped %d; rotation off by %.3g" %
              (what, a.features_p, a.features_q, a.matches, a.trials_admitted, a.best_trial, a.inliers, a.inliers_after, a.rms_after, a.stopped,
               np.abs(a.rotation - PLANTED_R).max()))
    both = med["features(q)"] + med["features(p)"]
    one_way, mutual = med["match_features(p, q), one way"] - both, med["match_features(p, q), mutual"] - both
    pairs = float(r.features_p) * float(r.features_q)
    print("    descriptors of both clouds %.3f ms; match alone: one way %.3f ms, mutual %.3f ms" % (both, one_way, mutual))
    for what, ms, n in (("one way", one_way, pairs), ("mutual", mutual, 2 * pairs)):
        rate = n / (ms * 1e-3)
        print("    match %-8s %.4g pairs in %.3f ms: %.4g pairs/s = %.4g binary32 operations/s, %.3f of the vector rate %.4g" %
              (what, n, ms, rate, rate * FLOPS_PER_PAIR, rate * FLOPS_PER_PAIR / VECTOR_FP32_FLOPS, VECTOR_FP32_FLOPS))
    print("    trials, count and refit over match_features (mutual): 1 trial %.3f ms, 4096 trials %.3f ms, 65536 trials %.3f ms" %
          tuple(med[w] - med["match_features(p, q), mutual"] for w in ("register(p, q), 1 trial", "register(p, q), 4096 trials", "register(p, q), 65536 trials")))
    import ctypes as C
    L = pkg.lib()
    L.apd_points_register_time_phases.argtypes = [C.c_int, C.POINTER(C.c_double)]
    L.apd_points_register_time_phases.restype = None
    rounds, ms = 5, (C.c_double * 7)()
    L.apd_points_register_time_phases(1, None)
    for _ in range(rounds):
        p.register(q, radius, distance)
    L.apd_points_register_time_phases(0, ms)
    names = ("sort into cells, with the uploads and the compaction of the first cloud", "SPFH, both clouds", "FPFH, both clouds",
             "match, both directions, with the compaction and the transfers of the matches", "trials on the host", "inlier count", "refit")
    print("    register(p, q), 4096 trials, under the phase clock: %.3f ms per call" % (sum(ms) / rounds))
    for name, v in zip(names, ms):
        print("        %-80s %9.3f ms" % (name, v / rounds))
    sys.stdout.flush()


if __name__ == "__main__":
    measure()
