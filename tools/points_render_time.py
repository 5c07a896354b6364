#!/usr/bin/env python3
"""What one rendering and the rendered visibility cost beside the fusion that made the cloud: Points.render(camera, splat) and
Points.with_rendered_visibility(cameras, splat, tolerance) on a real fused cloud of the synthetic ring -- "full_frame" of
tests/fusion_cases.py, 4 views of 1920 x 1080 with 3 sources each, fused by the ETH loop on the device -- and the times of that
fusion call (apd_fusion_last_timing).  And the same two calls on a cloud many layers deep, where nearly
every atomic of the scatter loses: points on random pixels of a 640 x 480 image at depths 2 .. 6.  Not part of bench.py; needs a GPU.

  tools/points_render_time.py                 per cloud 1 warm-up round, then 7 rounds that alternate the calls; the median, the
                                              minimum and the maximum of the host clock around each call (a call ends in a device
                                              synchronise inside the library)
  --library PATH                              loads that libapd_mi355x.so in place of the tree's: a lab build of the same sources
                                              with -DAPD_LAB_RENDER_NO_LOAD (k_render_scatter issues every atomic min, without the
                                              load that skips the ones that cannot win), to set its times beside the product's
  --points N                                  the size of the deep cloud (default 4 * 10^6: 13 points to a pixel)"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def option(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def clouds(pkg, n):
    import numpy as np
    import fusion_cases
    from oracle import binding as ob
    from test_gpu_points_average import fused
    from test_points_render import pinhole
    from test_points_voxel import cloud, from_cloud
    ob.lib()
    case = fusion_cases.case("full_frame")
    real = fused(pkg, ob, case, "eth", True)
    ms = (C.c_double * 3)()
    pkg.lib().apd_fusion_last_timing(C.byref(ms, 0), C.byref(ms, 8), C.byref(ms, 16))
    yield ("full_frame fused by the ETH loop: %d points; that fusion call: set-up %.1f ms, views %.1f ms" % (real.count, ms[0], ms[1]), real,
           list(case.cameras(pkg.make_camera)))
    rng = np.random.default_rng(51)
    W, H, f = 640, 480, 320.0
    d = rng.uniform(2.0, 6.0, n)
    xyz = np.stack([(rng.uniform(0, W - 1, n) - (W - 1) / 2.0) / f * d, (rng.uniform(0, H - 1, n) - (H - 1) / 2.0) / f * d, d], 1).astype(np.float32)
    yield ("deep: %d points on a 640 x 480 image, %.1f to a pixel" % (n, n / float(W * H)), from_cloud(pkg, cloud(xyz), [4], [5], [[]], on_device=True),
           [pinhole(pkg, W, H, f)] * 4)


def calls(pts, cams):
    for splat in (0, 1, 4):
        yield "render(view 0, splat %d)" % splat, (lambda splat=splat: pts.render(cams[0], splat))
    for splat in (0, 1):
        yield "with_rendered_visibility(%d views, splat %d, 0.01)" % (len(cams), splat), (lambda splat=splat: pts.with_rendered_visibility(cams, splat, 0.01)[0].close())


def measure(n, library):
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    if library:
        pkg.LIB_PATH = os.path.abspath(library)
    assert pkg.device_count() >= 1, "no HIP device visible"
    print("library: %s" % pkg.LIB_PATH, flush=True)
    for name, pts, cams in clouds(pkg, n):
        todo = list(calls(pts, cams))
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
        _, unseen = pts.with_rendered_visibility(cams, 1, 0.01)
        print("%s; %d points seen by no view at splat 1" % (name, unseen))
        for what, _ in todo:
            print("    %-52s call ms: median %9.3f  min %9.3f  max %9.3f" % (what, statistics.median(times[what]), min(times[what]), max(times[what])))
        sys.stdout.flush()


if __name__ == "__main__":
    measure(int(float(option("--points", "4e6"))), option("--library", None))
