#!/usr/bin/env python3
"""What a mesh costs beside the fusion that made the cloud: Volume.integrate of 4 views (with and without colour) and
Volume.extract_mesh on "full_frame" of tests/fusion_cases.py -- 4 views of 1920 x 1080 with 3 sources each -- on a grid of about
N^3 samples in the box of the cloud the ETH loop fuses of the same maps, beside the times of that fusion call
(apd_fusion_last_timing), and the bytes an integrate call must move -- the volume read once and written once -- over its time
(DESIGN.md section 6).  Not part of bench.py; needs a GPU.

  tools/volume_time.py                        per grid 1 warm-up round, then 7 rounds that alternate the calls; the median, the
                                              minimum and the maximum of the host clock around each call (a call ends in a device
                                              synchronise inside the library)
  --library PATH                              loads that libapd_mi355x.so in place of the tree's: a lab build of the same sources
                                              with -DAPD_LAB_VOLUME_LAUNCH_PER_VIEW (one launch of k_volume_integrate per view, the
                                              volume read and written once per view), to set its times beside the product's
  --sizes N,N                                 the grids (default 128,256)"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
HBM_TB_S = (8.0, 6.29)   # the peak of the data sheet, and what a float4 copy has been measured to reach


def option(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def measure(sizes, library):
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    if library:
        pkg.LIB_PATH = os.path.abspath(library)
    assert pkg.device_count() >= 1, "no HIP device visible"
    print("library: %s" % pkg.LIB_PATH, flush=True)
    import fusion_cases
    from apd_mvs_amd import pipeline
    from test_gpu_fusion_options import _scene
    case = fusion_cases.case("full_frame")
    scene, results = _scene(pkg, pipeline, case)
    _, points = pipeline.fuse(scene, results, None, return_points=True)
    ms = (C.c_double * 3)()
    pkg.lib().apd_fusion_last_timing(C.byref(ms, 0), C.byref(ms, 8), C.byref(ms, 16))
    print("full_frame fused by the ETH loop: %d points; that fusion call: set-up %.1f ms, views %.1f ms" % (points.count, ms[0], ms[1]))
    lo, hi = pipeline.mesh_bounds(points)
    maps = pipeline.filter_maps(scene, results, on_device=True)
    cams, images = pipeline.mesh_views(scene, results, None)
    depths = [m.depth for m in maps]
    images = [torch.from_numpy(a).cuda() for a in images]
    for size in sizes:
        voxel = float((hi - lo).max()) / (size - 1)
        plain = pkg.Volume.around(lo, hi, voxel, 4 * voxel, margin=0.0)
        coloured = pkg.Volume.around(lo, hi, voxel, 4 * voxel, margin=0.0, colour=True)
        todo = [("integrate(4 views)", lambda: plain.integrate(cams, depths, maps_on_device=True), 8 * 2),
                ("integrate(4 views, colour)", lambda: coloured.integrate(cams, depths, images, maps_on_device=True), 24 * 2),
                ("extract_mesh()", lambda: coloured.extract_mesh().close(), 0)]
        for _, f, _ in todo:   # warm-up
            f()
        times = {what: [] for what, _, _ in todo}
        for _ in range(7):
            for what, f, _ in todo:
                torch.cuda.synchronize()
                t = time.perf_counter()
                f()
                torch.cuda.synchronize()
                times[what].append(1e3 * (time.perf_counter() - t))
        mesh = coloured.extract_mesh()
        print("grid %d x %d x %d = %d samples, voxel %.5f: %d vertices, %d faces" % (plain.dims + (plain.samples, voxel, len(mesh.vertices), len(mesh.faces))))
        for what, _, bytes_per_sample in todo:
            med = statistics.median(times[what])
            line = "    %-32s call ms: median %9.3f  min %9.3f  max %9.3f" % (what, med, min(times[what]), max(times[what]))
            if bytes_per_sample:
                moved = bytes_per_sample * plain.samples
                line += "   volume read + written %.1f MB, over the median %.3f TB/s (derived from the call time, not from counters; HBM: %.1f TB/s peak, %.2f a copy)" % (
                    (moved / 1e6, moved / (med * 1e-3) / 1e12) + HBM_TB_S)
            print(line)
        sys.stdout.flush()
        mesh.close()
        plain.close()
        coloured.close()


if __name__ == "__main__":
    measure([int(s) for s in option("--sizes", "128,256").split(",")], option("--library", None))
