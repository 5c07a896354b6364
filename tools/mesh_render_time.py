#!/usr/bin/env python3
"""What rasterising a mesh into a 3200 x 2400 camera costs, call by call, for every split between the lane-per-face and the
wave-per-face kernel in SPLITS below (apd_mesh_render_split): 1, every face by a wave; 64, 256, 1024 and 4096, the candidates the
default is chosen from; the default itself; 2^30, every face by a lane.  Three device-resident meshes: a jittered sheet of about a
million faces (tests/test_mesh.py), the same sheet simplified to about 10^4 faces, and the mesh pipeline.mesh extracts from the small
synthetic scene of the tests.  For scale, apd_points_render with splat 1 of the same vertices, the existing call of the same
clear-scatter-resolve shape.  Not part of bench.py; needs a GPU.

  tools/mesh_render_time.py            1 warm-up round, then 7 rounds that alternate the splits; per split the median, the minimum and
                                       the maximum of the host clock around the library call, and the median of the call's own work
                                       time (apd_fusion_last_timing: from the first launch to the end of the copy of the depth map to
                                       the host, without the allocations).  The copy, 30 MB, is the same for every split: the
                                       differences between the rows are the kernels'
  --side N                             the sheet has N x (N - 4) vertices (default 710: 999,690 faces)
  --no-scene                           without the end-to-end scene's mesh"""
import ctypes as C
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
W, H = 3200, 2400
SPLITS = ((1, "split 1: every face by a wave"), (64, "split 64"), (256, "split 256"), (1024, "split 1024"), (4096, "split 4096"),
          (0, "the default split"), (2 ** 30, "split 2^30: every face by a lane"))


def option(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def default_split():
    """The built-in split, read from the header the library was built from (the library does not export it)."""
    text = open(os.path.join(ROOT, "apd-mvs_amd", "csrc", "apd_tuning.h")).read()
    return int(re.search(r"#define\s+APD_MESH_RENDER_SPLIT\s+(\d+)", text).group(1))


def facing_camera(pkg, vertices):
    """A 3200 x 2400 camera on the axis through the middle of the vertices' box, along z, far enough for the box to fill most of the frame."""
    lo, hi = vertices.min(0), vertices.max(0)
    mid, extent = (lo + hi) / 2, max(hi[0] - lo[0], (hi[1] - lo[1]) * W / H, 1e-6)
    f = 0.95 * W
    distance = f * extent / (0.9 * W)
    K = [f, 0, (W - 1) / 2.0, 0, f, (H - 1) / 2.0, 0, 0, 1]
    t = [-mid[0], -mid[1], distance - lo[2]]
    return pkg.make_camera(K, np.eye(3).reshape(9), t, W, H, 0.1, 1000.0)


def time_mesh(pkg, name, mesh):
    import torch
    L = pkg.lib()
    cam = facing_camera(pkg, mesh.vertices)
    depth = np.zeros((H, W), np.float32)
    from test_points_voxel import cloud, from_cloud
    points = from_cloud(pkg, cloud(mesh.vertices), [4], [5], [[]], on_device=True)
    todo = [(label if split else "%s (%d)" % (label, default_split()), split) for split, label in SPLITS]
    times = {label: [] for label, _ in todo}
    work = {label: [] for label, _ in todo}
    ms = (C.c_double * 3)()
    covered = None
    try:
        for round_ in range(8):   # the first is the warm-up
            for label, split in todo:
                L.apd_mesh_render_split(split)
                torch.cuda.synchronize()
                t = time.perf_counter()
                rc = L.apd_mesh_render(mesh._m, C.byref(cam), 0, C.c_void_p(depth.ctypes.data), None)
                took = 1e3 * (time.perf_counter() - t)
                assert rc == 0, L.apd_fusion_last_error()
                L.apd_fusion_last_timing(C.byref(ms, 0), C.byref(ms, 8), C.byref(ms, 16))
                if round_ > 0:
                    times[label].append(took)
                    work[label].append(ms[1])
                now = int((depth > 0).sum())
                assert covered in (None, now), (covered, now)
                covered = now
    finally:
        L.apd_mesh_render_split(0)
    print("%s: %d vertices, %d faces, %.1f %% of %d x %d covered, %.1f pixels a face" % (
        name, len(mesh.vertices), len(mesh.faces), 100.0 * covered / (W * H), W, H, covered / max(len(mesh.faces), 1)))
    for label, _ in todo:
        print("    %-36s call ms: median %9.3f  min %9.3f  max %9.3f   work ms: median %9.3f" % (
            label, statistics.median(times[label]), min(times[label]), max(times[label]), statistics.median(work[label])))
    took = []
    for round_ in range(8):   # device-resident points: the maps stay on the device, nothing is copied
        torch.cuda.synchronize()
        t = time.perf_counter()
        points.render(cam, 1)
        torch.cuda.synchronize()
        took.append(1e3 * (time.perf_counter() - t))
    print("    %-36s call ms: median %9.3f  min %9.3f  max %9.3f" % ("apd_points_render, splat 1, vertices", statistics.median(took[1:]), min(took[1:]), max(took[1:])))
    points.close()
    sys.stdout.flush()


def measure(side, with_scene):
    import __graft_entry__ as ge
    pkg = ge.load_package()
    assert pkg.device_count() >= 1, "no HIP device visible"
    print("the default split, APD_MESH_RENDER_SPLIT of csrc/apd_tuning.h, is %d pixels; a single run" % default_split(), flush=True)
    from test_mesh import sheet
    host = sheet(side, side - 4, 0.2)
    big = pkg.Mesh.from_arrays(host.vertices, host.faces)
    time_mesh(pkg, "sheet", big)
    small = big.simplify(side / 71.0)   # about 71 x 71 cells: 10^4 faces
    time_mesh(pkg, "sheet simplified", small)
    small.close()
    big.close()
    if with_scene:
        import fusion_cases
        from apd_mvs_amd import pipeline
        from test_gpu_fusion_options import _scene
        scene, results = _scene(pkg, pipeline, fusion_cases.case("mixed_sizes"))
        options = pkg.default_fusion_options(factor_strong=0.0, factor_weak=0.0)
        _, points = pipeline.fuse(scene, results, None, options=options, return_points=True)
        _, _, found = pipeline.mesh(scene, results, None, 0.05, bounds=points, options=options, return_mesh=True)
        points.close()
        time_mesh(pkg, "the synthetic scene's mesh", found)
        found.close()


if __name__ == "__main__":
    measure(int(option("--side", "710")), "--no-scene" not in sys.argv)
