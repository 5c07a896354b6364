#!/usr/bin/env python3
"""What colouring a mesh's vertices from 8 views of 3200 x 2400 costs (apd_mesh_colour_from_views), beside apd_mesh_face_visibility over
the same mesh and the same cameras in the same run: that call pays the same rasterisation per view, so the difference is the price of
the resolve, the two colour kernels and, for images in host memory, of the copies.  Three device-resident meshes, those of
tools/mesh_render_time.py: a jittered sheet of about a million faces, the same sheet simplified to about 10^4 faces, and the mesh
pipeline.mesh extracts from the small synthetic scene of the tests.  Images of three channels.  Not part of bench.py; needs a GPU.

  tools/mesh_colour_time.py            1 warm-up round, then 7 rounds that alternate the three calls; per call the median, the minimum
                                       and the maximum of the host clock around the library call, and the median of the call's own
                                       work time (apd_fusion_last_timing: without the allocations)
  --side N                             the sheet has N x (N - 4) vertices (default 710: 999,690 faces)
  --no-scene                           without the end-to-end scene's mesh"""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
W, H, VIEWS = 3200, 2400, 8


def cameras(pkg, vertices):
    """VIEWS cameras of 3200 x 2400 that look at the middle of the vertices' box from the side of -z, the first on the axis, the others
    up to 30 degrees off it, far enough for the box to fill most of the frame."""
    lo, hi = vertices.min(0), vertices.max(0)
    mid, extent = (lo + hi) / 2, max(hi[0] - lo[0], (hi[1] - lo[1]) * W / H, 1e-6)
    f = 0.95 * W
    distance = f * extent / (0.9 * W)
    K = [f, 0, (W - 1) / 2.0, 0, f, (H - 1) / 2.0, 0, 0, 1]
    cams = []
    for s in range(VIEWS):
        a = np.radians(30.0) * s / (VIEWS - 1) * (1 if s % 2 else -1)
        R = np.array([[np.cos(a), 0, -np.sin(a)], [0, 1, 0], [np.sin(a), 0, np.cos(a)]])   # about y: the camera swings in the x-z plane
        eye = mid + distance * np.array([-np.sin(a), 0, -np.cos(a)])
        cams.append(pkg.make_camera(K, R.reshape(9), -R @ eye, W, H, 0.1, 1000.0))
    return cams


def time_mesh(pkg, name, mesh, host_images, device_images):
    import torch
    L = pkg.lib()
    cams = cameras(pkg, mesh.vertices)
    ms = (C.c_double * 3)()
    calls = (("apd_mesh_face_visibility, cull none", lambda: mesh.face_visibility(cams, "none")),
             ("apd_mesh_colour_from_views, device images", lambda: mesh.colour_from_views(cams, device_images)),
             ("apd_mesh_colour_from_views, host images", lambda: mesh.colour_from_views(cams, host_images)))
    times, work = {label: [] for label, _ in calls}, {label: [] for label, _ in calls}
    uncoloured = None
    for round_ in range(8):   # the first is the warm-up
        for label, call in calls:
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = call()
            took = 1e3 * (time.perf_counter() - t)
            L.apd_fusion_last_timing(C.byref(ms, 0), C.byref(ms, 8), C.byref(ms, 16))
            if hasattr(out, "close"):
                assert uncoloured in (None, out.uncoloured), (uncoloured, out.uncoloured)
                uncoloured = out.uncoloured
                out.close()
            if round_ > 0:
                times[label].append(took)
                work[label].append(ms[1])
    print("%s: %d vertices, %d faces, %d views of %d x %d, %d vertices left uncoloured" % (name, len(mesh.vertices), len(mesh.faces), VIEWS, W, H, uncoloured))
    for label, _ in calls:
        print("    %-44s call ms: median %9.3f  min %9.3f  max %9.3f   work ms: median %9.3f" % (
            label, statistics.median(times[label]), min(times[label]), max(times[label]), statistics.median(work[label])))
    sys.stdout.flush()


def measure(side, with_scene):
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    assert pkg.device_count() >= 1, "no HIP device visible"
    rng = np.random.default_rng(4)
    host_images = [rng.uniform(0.0, 255.0, (H, W, 3)).astype(np.float32) for _ in range(VIEWS)]
    device_images = [torch.from_numpy(a).to("cuda:0") for a in host_images]
    print("%d images of %d x %d x 3 floats: %.1f MB each; the call's Python wrapper (the download of the result mesh) is inside the call time, "
          "not the work time; a single run" % (VIEWS, W, H, W * H * 12 / 1e6), flush=True)
    from test_mesh import sheet
    host = sheet(side, side - 4, 0.2)
    big = pkg.Mesh.from_arrays(host.vertices, host.faces[:, [0, 2, 1]])   # the normals towards the cameras
    time_mesh(pkg, "sheet", big, host_images, device_images)
    small = big.simplify(side / 71.0)   # about 71 x 71 cells: 10^4 faces
    time_mesh(pkg, "sheet simplified", small, host_images, device_images)
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
        time_mesh(pkg, "the synthetic scene's mesh", found, host_images, device_images)
        found.close()


if __name__ == "__main__":
    option = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    measure(int(option("--side", "710")), "--no-scene" not in sys.argv)
