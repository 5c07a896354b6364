#!/usr/bin/env python3
"""What cleaning a mesh costs beside the extraction that made it: Mesh.weld, Mesh.components, Mesh.remove_small_components and
Mesh.with_vertex_normals on the mesh Volume.extract_mesh takes from "full_frame" of tests/fusion_cases.py -- 4 views of 1920 x 1080
with 3 sources each, filtered without the consistency factors so that the surface is dense -- on a grid of about N^3 samples in the
box of the cloud the ETH loop fuses of the same maps (the grids of tools/volume_time.py), and which share of with_vertex_normals is
the sort.  Not part of bench.py; needs a GPU.

  tools/mesh_time.py                          per grid 1 warm-up round, then 7 rounds that alternate the calls; the median, the
                                              minimum and the maximum of the host clock around each call (a call ends in a device
                                              synchronise inside the library, and the Python call downloads the result into numpy,
                                              extract_mesh() too), and beside it the library's own "views" time of the last round
                                              (apd_fusion_last_timing: kernels and device copies, no download); then the sort of the
                                              3 F (vertex, corner) pairs alone, through the library's sort on the same keys
  --sizes N,N                                 the grids (default 128,256)"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def option(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def measure(sizes):
    import numpy as np
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    assert pkg.device_count() >= 1, "no HIP device visible"
    L = pkg.lib()
    print("library: %s" % pkg.LIB_PATH, flush=True)
    import fusion_cases
    from apd_mvs_amd import pipeline
    from test_gpu_fusion_options import _scene
    case = fusion_cases.case("full_frame")
    scene, results = _scene(pkg, pipeline, case)
    options = pkg.default_fusion_options(factor_strong=0.0, factor_weak=0.0)
    _, points = pipeline.fuse(scene, results, None, options=options, return_points=True)
    lo, hi = pipeline.mesh_bounds(points)
    maps = pipeline.filter_maps(scene, results, options=options, on_device=True)
    cams, images = pipeline.mesh_views(scene, results, None)
    depths = [m.depth for m in maps]
    images = [torch.from_numpy(a).cuda() for a in images]
    ms = (C.c_double * 3)()

    def views_ms():
        L.apd_fusion_last_timing(C.byref(ms, 0), C.byref(ms, 8), C.byref(ms, 16))
        return ms[1]

    for size in sizes:
        voxel = float((hi - lo).max()) / (size - 1)
        volume = pkg.Volume.around(lo, hi, voxel, 4 * voxel, margin=0.0, colour=True)
        volume.integrate(cams, depths, images, maps_on_device=True)
        mesh = volume.extract_mesh()
        tol = voxel * 1e-4
        welded = mesh.weld(tol)
        todo = [("extract_mesh()", lambda: volume.extract_mesh().close()),
                ("weld(voxel * 1e-4)", lambda: mesh.weld(tol).close()),
                ("components()", lambda: mesh.components()),
                ("remove_small_components(100)", lambda: mesh.remove_small_components(100).close()),
                ("with_vertex_normals()", lambda: mesh.with_vertex_normals().close()),
                ("welded: components()", lambda: welded.components()),
                ("welded: remove_small_components(100)", lambda: welded.remove_small_components(100).close()),
                ("welded: with_vertex_normals()", lambda: welded.with_vertex_normals().close())]
        for _, f in todo:   # warm-up
            f()
        times, device = {what: [] for what, _ in todo}, {}
        for _ in range(7):
            for what, f in todo:
                torch.cuda.synchronize()
                t = time.perf_counter()
                f()
                torch.cuda.synchronize()
                times[what].append(1e3 * (time.perf_counter() - t))
                device[what] = views_ms()
        print("grid %d x %d x %d = %d samples, voxel %.5f: %d vertices, %d faces; welded: %d vertices, %d faces, %d components" % (
            volume.dims + (volume.samples, voxel, len(mesh.vertices), len(mesh.faces), len(welded.vertices), len(welded.faces), welded.components()[2])))
        for what, _ in todo:
            print("    %-40s call ms: median %9.3f  min %9.3f  max %9.3f   library's own time of the last round %9.3f" % (
                what, statistics.median(times[what]), min(times[what]), max(times[what]), device[what]))
        # the sort alone: the library's own sort_pairs (a C++ symbol of the shared library, apd_sort.h) on the same 3 F keys and
        # payloads, made here as torch tensors, beside the whole call.  The name below is the Itanium mangling of
        #   hipError_t apd_sort::sort_pairs(uint64_t *, uint64_t *, uint32_t *, uint32_t *, size_t, int *, int *)
        # and the argtypes restate that signature by hand: a change of it in apd_sort.h must be made here too (the lookup then fails
        # with an AttributeError; a change of types alone would not).  tools/sort_check.hip is the caller that links it properly.
        sort_pairs = getattr(L, "_ZN8apd_sort10sort_pairsEPmS0_PjS1_mPiS2_")
        sort_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        for name, m in (("extracted", mesh), ("welded", welded)):
            corners = 3 * len(m.faces)
            if corners == 0:
                continue
            source = torch.from_numpy(m.faces.reshape(-1).astype(np.int64)).cuda()
            payload = torch.arange(corners, dtype=torch.int32, device="cuda")
            keys, vals = [torch.empty_like(source) for _ in range(2)], [torch.empty_like(payload) for _ in range(2)]
            side, passes, sort_ms, call_ms = C.c_int(0), C.c_int(0), [], []
            for k in range(8):   # the first is the warm-up
                keys[0].copy_(source)
                vals[0].copy_(payload)
                torch.cuda.synchronize()
                t = time.perf_counter()
                rc = sort_pairs(keys[0].data_ptr(), keys[1].data_ptr(), vals[0].data_ptr(), vals[1].data_ptr(), corners, C.byref(side), C.byref(passes))
                torch.cuda.synchronize()
                sort_ms.append(1e3 * (time.perf_counter() - t))
                assert rc == 0
                m.with_vertex_normals().close()
                call_ms.append(views_ms())
            a, b = statistics.median(sort_ms[1:]), statistics.median(call_ms[1:])
            print("    %-40s sort_pairs of its %d corners alone: median %9.3f ms in %d passes of 8; the whole call, library's own time: median %9.3f ms; "
                  "the sort's share %.0f %%" % (name + ": with_vertex_normals()", corners, a, passes.value, b, 100.0 * a / b))
        sys.stdout.flush()
        mesh.close()
        welded.close()
        volume.close()


if __name__ == "__main__":
    measure([int(s) for s in option("--sizes", "128,256").split(",")])
