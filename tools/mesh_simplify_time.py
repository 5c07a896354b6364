#!/usr/bin/env python3
"""What simplifying a mesh costs beside the cleaning calls: Mesh.simplify with both placements at cells of 2 and 4 voxels on the mesh
Volume.extract_mesh takes from "full_frame" of tests/fusion_cases.py, on the two grids of tools/mesh_time.py (whose method this
follows), the counts after, and which share of the call its four sorts are.  Not part of bench.py; needs a GPU.

  tools/mesh_simplify_time.py                 per grid 1 warm-up round, then 7 rounds that alternate the calls; the median, the
                                              minimum and the maximum of the host clock around each call (the library call, which
                                              ends in a device synchronise, and the download of the new mesh into numpy), beside it
                                              the library's own "views" time of the last round (apd_fusion_last_timing); then the
                                              library's sort_pairs alone on the keys the call sorts -- the vertices by cell, the
                                              faces by the last entry of their rotated triple and then by its first two, the corners
                                              by cluster --, made here with numpy
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
    from test_mesh_simplify import np_keys, np_rotated
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

    # the Itanium mangling of apd_sort::sort_pairs, as in tools/mesh_time.py
    sort_pairs = getattr(L, "_ZN8apd_sort10sort_pairsEPmS0_PjS1_mPiS2_")
    sort_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]

    def sort_alone(keys_np):
        """(median ms, passes) of sort_pairs on these keys with the payload 0 .. n - 1."""
        source = torch.from_numpy(keys_np.astype(np.int64)).cuda()
        payload = torch.arange(len(keys_np), dtype=torch.int32, device="cuda")
        keys, vals = [torch.empty_like(source) for _ in range(2)], [torch.empty_like(payload) for _ in range(2)]
        side, passes, took = C.c_int(0), C.c_int(0), []
        for k in range(8):   # the first is the warm-up
            keys[0].copy_(source)
            vals[0].copy_(payload)
            torch.cuda.synchronize()
            t = time.perf_counter()
            rc = sort_pairs(keys[0].data_ptr(), keys[1].data_ptr(), vals[0].data_ptr(), vals[1].data_ptr(), len(keys_np), C.byref(side), C.byref(passes))
            torch.cuda.synchronize()
            took.append(1e3 * (time.perf_counter() - t))
            assert rc == 0
        return statistics.median(took[1:]), passes.value

    for size in sizes:
        voxel = float((hi - lo).max()) / (size - 1)
        volume = pkg.Volume.around(lo, hi, voxel, 4 * voxel, margin=0.0, colour=True)
        volume.integrate(cams, depths, images, maps_on_device=True)
        mesh = volume.extract_mesh()
        volume_dims, samples = volume.dims, volume.samples
        volume.close()
        todo = [("with_vertex_normals()", lambda: mesh.with_vertex_normals().close())]
        for cells in (2, 4):
            for placement in ("mean", "quadric"):
                todo.append(("simplify(%d voxels, %s)" % (cells, placement), lambda c=cells, p=placement: mesh.simplify(c * voxel, placement=p).close()))
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
        print("grid %d x %d x %d = %d samples, voxel %.5f: %d vertices, %d faces" % (volume_dims + (samples, voxel, len(mesh.vertices), len(mesh.faces))))
        for what, _ in todo:
            print("    %-40s call ms: median %9.3f  min %9.3f  max %9.3f   library's own time of the last round %9.3f" % (
                what, statistics.median(times[what]), min(times[what]), max(times[what]), device[what]))
        for cells in (2, 4):
            cell = np.float32(cells * voxel)
            small = mesh.simplify(cell)
            inside, key = np_keys(mesh.vertices, cell)
            keys, cluster_of_inside = np.unique(key[inside], return_inverse=True)
            cluster_of = np.full(len(mesh.vertices), -1, np.int64)
            cluster_of[inside] = cluster_of_inside
            mapped = cluster_of[mesh.faces]
            live = (mapped >= 0).all(1) & (mapped[:, 0] != mapped[:, 1]) & (mapped[:, 0] != mapped[:, 2]) & (mapped[:, 1] != mapped[:, 2])
            rotated = np_rotated(mapped)
            first_key = np.where(live, rotated[:, 2], -1)
            order = np.argsort(first_key.astype(np.uint64), kind="stable")
            second_key = np.where(live, (rotated[:, 0] << 32) | rotated[:, 1], -1)[order]
            corner_key = np.where((mapped >= 0).all(1)[:, None], mapped, -1).reshape(-1)
            members = np.bincount(cluster_of_inside)
            per_cluster = np.bincount(corner_key[corner_key >= 0], minlength=len(keys))
            parts = [("vertices by cell", key[inside]), ("faces, last entry", first_key), ("faces, first two", second_key), ("corners by cluster", corner_key)]
            total, told = 0.0, []
            for name, k in parts:
                took, passes = sort_alone(k)
                total += took
                told.append("%s %.3f ms in %d passes" % (name, took, passes))
            whole = []
            for _ in range(7):
                mesh.simplify(cell).close()
                whole.append(views_ms())
            print("    simplify(%d voxels, quadric): %d clusters -> %d vertices, %d faces; members per cluster: mean %.1f, max %d; corners per cluster: mean %.1f, "
                  "max %d" % (cells, len(keys), len(small.vertices), len(small.faces), members.mean(), members.max(), per_cluster.mean(), per_cluster.max()))
            print("        sort_pairs alone: %s; together %.3f ms; the whole call, library's own time: median %.3f ms; the sorts' share %.0f %%" % (
                "; ".join(told), total, statistics.median(whole), 100.0 * total / statistics.median(whole)))
            small.close()
        sys.stdout.flush()
        mesh.close()


if __name__ == "__main__":
    measure([int(s) for s in option("--sizes", "128,256").split(",")])
