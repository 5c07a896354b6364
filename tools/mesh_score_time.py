#!/usr/bin/env python3
"""What scoring a mesh against a cloud costs (apd_mesh_score, apd_mesh_nearest: contract C27), beside apd_points_score of the mesh's
vertices against the same cloud at the same threshold in the same run: the same 27-cell walk with a point test in place of the
triangle test.  Two device-resident meshes: a jittered sheet of about a million faces (tools/mesh_render_time.py's) and the mesh
pipeline.mesh extracts from the small synthetic scene of the tests at voxel 0.05; the truth is the mesh's own samples.  Not part of
bench.py; needs a GPU.

  tools/mesh_score_time.py             1 warm-up round, then 5 rounds that alternate the calls; per call the median, the minimum and the
                                       maximum of the host clock around the library call; for apd_mesh_nearest also the medians of the pair
                                       build, the sorts and the search kernel (apd_fusion_last_timing); and, counted on the host, the
                                       (cell, face) pairs per face and the candidates evaluated per query for both searches
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


def cells(xyz, size):
    return np.floor(xyz.astype(np.float32) / np.float32(size)).astype(np.int64)


def key(c):
    return ((c[..., 2] + (1 << 20)) << 42) | ((c[..., 1] + (1 << 20)) << 21) | (c[..., 0] + (1 << 20))


def around(query_cells, keys, counts):
    """per query the sum of counts[k] over the 27 cells around it; keys ascending."""
    total = np.zeros(len(query_cells), np.int64)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                want = key(query_cells + np.array([dx, dy, dz]))
                at = np.minimum(np.searchsorted(keys, want), len(keys) - 1)
                total += np.where(keys[at] == want, counts[at], 0)
    return total


def margin(t):
    return 2.0 ** -21 * (np.abs(t.astype(np.float64)) + 2.0)


def work(vertices, faces, truth, tau):
    """(pairs per face, face candidates per truth point, vertex candidates per truth point), origin 0: the cells a face is binned
    into as csrc/apd_mesh_nearest_math.h has them (mesh_cell_range)."""
    corner = vertices.astype(np.float32)[faces]
    least, most = corner.min(1), corner.max(1)
    t_lo, t_hi = least / np.float32(tau), most / np.float32(tau)
    lo, hi = np.floor(t_lo).astype(np.int64), np.floor(t_hi).astype(np.int64)
    lo -= (t_lo.astype(np.float64) - lo <= margin(t_lo)).astype(np.int64)
    hi += (t_hi.astype(np.float64) - hi >= 1.0 - margin(t_hi)).astype(np.int64)
    extent = hi - lo + 1
    per_face = extent.prod(1)
    pair_keys = []
    for dz in range(int(extent[:, 2].max())):   # the pairs themselves, as the device emits them
        for dy in range(int(extent[:, 1].max())):
            for dx in range(int(extent[:, 0].max())):
                has = (extent[:, 0] > dx) & (extent[:, 1] > dy) & (extent[:, 2] > dz)
                pair_keys.append(key(lo[has] + np.array([dx, dy, dz])))
    keys, counts = np.unique(np.concatenate(pair_keys), return_counts=True)
    q = cells(truth, tau)
    vkeys, vcounts = np.unique(key(cells(vertices, tau)), return_counts=True)
    return per_face.mean(), around(q, keys, counts).mean(), around(q, vkeys, vcounts).mean()


def time_mesh(pkg, name, mesh, tau, count_work):
    import torch
    L = pkg.lib()
    ms = (C.c_double * 3)()
    truth = mesh.sample_points(1.0 / (tau * tau), seed=1)
    n = len(mesh.vertices)
    vertices = pkg.Points.from_arrays(mesh.vertices, np.zeros((n, 3), np.float32), np.zeros((n, 3), np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.int32),
                                      np.zeros(n, np.int32), np.zeros(n, np.uint32), [1], [1], [[]], on_device=True)
    calls = (("apd_mesh_score", lambda: mesh.score(truth, tau)), ("apd_mesh_nearest of the truth", lambda: mesh.nearest(truth, tau)),
             ("apd_mesh_sample_points, 4 / tau^2", lambda: mesh.sample_points(4.0 / (tau * tau))),
             ("apd_points_score of the vertices", lambda: vertices.score(truth, tau)))
    times = {label: [] for label, _ in calls}
    parts = []
    results = {}
    for round_ in range(6):   # the first is the warm-up
        for label, call in calls:
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = call()
            took = 1e3 * (time.perf_counter() - t)
            L.apd_fusion_last_timing(C.byref(ms, 0), C.byref(ms, 8), C.byref(ms, 16))
            if label.startswith("apd_mesh_nearest") and round_ > 0:
                parts.append(list(ms))
            if hasattr(out, "close"):
                results[label] = len(out)
                out.close()
            elif hasattr(out, "fscore"):
                results[label] = out
            if round_ > 0:
                times[label].append(took)
    print("%s: %d vertices, %d faces, threshold %g, truth: %d of its own samples" % (name, n, len(mesh.faces), tau, len(truth)))
    for label, _ in calls:
        print("    %-36s call ms: median %9.3f  min %9.3f  max %9.3f" % (label, statistics.median(times[label]), min(times[label]), max(times[label])))
    print("    apd_mesh_nearest's parts, medians:   pair build %.3f ms, sorts (pairs and queries) %.3f ms, search kernel %.3f ms" % tuple(
        statistics.median(p[k] for p in parts) for k in range(3)))
    s, p = results["apd_mesh_score"], results["apd_points_score of the vertices"]
    print("    mesh score:   n_p %d precision %.4f recall %.4f fscore %.4f mean_p %.3g mean_q %.3g" % (s.n_p, s.precision, s.recall, s.fscore, s.mean_p, s.mean_q))
    print("    vertex score: n_p %d precision %.4f recall %.4f fscore %.4f mean_p %.3g mean_q %.3g" % (p.n_p, p.precision, p.recall, p.fscore, p.mean_p, p.mean_q))
    if count_work:
        per_face, face_candidates, vertex_candidates = work(mesh.vertices, mesh.faces, truth.xyz.cpu().numpy(), tau)
        print("    %.2f (cell, face) pairs per face; per truth point %.1f faces evaluated by apd_mesh_nearest, %.1f vertices tested by apd_points_score's "
              "recall side" % (per_face, face_candidates, vertex_candidates))
    sys.stdout.flush()
    truth.close()
    vertices.close()


def measure(side, with_scene):
    import __graft_entry__ as ge
    pkg = ge.load_package()
    assert pkg.device_count() >= 1, "no HIP device visible"
    from test_mesh import sheet
    host = sheet(side, side - 4, 0.2)
    big = pkg.Mesh.from_arrays(host.vertices, host.faces)
    time_mesh(pkg, "sheet", big, 0.5, True)
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
        time_mesh(pkg, "the synthetic scene's mesh", found, 0.05, True)
        found.close()


if __name__ == "__main__":
    option = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    measure(int(option("--side", "710")), "--no-scene" not in sys.argv)
