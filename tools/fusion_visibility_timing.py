"""What the agreeing-sources mask costs the fusions, and what the first apd_points_visibility call costs: apd_fuse_views_opt with
the points asked for on the device (no file), maps on the device, on blocks_641x409 of tests/fusion_cases.py and on a synthetic ring
of 1920 x 1080 views with 10 sources each; `views_ms` of apd_fusion_last_timing per repeat.
Usage: python tools/fusion_visibility_timing.py [--package DIR] [--reps N] [--views V]
--package DIR: the apd-mvs_amd directory of another build of the project (e.g. the parent commit's, built beside this tree) to
load instead of this tree's; a library without apd_points_visibility is timed for the fusion alone."""
import ctypes as C
import importlib.util
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

args = sys.argv[1:]


def option(name, default):
    if name in args:
        value = args.pop(args.index(name) + 1)
        args.remove(name)
        return value
    return default


reps = int(option("--reps", 5))
V_ring = int(option("--views", 12))
package = option("--package", os.path.join(ROOT, "apd-mvs_amd"))
spec = importlib.util.spec_from_file_location("apd_mvs_amd", os.path.join(package, "__init__.py"), submodule_search_locations=[package])
pkg = importlib.util.module_from_spec(spec)
sys.modules["apd_mvs_amd"] = pkg
spec.loader.exec_module(pkg)
from apd_mvs_amd import pipeline, synth
import fusion_cases
import test_gpu_dropin_binary as T

L = pkg.lib()
has_visibility = hasattr(L, "apd_points_visibility")
print("package %s, build id %s, apd_points_visibility: %s" % (package, pkg.build_id(), "yes" if has_visibility else "no"), flush=True)


def timing():
    ms = [C.c_double() for _ in range(3)]
    L.apd_fusion_last_timing(*[C.byref(m) for m in ms])
    return [m.value for m in ms]


def run(label, cams, images, depths, normals, weaks, blocks, pairs):
    V = len(images)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()
    dev = [[up(a, dt) for a in arrs] for arrs, dt in ((images, np.float32), (depths, np.float32), (normals, np.float32), (weaks, np.uint8))]
    dblocks = None if blocks is None else [None if b is None else up(b, np.uint8) for b in blocks]
    torch.cuda.synchronize()
    table = lambda ts: (C.c_void_p * V)(*[None if t is None else t.data_ptr() for t in ts])
    rows = (C.c_int * V)(*[d.shape[0] for d in depths])
    cols = (C.c_int * V)(*[d.shape[1] for d in depths])
    flat = [s for p in pairs for s in p]
    offs = (C.c_int * (V + 1))(*np.cumsum([0] + [len(p) for p in pairs]).tolist())
    idx = (C.c_int * max(len(flat), 1))(*flat)
    for variant, name in ((0, "eth"), (2, "tat_advanced")):
        views_ms, vis_ms = [], []
        for rep in range(reps + 1):
            opt = pkg.default_fusion_options(variant=variant, result_on_device=1)
            n, handle = C.c_longlong(-1), C.c_void_p()
            rc = L.apd_fuse_views_opt(C.byref(opt), 0, V, cams, table(dev[0]), 1, table(dev[1]), table(dev[2]), table(dev[3]),
                                      None if dblocks is None else table(dblocks), rows, cols, offs, idx, 1, None, C.byref(n), C.byref(handle))
            assert rc == 0, L.apd_fusion_last_error()
            t = timing()
            entries = 0
            if has_visibility:
                o, w = C.c_void_p(), C.c_void_p()
                t0 = time.perf_counter()
                rc = L.apd_points_visibility(handle, C.byref(o), C.byref(w))   # ends in a device synchronisation
                ms = 1e3 * (time.perf_counter() - t0)
                assert rc == 0, L.apd_fusion_last_error()
                last = torch.empty(1, dtype=torch.int64, device="cuda")
                L.apd_device_memcpy(0, last.data_ptr(), o.value + 8 * n.value, 8)
                entries = int(last[0])
                if rep:
                    vis_ms.append(ms)
            L.apd_points_destroy(handle)
            if rep:   # rep 0 warms up
                views_ms.append(t[1])
        print("%s %s: %d points; views_ms %s; min %.2f max %.2f mean %.2f" % (label, name, n.value, " ".join("%.2f" % m for m in views_ms),
                                                                            min(views_ms), max(views_ms), float(np.mean(views_ms))), flush=True)
        if vis_ms:
            # read: sources + view per point in both passes; written: one offset per point and the entries
            moved = n.value * (2 * 8 + 8) + entries * 4
            m = float(np.median(vis_ms))
            print("%s %s: first apd_points_visibility %s ms; median %.3f ms = %.0f Mpoints/s; %d entries, %.1f MB moved, %.1f GB/s"
                  % (label, name, " ".join("%.3f" % v for v in vis_ms), m, n.value / m / 1e3, entries, moved / 1e6, moved / m / 1e6), flush=True)


case = fusion_cases.case("blocks_641x409")
run("blocks_641x409", case.cameras(pkg.make_camera), case.images, case.depths, case.normals, case.weaks, case.blocks, case.pairs)
scene, results = T._fusion_inputs(synth, pipeline, pkg, 1920, 1080, V_ring, 10, 0.0005, seed=5)
cams = (type(scene.cameras[0]) * V_ring)(*scene.cameras)
run("ring_1920x1080_%dviews_10src" % V_ring, cams, [scene.images[v] for v in range(V_ring)], [results[v].depth for v in range(V_ring)],
    [results[v].normal for v in range(V_ring)], [results[v].weak for v in range(V_ring)], None, scene.pairs)
