"""The geometric filter (apd_filter_views) against the ETH fusion (apd_fuse_views_opt) on the same device-resident maps of a synthetic
ring, from one process: where each call spent its time (apd_fusion_last_timing).
Usage: python tools/filter_timing.py [W H views sources] [--reps N]
With maps and outputs on the device the filter's `views` time is its kernels and the one wait behind them: one launch per view, no
copy, no host synchronisation in between.  The fusion returns its points on the device and writes no file, so its `views` time is
kernels, consumption rounds and compaction."""
import ctypes as C
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import __graft_entry__ as ge
pkg = ge.load_package()
from apd_mvs_amd import pipeline, synth
import test_gpu_dropin_binary as T

args = sys.argv[1:]
reps = 3
if "--reps" in args:
    reps = int(args.pop(args.index("--reps") + 1))
    args.remove("--reps")
W, H, V, S = (int(v) for v in (args[0:4] if len(args) > 3 else (1920, 1080, 24, 10)))
scene, results = T._fusion_inputs(synth, pipeline, pkg, W, H, V, S, 0.0005, seed=5)
L = pkg.lib()
up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()
imgs = [up(scene.images[v], np.float32) for v in range(V)]
deps = [up(results[v].depth, np.float32) for v in range(V)]
nors = [up(results[v].normal, np.float32) for v in range(V)]
weaks = [up(results[v].weak, np.uint8) for v in range(V)]
outs = [[torch.empty((H, W), dtype=dt, device="cuda") for _ in range(V)] for dt in (torch.float32, torch.uint8, torch.float32)]
torch.cuda.synchronize()
table = lambda ts: (C.c_void_p * V)(*[t.data_ptr() for t in ts])
cams = (type(scene.cameras[0]) * V)(*scene.cameras)
rows, cols = (C.c_int * V)(*[H] * V), (C.c_int * V)(*[W] * V)
flat = [s for p in scene.pairs for s in p]
offs = (C.c_int * (V + 1))(*np.cumsum([0] + [len(p) for p in scene.pairs]).tolist())
idx = (C.c_int * len(flat))(*flat)


def timing():
    ms = [C.c_double() for _ in range(3)]
    L.apd_fusion_last_timing(*[C.byref(m) for m in ms])
    return [m.value for m in ms]


print("%d views of %dx%d, %d sources each, maps on the device" % (V, W, H, S), flush=True)
for rep in range(reps + 1):
    tag = "warm-up" if rep == 0 else "rep %d" % rep
    opt = pkg.default_fusion_options()
    rc = L.apd_filter_views(C.byref(opt), 0, V, cams, table(deps), table(nors), table(weaks), None, rows, cols, offs, idx, 1,
                            table(outs[0]), table(outs[1]), table(outs[2]), 1)
    assert rc == 0, L.apd_fusion_last_error()
    t = timing()
    kept = sum(int((d > 0).sum()) for d in outs[0])
    print("%-8s apd_filter_views: setup_ms %.2f views_ms %.2f (%.3f ms per view; %.1f Gpixel-sources/s); %d pixels kept"
          % (tag, t[0], t[1], t[1] / V, V * W * H * S / t[1] / 1e6, kept), flush=True)
    opt = pkg.default_fusion_options(result_on_device=1)
    n, handle = C.c_longlong(-1), C.c_void_p()
    rc = L.apd_fuse_views_opt(C.byref(opt), 0, V, cams, table(imgs), 1, table(deps), table(nors), table(weaks), None, rows, cols, offs, idx, 1, None,
                              C.byref(n), C.byref(handle))
    assert rc == 0, L.apd_fusion_last_error()
    t = timing()
    L.apd_points_destroy(handle)
    print("%-8s apd_fuse_views_opt (ETH, points on the device, no file): setup_ms %.2f views_ms %.2f; %d points" % (tag, t[0], t[1], n.value),
          flush=True)
