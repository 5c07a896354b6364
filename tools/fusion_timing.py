"""Device fusion (apd_fuse_views_variant) against the reference's sequential host loop on a synthetic ring: time and byte equality.
Usage: python tools/fusion_timing.py [W H views sources] [--variant eth|tat_intermediate|tat_advanced] [--reps N] [--no-check]
(the ETH loop's checker is oracle/fusion_oracle.cpp, the T&T loops' tests/helpers/tat_fusion_ref.cpp)
Every timed call also prints where the library spent it (apd_fusion_last_timing: set-up, views, file).  --reps N: N timed calls after
the warm-up (default 1).  --no-check: without the host loop, to compare two builds of the library on the device side alone."""
import ctypes as C
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import __graft_entry__ as ge
pkg = ge.load_package()
from apd_mvs_amd import pipeline, synth
import test_gpu_dropin_binary as T

args = sys.argv[1:]
variant = "eth"
if "--variant" in args:
    variant = args.pop(args.index("--variant") + 1)
    args.remove("--variant")
reps = 1
if "--reps" in args:
    reps = int(args.pop(args.index("--reps") + 1))
    args.remove("--reps")
check = "--no-check" not in args
if not check:
    args.remove("--no-check")
W, H, V, S = (int(v) for v in (args[0:4] if len(args) > 3 else (1920, 1080, 12, 8)))
scene, results = T._fusion_inputs(synth, pipeline, pkg, W, H, V, S, 0.0005, seed=5)
out = "/tmp/fusion_timing"
os.makedirs(out, exist_ok=True)
from oracle import binding as ob
pipeline.fuse(scene, results, os.path.join(out, "gpu_warm.ply"), variant=variant)
for rep in range(reps):
    t0 = time.time()
    n = pipeline.fuse(scene, results, os.path.join(out, "gpu.ply"), variant=variant)
    t_gpu = time.time() - t0
    ms = [C.c_double() for _ in range(3)]
    pkg.lib().apd_fusion_last_timing(*[C.byref(m) for m in ms])
    print(variant + " device fusion: %d points from %d views of %dx%d with %d sources each in %.2f s; setup_ms %.1f views_ms %.1f file_ms %.1f"
          % (n, V, W, H, S, t_gpu, ms[0].value, ms[1].value, ms[2].value), flush=True)
if not check:
    sys.exit(0)
cams = (type(scene.cameras[0]) * V)(*scene.cameras)
if variant == "eth":
    t0 = time.time()
    n = ob.fuse(cams, scene.images, [results[v].depth for v in range(V)], [results[v].normal for v in range(V)],
                [results[v].weak for v in range(V)], scene.pairs, os.path.join(out, "cpu.ply"))
    t_cpu = time.time() - t0
else:
    import tat_checker
    L = tat_checker.build(ob, out)
    t0 = time.time()
    n, stale = tat_checker.fuse(L, variant, cams, scene.images, [results[v].depth for v in range(V)], [results[v].normal for v in range(V)],
                                scene.pairs, os.path.join(out, "cpu.ply"))
    t_cpu = time.time() - t0
print("sequential host loop (checker): %d points in %.2f s" % (n, t_cpu), flush=True)
same = open(os.path.join(out, "gpu.ply"), "rb").read() == open(os.path.join(out, "cpu.ply"), "rb").read()
print("identical files:", same, " speed-up %.1fx" % (t_cpu / t_gpu))
