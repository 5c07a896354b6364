"""Randomised check of a device fusion against its sequential loop (ETH: oracle/fusion_oracle.cpp; Tanks and Temples:
tests/helpers/tat_fusion_ref.cpp) on the cases of tests/fusion_cases.random_case: random sizes down to one pixel, view counts,
shuffled or duplicated source lists, a half-resolution view, holes and zero bands, non-finite depths, colour or grey images,
block masks; through the C ABI with maps on the host and on the device.  The PLY files must be byte-identical but for the
sign and payload of NaN coordinates.
Usage: python tools/fusion_fuzz.py [--variant eth|tat_intermediate|tat_advanced] [cases] [first_seed]"""
import argparse, os, pathlib, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge
pkg = ge.load_package()
from oracle import binding as ob
import fusion_cases
import tat_checker
from test_fusion_cases import reference
from test_gpu_fusion_scale import _assert_same_ply, _device

ap = argparse.ArgumentParser()
ap.add_argument("--variant", default="eth", choices=["eth", "tat_intermediate", "tat_advanced"])
ap.add_argument("cases", nargs="?", type=int, default=20)
ap.add_argument("first_seed", nargs="?", type=int, default=0)
args = ap.parse_args()
out = pathlib.Path(tempfile.mkdtemp(prefix="fusion_fuzz_"))
checker = tat_checker.build(ob, out) if args.variant != "eth" else None
bad = 0
t0 = time.time()
for seed in range(args.first_seed, args.first_seed + args.cases):
    case = fusion_cases.random_case(seed)
    n_ref = reference(ob, checker, case, args.variant, out / "ref.ply")
    label = "seed %d: %s sources=%s points=%d tags=%s" % (seed, "/".join("%dx%d" % (d.shape[1], d.shape[0]) for d in case.depths),
                                                          [len(p) for p in case.pairs], n_ref, ",".join(sorted(case.tags)))
    try:
        for on_device in (False, True):
            assert _device(pkg, ob, case, args.variant, out / "gpu.ply", on_device) == n_ref, "count (on_device=%d)" % on_device
            _assert_same_ply(out / "gpu.ply", out / "ref.ply", nan_bits_may_differ=True)
        print("ok   " + label, flush=True)
    except AssertionError as e:
        bad += 1
        print("FAIL " + label + ": " + str(e)[:300], flush=True)
print("%s: %d case(s), %d failure(s), %.0f s" % (args.variant, args.cases, bad, time.time() - t0))
sys.exit(1 if bad else 0)
