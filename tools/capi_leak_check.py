"""Does a handle give back all the device memory it took?  Usage: python tools/capi_leak_check.py [rounds]

Each round: apd_create, apd_upload_mask, apd_upload_views, apd_upload_prior with WEAK pixels, apd_run, apd_download under the
mask, apd_destroy; then shared images (apd_image_create) used by a FIRST_INIT handle, which makes their tiled copies on
demand, and destroyed.  That reaches every lazily allocated buffer of csrc/apd_capi.hip.  Free device memory (hipMemGetInfo)
is read before the loop and after every round: after the last round it must equal the figure after the first one (the first
round may grow the runtime's own pools once)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import __graft_entry__ as ge

pkg = ge.load_package()
from apd_mvs_amd import synth

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 30
W, H, N = 320, 240, 3
WEAK, UNKNOWN = 0, 2


def free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


sc = synth.make_scene(W, H, N, seed=3, textureless=0.25)
imgs = sc.images_numpy()
cams = [pkg.make_camera(sc.K[i], sc.R[i], sc.t[i], W, H, sc.depth_min, sc.depth_max) for i in range(N + 1)]
base = dict(num_images=N + 1, depth_min=0.6 * sc.depth_min, depth_max=1.2 * sc.depth_max, max_iterations=1, seed=11)
first = dict(base, state=pkg.FIRST_INIT, use_APD=0, weak_peak_radius=6)
refine = dict(base, state=pkg.REFINE_INIT, use_APD=1, weak_peak_radius=6, rotate_time=2, ransac_threshold=0.00875)

# the prior of the refinement pass: what a FIRST_INIT pass leaves (K14 marks the WEAK pixels), post-processed like main.cpp:105-115
h = pkg.Handle(W, H, pkg.default_params(**first), device=0)
h.upload_views(cams, imgs)
h.run()
planes, weak, views = h.download()
h.close()
bad = (planes[..., 3] < first["depth_min"]) | (planes[..., 3] > first["depth_max"])
planes[..., 3][bad] = 0
weak[bad] = UNKNOWN
assert int((weak == WEAK).sum()) > 0, "the prior has no WEAK pixel: the weak lists would not be allocated"
ys, xs = np.mgrid[0:H, 0:W]
mask = np.where((0.61 * xs + ys) < 0.47 * (0.61 * W + H), 0, 255).astype(np.uint8)


def one_round():
    h = pkg.Handle(W, H, pkg.default_params(**refine), device=0)
    h.upload_mask(mask)
    h.upload_views(cams, imgs)
    h.upload_prior(planes, views, weak)
    h.run()
    assert h.weak_count > 0
    h.download()
    h.close()
    shared = [pkg.SharedImage(W, H, im, device=0) for im in imgs]
    h = pkg.Handle(W, H, pkg.default_params(**first), device=0)
    h.upload_views_shared(cams, shared)
    h.run()
    h.download()
    h.close()
    for s in shared:
        s.close()


before = free_bytes()
after = []
for r in range(ROUNDS):
    one_round()
    after.append(free_bytes())
print("free device memory: before the loop %d bytes, after round 1 %d, after round %d %d" % (before, after[0], ROUNDS, after[-1]))
print("min / max over rounds 1..%d: %d / %d" % (ROUNDS, min(after), max(after)))
if after[-1] != after[0]:
    print("LEAK: %d bytes over %d rounds" % (after[0] - after[-1], ROUNDS - 1))
    sys.exit(1)
print("OK: nothing is left behind after round 1")
