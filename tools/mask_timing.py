#!/usr/bin/env python3
"""Whole-pass and K6/K7, K9/K10, K14 times of a REFINE_INIT pass with adaptive patches under per-view pixel masks
(apd_upload_mask), for any build of the library -- an older one without the entry point can run the unmasked case, which is
how the no-mask cost of the feature is measured (same command, two libraries, alternated).

  python tools/mask_timing.py LIB.so W H N [reps] [variant ...]     variants: none band30 disc40 speckle50 (default: none)

band30: the top 30 % of the frame masked (sky); disc40: a centred disc that leaves 40 % live (object scan); speckle50: every
other pixel of a bit pattern of the coordinates (no wave fully masked: the worst case).  The prior of the timed pass is an unmasked
FIRST_INIT pass of the same library."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import __graft_entry__ as ge

pkg = ge.load_package()   # structs, camera helper and the scene generator only: the library under test is loaded below
from apd_mvs_amd import synth


def make_mask(variant, W, H):
    ys, xs = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
    if variant == "band30":
        out = ys < int(0.3 * H)
    elif variant == "disc40":
        r2 = 0.4 * W * H / np.pi
        out = ((xs - W / 2) ** 2 + (ys - H / 2) ** 2).to(torch.float32) >= r2
    elif variant == "speckle50":
        out = ((xs ^ (ys >> 1) ^ (xs >> 2)) & 1) == 0
    else:
        raise KeyError(variant)
    return torch.where(out, 0, 255).to(torch.uint8).contiguous()


def main():
    lib_path, W, H, N = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
    reps = int(sys.argv[5]) if len(sys.argv) > 5 else 2
    variants = sys.argv[6:] or ["none"]
    L = C.CDLL(os.path.abspath(lib_path))
    V = C.c_void_p
    L.apd_default_params.argtypes = [C.POINTER(pkg.Params)]
    L.apd_create.argtypes = [C.POINTER(V), C.c_int, C.c_int, C.c_int, C.POINTER(pkg.Params)]
    L.apd_reset.argtypes = [V, C.POINTER(pkg.Params)]
    L.apd_destroy.argtypes = [V]
    L.apd_upload_views.argtypes = [V, C.c_int, C.POINTER(pkg.Camera), C.POINTER(V), C.POINTER(V)]
    L.apd_upload_prior.argtypes = [V, V, V, V]
    L.apd_run.argtypes = [V]
    L.apd_synchronize.argtypes = [V]
    L.apd_export_state_device.argtypes = [V, V, V, V, V]
    L.apd_profile_enable.argtypes = [V, C.c_int]
    L.apd_profile_reset.argtypes = [V]
    L.apd_profile_get.argtypes = [V, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)]
    L.apd_weak_count.argtypes = [V]
    L.apd_last_error.restype = C.c_char_p
    L.apd_build_id.restype = C.c_char_p
    has_masks = hasattr(L, "apd_upload_mask")
    if has_masks:
        L.apd_upload_mask.argtypes = [V, V]
        L.apd_masked_count.argtypes = [V]

    def check(rc):
        if rc != 0:
            raise RuntimeError("apd error %d: %s" % (rc, L.apd_last_error().decode()))

    sc = synth.make_scene(W, H, N, seed=3, textureless=0.2, device="cuda")
    cams = (pkg.Camera * (N + 1))(*[pkg.make_camera(sc.K[i], sc.R[i], sc.t[i], W, H, sc.depth_min, sc.depth_max) for i in range(N + 1)])
    imgs = [im.to(torch.float32).contiguous() for im in sc.images]
    ip = (V * (N + 1))(*[im.data_ptr() for im in imgs])

    def params(**kw):
        p = pkg.Params()
        L.apd_default_params(C.byref(p))
        for k, v in dict(num_images=N + 1, depth_min=0.6 * sc.depth_min, depth_max=1.2 * sc.depth_max, max_iterations=3, **kw).items():
            setattr(p, k, v)
        return p

    h = V()
    check(L.apd_create(C.byref(h), 0, W, H, C.byref(params(state=0, use_APD=0, weak_peak_radius=6, seed=5))))
    check(L.apd_upload_views(h, N + 1, cams, ip, None))
    check(L.apd_run(h))
    planes = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    weak = torch.empty((H, W), dtype=torch.uint8, device="cuda")
    views = torch.empty((H, W), dtype=torch.int32, device="cuda")
    check(L.apd_export_state_device(h, planes.data_ptr(), weak.data_ptr(), views.data_ptr(), None))
    print("library %s (build id %s), %dx%d, %d sources; prior: %s WEAK/STRONG/UNKNOWN" %
          (lib_path, L.apd_build_id().decode(), W, H, N, torch.bincount(weak.reshape(-1).to(torch.int64), minlength=3).tolist()), flush=True)
    p1 = params(state=1, use_APD=1, weak_peak_radius=6, rotate_time=4, ransac_threshold=0.01 - 0.00125 * 3, seed=6)
    for variant in variants:
        mask = None if variant == "none" else make_mask(variant, W, H)
        if mask is not None and not has_masks:
            raise RuntimeError("this library has no apd_upload_mask")
        for rep in range(reps + 1):   # the first repetition warms up and is not printed
            check(L.apd_reset(h, C.byref(p1)))
            check(L.apd_upload_views(h, N + 1, cams, ip, None))
            check(L.apd_upload_prior(h, planes.data_ptr(), views.data_ptr(), weak.data_ptr()))
            masked = 0
            if mask is not None:
                check(L.apd_upload_mask(h, mask.data_ptr()))
                masked = L.apd_masked_count(h)
            check(L.apd_profile_enable(h, 1))
            check(L.apd_profile_reset(h))
            check(L.apd_synchronize(h))
            t0 = time.perf_counter()
            check(L.apd_run(h))
            check(L.apd_synchronize(h))
            wall = (time.perf_counter() - t0) * 1e3
            ms = {}
            for k in range(1, 16):
                t, n = C.c_double(), C.c_int()
                check(L.apd_profile_get(h, k, C.byref(t), C.byref(n)))
                ms[k] = t.value
            if rep > 0:
                print("%-10s rep %d: live %5.1f %%  WEAK %8d  pass %8.1f ms  kernels %8.1f ms  K6+K7 %8.1f  K9+K10 %8.1f  K14 %7.1f  K15 %6.1f" %
                      (variant, rep, 100.0 * (1.0 - masked / float(W * H)), L.apd_weak_count(h), wall, sum(ms.values()), ms[6] + ms[7],
                       ms[9] + ms[10], ms[14], ms[15]), flush=True)
    check(L.apd_destroy(h))


if __name__ == "__main__":
    main()
