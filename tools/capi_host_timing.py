"""Host-side wall time of a handle's life without a kernel of the pass: apd_create + apd_upload_views + apd_upload_prior +
apd_destroy.  Usage: python tools/capi_host_timing.py [W H sources reps]   (default 1920 1080 10 5)

Prints one line per repetition and the median / min / max, in ms.  The first handle of the process is created and destroyed
before the clock starts (it pays for loading the code objects)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import __graft_entry__ as ge

pkg = ge.load_package()
from apd_mvs_amd import synth

W, H, N, REPS = (int(v) for v in sys.argv[1:5]) if len(sys.argv) > 4 else (1920, 1080, 10, 5)
sc = synth.make_scene(W, H, N, seed=3, textureless=0.2)
imgs = sc.images_numpy()
cams = [pkg.make_camera(sc.K[i], sc.R[i], sc.t[i], W, H, sc.depth_min, sc.depth_max) for i in range(N + 1)]
kw = dict(num_images=N + 1, depth_min=0.6 * sc.depth_min, depth_max=1.2 * sc.depth_max, state=pkg.REFINE_INIT, use_APD=1, seed=11)
rng = np.random.default_rng(5)
planes = rng.standard_normal((H, W, 4)).astype(np.float32)
views = rng.integers(0, 1 << N, (H, W)).astype(np.uint32)
weak = rng.integers(0, 3, (H, W)).astype(np.uint8)   # a third of the pixels WEAK: the index map, the neighbour table, the lists


def life():
    h = pkg.Handle(W, H, pkg.default_params(**kw), device=0)
    h.upload_views(cams, imgs)
    h.upload_prior(planes, views, weak)
    h.close()


life()
ms = []
for r in range(REPS):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    life()
    ms.append(1e3 * (time.perf_counter() - t0))
    print("rep %d: %.2f ms" % (r, ms[-1]), flush=True)
print("create+upload_views+upload_prior+destroy %dx%d, %d sources: median %.2f ms, min %.2f, max %.2f (max - min %.2f)"
      % (W, H, N, float(np.median(ms)), min(ms), max(ms), max(ms) - min(ms)))
