"""Named cases off the parameter values one reference schedule produces: 19 to 31 source views through every pass kind, and
top_k, rotate_time = 1, geom_factor, max_iterations = 6 and depth ranges without a distance cut.  tests/test_param_space_cases.py
runs the ORACLE ALONE on every case and asserts that the case can catch a kernel that ignores the parameter;
tests/test_gpu_param_space.py compares the HIP path with the oracle on the same cases after every kernel.

A case is a scene (size, N, scene seed, textureless share, 8-bit or non-integer images), the parameter dicts of its passes in
order -- each pass starts from common.postprocess of the one before -- and the kernels stepped in its LAST pass (None: the
whole schedule of frame_limits_cases.schedule).  A variation case names the field it moves off its default (`vary`) and the
default it is compared with; the passes before the last one are the same in both and only build the prior."""
import numpy as np

import common
import frame_limits_cases as fl

# the per-pass parameters of main.cpp:168-215 as tests/test_gpu_parity.py::test_three_pass_pipeline_with_apd_and_geometric_term
# states them
FIRST = dict(state=0, use_APD=0, weak_peak_radius=6)
APD = dict(state=1, use_APD=1, weak_peak_radius=6, rotate_time=2, ransac_threshold=0.01 - 0.00125)
GEOM = dict(state=2, use_APD=1, weak_peak_radius=4, rotate_time=4, ransac_threshold=0.01 - 0.0025, geom_consistency=1)


class Case:
    def __init__(self, name, W, H, N, scene_seed, textureless, passes, kernels=None, floats=False, vary=None, default=None, nans=False):
        self.name, self.W, self.H, self.N = name, W, H, N
        self.scene_seed, self.textureless, self.floats = scene_seed, textureless, floats
        self.passes = [dict(p) for p in passes]
        self.kernels = kernels       # of the last pass; None: fl.schedule(max_iterations, weak_count > 0)
        self.vary = vary             # the field of the last pass this case moves
        # the oracle leaves NaN words (their sign and payload differ between x86 and gfx950: compared with common.canon_nan)
        self.nans = nans
        self.default = default       # ... and the value the oracle-alone test compares it with ("depth_range": base_params' range)

    def __repr__(self):
        return self.name


_SCENES = {}


def scene(synth, case):
    """(scene, images, depth maps), made once per (size, N, seed, share, image kind) and never written to."""
    key = (case.W, case.H, case.N, case.scene_seed, case.textureless, case.floats)
    if key not in _SCENES:
        sc, imgs = common.scene_inputs(synth, case.W, case.H, case.N, seed=case.scene_seed, textureless=case.textureless)
        if case.floats:
            imgs = fl.float_images(imgs)
        _SCENES[key] = (sc, imgs, common.fake_depth_maps(case.W, case.H, case.N + 1))
    return _SCENES[key]


def pass_params(case, sc, pi, default=False):
    """Parameters of pass `pi`; default=True: the last pass with the varied field back at its default."""
    p = common.base_params(sc, case.N, **case.passes[pi])
    if pi == len(case.passes) - 1 and case.vary is not None:
        if case.vary == "depth_range":
            if not default:
                p["depth_min"], p["depth_max"] = depth_range(case, sc)
        elif default:
            p[case.vary] = case.default
    return p


def steps(case, pi, params, weak_count):
    """(kernel id, iteration) of pass `pi` in launch order."""
    if pi == len(case.passes) - 1 and case.kernels is not None:
        return list(case.kernels)
    return fl.schedule(params["max_iterations"], weak_count > 0)


def _three(seed, iters=2, **last):
    """The three pass kinds with one seed and iteration count; `last` overrides fields of the geometric pass."""
    return [dict(FIRST, seed=seed, max_iterations=iters), dict(APD, seed=seed, max_iterations=iters),
            dict(GEOM, seed=seed, max_iterations=iters, **last)]


# ---- 19 to 31 source views: the NMAX = 32 instantiations of K6/K7 and K9/K10, the fourth word of ViewWeights<32>, K14's
# (sample, lane)-pair walk and K15 with more than 18 selected views; every pass of these cases is stepped and compared ---------
# W, H, scene seed, textureless share: 2.5 x 3.75 checkerboard tiles of 32 x 16 and 5 x 3.75 full-frame tiles of 16 x 16, no axis a
# multiple of either.  Shrunk from 96 x 72 while test_param_space_cases.py holds: 72 x 56 leaves 60 WEAK pixels at N = 31 (the bound
# is 50), 64 x 48 leaves 35
VIEW_FRAME = (80, 60, 3, 0.25)


def _views(N, floats=False):
    W, H, seed, share = VIEW_FRAME
    return Case("views%d%s" % (N, "_float" if floats else ""), W, H, N, seed, share, _three(61), floats=floats)


VIEW_CASES = [_views(19), _views(24), _views(31), _views(31, floats=True)]

# ---- top_k: K5's arms top_k <= 0, 1, below / at / above the number of valid views (APD.cu:616-662), FIRST_INIT, K1..K8.  With no
# view selected the sweep divides a zero cost sum by a zero weight sum: top_k <= 0 leaves NaN costs after K6 ---------------------------
TOP_K_KERNELS = [(1, 0), (2, 0), (5, 0), (6, 0), (7, 0), (8, 0)]
TOP_K_CASES = [Case("top_k=%d" % k, 72, 56, 5, 1, 0.0, [dict(FIRST, seed=23, max_iterations=1, top_k=k)], kernels=TOP_K_KERNELS,
                    vary="top_k", default=4, nans=k <= 0) for k in (0, -3, 1, 2, 5, 10)]

# ---- rotate_time = 1: one ray per direction and the widest jitter range (8) of K3's jittered arm; the REFINE_INIT pass of the
# 96 x 72, N = 4 scene of test_three_pass_pipeline_with_apd_and_geometric_term, whole pass ---------------------------------------
ROTATE_CASES = [Case("rotate_time=1 thr=%g" % thr, 96, 72, 4, 3, 0.25,
                     [dict(FIRST, seed=11, max_iterations=2), dict(APD, seed=11, max_iterations=2, rotate_time=1, ransac_threshold=thr)],
                     vary="rotate_time", default=4) for thr in (0.005, 0.00875)]

# ---- geom_factor: zero (the geometric term vanishes), negative (the refinement bound of K9/K10 and K15 is switched off), large --
GEOM_FACTOR_CASES = [Case("geom_factor=%g" % g, 96, 72, 4, 3, 0.25, _three(11, geom_factor=g), vary="geom_factor", default=0.2)
                     for g in (0.0, -0.2, 1.5)]

# ---- max_iterations = 6: select_views thresholds with exp_poly(iter^2 / -90) and the windows move with the iteration -----------
ITER_CASES = [Case("max_iterations=6", 64, 48, 3, 1, 0.0, [dict(FIRST, seed=7, max_iterations=6)], vary="max_iterations", default=3)]

# ---- depth ranges for which ransac_distance_cut finds no cut: K3 divides by depth_max - depth_min == 0 (no inlier: x / 0 is
# never below the threshold) or < 0 (every point an inlier).  depth_max == depth_min sits inside the scene's range ------------------
DEPTH_CASES = [Case("depth_max==depth_min", 96, 72, 4, 3, 0.25, [dict(FIRST, seed=11, max_iterations=2), dict(APD, seed=11, max_iterations=2)],
                    vary="depth_range"),
               Case("depth_max<depth_min", 96, 72, 4, 3, 0.25, [dict(FIRST, seed=11, max_iterations=2), dict(APD, seed=11, max_iterations=2)],
                    vary="depth_range")]


def depth_range(case, sc):
    """(depth_min, depth_max) of the last pass of a DEPTH_CASES entry, as binary32 values."""
    lo, hi = np.float32(0.6 * sc.depth_min), np.float32(1.2 * sc.depth_max)
    if case.name == "depth_max==depth_min":
        mid = np.float32(0.5) * (lo + hi)
        return float(mid), float(mid)
    return float(hi), float(lo)


VARIATION_CASES = TOP_K_CASES + ROTATE_CASES + GEOM_FACTOR_CASES + ITER_CASES + DEPTH_CASES
ALL_CASES = VIEW_CASES + VARIATION_CASES
