"""Named cases off the VALUES a caller uploads: pixel values far from 0..255 (scaled, shifted, negative, flat, saturated, NaN, inf,
past FLT_MAX in a variance product), depth maps with NaN, +-inf, -0.0, denormal, huge and negative entries and maps that are zero
everywhere, and crafted priors (zero, NaN, long and back-facing normals; zero, negative, infinite and out-of-range depths; view words
with no bit or with bits past the last source; WEAK maps without a STRONG pixel, all STRONG, all UNKNOWN, a checkerboard).
tests/test_value_space_cases.py runs the ORACLE ALONE on every case and asserts that the case contains what its name says and moves
what the oracle computes; tests/test_gpu_value_space.py compares the HIP path with the oracle after every kernel.

One scene serves every case: 80 x 60, N = 3, the textureless share of param_space_cases.VIEW_FRAME (scene seed: below), the pass
dicts FIRST / APD / GEOM of that module with two iterations.  A case changes one of three inputs of that scene:

  group "image": `edit(images) -> images`; the passes FIRST and APD run on the edited images, every kernel of both stepped;
  group "depth": `edit(depth maps) -> depth maps`; FIRST and APD run clean (they never read a depth map), every kernel of GEOM stepped;
  group "prior": `edit(prior, params) -> prior` on common.postprocess of the clean FIRST pass; every kernel of APD stepped.

None of these values enters an address: pixels and depths are arithmetic operands only, and a prior plane reaches sample coordinates
through the guarded paths that NaN and inf coordinates already take (tests/test_gpu_edge_cases.py)."""
import numpy as np

import common
import frame_limits_cases as fl
import param_space_cases as pc

W, H, N = 80, 60, 3
# the textureless share of param_space_cases.VIEW_FRAME.  Its scene seed, 3, leaves 2.42 % of the pixels with a variance near kMinVar
# (test_power_of_two_scale_leaves_the_costs_bit_for_bit allows 2 %; seed 1: 2.52 %), seed 2 leaves 0.96 % and 102 WEAK pixels
SCENE_SEED, TEXTURELESS = 2, pc.VIEW_FRAME[3]
PASS_SEED, ITERS = 61, 2
FIRST = dict(pc.FIRST, seed=PASS_SEED, max_iterations=ITERS)
APD = dict(pc.APD, seed=PASS_SEED, max_iterations=ITERS)
GEOM = dict(pc.GEOM, seed=PASS_SEED, max_iterations=ITERS)

# the pixel domain of the C ABI (include/apd_mi355x.h): every pixel finite and |v| <= 2^20
PIXEL_LIMIT = 2.0 ** 20
K_MIN_VAR = np.float32(1e-5)

POISONED_SOURCE = 2     # the one source (view index) the single-view image and depth cases change


class Case:
    def __init__(self, name, group, edit, nans=(), refused=False, options=None, clean_equal=False):
        self.name, self.group, self.edit = name, group, edit
        self.W, self.H, self.N = W, H, N
        self.passes = {"image": [FIRST, APD], "depth": [FIRST, APD, GEOM], "prior": [FIRST, APD]}[group]
        # the first pass whose kernels are stepped and compared; the passes before it only build the prior, on the clean inputs
        self.first_stepped = {"image": 0, "depth": 2, "prior": 1}[group]
        # the state arrays in which the ORACLE holds a NaN word after some kernel of the stepped passes, as
        # tests/test_value_space_cases.py measures them (their sign and payload differ between x86 and gfx950: the GPU test
        # compares flagged cases with common.assert_state_equal_nan_canonical, every other case as raw bits)
        self.nans = tuple(nans)
        self.refused = refused      # the upload answers APD_ERR_UNSUPPORTED: a pixel outside the domain
        self.options = options      # apd_set_option values of the GPU test (depth_mixed on the other arms)
        # the oracle computes the bits of the clean input, in every array: binary32 arithmetic is covariant under a power-of-two scale
        # and on this scene no variance crosses kMinVar when scaled by 2^16.  The host test asserts that equality instead of the rule
        # that a case moves the oracle's result; what the case moves is the path (float texel quads, other exponents in every moment)
        self.clean_equal = clean_equal

    def __repr__(self):
        return self.name


# ---- the scene ------------------------------------------------------------------------------------------------------------------

_SCENE = []


def scene(synth):
    """(scene, 8-bit images, common.fake_depth_maps), made once and never written to."""
    if not _SCENE:
        sc, imgs = common.scene_inputs(synth, W, H, N, seed=SCENE_SEED, textureless=TEXTURELESS)
        deps = common.fake_depth_maps(W, H, N + 1)
        for a in imgs + deps:
            a.setflags(write=False)
        _SCENE.append((sc, imgs, deps))
    return _SCENE[0]


def params(sc, pi, case):
    return common.base_params(sc, N, **case.passes[pi])


def steps(p, weak_count):
    return fl.schedule(p["max_iterations"], weak_count > 0)


def inputs(synth, case):
    """(scene, images, depth maps) of `case`: the scene's own arrays where the case does not edit them."""
    sc, imgs, deps = scene(synth)
    if case.group == "image":
        imgs = [np.ascontiguousarray(im, np.float32) for im in case.edit([im.copy() for im in imgs])]
    elif case.group == "depth":
        deps = [np.ascontiguousarray(d, np.float32) for d in case.edit([d.copy() for d in deps])]
    return sc, imgs, deps


def crafted_prior(case, prior, p):
    """The prior of a "prior" case from the clean one ((planes, views, weak) of common.postprocess); `p`: the APD pass's parameters."""
    planes, views, weak = (a.copy() for a in prior)
    case.edit(planes, views, weak, p)
    return planes, views, weak


# ---- image cases ----------------------------------------------------------------------------------------------------------------

def _f32(x):
    return np.float32(x)


def _scaled(factor):
    return lambda imgs: [im * _f32(factor) for im in imgs]


def _one_pixel(value):
    """One pixel of one source off the 8-bit values: the whole upload leaves the 8-bit path."""
    def edit(imgs):
        imgs[POISONED_SOURCE][H // 2, W // 2] = _f32(value)
        return imgs
    return edit


DARK = 64.0     # synth's images hold no zero: u8_neg_zero clips every pixel below this to zero first


def _neg_zero(imgs, zero=-0.0):
    for im in imgs:
        im[im < DARK] = _f32(zero)
    return imgs


def saturated_image():
    ys, xs = np.mgrid[0:H, 0:W]
    return np.where(((xs // 3) + (ys // 3)) % 2 == 0, 0.0, 255.0).astype(np.float32)


def _flat_source(imgs):
    imgs[POISONED_SOURCE][:] = 128.0
    return imgs


def _nan_source(imgs):
    imgs[POISONED_SOURCE][:] = np.nan
    return imgs


def _inf_pixels(imgs):
    imgs[POISONED_SOURCE][np.random.RandomState(7).rand(H, W) < 0.01] = np.inf
    return imgs


IMAGE_CASES = [
    # power-of-two scales: the same mantissas at other exponents
    Case("scale_2^8", "image", _scaled(256.0), clean_equal=True), Case("scale_2^-8", "image", _scaled(1.0 / 256.0)),
    Case("scale_257", "image", _scaled(257.0)),                                  # exact 16-bit replication, 0..65535
    Case("unit", "image", lambda imgs: [im / _f32(255.0) for im in imgs]),       # [0, 1] in binary32
    Case("centred", "image", lambda imgs: [im - _f32(128.0) for im in imgs]),    # negative integers: not 8-bit
    Case("offset_1e6", "image", lambda imgs: [im + _f32(1e6) for im in imgs], nans=('costs',)),   # a large mean, the same variance
    Case("u8_edge_256", "image", _one_pixel(256.0)), Case("u8_edge_half", "image", _one_pixel(254.5)),
    Case("u8_edge_neg", "image", _one_pixel(-1.0)),
    Case("u8_neg_zero", "image", _neg_zero),
    Case("saturated", "image", lambda imgs: [saturated_image() for _ in imgs], nans=('costs',)),  # the largest 8-bit variance and covariance
    # every NCC is 2.0 and no view is selected anywhere: K14 finds no valid view and marks every pixel UNKNOWN (APD.cu:1990-2144), so the
    # APD pass starts without a WEAK or a STRONG pixel and skips K3, K4, K9 and K10
    Case("flat_all", "image", lambda imgs: [np.full((H, W), 128.0, np.float32) for _ in imgs], nans=('costs',)),
    Case("flat_source", "image", _flat_source, nans=('costs',)),
    Case("nan_source", "image", _nan_source, refused=True, nans=('costs',)), Case("inf_pixels", "image", _inf_pixels, refused=True, nans=('costs',)),
    # variance products past 2^96 (the range sqrt_rn_mid was checked over ends at 2^96) and past FLT_MAX
    Case("huge_2^40", "image", _scaled(2.0 ** 40), refused=True, nans=('costs',)), Case("huge_2^70", "image", _scaled(2.0 ** 70), refused=True, nans=('costs',)),
]

# ---- depth-map cases: the shares of fusion_cases.non_finite ------------------------------------------------------------------------

DEPTH_VALUES = {"depth_nan": (0.01, np.nan), "depth_inf": (0.005, np.inf), "depth_neg_inf": (0.005, -np.inf), "depth_neg_zero": (0.005, -0.0),
                "depth_denormal": (0.005, 1e-40), "depth_huge": (0.005, 1e30), "depth_negative": (0.005, -2.2)}


def depth_mask(view, lo, hi):
    """The pixels of `view` whose draw lies in [lo, hi): one draw per (view, pixel), shared by every depth case."""
    u = np.random.RandomState(100 + view).rand(H, W)
    return (u >= lo) & (u < hi)


def _poison(name, value=None):
    share, val = DEPTH_VALUES[name]

    def edit(deps):
        for v in range(len(deps)):
            deps[v][depth_mask(v, 0.0, share)] = _f32(val if value is None else value)
        return deps
    return edit


def _zero_view(deps):
    deps[POISONED_SOURCE][:] = 0.0
    return deps


def _zero_all(deps):
    for d in deps:
        d[:] = 0.0
    return deps


def _mixed(deps):
    """Every value of DEPTH_VALUES in every view, in disjoint shares, and the last source's map zero everywhere (a rig with every
    map zero has no other value left: depth_zero_all stays a case of its own)."""
    for v in range(len(deps)):
        lo = 0.0
        for share, val in DEPTH_VALUES.values():
            deps[v][depth_mask(v, lo, lo + share)] = _f32(val)
            lo += share
    deps[N][:] = 0.0
    return deps


DEPTH_CASES = [Case(name, "depth", _poison(name)) for name in DEPTH_VALUES]
DEPTH_CASES += [Case("depth_zero_view", "depth", _zero_view), Case("depth_zero_all", "depth", _zero_all), Case("depth_mixed", "depth", _mixed)]
# the early-out's monotonicity argument (the geometric term is non-negative and capped) on these values, and the window-less kernels
DEPTH_ARM_CASES = [Case("depth_mixed-%s=0" % o, "depth", _mixed, options={o: 0}) for o in ("k67_windows", "k1415_windows", "early_out")]

# ---- prior cases ----------------------------------------------------------------------------------------------------------------------

STRIPE = slice(H // 3, H // 3 + 8)      # rows 20..27, every column: 640 pixels (12 rows of lost planes leave no STRONG majority)


def _normal(fn):
    def edit(planes, views, weak, p):
        planes[STRIPE, :, :3] = fn(planes[STRIPE, :, :3])
    return edit


def _depth(fn):
    def edit(planes, views, weak, p):
        planes[STRIPE, :, 3] = fn(planes[STRIPE, :, 3], p)
    return edit


def _outside(d, p):
    d = d.copy()
    d[:, :W // 2] = _f32(0.1 * p["depth_min"])
    d[:, W // 2:] = _f32(10.0 * p["depth_max"])
    return d


def _views(fn):
    def edit(planes, views, weak, p):
        views[STRIPE] = fn(views[STRIPE])
    return edit


def _weak(fn):
    def edit(planes, views, weak, p):
        weak[...] = fn(weak)
    return edit


HIGH_BITS = np.uint32(0xFFFFFFFF ^ ((1 << N) - 1))      # bits N..31


def _checker(weak):
    ys, xs = np.mgrid[0:H, 0:W]
    return np.where((xs + ys) % 2 == 0, fl.WEAK, np.where(weak == fl.WEAK, fl.STRONG, weak)).astype(np.uint8)


PRIOR_CASES = [
    Case("prior_zero_normal", "prior", _normal(lambda n: n * _f32(0.0)), nans=('costs', 'planes')),
    Case("prior_nan_normal", "prior", _normal(lambda n: n * _f32(np.nan)), nans=('costs', 'fit', 'planes')),
    Case("prior_unnormalised", "prior", _normal(lambda n: n * _f32(3.0))),
    Case("prior_backfacing", "prior", _normal(lambda n: -n)),
    Case("prior_depth_0", "prior", _depth(lambda d, p: d * _f32(0.0)), nans=('costs',)),
    Case("prior_depth_negative", "prior", _depth(lambda d, p: -d)),
    Case("prior_depth_inf", "prior", _depth(lambda d, p: np.full_like(d, np.inf)), nans=('costs', 'fit', 'planes')),
    Case("prior_depth_outside", "prior", _depth(_outside), nans=('costs',)),
    Case("prior_views_0", "prior", _views(lambda v: v * np.uint32(0))),
    Case("prior_views_high_bits", "prior", _views(lambda v: v | HIGH_BITS)),
    Case("prior_all_weak", "prior", _weak(lambda w: np.full_like(w, fl.WEAK))),
    Case("prior_all_strong", "prior", _weak(lambda w: np.full_like(w, fl.STRONG))),
    Case("prior_all_unknown", "prior", _weak(lambda w: np.full_like(w, fl.UNKNOWN))),
    Case("prior_weak_checker", "prior", _weak(_checker)),
]

ALL_CASES = IMAGE_CASES + DEPTH_CASES + PRIOR_CASES
BY_NAME = {c.name: c for c in ALL_CASES + DEPTH_ARM_CASES}
# cases after which the frame is without the usual mix of WEAK and STRONG pixels: by design, or because of what the values do to the
# oracle -- at a mean of 1e6 the binary32 moments keep none of the texture's variance (about 1e3 against a rounding error of
# 2^-24 * 1e12 = 6e4 in sum_ss): most NCCs are noise and 127 pixels stay STRONG; with every depth map zero every geometric term is
# max_cost and K14 leaves no pixel STRONG
NO_WORK_BOUND = {"flat_all", "prior_all_weak", "prior_all_strong", "prior_all_unknown", "huge_2^40", "huge_2^70", "offset_1e6", "depth_zero_all"}
# the oracle never reads a bit at or above num_src (bit_test runs over the sources) and carries the bits through every kernel, so the
# case moves `views` alone: a kernel that counted or shifted the whole word would differ there and in what follows
MOVES_VIEWS_ONLY = {"prior_views_high_bits"}


def in_pixel_domain(imgs):
    return all(bool(np.isfinite(im).all()) and float(np.abs(im).max()) <= PIXEL_LIMIT for im in imgs)
