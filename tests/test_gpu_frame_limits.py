"""HIP path vs CPU oracle at both ends of the frame sizes apd_create accepts: 1 x 1 ... 33 x 17 and axes of 16384 px.

The hand-written index arithmetic of the kernels rests on claims about exactly these ends -- LDS window addresses formed in
binary32 (csrc/apd_window.h), 24-bit multiply-adds with the row pitch of a 16384-px frame (quad_byte_offset, fquad_byte_offset),
the multiply-shift division by 7 of the tiled copy, short2 coordinates in K2 / K3 at the top; waves with more lanes than the
frame has pixels, an empty checkerboard colour, patches whose every tap is clamped, frames inside K14's margin and passes
without a WEAK pixel at the bottom.  A coarsest pyramid level or a crop handed to the C ABI can be any of these.

Every comparison is HIP against oracle over all arrays of common.ORACLE_STATES as raw bits after EVERY kernel, with the one
exception tests/test_gpu_edge_cases.py already makes: a float word that is NaN on both sides compares equal whatever its sign
and payload (tiny frames do produce NaN costs in the oracle); a NaN on one side only is a difference.  The oracle's own
behaviour at the tiny shapes has its witnesses in tests/test_oracle_frame_limits.py.

Lines starting with FRAME_LIMITS carry the non-vacuity figures the tests measured (profiles/frame_limits/test_times.txt).

Frames with both axes large, 2^26 px up to 16384 x 16382, where 32-bit index products can wrap: tests/test_gpu_frame_area.py."""
import ctypes as C

import numpy as np
import pytest

import common
import frame_limits_cases as fl

pytestmark = pytest.mark.gpu

# every bit-preserving option on its other arm (source_quads = 0 sends 8-bit input down the float texel-quad path, so no tiled
# copy is built whatever tiled_copy says) ...
OTHER_ARM = dict(k67_windows=0, k1415_windows=0, source_quads=0, tiled_copy=2, early_out=0)
# ... so the tiled copy "used by every global gather" gets an arm of its own, with the LDS windows off: every sample of every
# pass goes through quad_tiled_offset_tu
TILED_EVERYWHERE = dict(k67_windows=0, k1415_windows=0, tiled_copy=2)


def _assert_states(pkg, h, o, where):
    for name, hs, oa in common.ORACLE_STATES:
        if name == "neighbours" and h.weak_count == 0:
            continue
        a, b = h.state(getattr(pkg, hs)), getattr(o, oa)
        if not np.array_equal(common.canon_nan(a), common.canon_nan(b)):
            neq = common.canon_nan(a).reshape(a.shape[0], -1) != common.canon_nan(b).reshape(a.shape[0], -1)
            raise AssertionError("%s: HIP and oracle differ in `%s` (%d bytes differ)" % (where, name, int(neq.sum())))


_SCENES = {}


def _tiny_scene(synth, W, H, N, floats):
    key = (W, H, N, floats)
    if key not in _SCENES:
        sc, imgs = common.scene_inputs(synth, W, H, N, seed=3, textureless=0.25)
        _SCENES[key] = (sc, fl.float_images(imgs) if floats else imgs, common.fake_depth_maps(W, H, N + 1))
    return _SCENES[key]


def _next_prior(h, p, W, H):
    """common.postprocess of the pass just run, with the weak map replaced by the crafted one."""
    planes, weak, views = h.download()
    planes, views, _ = common.postprocess(planes, weak, views, p["depth_min"], p["depth_max"])
    return planes, views, fl.crafted_weak_map(W, H)


TINY_CASES = [(W, H, 2) for (W, H) in fl.TINY_SHAPES] + [(24, 20, 17)]


@pytest.mark.parametrize("floats", [False, True], ids=["u8", "float"])
@pytest.mark.parametrize("W,H,N", TINY_CASES)
def test_tiny_frames_lockstep(gpu_pkg, ob, synth, W, H, N, floats):
    """Three pass kinds, two iterations each, every kernel compared; default options, then every bit-preserving option on its
    other arm, then the tiled copy in every gather.  Passes 2 and 3 run on the crafted WEAK map."""
    sc, imgs, deps = _tiny_scene(synth, W, H, N, floats)
    x0, y0, x1, y1 = fl.weak_block(W, H)
    want_weak = (x1 - x0) * (y1 - y0)
    for arm, options in (("default", {}), ("other arm", OTHER_ARM), ("tiled everywhere", TILED_EVERYWHERE)):
        prior = None
        for pi, extra in enumerate(fl.PASSES):
            p = common.base_params(sc, N, seed=31, max_iterations=2, **extra)
            geom = bool(p.get("geom_consistency"))
            h = common.make_handle(gpu_pkg, sc, imgs, N, p, depths=deps if geom else None, prior=prior, options=options)
            o = common.make_oracle(ob, sc, imgs, N, p, depths=deps if geom else None, prior=prior)
            label = "%dx%d N=%d %s, %s, pass %d" % (W, H, N, "float" if floats else "8-bit", arm, pi)
            assert h.weak_count == o.weak_count == (want_weak if pi else 0), label
            if pi and W >= 4 and H >= 4:
                assert h.weak_count > 0, label
            # a pass without a WEAK pixel skips K3, K4, K9 and K10 (the oracle's kernels would visit nothing)
            for kid, it in fl.schedule(2, h.weak_count > 0):
                h.run_kernel(kid, it)
                o.run_kernel(kid, it)
                _assert_states(gpu_pkg, h, o, "%s after K%d(iter %d)" % (label, kid, it))
                if kid == 3:
                    reliable = int((o.weak_reliable != 0).sum())
                    if arm == "default":
                        print("FRAME_LIMITS tiny %s: weak_count %d, weak_reliable after K3 %d" % (label, o.weak_count, reliable))
                    if W >= 24 and H >= 20:
                        assert reliable > 0, label
            prior = _next_prior(h, p, W, H)
            h.close()
            o.close()


@pytest.mark.parametrize("floats", [False, True], ids=["u8", "float"])
@pytest.mark.parametrize("W,H", [(1, 1), (1, 40), (40, 1)])
def test_passes_without_a_weak_pixel_skip_the_weak_kernels(gpu_pkg, ob, synth, W, H, floats):
    """The crafted block is empty on these frames: apd_run launches no K3, K4, K9 or K10 in the APD passes, and leaves the bits
    of the oracle's orc_run, whose weak kernels find no pixel to visit."""
    N = 2
    sc, imgs, deps = _tiny_scene(synth, W, H, N, floats)
    prior = None
    for pi, extra in enumerate(fl.PASSES):
        p = common.base_params(sc, N, seed=31, max_iterations=2, **extra)
        geom = bool(p.get("geom_consistency"))
        h = common.make_handle(gpu_pkg, sc, imgs, N, p, depths=deps if geom else None, prior=prior)
        o = common.make_oracle(ob, sc, imgs, N, p, depths=deps if geom else None, prior=prior)
        assert h.weak_count == 0 and o.weak_count == 0
        h.profile_enable(True)
        h.run()
        o.run()
        launched = set(h.profile())
        assert launched == {1, 2, 5, 6, 7, 8, 11, 12, 13, 14, 15}, launched
        assert not (o.weak_reliable != 0).any()
        _assert_states(gpu_pkg, h, o, "%dx%d pass %d, apd_run" % (W, H, pi))
        prior = _next_prior(h, p, W, H)
        h.close()
        o.close()


@pytest.mark.parametrize("floats", [False, True], ids=["u8", "float"])
@pytest.mark.parametrize("W,H", [(5, 7), (16, 4), (31, 32)])
def test_tiny_frames_whole_pass_on_a_recycled_handle(gpu_pkg, ob, synth, W, H, floats):
    """apd_run == orc_run for each of the three passes, on ONE handle re-armed with apd_reset between them."""
    N = 2
    sc, imgs, deps = _tiny_scene(synth, W, H, N, floats)
    cams = [gpu_pkg.make_camera(sc.K[i], sc.R[i], sc.t[i], W, H, sc.depth_min, sc.depth_max) for i in range(N + 1)]
    for arm, options in (("default", {}), ("other arm", OTHER_ARM), ("tiled everywhere", TILED_EVERYWHERE)):
        h, prior = None, None
        for pi, extra in enumerate(fl.PASSES):
            p = common.base_params(sc, N, seed=32, max_iterations=2, **extra)
            geom = bool(p.get("geom_consistency"))
            if h is None:
                h = gpu_pkg.Handle(W, H, gpu_pkg.default_params(**p), device=0)
                for name, value in options.items():
                    h.set_option(name, value)
            else:
                h.reset(gpu_pkg.default_params(**p))
            for name, value in options.items():
                assert h.get_option(name) == value   # options outlive apd_reset
            h.upload_views(cams, imgs, deps if geom else None)
            if prior is not None:
                h.upload_prior(*prior)
            o = common.make_oracle(ob, sc, imgs, N, p, depths=deps if geom else None, prior=prior)
            assert h.weak_count == o.weak_count and (pi == 0 or h.weak_count > 0)
            h.run()
            o.run()
            _assert_states(gpu_pkg, h, o, "%dx%d %s, %s, pass %d, apd_run on a recycled handle" % (W, H, "float" if floats else "8-bit", arm, pi))
            prior = _next_prior(h, p, W, H)
            o.close()
        h.close()


# ---- long axes ---------------------------------------------------------------------------------------------------------------

LONG = 16384


def _long_windows(W, H):
    """Three windows spanning the whole short axis: the first 128, the last 128 and [8128, 8256) of the long axis (the last one
    straddles 8192)."""
    spans = [(0, 128), (LONG - 128, LONG), (8128, 8256)]
    return [(a, 0, b, H) for a, b in spans] if W == LONG else [(0, a, W, b) for a, b in spans]


def _stripes(W, H):
    """WEAK stripes across the short axis, 5 px of every 48 along the long one (each 128-px window holds at least two), and one
    2-px stripe along the whole long axis."""
    weak = np.zeros((H, W), bool)
    along = (np.arange(LONG) % 48) >= 43
    if W == LONG:
        weak[:, along] = True
        weak[H // 2:H // 2 + 2, :] = True
    else:
        weak[along, :] = True
        weak[:, W // 2:W // 2 + 2] = True
    return weak


_LONG = {}


def _long_case(synth, ob, W, H, floats):
    """Scene, images and the non-vacuity figures of one (shape, image kind), computed once from the ORACLE ALONE: a FIRST_INIT pass
    of two iterations on the three windows; share of pixels per window whose cost is finite and below 1.0, i.e. whose samples
    landed inside the sources."""
    key = (W, H, floats)
    if key in _LONG:
        return _LONG[key]
    N = 2
    # focal length 0.9 W: at 16384 px the default baseline puts every projection hundreds of rows outside a 40-row source
    kw = dict(baseline=7.5e-4) if W == LONG else {}
    sc = synth.make_scene(W, H, N, seed=3, textureless=0.3, **kw)
    imgs = sc.images_numpy()
    if floats:
        imgs = fl.float_images(imgs)
    p = common.base_params(sc, N, seed=41, max_iterations=2, **fl.PASSES[0])
    o = common.make_oracle(ob, sc, imgs, N, p)
    windows = _long_windows(W, H)
    for (x0, y0, x1, y1) in windows:
        o.set_roi(x0, y0, x1, y1)
        o.run()
    costs = o.costs.copy()
    o.close()
    shares = []
    for (x0, y0, x1, y1) in windows:
        c = costs[y0:y1, x0:x1]
        shares.append(float((np.isfinite(c) & (c < 1.0)).mean()))
    print("FRAME_LIMITS long %dx%d %s: share of in-frame costs per window (first 128, last 128, [8128, 8256)) %s"
          % (W, H, "float" if floats else "8-bit", " ".join("%.3f" % s for s in shares)))
    _LONG[key] = (sc, imgs, common.fake_depth_maps(W, H, N + 1), windows, shares)
    return _LONG[key]


LONG_CASES = [(LONG, 24, False), (LONG, 40, False), (24, LONG, False), (40, LONG, False), (LONG, 24, True), (24, LONG, True)]
LONG_ARMS = [("default", {}), ("no-windows", dict(k67_windows=0, k1415_windows=0)), ("fquads", dict(source_quads=0, tiled_copy=2)),
             ("tiled-everywhere", TILED_EVERYWHERE)]


# the tiled copy holds 8-bit texels: no such arm for float images
LONG_PARAMS = [(w, h, f, a, o) for (w, h, f) in LONG_CASES for (a, o) in LONG_ARMS if not (f and a == "tiled-everywhere")]


@pytest.mark.parametrize("W,H,floats,arm,options", LONG_PARAMS, ids=["%dx%d-%s-%s" % (w, h, "float" if f else "u8", a) for w, h, f, a, _ in LONG_PARAMS])
def test_long_axes_lockstep(gpu_pkg, ob, synth, W, H, floats, arm, options):
    """A 16384-px axis: the HIP path runs the whole frame, the oracle three windows of it from the HIP path's pre-kernel state
    (common.fullsize_lockstep), compared after every kernel of the three pass kinds.  `fquads`: the float-quad pitch of
    (16384 + 1) * 16 = 262,160 bytes in the 24-bit multiply-add; `tiled-everywhere`: the tiled copy's divide at t ~ 16385."""
    N = 2
    sc, imgs, deps, windows, shares = _long_case(synth, ob, W, H, floats)
    assert min(shares) >= 0.25, shares   # the inputs put the window path to work at those coordinates
    stripes = _stripes(W, H)
    prior = None
    for pi, extra in enumerate(fl.PASSES):
        p = common.base_params(sc, N, seed=41, max_iterations=2, **extra)
        geom = bool(p.get("geom_consistency"))
        if prior is not None:
            in_windows = [int((prior[2][y0:y1, x0:x1] == fl.WEAK).sum()) for (x0, y0, x1, y1) in windows]
            assert min(in_windows) > 0, in_windows
            if arm == "default":
                print("FRAME_LIMITS long %dx%d %s pass %d: weak_count per window %s" % (W, H, "float" if floats else "8-bit", pi, in_windows))
        h = common.make_handle(gpu_pkg, sc, imgs, N, p, depths=deps if geom else None, prior=prior, options=options)
        o = common.make_oracle(ob, sc, imgs, N, p, depths=deps if geom else None, prior=prior)
        assert h.weak_count == o.weak_count == (int(stripes.sum()) if pi else 0)
        if pi:
            assert np.array_equal(h.state(gpu_pkg.STATE_NEIGHBOURS_MAP), o.neighbours_map)
        sched = fl.schedule(2, h.weak_count > 0)
        n = common.fullsize_lockstep(gpu_pkg, h, o, sched, windows, "%dx%d %s, %s, pass %d" % (W, H, "float" if floats else "8-bit", arm, pi),
                                     bits=common.canon_nan)
        assert n == len(sched)
        planes, weak, views = h.download()
        planes, views, weak = common.postprocess(planes, weak, views, p["depth_min"], p["depth_max"])
        prior = (planes, views, np.where(stripes, fl.WEAK, np.where(weak == fl.UNKNOWN, fl.UNKNOWN, fl.STRONG)).astype(np.uint8))
        h.close()
        o.close()


# ---- helpers of the C ABI at the limits ---------------------------------------------------------------------------------------

def _exchange_lib(pkg):
    L = pkg.lib()
    L.apd_device_malloc.argtypes = [C.c_int, C.c_size_t, C.POINTER(C.c_void_p)]
    L.apd_device_free.argtypes = [C.c_int, C.c_void_p]
    L.apd_device_memcpy.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    L.apd_rescale_nearest_device.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int]
    return L


@pytest.mark.parametrize("elem,dtype,ch", [(1, np.uint8, 1), (4, np.uint32, 1), (16, np.float32, 4)])
def test_rescale_nearest_at_the_limits(gpu_pkg, elem, dtype, ch):
    """apd_rescale_nearest_device against the host restatement of RescaleMatToTargetSize (APD.cpp:752-774) that
    tests/test_gpu_exchange.py uses: a 16384-px row halved and doubled back, a 16384-px column halved, one pixel blown up."""
    from test_gpu_exchange import _rescale_reference
    L = _exchange_lib(gpu_pkg)
    rng = np.random.default_rng(11)
    for (sw, sh), (dw, dh) in (((LONG, 24), (8192, 12)), ((8192, 12), (LONG, 24)), ((24, LONG), (12, 8192)), ((1, 1), (3, 2))):
        a = rng.integers(0, 250, (sh, sw, ch) if ch > 1 else (sh, sw)).astype(dtype)
        want = _rescale_reference(a, dw, dh)
        ds, dd = C.c_void_p(), C.c_void_p()
        assert L.apd_device_malloc(0, a.nbytes, C.byref(ds)) == 0 and L.apd_device_malloc(0, want.nbytes, C.byref(dd)) == 0
        try:
            assert L.apd_device_memcpy(0, ds, a.ctypes.data_as(C.c_void_p), a.nbytes) == 0
            assert L.apd_rescale_nearest_device(0, ds, sw, sh, dd, dw, dh, elem) == 0
            got = np.empty_like(want)
            assert L.apd_device_memcpy(0, got.ctypes.data_as(C.c_void_p), dd, want.nbytes) == 0
            assert np.array_equal(got, want), ((sw, sh), (dw, dh), elem)
        finally:
            L.apd_device_free(0, ds)
            L.apd_device_free(0, dd)


@pytest.mark.parametrize("floats", [False, True], ids=["u8", "float"])
@pytest.mark.parametrize("W,H", [(5, 7), (LONG, 24)])
def test_shared_images_equal_the_copying_upload(gpu_pkg, synth, W, H, floats):
    """apd_image_create + apd_upload_views_shared: the bits of apd_upload_views after K5 (initial costs: one NCC per source through
    the derived copies) and after K6."""
    N = 2
    sc = synth.make_scene(W, H, N, seed=3, textureless=0.3, **(dict(baseline=7.5e-4) if W == LONG else {}))
    imgs = fl.float_images(sc.images_numpy()) if floats else sc.images_numpy()
    p = common.base_params(sc, N, seed=51, max_iterations=1, **fl.PASSES[0])
    cams = [gpu_pkg.make_camera(sc.K[i], sc.R[i], sc.t[i], W, H, sc.depth_min, sc.depth_max) for i in range(N + 1)]
    a = common.make_handle(gpu_pkg, sc, imgs, N, p)
    shared = [gpu_pkg.SharedImage(W, H, im) for im in imgs]
    b = gpu_pkg.Handle(W, H, gpu_pkg.default_params(**p), device=0)
    b.upload_views_shared(cams, shared)
    try:
        for kid in (1, 2, 5, 6):
            a.run_kernel(kid)
            b.run_kernel(kid)
            if kid >= 5:
                for name, hs, _ in common.ORACLE_STATES[:5]:
                    x, y = a.state(getattr(gpu_pkg, hs)), b.state(getattr(gpu_pkg, hs))
                    assert np.array_equal(common.bits(x), common.bits(y)), "%dx%d: `%s` differs after K%d" % (W, H, name, kid)
        costs = a.state(gpu_pkg.STATE_COSTS)
        if W == LONG:
            assert (np.isfinite(costs) & (costs < 1.0)).mean() > 0.25   # K5 and K6 sampled inside the sources
    finally:
        a.close()
        b.close()
        for im in shared:
            im.close()


@pytest.mark.parametrize("W,H", [(1, 1), (5, 7), (LONG, 24)])
def test_exports_equal_the_host_postprocessing(gpu_pkg, synth, W, H):
    """apd_export_state_device and apd_export_depth_normal_device against common.postprocess (main.cpp:105-115) of the raw
    download, with depths below, inside and above the range at every frame size."""
    import torch
    N = 2
    sc = synth.make_scene(W, H, N, seed=3, **(dict(baseline=7.5e-4) if W == LONG else {}))
    imgs = sc.images_numpy()
    p = common.base_params(sc, N, seed=52, max_iterations=1, **fl.PASSES[0])
    h = common.make_handle(gpu_pkg, sc, imgs, N, p)
    h.run()
    planes = h.state(gpu_pkg.STATE_PLANES)
    flat = planes.reshape(-1, 4)
    flat[0::3, 3] = 100.0   # out of [depth_min, depth_max] -> exported as 0 and UNKNOWN
    flat[1::3, 3] = 0.01
    h.set_state(gpu_pkg.STATE_PLANES, planes)
    planes, weak, views = h.download()
    rp, rv, rw = common.postprocess(planes, weak, views, p["depth_min"], p["depth_max"])
    assert (rp[..., 3] == 0).any() and (W * H < 3 or (rp[..., 3] != 0).any())
    d_planes = torch.empty((H, W, 4), device="cuda", dtype=torch.float32)
    d_weak = torch.empty((H, W), device="cuda", dtype=torch.uint8)
    d_views = torch.empty((H, W), device="cuda", dtype=torch.int32)
    d_depth = torch.empty((H, W), device="cuda", dtype=torch.float32)
    h.export_state(d_planes, d_weak, d_views, d_depth)
    canon = common.canon_nan
    assert np.array_equal(canon(d_planes.cpu().numpy()), canon(rp))
    assert np.array_equal(d_weak.cpu().numpy(), rw)
    assert np.array_equal(d_views.cpu().numpy().view(np.uint32), rv)
    assert np.array_equal(canon(d_depth.cpu().numpy()), canon(rp[..., 3]))
    d_normal = torch.empty((H, W, 3), device="cuda", dtype=torch.float32)
    d_depth.zero_()
    torch.cuda.synchronize()   # the export runs on the handle's own non-blocking stream: torch's fill must have ended before it
    h.export_depth_normal(d_depth, d_normal)
    assert np.array_equal(canon(d_depth.cpu().numpy()), canon(rp[..., 3]))
    assert np.array_equal(canon(d_normal.cpu().numpy()), canon(rp[..., :3]))
    h.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------

APD_ERR_INVALID, APD_ERR_UNSUPPORTED = -1, -5


@pytest.mark.parametrize("W,H,status", [(LONG + 1, 1, APD_ERR_UNSUPPORTED), (1, LONG + 1, APD_ERR_UNSUPPORTED), (0, 8, APD_ERR_INVALID),
                                        (8, -1, APD_ERR_INVALID),
                                        # a float-quad image of (W + 1) x (H + 1) 16-byte entries must stay below 2^32 bytes: byte offsets are 32-bit
                                        (LONG, LONG, APD_ERR_UNSUPPORTED), (LONG - 1, LONG - 1, APD_ERR_UNSUPPORTED)])
def test_sizes_outside_the_limits_are_refused(gpu_pkg, W, H, status):
    L = gpu_pkg.lib()
    L.apd_last_error.restype = C.c_char_p
    params = gpu_pkg.default_params()
    out = C.c_void_p()
    assert L.apd_create(C.byref(out), 0, W, H, C.byref(params)) == status
    assert out.value is None, "no handle may be returned"
    assert L.apd_last_error(), "apd_last_error must say why"
    assert b"apd_create" in L.apd_last_error()
    # apd_image_create: APD_ERR_INVALID for every size no handle can have (include/apd_mi355x.h); it must not read `pixels` first
    pixels = np.zeros(16, np.float32)
    img = C.c_void_p()
    assert L.apd_image_create(C.byref(img), 0, W, H, pixels.ctypes.data_as(C.c_void_p)) == APD_ERR_INVALID
    assert img.value is None
    assert b"apd_image_create" in L.apd_last_error()
