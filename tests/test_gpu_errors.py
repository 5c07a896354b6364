"""Error behaviour of the C ABI: the reference exit()s (APD.cpp:321, 430); the library returns codes."""
import ctypes as C

import numpy as np
import pytest

import common

pytestmark = pytest.mark.gpu


def test_too_many_images(gpu_pkg, synth):
    W, H = 32, 32
    sc, imgs = common.scene_inputs(synth, W, H, 1)
    cams = [gpu_pkg.make_camera(sc.K[0], sc.R[0], sc.t[0], W, H, 1, 4)] * 33
    h = gpu_pkg.Handle(W, H, gpu_pkg.default_params())
    with pytest.raises(gpu_pkg.ApdError, match="so much images"):
        h.upload_views(cams, [imgs[0]] * 33)
    h.close()


def test_run_before_upload(gpu_pkg):
    h = gpu_pkg.Handle(32, 32, gpu_pkg.default_params())
    with pytest.raises(gpu_pkg.ApdError, match="apd_upload_views"):
        h.run()
    h.close()


def test_refine_state_needs_prior(gpu_pkg, synth):
    W, H, N = 32, 32, 2
    sc, imgs = common.scene_inputs(synth, W, H, N)
    h = common.make_handle(gpu_pkg, sc, imgs, N, common.base_params(sc, N, state=gpu_pkg.REFINE_INIT, use_APD=1))
    with pytest.raises(gpu_pkg.ApdError, match="apd_upload_prior"):
        h.run()
    h.close()


def test_geometric_pass_needs_depth_maps(gpu_pkg, synth):
    W, H, N = 32, 32, 2
    sc, imgs = common.scene_inputs(synth, W, H, N)
    with pytest.raises(gpu_pkg.ApdError, match="depth maps"):
        common.make_handle(gpu_pkg, sc, imgs, N, common.base_params(sc, N, geom_consistency=1))


def test_unsupported_patch_geometry(gpu_pkg):
    with pytest.raises(gpu_pkg.ApdError, match="patch geometry"):
        gpu_pkg.Handle(32, 32, gpu_pkg.default_params(strong_radius=7))


APD_ERR_UNSUPPORTED = -5


@pytest.mark.parametrize("rotate_time", [0, -1, 5, 8])
def test_rotate_time_outside_1_to_4_is_refused_by_apd_create(gpu_pkg, rotate_time):
    """K3 keeps 8 x 4 ray slots (short2 strong_pts[32] and a 32-bit mask): rotate_time = 5 would write slot 32.  The value is
    refused before any device work; no kernel is ever launched with it."""
    L = gpu_pkg.lib()
    params = gpu_pkg.default_params(rotate_time=rotate_time)
    out = C.c_void_p()
    assert L.apd_create(C.byref(out), 0, 32, 32, C.byref(params)) == APD_ERR_UNSUPPORTED
    assert out.value is None, "no handle may be returned"
    message = L.apd_last_error().decode()
    assert "apd_create" in message and "rotate_time %d" % rotate_time in message, message
    with pytest.raises(gpu_pkg.ApdError, match="rotate_time"):
        gpu_pkg.Handle(32, 32, params)


@pytest.mark.parametrize("rotate_time", [0, -1, 5, 8])
def test_rotate_time_outside_1_to_4_is_refused_by_apd_reset(gpu_pkg, ob, synth, rotate_time):
    """... and a refused apd_reset leaves the handle as it was: its parameters, its uploaded views, its state -- the pass it was
    armed for still gives the oracle's bits, and so does the next one after an accepted apd_reset."""
    W, H, N = 40, 33, 2
    sc, imgs = common.scene_inputs(synth, W, H, N)
    p = common.base_params(sc, N, max_iterations=1, weak_peak_radius=6)
    h = common.make_handle(gpu_pkg, sc, imgs, N, p)
    L = gpu_pkg.lib()
    bad = gpu_pkg.default_params(**dict(p, rotate_time=rotate_time, seed=99))
    assert L.apd_reset(h._h, C.byref(bad)) == APD_ERR_UNSUPPORTED
    message = L.apd_last_error().decode()
    assert "apd_reset" in message and "rotate_time %d" % rotate_time in message, message
    with pytest.raises(gpu_pkg.ApdError, match="rotate_time"):
        h.reset(bad)
    o = common.make_oracle(ob, sc, imgs, N, p)
    h.run()
    o.run()
    common.assert_state_equal(gpu_pkg, h, o, "the armed pass after a refused apd_reset")
    o.close()
    p2 = dict(p, seed=8, rotate_time=1)
    h.reset(gpu_pkg.default_params(**p2))
    cams = [gpu_pkg.make_camera(sc.K[i], sc.R[i], sc.t[i], W, H, sc.depth_min, sc.depth_max) for i in range(N + 1)]
    h.upload_views(cams, imgs)
    o = common.make_oracle(ob, sc, imgs, N, p2)
    h.run()
    o.run()
    common.assert_state_equal(gpu_pkg, h, o, "an accepted apd_reset after a refused one")
    h.close()
    o.close()


OUTSIDE_PIXELS = [float("nan"), float("inf"), float("-inf"), 2.0 ** 20 + 0.125, -(2.0 ** 20) - 0.125, 3.0e38]


@pytest.mark.parametrize("value", OUTSIDE_PIXELS, ids=["nan", "inf", "-inf", "above_2^20", "below_-2^20", "3e38"])
@pytest.mark.parametrize("view", [0, 2])
def test_a_pixel_outside_the_domain_is_refused_by_every_upload(gpu_pkg, ob, synth, value, view):
    """The NCC tail (csrc/apd_device.h: sqrt_rn_mid, div_rn_mid) is exact for finite pixels in [-2^20, 2^20]; one pixel outside, in the
    reference view or a source, and apd_upload_views, apd_upload_views_split and apd_image_create answer APD_ERR_UNSUPPORTED and name the
    view.  The test that finds it is the upload's own pass over the pixels; no kernel of a pass runs.  Afterwards the handle holds no
    views, and takes a clean upload with the oracle's bits."""
    W, H, N = 40, 33, 2
    sc, imgs = common.scene_inputs(synth, W, H, N)
    bad = [im.copy() for im in imgs]
    bad[view][H - 1, W - 1] = np.float32(value)     # the last pixel of the plane
    p = common.base_params(sc, N, max_iterations=1, weak_peak_radius=6)
    L = gpu_pkg.lib()
    cams = [gpu_pkg.make_camera(sc.K[i], sc.R[i], sc.t[i], W, H, sc.depth_min, sc.depth_max) for i in range(N + 1)]
    cam_arr = (gpu_pkg.Camera * (N + 1))(*cams)
    ptrs = (C.c_void_p * (N + 1))(*[im.ctypes.data for im in bad])
    h = common.make_handle(gpu_pkg, sc, imgs, N, p)      # armed with a clean upload first
    for name, args in (("apd_upload_views", (ptrs, None)), ("apd_upload_views_split", (ptrs,))):
        assert getattr(L, name)(h._h, N + 1, cam_arr, *args) == APD_ERR_UNSUPPORTED
        message = L.apd_last_error().decode()
        assert message.startswith(name + ":") and "view %d" % view in message and "2^20" in message, message
        with pytest.raises(gpu_pkg.ApdError, match="apd_upload_views"):
            h.run()
    out = C.c_void_p()
    assert L.apd_image_create(C.byref(out), 0, W, H, C.c_void_p(bad[view].ctypes.data)) == APD_ERR_UNSUPPORTED
    assert out.value is None and "apd_image_create" in L.apd_last_error().decode()
    with pytest.raises(gpu_pkg.ApdError, match="2\\^20"):
        gpu_pkg.SharedImage(W, H, bad[view])
    h.upload_views(cams, imgs)
    o = common.make_oracle(ob, sc, imgs, N, p)
    h.run()
    o.run()
    common.assert_state_equal(gpu_pkg, h, o, "a clean upload after a refused one")
    h.close()
    o.close()


def test_pixels_at_the_edge_of_the_domain_are_accepted(gpu_pkg, ob, synth):
    """+-2^20 exactly, -0.0 and a denormal are inside the domain: the upload is accepted and the pass has the oracle's bits."""
    W, H, N = 40, 33, 2
    sc, imgs = common.scene_inputs(synth, W, H, N)
    imgs = [im.copy() for im in imgs]
    imgs[0][0, 0], imgs[1][5, 7], imgs[2][H - 1, W - 1], imgs[2][3, 3] = np.float32(2.0 ** 20), np.float32(-(2.0 ** 20)), np.float32(-0.0), np.float32(1e-40)
    p = common.base_params(sc, N, max_iterations=1, weak_peak_radius=6)
    h = common.make_handle(gpu_pkg, sc, imgs, N, p)
    o = common.make_oracle(ob, sc, imgs, N, p)
    h.run()
    o.run()
    common.assert_state_equal_nan_canonical(gpu_pkg, h, o, "pixels at +-2^20")
    h.close()
    o.close()


def test_camera_size_mismatch(gpu_pkg, synth):
    W, H = 32, 32
    sc, imgs = common.scene_inputs(synth, W, H, 1)
    cams = [gpu_pkg.make_camera(sc.K[i], sc.R[i], sc.t[i], W + 1, H, 1, 4) for i in range(2)]
    h = gpu_pkg.Handle(W, H, gpu_pkg.default_params())
    with pytest.raises(gpu_pkg.ApdError, match="camera"):
        h.upload_views(cams, imgs)
    h.close()


def test_profile_counters(gpu_pkg, synth):
    W, H, N = 64, 48, 2
    sc, imgs = common.scene_inputs(synth, W, H, N)
    h = common.make_handle(gpu_pkg, sc, imgs, N, common.base_params(sc, N))
    for k in (1, 2, 5):
        h.run_kernel(k)
    h.profile_enable(True)
    h.profile_reset()
    h.run_sweeps(0, 2)
    prof = h.profile()
    assert prof[gpu_pkg.K6][1] == 2 and prof[gpu_pkg.K7][1] == 2 and prof[gpu_pkg.K8][1] == 2
    assert prof[gpu_pkg.K6][0] > 0
    assert gpu_pkg.K9 not in prof  # no WEAK pixel -> weak kernels are not launched
    h.close()


def test_weak_lists_cannot_be_overrun_by_a_second_pass(gpu_pkg, ob, synth):
    """the WEAK lists, the neighbour table and its index map are sized by the weak map apd_upload_prior loads.
    K14 rewrites that map (usually with more WEAK pixels) and apd_upload_state can too; the kernels that walk the lists must
    then be refused (APD_ERR_STATE), not run past the end of them -- and a new apd_upload_prior / apd_reset re-arms the
    handle with the oracle's bits."""
    W, H, N = 96, 72, 4
    sc, imgs = common.scene_inputs(synth, W, H, N, seed=3, textureless=0.25)
    p0 = common.base_params(sc, N, seed=11, state=0, use_APD=0, weak_peak_radius=6)
    h = common.make_handle(gpu_pkg, sc, imgs, N, p0)
    h.run()
    planes, weak, views = h.download()
    with pytest.raises(gpu_pkg.ApdError, match="apd_reset or apd_upload_prior"):
        h.run()                      # a second pass on the same object
    for kid in (3, 8, 9, 10):
        with pytest.raises(gpu_pkg.ApdError, match="rewritten"):
            h.run_kernel(kid)        # K14 followed by a list walker
    prior = common.postprocess(planes, weak, views, p0["depth_min"], p0["depth_max"])
    assert (prior[2] == 0).sum() > 50
    p1 = common.base_params(sc, N, seed=11, state=1, use_APD=1, weak_peak_radius=6)
    # the same handle re-armed == a fresh oracle, through a whole APD pass whose K14 grows the WEAK set again
    h.reset(gpu_pkg.default_params(**p1))
    cams = [gpu_pkg.make_camera(sc.K[i], sc.R[i], sc.t[i], W, H, sc.depth_min, sc.depth_max) for i in range(N + 1)]
    h.upload_views(cams, imgs)
    h.upload_prior(*prior)
    o = common.make_oracle(ob, sc, imgs, N, p1, prior=prior)
    h.run()
    o.run()
    common.assert_state_equal(gpu_pkg, h, o, "APD pass on a re-armed handle")
    # a grown map through apd_upload_state: refused as well, until the prior is uploaded again
    grown = np.zeros((H, W), np.uint8)   # every pixel WEAK: twice what any list has room for
    h.set_state(gpu_pkg.STATE_WEAK_INFO, grown)
    with pytest.raises(gpu_pkg.ApdError, match="rewritten"):
        h.run_kernel(9)
    h.upload_prior(prior[0], prior[1], grown)
    assert h.weak_count == W * H
    for kid in (1, 2, 3, 4, 5):
        h.run_kernel(kid)
    h.run_sweeps(0, 1)                   # every list at its maximum length
    h.synchronize()
    h.close()
    o.close()
