"""HIP path vs CPU oracle off the value range of the uploaded arrays (tests/value_space_cases.py): pixel values scaled by 2^8, 2^-8
and 257, in [0, 1], centred on zero, offset by 1e6, one pixel off the 8-bit values in one source, -0.0 pixels, a 0 / 255 checker, flat
images and a flat source; depth maps with NaN, +-inf, -0.0, denormal, huge and negative entries and maps that are zero everywhere;
priors with zero, NaN, long and back-facing normals, depths of 0, below 0, inf and outside the range, view words without a bit and
with bits past the last source, and WEAK maps that are all WEAK, all STRONG, all UNKNOWN and a checkerboard.

Every array of common.ORACLE_STATES is compared as raw bits after EVERY kernel of the stepped passes; cases whose oracle state holds
NaN words (`nans`, measured by tests/test_value_space_cases.py) compare through common.assert_state_equal_nan_canonical.  That each
case moves what the oracle computes is asserted on the host by that file.

Images with a pixel outside the domain of the C ABI (non-finite, or |v| > 2^20: `refused`) are not compared: every upload entry point
answers APD_ERR_UNSUPPORTED and names the view, and the handle takes a clean upload afterwards."""
import ctypes as C

import numpy as np
import pytest

import common
import value_space_cases as vc

pytestmark = pytest.mark.gpu

APD_ERR_UNSUPPORTED = -5
_PRIORS = {}


def _equal(case):
    return common.assert_state_equal_nan_canonical if case.nans else common.assert_state_equal


def _cams(pkg, sc):
    return [pkg.make_camera(sc.K[i], sc.R[i], sc.t[i], vc.W, vc.H, sc.depth_min, sc.depth_max) for i in range(vc.N + 1)]


def _clean_prior(pkg, synth, pi):
    """common.postprocess of pass `pi` of the clean scene (apd_run), built once and never written to."""
    if pi not in _PRIORS:
        sc, imgs, _ = vc.scene(synth)
        p = common.base_params(sc, vc.N, **[vc.FIRST, vc.APD][pi])
        h = common.make_handle(pkg, sc, imgs, vc.N, p, prior=_clean_prior(pkg, synth, pi - 1) if pi else None)
        h.run()
        planes, weak, views = h.download()
        _PRIORS[pi] = common.postprocess(planes, weak, views, p["depth_min"], p["depth_max"])
        h.close()
    return _PRIORS[pi]


def _walk(pkg, ob, synth, case, shared=False):
    """The stepped passes of `case` in lock-step with the oracle, compared after every kernel; shared: the images go through
    apd_image_create + apd_upload_views_shared.  Returns the number of comparisons, each over every state array."""
    sc, imgs, deps = vc.inputs(synth, case)
    equal = _equal(case)
    prior = _clean_prior(pkg, synth, case.first_stepped - 1) if case.first_stepped else None
    compared, images = 0, []
    for pi in range(case.first_stepped, len(case.passes)):
        p = vc.params(sc, pi, case)
        if case.group == "prior":
            prior = vc.crafted_prior(case, prior, p)
        d = deps if p.get("geom_consistency") else None
        label = "%s%s%s, pass %d" % (case, " %r" % (case.options,) if case.options else "", " shared" if shared else "", pi)
        if shared:
            images = images or [pkg.SharedImage(vc.W, vc.H, im) for im in imgs]
            h = pkg.Handle(vc.W, vc.H, pkg.default_params(**p), device=0)
            h.upload_views_shared(_cams(pkg, sc), images)
            if prior is not None:
                h.upload_prior(*prior)
        else:
            h = common.make_handle(pkg, sc, imgs, vc.N, p, depths=d, prior=prior, options=case.options)
        o = common.make_oracle(ob, sc, imgs, vc.N, p, depths=d, prior=prior)
        assert h.weak_count == o.weak_count, label
        for kid, it in vc.steps(p, h.weak_count):
            h.run_kernel(kid, it)
            o.run_kernel(kid, it)
            equal(pkg, h, o, "%s after K%d(iter %d)" % (label, kid, it))
            compared += 1
        planes, weak, views = h.download()
        prior = common.postprocess(planes, weak, views, p["depth_min"], p["depth_max"])
        h.close()
        o.close()
    for im in images:
        im.close()
    return compared


def _refusal(pkg, synth, case, shared):
    """Every upload entry point answers APD_ERR_UNSUPPORTED for the images of `case` and names the first offending view; no kernel of a
    pass has run, and the same handle then takes the clean images and gives the oracle's bits (asserted by the caller)."""
    L = pkg.lib()
    sc, imgs, _ = vc.inputs(synth, case)
    bad = [v for v, im in enumerate(imgs) if not vc.in_pixel_domain([im])]
    assert bad
    p = vc.params(sc, 0, case)
    h = pkg.Handle(vc.W, vc.H, pkg.default_params(**p), device=0)
    cams = _cams(pkg, sc)
    cam_arr = (pkg.Camera * len(cams))(*cams)
    ptrs = (C.c_void_p * len(imgs))(*[im.ctypes.data for im in imgs])
    if shared:
        for v, im in enumerate(imgs):
            out = C.c_void_p()
            rc = L.apd_image_create(C.byref(out), 0, vc.W, vc.H, C.c_void_p(im.ctypes.data))
            if v in bad:
                assert rc == APD_ERR_UNSUPPORTED and out.value is None, (case, v, rc)
                message = L.apd_last_error().decode()
                assert "apd_image_create" in message and "2^20" in message, message
            else:
                assert rc == 0
                L.apd_image_destroy(out)
    else:
        for name, args in (("apd_upload_views", (ptrs, None)), ("apd_upload_views_split", (ptrs,))):
            assert getattr(L, name)(h._h, len(cams), cam_arr, *args) == APD_ERR_UNSUPPORTED, (case, name)
            message = L.apd_last_error().decode()
            assert name in message and "view %d" % bad[0] in message and "2^20" in message, message
            with pytest.raises(pkg.ApdError, match="apd_upload_views"):
                h.run()      # the refused upload armed nothing
    return h


@pytest.mark.parametrize("shared", [False, True], ids=["upload", "shared"])
@pytest.mark.parametrize("case", vc.IMAGE_CASES, ids=repr)
def test_image_values(gpu_pkg, ob, synth, case, shared):
    """FIRST_INIT, then REFINE_INIT + APD, on the edited images: the 8-bit test of the upload, the float texel-quad path at other
    exponents, the NCC tail at variances up to 9e7 (the 8-bit bound is 1.7e4), flat and saturated patches.  `shared`: apd_image_create decides 8-bit or not per
    image and apd_upload_views_shared ANDs the answers -- u8_edge_* has one float image among 8-bit ones."""
    if not case.refused:
        assert _walk(gpu_pkg, ob, synth, case, shared=shared) >= 2 * (3 + 2 * 3 + 5)
        return
    h = _refusal(gpu_pkg, synth, case, shared)
    sc, imgs, _ = vc.scene(synth)
    p = vc.params(sc, 0, case)
    if shared:
        images = [gpu_pkg.SharedImage(vc.W, vc.H, im) for im in imgs]
        h.upload_views_shared(_cams(gpu_pkg, sc), images)
    else:
        h.upload_views(_cams(gpu_pkg, sc), imgs)
    o = common.make_oracle(ob, sc, imgs, vc.N, p)
    h.run()
    o.run()
    common.assert_state_equal(gpu_pkg, h, o, "%s: a clean upload after the refused one" % case)
    h.close()
    o.close()


@pytest.mark.parametrize("case", vc.DEPTH_CASES + vc.DEPTH_ARM_CASES, ids=repr)
def test_depth_map_values(gpu_pkg, ob, synth, case):
    """The geometric pass on poisoned depth maps: src_depth == 0.0f must hold for -0.0 and for nothing else, and a NaN, infinite,
    negative or huge reprojection error must cap at max_cost as fminf does in the oracle -- with the refinement bound of K9/K10 and
    K15 (early_out) on and off, and on the window-less kernels."""
    assert _walk(gpu_pkg, ob, synth, case) == 5 + 2 * 5 + 5


@pytest.mark.parametrize("case", vc.PRIOR_CASES, ids=repr)
def test_prior_values(gpu_pkg, ob, synth, case):
    """REFINE_INIT + APD from a crafted prior: K5's stored-view arm, K2 / K3 / K8 and K9 / K10 on planes, view words and WEAK maps no
    pass of the library produces."""
    n = _walk(gpu_pkg, ob, synth, case)
    assert n == (5 + 2 * 5 + 5 if case.name not in ("prior_all_strong", "prior_all_unknown") else 3 + 2 * 3 + 5)
