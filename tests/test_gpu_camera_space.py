"""HIP path vs CPU oracle off the camera ring (tests/camera_space_cases.py): sources rolled by 37, 90 and 180 degrees, zoomed in and
out, fx != fy, principal points off the centre and outside the frame, forward motion, 40 to 50 degrees of convergence, sources that
see half of the reference frame, and sources with the surface behind them -- per-source intrinsics and rotations in ViewConst, the
LDS windows where a wave's footprint does not fit them, the fetch clamps far outside an image, the geometric term with real depth
maps of every view.

Every array of common.ORACLE_STATES is compared as raw bits after EVERY kernel of the three passes (FIRST_INIT, REFINE_INIT + APD,
REFINE_ITER + APD + geometric term).  Cases flagged `nans` leave NaN costs in the oracle (pixels no source sees): there, in an array
in which the oracle holds a NaN, a word that is NaN on both sides compares equal (common.assert_state_equal_nan_canonical).  That each case contains the geometry its name says is
asserted on the host by tests/test_camera_space_cases.py."""
import pytest

import camera_space_cases as cc
import common

pytestmark = pytest.mark.gpu

# kernels of fl.schedule with two iterations: FIRST_INIT has no WEAK pixel (no K3, K4, K9, K10), the two APD passes have
STEPS = (3 + 2 * 3 + 5) + 2 * (5 + 2 * 5 + 5)


def _equal(case):
    return common.assert_state_equal_nan_canonical if case.nans else common.assert_state_equal


def _walk(pkg, ob, synth, case, options=None, whole_run=False, split=False):
    """The three passes of `case`, each from common.postprocess of the one before, in lock-step with the oracle and compared after
    every kernel -- or, with whole_run, apd_run (split: the split entry points) against orc_run, compared after every pass.
    Returns the number of comparisons, each over every state array."""
    sc, imgs, deps = cc.scene(synth, case)
    equal = _equal(case)
    prior, compared = None, 0
    for pi in range(3):
        p = cc.pass_params(case, sc, pi)
        geom = bool(p.get("geom_consistency"))
        label = "%s%s, pass %d" % (case, " %r" % (options,) if options else "", pi)
        if split:
            cams = [pkg.make_camera(sc.K[i], sc.R[i], sc.t[i], case.W, case.H, sc.depth_min, sc.depth_max) for i in range(case.N + 1)]
            h = pkg.Handle(case.W, case.H, pkg.default_params(**p), device=0)
            h.upload_views_split(cams, imgs)
            if prior is not None:
                h.upload_prior(*prior)
        else:
            h = common.make_handle(pkg, sc, imgs, case.N, p, depths=deps if geom else None, prior=prior, options=options)
        o = common.make_oracle(ob, sc, imgs, case.N, p, depths=deps if geom else None, prior=prior)
        assert h.weak_count == o.weak_count, label
        if pi > 0:
            assert h.weak_count > 50, label   # the pass goes through K3, K4, K9 and K10
        if whole_run:
            if split:
                h.run_before_depths()
                if geom:
                    h.upload_depths(deps)
                h.run_after_depths()
            else:
                h.run()
            o.run()
            equal(pkg, h, o, label + ", apd_run")
            compared += 1
        else:
            for kid, it in cc.steps(p, h.weak_count):
                h.run_kernel(kid, it)
                o.run_kernel(kid, it)
                equal(pkg, h, o, "%s after K%d(iter %d)" % (label, kid, it))
                compared += 1
        planes, weak, views = h.download()
        prior = common.postprocess(planes, weak, views, p["depth_min"], p["depth_max"])
        h.close()
        o.close()
    print("CAMERA_SPACE %s%s: %d comparisons x %d arrays" % (case, " %r" % (options,) if options else "", compared, len(common.ORACLE_STATES)))
    return compared


@pytest.mark.parametrize("case", cc.CASES, ids=repr)
def test_every_kernel_of_three_passes(gpu_pkg, ob, synth, case):
    assert _walk(gpu_pkg, ob, synth, case) == STEPS


# window-less kernel against windowed kernel against oracle, and every NCC the reference evaluates, where the footprints leave the
# windows, the projections leave the image and the surface lies behind a source
ARM_CASES = ["roll90", "zoom_in2", "partial", "behind", "mixed"]
ARMS = [(cc.BY_NAME[n], {o: 0}) for n in ARM_CASES for o in ("k67_windows", "k1415_windows", "early_out")]
# the float texel-quad path on 8-bit input; the tiled copy never built, and built always and used by every global gather (with the
# windows off every sample goes through its offsets, the fetch positions far outside the image included)
ARMS += [(cc.BY_NAME["mixed"], o) for o in (dict(source_quads=0), dict(tiled_copy=0), dict(tiled_copy=2, k67_windows=0, k1415_windows=0))]


@pytest.mark.parametrize("case,options", ARMS, ids=["%s%s" % (c, "".join("-%s=%d" % kv for kv in o.items())) for c, o in ARMS])
def test_other_arms(gpu_pkg, ob, synth, case, options):
    assert _walk(gpu_pkg, ob, synth, case, options=options) == STEPS


@pytest.mark.parametrize("name,split", [("mixed", False), ("partial", False), ("mixed", True)], ids=["mixed", "partial", "mixed-split"])
def test_whole_pass(gpu_pkg, ob, synth, name, split):
    """apd_run, and apd_upload_views_split / apd_run_before_depths / apd_upload_depths / apd_run_after_depths, against orc_run."""
    assert _walk(gpu_pkg, ob, synth, cc.BY_NAME[name], whole_run=True, split=split) == 3
