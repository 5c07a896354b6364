"""HIP path vs CPU oracle off the parameter values one reference schedule produces (tests/param_space_cases.py): 19, 24 and 31
source views through FIRST_INIT, REFINE_INIT + APD and REFINE_ITER + APD + geometric term; top_k at every arm of K5;
rotate_time = 1; geom_factor zero, negative and large; six iterations; depth ranges that leave K3 without a distance cut.

Every array of common.ORACLE_STATES is compared as raw bits after EVERY kernel (top_k <= 0 leaves NaN costs in the oracle: there
a word that is NaN on both sides compares equal, as in tests/test_gpu_edge_cases.py).  That the oracle's own result moves with each
of these parameters -- so that a kernel which ignored one could not pass -- is asserted on the host by
tests/test_param_space_cases.py.  No case has a rotate_time outside 1..4: apd_create refuses those (tests/test_gpu_errors.py)."""
import ctypes as C

import numpy as np
import pytest

import common
import param_space_cases as pc

pytestmark = pytest.mark.gpu

_PRIORS = {}


# a float word that is NaN on both sides compares equal whatever its sign and payload; a NaN on one side only differs
_states_equal_nan_canonical = common.assert_state_equal_nan_canonical


def _walk(pkg, ob, synth, case, options=None, every_pass=False, equal=common.assert_state_equal, whole_run=False):
    """The passes of `case` in order, each from common.postprocess of the one before.  The last pass (every pass with every_pass)
    runs in lock-step with the oracle over pc.steps, compared after every kernel -- or, with whole_run, as apd_run against orc_run.
    The passes before it only build the prior: apd_run with default options, kept per (scene, parameters) and never written to."""
    sc, imgs, deps = pc.scene(synth, case)
    prior, plist, last = None, [], len(case.passes) - 1
    compared = 0
    for pi in range(len(case.passes)):
        p = pc.pass_params(case, sc, pi)
        plist.append(sorted(p.items()))
        d = deps if p.get("geom_consistency") else None
        if pi < last and not every_pass:
            key = (case.W, case.H, case.N, case.scene_seed, case.textureless, case.floats, repr(plist))
            if key not in _PRIORS:
                h = common.make_handle(pkg, sc, imgs, case.N, p, depths=d, prior=prior)
                h.run()
                planes, weak, views = h.download()
                _PRIORS[key] = common.postprocess(planes, weak, views, p["depth_min"], p["depth_max"])
                h.close()
            prior = _PRIORS[key]
            continue
        h = common.make_handle(pkg, sc, imgs, case.N, p, depths=d, prior=prior, options=options)
        o = common.make_oracle(ob, sc, imgs, case.N, p, depths=d, prior=prior)
        label = "%s%s, pass %d" % (case, " %r" % (options,) if options else "", pi)
        assert h.weak_count == o.weak_count, label
        if pi > 0:
            assert h.weak_count > 50, label   # the pass goes through K3, K4, K9 and K10
        if whole_run:
            h.run()
            o.run()
            equal(pkg, h, o, label + ", apd_run")
            compared += 1
        else:
            for kid, it in pc.steps(case, pi, p, h.weak_count):
                h.run_kernel(kid, it)
                o.run_kernel(kid, it)
                equal(pkg, h, o, "%s after K%d(iter %d)" % (label, kid, it))
                compared += 1
        planes, weak, views = h.download()
        prior = common.postprocess(planes, weak, views, p["depth_min"], p["depth_max"])
        h.close()
        o.close()
    return compared


# every bit-preserving option of the sweep and refinement kernels on its other arm, one at a time, at N = 31 on 8-bit images
# (source_quads = 0 sends them down the float texel-quad path)
VIEW_ARMS = [(c, {}) for c in pc.VIEW_CASES] + [(pc.VIEW_CASES[2], {name: 0}) for name in ("k67_windows", "k1415_windows", "early_out", "source_quads")]


@pytest.mark.parametrize("case,options", VIEW_ARMS, ids=["%s%s" % (c, "".join("-%s=%d" % kv for kv in o.items())) for c, o in VIEW_ARMS])
def test_19_to_31_source_views_through_every_pass_kind(gpu_pkg, ob, synth, case, options):
    """The NMAX = 32 instantiations of K6/K7 and K9/K10 with and without the LDS source windows, K14's pair walk and K15 over up to
    31 selected views, the geometric term of every upper view: three pass kinds of two iterations, every kernel compared."""
    assert case.N > 18 and pc.VIEW_CASES[2].N == 31 and not pc.VIEW_CASES[2].floats
    n = _walk(gpu_pkg, ob, synth, case, options=options, every_pass=True)
    assert n == (3 + 2 * 3 + 5) + 2 * (5 + 2 * 5 + 5)   # FIRST_INIT has no K3, K4, K9, K10; the two APD passes have all of them


@pytest.mark.parametrize("case", pc.TOP_K_CASES, ids=repr)
def test_top_k_at_every_arm_of_the_initial_costs(gpu_pkg, ob, synth, case):
    """K5 with top_k <= 0 (cost 2.0, no view), 1, 2, N and above N at N = 5, and the sweep that starts from its result.  With no
    view selected K6 leaves NaN costs in the oracle too (0 / 0): those two cases compare NaN words as one pattern."""
    equal = _states_equal_nan_canonical if case.nans else common.assert_state_equal
    assert _walk(gpu_pkg, ob, synth, case, equal=equal) == len(pc.TOP_K_KERNELS)


@pytest.mark.parametrize("case", pc.ROTATE_CASES, ids=repr)
def test_rotate_time_one(gpu_pkg, ob, synth, case):
    """One ray per direction; the jitter range of K3 is 8, the widest its jittered arm sees."""
    _walk(gpu_pkg, ob, synth, case)


GEOM_ARMS = [(c, dict(early_out=e)) for c in pc.GEOM_FACTOR_CASES for e in (1, 0)]
# the negative value again on the window-less K14 / K15
GEOM_ARMS += [(pc.GEOM_FACTOR_CASES[1], dict(early_out=e, k1415_windows=0)) for e in (1, 0)]


@pytest.mark.parametrize("case,options", GEOM_ARMS, ids=["%s%s" % (c, "".join("-%s=%d" % kv for kv in o.items())) for c, o in GEOM_ARMS])
def test_geom_factor_zero_negative_and_large(gpu_pkg, ob, synth, case, options):
    """The geometric pass.  A negative factor switches the refinement bound of K9/K10 and K15 off (the bound needs a non-negative
    geometric term): with APD_OPT_EARLY_OUT = 1 the kernels must then compute what they compute with 0 -- the oracle's bits."""
    assert pc.GEOM_FACTOR_CASES[1].passes[-1]["geom_factor"] < 0
    _walk(gpu_pkg, ob, synth, case, options=options)


@pytest.mark.parametrize("whole_run", [False, True], ids=["lockstep", "apd_run"])
def test_six_iterations(gpu_pkg, ob, synth, whole_run):
    """Iterations 3, 4 and 5: the view-selection threshold exp(iter^2 / -90) and the iteration-dependent windows of K6/K7."""
    case = pc.ITER_CASES[0]
    n = _walk(gpu_pkg, ob, synth, case, whole_run=whole_run)
    assert n == (1 if whole_run else 3 + 6 * 3 + 5)


@pytest.mark.parametrize("case", pc.DEPTH_CASES, ids=repr)
def test_depth_range_without_a_distance_cut(gpu_pkg, ob, synth, case):
    """depth_max == depth_min and depth_max < depth_min in a REFINE_INIT pass: ransac_distance_cut finds no cut and K3 divides by
    the range as the reference does (no inlier at 0, every point an inlier below 0); the sweeps draw their depths from the same
    range."""
    sc = pc.scene(synth, case)[0]
    lo, hi = pc.depth_range(case, sc)
    cut = gpu_pkg.lib().apd_ransac_distance_cut
    cut.argtypes = [C.c_float, C.c_float, C.c_float, C.POINTER(C.c_float)]
    assert cut(lo, hi, case.passes[-1]["ransac_threshold"], None) == 0   # the arm under test is the one without a cut
    assert not case.nans   # the oracle leaves no NaN here (tests/test_param_space_cases.py): raw bits
    _walk(gpu_pkg, ob, synth, case)
