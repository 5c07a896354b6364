"""The ORACLE ALONE on every case of tests/value_space_cases.py: bit equality of the HIP path with the oracle
(tests/test_gpu_value_space.py) shows something only where the case's values change what the oracle computes and where the frame
still holds work for every kernel, so each case is held to that here, on the host -- the refused image cases too (the oracle
takes any float).

  * every case: planes or costs after its last pass differ from the same pass on the clean input (scale_2^8 equals it in every bit,
    and bits of a view word past the last source move that word alone: value_space_cases says why);
  * the property its name promises, counted;
  * its `nans` flag is the set of state arrays in which the oracle holds a NaN word after some stepped kernel;
  * more than 50 WEAK pixels and a STRONG majority remain, except where the case is about having none;
  * scale_2^8: the costs after K5 are the byte images' costs, bit for bit, wherever no variance is near kMinVar.

Lines starting with VALUE_SPACE carry the counts."""
import numpy as np
import pytest

import common
import value_space_cases as vc
from test_oracle_float64 import _ncc_old64

fl = vc.fl
_CLEAN = {}
_RUNS = {}


def _state(o):
    return {name: getattr(o, oa).copy() for name, _, oa in common.ORACLE_STATES if name != "neighbours" or o.weak_count > 0}


def run_oracle(ob, synth, case, observe=None):
    """The oracle through the passes of `case` (None: the clean scene through FIRST, APD, GEOM); observe(pi, kid, it, oracle) after
    every kernel of a stepped pass.  Returns {pass index: state arrays after its last kernel}, the arrays that held a NaN after some
    stepped kernel, and the prior each pass left."""
    clean = case is None
    if clean:
        sc, imgs, deps = vc.scene(synth)
        passes, first = [vc.FIRST, vc.APD, vc.GEOM], 0
    else:
        sc, imgs, deps = vc.inputs(synth, case)
        passes, first = case.passes, case.first_stepped
    out, nans, priors, prior = {}, set(), {}, None
    for pi in range(len(passes)):
        p = common.base_params(sc, vc.N, **passes[pi])
        if pi < first:          # the clean run's prior: those passes read nothing the case edits
            prior = clean_run(ob, synth)[2][pi]
            continue
        if not clean and case.group == "prior":
            prior = vc.crafted_prior(case, prior, p)
        o = common.make_oracle(ob, sc, imgs, vc.N, p, depths=deps if p.get("geom_consistency") else None, prior=prior)
        for kid, it in vc.steps(p, o.weak_count):
            o.run_kernel(kid, it)
            nans |= {name for name, _, oa in common.ORACLE_STATES
                     if getattr(o, oa).dtype == np.float32 and (name != "neighbours" or o.weak_count > 0) and bool(np.isnan(getattr(o, oa)).any())}
            if observe is not None:
                observe(pi, kid, it, o)
        out[pi] = _state(o)
        prior = common.postprocess(o.planes.copy(), o.weak_info.copy(), o.selected_views.copy(), np.float32(p["depth_min"]), np.float32(p["depth_max"]))
        priors[pi] = prior
        o.close()
    return out, nans, priors


def clean_run(ob, synth):
    if not _CLEAN:
        _CLEAN["run"] = run_oracle(ob, synth, None)
    return _CLEAN["run"]


def case_run(ob, synth, case):
    """run_oracle of a case, once per case (the tests of this file share it and never write to it)."""
    if case.name not in _RUNS:
        seen = {}

        def observe(pi, kid, it, o):
            if kid == 2:
                seen["strong_in"] = int((o.weak_info == fl.STRONG).sum())
                seen["nearest"] = o.nearest_strong.copy()
            if kid == 5 and pi == 0:
                seen["k5_views"], seen["k5_costs"] = o.selected_views.copy(), o.costs.copy()
            if kid == 6 and it == 0 and pi == 0:
                seen["k6_costs"] = o.costs.copy()
            if kid == 14 and pi == 0:
                seen["k14_weak"] = o.weak_info.copy()
        _RUNS[case.name] = run_oracle(ob, synth, case, observe) + (seen,)
    return _RUNS[case.name]


def _differing(a, b):
    """{state: pixels (rows) whose bytes differ}; NaNs of both sides compare equal."""
    out = {}
    for name in a:
        if name not in b or a[name].shape != b[name].shape:
            out[name] = -1   # the neighbour table exists on one side only, or has another length
            continue
        rows = a[name].shape[0] * (1 if name == "neighbours" else a[name].shape[1])
        n = int((common.canon_nan(a[name]).reshape(rows, -1) != common.canon_nan(b[name]).reshape(rows, -1)).any(axis=1).sum())
        if n:
            out[name] = n
    return out


def ref_variance(img):
    """The reference patch's variance at every pixel, float64: 36 samples at offsets -5..5 step 2, clamped coordinates."""
    img = img.astype(np.float64)
    ys, xs = np.mgrid[0:vc.H, 0:vc.W]
    s = np.stack([img[np.clip(ys + j, 0, vc.H - 1), np.clip(xs + i, 0, vc.W - 1)] for i in range(-5, 6, 2) for j in range(-5, 6, 2)])
    return (s * s).mean(0) - s.mean(0) ** 2


@pytest.mark.parametrize("case", vc.ALL_CASES, ids=repr)
def test_a_case_moves_the_oracle_flags_its_nans_and_leaves_work(ob, synth, case):
    out, nans, _, _ = case_run(ob, synth, case)
    last = len(case.passes) - 1
    clean = clean_run(ob, synth)[0][last]
    diff = _differing(out[last], clean)
    weak, strong = int((out[last]["weak"] == fl.WEAK).sum()), int((out[last]["weak"] == fl.STRONG).sum())
    print("VALUE_SPACE %s: pixels that differ from the clean input after pass %d %s; NaN words in %s; WEAK %d, STRONG %d of %d"
          % (case, last, diff or "NONE", sorted(nans) or "no array", weak, strong, vc.W * vc.H))
    if case.clean_equal:
        assert not diff, "a power-of-two scale that moves no variance across kMinVar leaves every bit of the oracle's state"
    elif case.name in vc.MOVES_VIEWS_ONLY:
        assert set(diff) == {"views"}
    else:
        assert "planes" in diff or "costs" in diff, "the oracle computes the same with and without the case's values: it can catch nothing"
    assert nans == set(case.nans), "tests/test_gpu_value_space.py compares NaN words as one pattern exactly where the oracle leaves some"
    if case.name not in vc.NO_WORK_BOUND:
        assert weak > 50 and 2 * strong > vc.W * vc.H, (weak, strong)
    if case.group == "image":
        sc, imgs, _ = vc.inputs(synth, case)
        assert case.refused == (not vc.in_pixel_domain(imgs)), "refused are exactly the cases with a pixel outside the domain"


def test_scale_257_has_variances_past_the_8_bit_bound(ob, synth):
    _, imgs, _ = vc.inputs(synth, vc.BY_NAME["scale_257"])
    var = ref_variance(imgs[0])
    textured = var >= 257.0 ** 2 * 1e-5
    above = int((var[textured] > 1.7e4).sum())
    print("VALUE_SPACE scale_257: %d of %d non-flat reference patches have a variance above 1.7e4, the largest %.3g" % (above, int(textured.sum()), var.max()))
    assert 2 * above > int(textured.sum()) > 1000
    assert float(imgs[0].max()) <= 65535.0 and float(imgs[0].max()) > 255.0 * 200


def _flat_nccs(ob, sc, imgs):
    """(pixel, source) pairs whose NCC at the pixel's initial plane projects inside the source and still costs 2.0: a flat patch."""
    p = common.base_params(sc, vc.N, **vc.FIRST)
    o = common.make_oracle(ob, sc, imgs, vc.N, p)
    for kid in (1, 2, 5):
        o.run_kernel(kid, 0)
    planes, n = o.planes.copy(), 0
    for y in range(vc.H):
        for x in range(vc.W):
            for src in range(1, vc.N + 1):
                if o.ncc_old(x, y, src, planes[y, x]) == 2.0 and _ncc_old64(sc, imgs, x, y, src, planes[y, x].astype(np.float64))[1] < 1.0:
                    n += 1
    o.close()
    return n


def test_unit_has_more_flat_patches_than_the_bytes(ob, synth):
    """synth's noise keeps the variance of every 36-sample REFERENCE patch above 0.7 grey levels^2, and 0.7 / 255^2 = 1.08e-5 is still
    above kMinVar: neither image kind has a flat reference patch (both counts are printed).  The bilinear taps smooth that noise in the
    source patches: there the [0, 1] images have flat patches and the bytes have none, counted over the NCCs of K5."""
    sc, bytes_, _ = vc.scene(synth)
    _, unit, _ = vc.inputs(synth, vc.BY_NAME["unit"])
    ref_b, ref_u = int((ref_variance(bytes_[0]) < vc.K_MIN_VAR).sum()), int((ref_variance(unit[0]) < vc.K_MIN_VAR).sum())
    flat_b, flat_u = _flat_nccs(ob, sc, bytes_), _flat_nccs(ob, sc, unit)
    print("VALUE_SPACE unit: flat reference patches %d (bytes %d), smallest reference variance %.3g (bytes %.3g); NCCs of K5 with a flat patch %d (bytes %d)"
          % (ref_u, ref_b, ref_variance(unit[0]).min(), ref_variance(bytes_[0]).min(), flat_u, flat_b))
    assert ref_u >= ref_b and flat_u > flat_b
    assert float(unit[0].max()) <= 1.0 and float(unit[0].min()) >= 0.0


@pytest.mark.parametrize("name", ["centred", "u8_edge_256", "u8_edge_half", "u8_edge_neg", "u8_neg_zero", "saturated"])
def test_the_8_bit_edge_cases_hold_the_value_they_name(synth, name):
    _, clean, _ = vc.scene(synth)
    _, imgs, _ = vc.inputs(synth, vc.BY_NAME[name])
    is_u8 = [bool(((im >= 0) & (im <= 255) & (im == np.floor(im))).all()) for im in imgs]
    if name.startswith("u8_edge"):
        off = [int((a != b).sum()) for a, b in zip(imgs, clean)]
        assert off == [1 if v == vc.POISONED_SOURCE else 0 for v in range(vc.N + 1)], off      # one pixel of one source
        assert is_u8 == [v != vc.POISONED_SOURCE for v in range(vc.N + 1)]                      # ... takes that image off the 8-bit values
    elif name == "centred":
        assert not any(is_u8) and all(bool((im == np.floor(im)).all()) and float(im.min()) < 0 for im in imgs)
    elif name == "u8_neg_zero":
        zeros = [int(((im == 0) & np.signbit(im)).sum()) for im in imgs]
        print("VALUE_SPACE u8_neg_zero: -0.0 pixels per view", zeros)
        assert all(is_u8) and min(zeros) >= 30 and not any(bool(((im == 0) & ~np.signbit(im)).any()) for im in imgs)
    else:
        assert all(is_u8) and all(set(np.unique(im)) == {0.0, 255.0} for im in imgs)
        assert ref_variance(imgs[0]).max() > 0.24 * 255.0 ** 2      # (255 / 2)^2 is the largest variance of values in 0..255


def test_neg_zero_pixels_compute_what_zero_pixels_do(ob, synth):
    """Every sum of an NCC starts at +0.0f and a bilinear tap of -0.0 texels adds to one, so the oracle's state on -0.0 pixels is, bit
    for bit, its state on +0.0 pixels: an upload that treats -0.0 as the 8-bit value 0 loses nothing."""
    case = vc.BY_NAME["u8_neg_zero"]
    as_zero = vc.Case("u8_pos_zero", "image", lambda imgs: vc._neg_zero(imgs, 0.0))
    a, b = case_run(ob, synth, case)[0], run_oracle(ob, synth, as_zero)[0]
    assert not _differing(a[0], b[0]) and not _differing(a[1], b[1])


def test_flat_source_is_selected_nowhere(ob, synth):
    seen = case_run(ob, synth, vc.BY_NAME["flat_source"])[3]
    bit = np.uint32(1 << (vc.POISONED_SOURCE - 1))
    chosen = int(((seen["k5_views"] & bit) != 0).sum())
    others = int(((seen["k5_views"] & ~bit) != 0).sum())
    print("VALUE_SPACE flat_source: pixels that select the flat view after K5 %d, another view %d" % (chosen, others))
    assert chosen == 0 and others > vc.W * vc.H // 2


def test_flat_all_costs_two_everywhere_and_leaves_every_pixel_unknown(ob, synth):
    """Every NCC of constant images is 2.0 (var < kMinVar) and K5 selects no view.  K14 then finds no valid view at any pixel inside
    its 6-px margin and marks it UNKNOWN as it marks the margin (APD.cu:1990-2144: not WEAK -- a pixel is WEAK only with a view to
    measure its cost profile in), so the APD pass starts from a prior without one WEAK or STRONG pixel."""
    out, _, priors, seen = case_run(ob, synth, vc.BY_NAME["flat_all"])
    assert (seen["k5_costs"] == np.float32(2.0)).all() and not seen["k5_views"].any()
    # the sweep divides a zero cost sum by a zero weight sum where it scores a hypothesis
    assert ((seen["k6_costs"] == np.float32(2.0)) | np.isnan(seen["k6_costs"])).all()
    weak = seen["k14_weak"]
    print("VALUE_SPACE flat_all: after K14 of the first pass WEAK %d, STRONG %d, UNKNOWN %d; STRONG pixels the APD pass starts from %d"
          % (int((weak == fl.WEAK).sum()), int((weak == fl.STRONG).sum()), int((weak == fl.UNKNOWN).sum()), seen["strong_in"]))
    assert (weak == fl.UNKNOWN).all() and (priors[0][2] == fl.UNKNOWN).all()
    assert seen["strong_in"] == 0 and "neighbours" not in out[1]
    assert ((out[1]["costs"] == np.float32(2.0)) | np.isnan(out[1]["costs"])).all()


def test_prior_all_weak_gives_k2_no_strong_pixel(ob, synth):
    seen = case_run(ob, synth, vc.BY_NAME["prior_all_weak"])[3]
    assert seen["strong_in"] == 0
    assert (seen["nearest"] == -1).all()


@pytest.mark.parametrize("name", ["prior_all_strong", "prior_all_unknown", "prior_weak_checker", "prior_views_0", "prior_views_high_bits"])
def test_crafted_maps_and_view_words_are_what_they_name(ob, synth, name):
    case = vc.BY_NAME[name]
    sc = vc.scene(synth)[0]
    clean = clean_run(ob, synth)[2][0]
    planes, views, weak = vc.crafted_prior(case, clean, vc.params(sc, 1, case))
    ys, xs = np.mgrid[0:vc.H, 0:vc.W]
    if name == "prior_all_strong":
        assert (weak == fl.STRONG).all()
    elif name == "prior_all_unknown":
        assert (weak == fl.UNKNOWN).all()
    elif name == "prior_weak_checker":
        assert ((weak == fl.WEAK) == ((xs + ys) % 2 == 0)).all()
    elif name == "prior_views_0":
        assert not views[vc.STRIPE].any() and int((clean[1][vc.STRIPE] != 0).sum()) > 500
    else:
        assert ((views[vc.STRIPE] >> vc.N) == (0xFFFFFFFF >> vc.N)).all() and ((views[vc.STRIPE] & 7) == (clean[1][vc.STRIPE] & 7)).all()


def _geom_costs(ob, synth, deps, planes):
    """The oracle's geometric term of every (source, pixel) at the given camera-frame planes."""
    sc, imgs, _ = vc.scene(synth)
    o = common.make_oracle(ob, sc, imgs, vc.N, common.base_params(sc, vc.N, **vc.GEOM), depths=deps, prior=clean_run(ob, synth)[2][1])
    out = np.array([[[o.geom_cost(x, y, v, planes[y, x]) for x in range(vc.W)] for y in range(vc.H)] for v in range(1, vc.N + 1)], np.float32)
    o.close()
    return out


@pytest.fixture(scope="module")
def geom_planes(ob, synth):
    """Camera-frame planes of the clean geometric pass after K5, and the clean depth maps' geometric terms at them."""
    sc, imgs, deps = vc.scene(synth)
    o = common.make_oracle(ob, sc, imgs, vc.N, common.base_params(sc, vc.N, **vc.GEOM), depths=deps, prior=clean_run(ob, synth)[2][1])
    for kid, it in ((1, 0), (2, 0), (3, 0), (4, 0), (5, 0)):
        o.run_kernel(kid, it)
    planes = o.planes.copy()
    o.close()
    return planes, _geom_costs(ob, synth, deps, planes)


@pytest.mark.parametrize("case", vc.DEPTH_CASES, ids=repr)
def test_a_depth_case_changes_the_geometric_term_in_every_poisoned_view(ob, synth, case, geom_planes):
    planes, clean = geom_planes
    _, _, deps = vc.inputs(synth, case)
    _, _, clean_deps = vc.scene(synth)
    poisoned = [v for v in range(1, vc.N + 1) if not np.array_equal(common.bits(deps[v]), common.bits(clean_deps[v]))]
    costs = _geom_costs(ob, synth, deps, planes)
    changed = [int((common.canon_nan(costs[v - 1]).view(np.uint32) != common.canon_nan(clean[v - 1]).view(np.uint32)).sum()) for v in range(1, vc.N + 1)]
    print("VALUE_SPACE %s: poisoned sources %s, pixels whose geometric term changed per source %s" % (case, poisoned, changed))
    assert poisoned == ([vc.POISONED_SOURCE] if case.name == "depth_zero_view" else list(range(1, vc.N + 1)))
    assert all(changed[v - 1] > 0 for v in poisoned)
    if case.name == "depth_zero_all":
        assert (costs == np.float32(3.0)).all()     # every geometric term is max_cost
    if case.name == "depth_neg_zero":
        # -0.0 == 0.0f: a hole.  The same pixels set to +0.0 give the same terms, and the same state after the whole pass
        share = vc.DEPTH_VALUES["depth_neg_zero"][0]
        as_zero = vc.Case("depth_pos_zero", "depth", vc._poison("depth_neg_zero", 0.0))
        zdeps = vc.inputs(synth, as_zero)[2]
        assert all(int(((deps[v] == 0) & np.signbit(deps[v])).sum()) >= int(vc.depth_mask(v, 0.0, share).sum()) > 0 for v in poisoned)
        assert np.array_equal(common.bits(costs), common.bits(_geom_costs(ob, synth, zdeps, planes)))
        assert not _differing(case_run(ob, synth, case)[0][2], run_oracle(ob, synth, as_zero)[0][2])


def test_power_of_two_scale_leaves_the_costs_bit_for_bit(ob, synth):
    """Binary32 arithmetic is scale-covariant under a power of two while nothing over- or underflows: sums, variances and the
    covariance of the images times 2^8 are the byte images' times 2^8 and 2^16, and the quotient is the same -- only the test
    against kMinVar is absolute.  Outside the pixels where a variance (reference patch, or a source patch at the pixel's plane,
    float64) or its 2^16-fold lies within a factor 2^16 of kMinVar the costs after K5 are equal bit for bit."""
    sc, imgs, _ = vc.scene(synth)
    seen = case_run(ob, synth, vc.BY_NAME["scale_2^8"])[3]
    p = common.base_params(sc, vc.N, **vc.FIRST)
    o = common.make_oracle(ob, sc, imgs, vc.N, p)
    for kid in (1, 2, 5):
        o.run_kernel(kid, 0)
    costs, planes = o.costs.copy(), o.planes.copy()
    o.close()
    lo, hi = float(vc.K_MIN_VAR) / 2.0 ** 32, float(vc.K_MIN_VAR) * 2.0 ** 16

    def near(v):
        return (v >= lo) & (v <= hi)
    excluded = near(ref_variance(imgs[0]))
    for y in range(vc.H):
        for x in range(vc.W):
            for src in range(1, vc.N + 1):
                excluded[y, x] |= bool(near(_ncc_old64(sc, imgs, x, y, src, planes[y, x].astype(np.float64))[1]))
    differ = costs.view(np.uint32) != seen["k5_costs"].view(np.uint32)
    print("VALUE_SPACE scale_2^8: excluded pixels %d of %d (%.2f %%), costs that differ after K5 %d, outside the excluded pixels %d; costs below 2 %d"
          % (int(excluded.sum()), excluded.size, 100.0 * excluded.mean(), int(differ.sum()), int((differ & ~excluded).sum()), int((costs < 2).sum())))
    assert excluded.mean() <= 0.02
    assert not (differ & ~excluded).any()
    assert int((costs < 2).sum()) > vc.W * vc.H // 2      # the equality is one of real NCC values, not of 2.0 = 2.0
