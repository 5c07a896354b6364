"""The ORACLE ALONE on every case of tests/camera_space_cases.py: bit equality of the HIP path with the oracle
(tests/test_gpu_camera_space.py) exercises a camera geometry only where the case really contains it, so each case is held to what
its name says here, on the host, from the oracle's state and the cameras in numpy.

  * footprints: the 32 x 4 checkerboard footprint of a K6/K7 wave and the 8 x 8 footprint of K14/K15, projected into every source
    with the depths the oracle holds after its FIRST pass, fit a 64 x 20 (64 x 32) window with 6 texels of margin -- always on the
    ring (the control: what the suite covered before these cases), never by rows under a 90 degree roll, never by columns at twice
    the focal length;
  * partial / behind: the shares of reference pixels that project left of, right of, above and below a source, and behind one;
  * every case: more than 50 WEAK pixels enter the APD and the geometric pass, and the share of interior pixels within 1 % of the
    rendered depth after the three passes is the one written into the case table (minus 2 points).

Lines starting with CAMERA_SPACE carry the figures."""
import numpy as np
import pytest

import camera_space_cases as cc
import common

_RECORDS = {}
MARGIN = 6     # texels on each side of the box of projected centres: the 11 x 11 patch (radius 5) and one entry for rounding


def record(ob, synth, case):
    """The oracle through the three passes of `case`, every kernel stepped; what the tests below read of it, kept per case."""
    if case.name in _RECORDS:
        return _RECORDS[case.name]
    sc, imgs, deps = cc.scene(synth, case)
    rec = dict(weak=[], after_k5=[], selected=np.zeros((case.H, case.W), np.uint32), nans=False)
    prior = None
    for pi in range(3):
        p = cc.pass_params(case, sc, pi)
        o = common.make_oracle(ob, sc, imgs, case.N, p, depths=deps if p.get("geom_consistency") else None, prior=prior)
        rec["weak"].append(o.weak_count)
        for kid, it in cc.steps(p, o.weak_count):
            o.run_kernel(kid, it)
            if kid == 5:
                rec["after_k5"].append(o.selected_views.copy())
            if kid in (5, 6, 7, 9, 10):
                rec["selected"] |= o.selected_views
            rec["nans"] |= any(bool(np.isnan(getattr(o, oa)).any()) for _, _, oa in common.ORACLE_STATES
                               if getattr(o, oa).dtype == np.float32 and (oa != "neighbours"))
        if pi == 0:
            rec["first_depth"] = o.planes[..., 3].astype(np.float64)   # after K11 the fourth component is the depth
        rec["depth"] = o.planes[..., 3].astype(np.float64)
        prior = common.postprocess(o.planes.copy(), o.weak_info.copy(), o.selected_views.copy(), np.float32(p["depth_min"]), np.float32(p["depth_max"]))
        o.close()
    _RECORDS[case.name] = rec
    return rec


def project(case, depth, src):
    """Every reference pixel at its depth into view `src` with the cameras the oracle got (binary32 values, float64 algebra):
    (X, Y, z) maps; X and Y are x / z and y / z whatever the sign of z, as the reference's centre test sees them."""
    views = cc.scene_views(case)
    (Kr, Rr, cr), (Ks, Rs, cs) = views[0], views[src]
    ys, xs = np.mgrid[0:case.H, 0:case.W].astype(np.float64)
    cam = np.stack([(xs - Kr[2]) / Kr[0], (ys - Kr[5]) / Kr[4], np.ones_like(xs)], -1) * depth[..., None]
    world = cam @ Rr + cr
    q = (world - cs) @ Rs.T
    with np.errstate(divide="ignore", invalid="ignore"):
        return Ks[0] * q[..., 0] / q[..., 2] + Ks[2], Ks[4] * q[..., 1] / q[..., 2] + Ks[5], q[..., 2]


def footprints(case, depth, fw, fh, rows):
    """Per (footprint, source) with every centre in front of the source: does the box of projected centres plus MARGIN on each side
    fit 64 columns / `rows` rows?  Returns (pairs, misfits by columns, misfits by rows)."""
    n = by_cols = by_rows = 0
    for src in range(1, case.N + 1):
        X, Y, z = project(case, depth, src)
        for y0 in range(0, case.H, fh):
            for x0 in range(0, case.W, fw):
                sl = (slice(y0, y0 + fh), slice(x0, x0 + fw))
                if not (z[sl] > 0).all():
                    continue
                n += 1
                by_cols += (X[sl].max() - X[sl].min()) + 2 * MARGIN > 64
                by_rows += (Y[sl].max() - Y[sl].min()) + 2 * MARGIN > rows
    return n, int(by_cols), int(by_rows)


def _populations(ob, synth, case):
    d = record(ob, synth, case)["first_depth"]
    wave, block = footprints(case, d, 32, 4, 20), footprints(case, d, 8, 8, 32)
    print("CAMERA_SPACE %s: 32x4 footprints x sources %d, misfit by columns %d, by rows %d; 8x8 footprints x sources %d, misfit by columns %d, by rows %d"
          % ((case,) + wave + block))
    return wave, block


def test_on_the_ring_every_footprint_fits(ob, synth):
    """The control: with synth's ring at this size no wave's footprint misses its window for a reason of geometry."""
    wave, block = _populations(ob, synth, cc.RING)
    assert wave[0] > 0 and wave[1:] == (0, 0) and block[0] > 0 and block[1:] == (0, 0)


def test_footprint_populations(ob, synth):
    wave, _ = _populations(ob, synth, cc.BY_NAME["roll90"])
    assert 2 * wave[2] >= wave[0] > 0                       # a 32 x 4 footprint is about 4 x 32 in a rolled source: 20 rows cannot hold it
    wave, _ = _populations(ob, synth, cc.BY_NAME["zoom_in2"])
    assert 2 * wave[1] >= wave[0] > 0                       # ... and about 64 x 8 at twice the focal length
    for name in ("zoom_out_half", "roll180"):
        wave, block = _populations(ob, synth, cc.BY_NAME[name])
        assert wave[0] > 0 and wave[1:] == (0, 0) and block[1:] == (0, 0), name
    wave, _ = _populations(ob, synth, cc.BY_NAME["mixed"])
    d = record(ob, synth, cc.BY_NAME["mixed"])["first_depth"]
    # both populations: (footprint, view) pairs that fit and pairs that do not, each at least a tenth
    n, fit = 0, 0
    for src in range(1, cc.BY_NAME["mixed"].N + 1):
        one = _single_source(cc.BY_NAME["mixed"], d, src)
        n += one[0]
        fit += one[0] - one[1]
    print("CAMERA_SPACE mixed: %d of %d (32x4 footprint, source) pairs fit" % (fit, n))
    assert 10 * fit >= n and 10 * (n - fit) >= n


def _single_source(case, depth, src):
    """(pairs, pairs that fit neither by columns or by rows) of the 32 x 4 footprints in one source."""
    X, Y, z = project(case, depth, src)
    n = bad = 0
    for y0 in range(0, case.H, 4):
        for x0 in range(0, case.W, 32):
            sl = (slice(y0, y0 + 4), slice(x0, x0 + 32))
            if not (z[sl] > 0).all():
                continue
            n += 1
            bad += bool((X[sl].max() - X[sl].min()) + 2 * MARGIN > 64 or (Y[sl].max() - Y[sl].min()) + 2 * MARGIN > 20)
    return n, bad


def test_partial_sources_lose_the_reference_on_their_side(ob, synth):
    case = cc.BY_NAME["partial"]
    d = record(ob, synth, case)["depth"]
    for src, side in enumerate(cc.PARTIAL_SIDES, 1):
        X, Y, z = project(case, d, src)
        assert (z > 0).all()
        out = {"left": X < 0, "right": X >= case.W, "above": Y < 0, "below": Y >= case.H}[side]
        inside = (X >= 0) & (X < case.W) & (Y >= 0) & (Y < case.H)
        print("CAMERA_SPACE partial: source %d, %.1f %% of the reference pixels project %s it, %.1f %% inside" % (src, 100 * out.mean(), side, 100 * inside.mean()))
        assert out.mean() >= 0.05 and inside.mean() >= 0.25, (src, side)


def test_behind_sources_have_the_surface_behind_them(ob, synth):
    case = cc.BY_NAME["behind"]
    rec = record(ob, synth, case)
    _, _, z_near = project(case, rec["depth"], cc.BEHIND_NEAR)
    _, _, z_away = project(case, rec["depth"], cc.BEHIND_AWAY)
    print("CAMERA_SPACE behind: %.1f %% of the reference pixels have z <= 0 in the near source, %.1f %% z > 0; z < 0 in the source facing away: %s"
          % (100 * (z_near <= 0).mean(), 100 * (z_near > 0).mean(), bool((z_away < 0).all())))
    assert (z_near <= 0).mean() >= 0.05 and (z_near > 0).mean() >= 0.05
    assert (z_away < 0).all()
    # APD.cu:546-548: the centre of every hypothesis projects outside a source the whole scene is behind, its cost is 2.0 and K5
    # counts only costs below 2.0 as valid -- in every pass
    bit = np.uint32(1 << (cc.BEHIND_AWAY - 1))
    assert len(rec["after_k5"]) == 3 and not any((s & bit).any() for s in rec["after_k5"])


@pytest.mark.parametrize("case", cc.CASES, ids=repr)
def test_weak_pixels_nan_flag_and_convergence(ob, synth, case):
    rec = record(ob, synth, case)
    sc = cc.scene(synth, case)[0]
    gt = sc.gt_depth.numpy().astype(np.float64)
    m = 6
    err = np.abs(rec["depth"] - gt)[m:-m, m:-m] / gt[m:-m, m:-m]
    share = float((err < 0.01).mean())
    used = [int(((rec["selected"] >> v) & 1).sum()) for v in range(case.N)]
    print("CAMERA_SPACE %s: WEAK pixels entering the APD pass %d, the geometric pass %d; NaN words %s; %.1f %% of the interior within 1 %% of the "
          "rendered depth (table: %.1f); pixels that selected source 1..%d in some kernel: %s"
          % (case, rec["weak"][1], rec["weak"][2], rec["nans"], 100 * share, 100 * case.converged, case.N, used))
    assert rec["weak"][1] > 50 and rec["weak"][2] > 50          # the passes go through K3, K4, K9 and K10
    assert rec["nans"] == case.nans, "tests/test_gpu_camera_space.py compares NaN words as one pattern exactly where the oracle leaves some"
    assert share >= case.converged - 0.02
    assert case.converged > 0.0, "write the measured share into the case table"
    if case.name.startswith("mixed"):
        assert all(used), used     # one pixel's view loop crosses every kind of source only if every source is in use
