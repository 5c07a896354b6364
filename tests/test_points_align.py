"""The alignment of one cloud to another and the move of a cloud by a transform (arithmetic contract C18, DESIGN.md;
csrc/apd_align_math.h), without a device: the sequential checker (tests/helpers/points_align_ref.cpp) in its brute-force and grid
modes against each other, against a binary64 numpy SVD (Kabsch / Umeyama) on planted pairs and against hand-made cases of every
way the iteration ends; the move against numpy; what the C ABI refuses and answers without a device; and the resources of the
three kernels of csrc/apd_points_align.hip as the compiler reports them.  The clouds made here are those of the device tests
(test_gpu_points_align.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from common import kernel_resources
import points_align_checker as PA
from test_points_nearest import bits32, pair_cases
from test_points_radius import BAD as BAD_RADIUS, dressed
from test_points_voxel import cloud, from_cloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("apd_points_align", "apd_points_transformed")
PLANTED_RADIUS = 0.75
SETTINGS = [(1, False), (1, True), (5, False), (5, True)]     # (iterations, with_scale) of every bitwise comparison
IDENTITY = (1.0, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return PA.build(tmp_path_factory.mktemp("points_align_checker"))


# --------------------------------------------------------------------------------------------------------------------
# the clouds
# --------------------------------------------------------------------------------------------------------------------

def rotation(degrees, axis=(1.0, 2.0, 3.0)):
    """Rodrigues' formula in binary64."""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(degrees)
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def moved_back(x, scale, R, t):
    """The float32 positions that scale * R x' + t takes to x: R^T (x - t) / scale in binary64."""
    return (((np.asarray(x, np.float64) - t) @ R) / scale).astype(np.float32)


def planted_case(scale=1.0, degrees=2.0, shift=0.2, n_p=600, side=9):
    """Q: a lattice of side^3 points of spacing 1 around the origin, each moved by at most 0.1 per axis; P: n_p of them moved by the
    inverse of x' = scale * R x + t, R `degrees` about (1, 2, 3) / sqrt(14) and t = `shift` per axis.  (P, Q, the indices P was made
    from, scale, R, t)."""
    rng = np.random.default_rng(1)
    g = np.arange(side) - (side - 1) / 2
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    q = (np.stack([x, y, z], axis=-1).reshape(-1, 3) + rng.uniform(-0.1, 0.1, (side ** 3, 3))).astype(np.float32)
    chosen = np.sort(rng.choice(len(q), n_p, replace=False))
    R, t = rotation(degrees), np.full(3, shift)
    return moved_back(q[chosen], scale, R, t), q, chosen, scale, R, t


def far_start_case():
    """A start several steps away: Q 800 points scattered in a cube of side 8, P 600 of them with a Gaussian of 0.02 per axis on
    them -- so that the rms distance ends at a level that the binary32 positions do not disturb -- moved by the inverse of 8 degrees
    and 0.6 per axis; the radius 1.5.  (P, Q, radius, R, t)."""
    rng = np.random.default_rng(2)
    q = rng.uniform(-4, 4, (800, 3)).astype(np.float32)
    chosen = np.sort(rng.choice(len(q), 600, replace=False))
    R, t = rotation(8.0), np.full(3, 0.6)
    return moved_back(q[chosen].astype(np.float64) + rng.normal(size=(600, 3)) * 0.02, 1.0, R, t), q, 1.5, R, t


FEW_TARGETS = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5]])


def few_matched_case(matched):
    """Four points of which `matched` stand 0.1 per axis from a target and the others far from any; radius 0.75."""
    return np.concatenate([FEW_TARGETS[:matched] + np.float32(0.1), np.full((4 - matched, 3), 50, np.float32)]), FEW_TARGETS


def last_chunk_case():
    """257 points of which only the last, alone in the second chunk of 256, has a target within the radius -- and a second P whose
    last three have."""
    q = planted_case()[1]
    far = np.full((257, 3), 40, np.float32) + np.arange(257, dtype=np.float32)[:, None]
    one, three = far.copy(), far.copy()
    one[256] = q[5] + np.float32(0.05)
    three[254:] = q[[5, 100, 333]] + np.float32([0.05, -0.05, 0.1])
    return one, three, q


def align_cases(pkg):
    """name -> (P, Q, radius, origin): the pairs of test_points_nearest.py and the ones made here."""
    out = dict(pair_cases(pkg))
    for name, scale in (("planted rigid", 1.0), ("planted scaled", 1.03)):
        p, q = planted_case(scale)[:2]
        out[name] = (p, q, PLANTED_RADIUS, None)
    p, q, radius = far_start_case()[:3]
    out["far start"] = (p, q, radius, None)
    for matched in range(4):
        out["%d matched" % matched] = few_matched_case(matched) + (PLANTED_RADIUS, None)
    one, three, q = last_chunk_case()
    out["one match in the last chunk"] = (one, q, PLANTED_RADIUS, None)
    out["three matches at the end"] = (three, q, PLANTED_RADIUS, None)
    out["coincident"] = (np.full((10, 3), 0.1, np.float32), FEW_TARGETS, PLANTED_RADIUS, None)
    return out


def as_matrix(a):
    return np.asarray(a.rotation, np.float64).reshape(3, 3)


# --------------------------------------------------------------------------------------------------------------------
# the checker: its two modes, numpy, and how the iteration ends
# --------------------------------------------------------------------------------------------------------------------

def test_brute_force_and_grid_agree_on_every_device_case(pkg, checker):
    """The double loop over all pairs and the 27 lookups under every step's search: the same bits in every field, at 1 and 5
    iterations, rigid and with scale."""
    stops = set()
    for name, (p, q, radius, origin) in align_cases(pkg).items():
        assert len(p) * len(q) <= 4e8, name
        for iterations, with_scale in SETTINGS:
            grid = PA.align(checker, p, q, radius, origin, iterations, 1e-6, with_scale)
            brute = PA.align(checker, p, q, radius, origin, iterations, 1e-6, with_scale, mode=PA.BRUTE)
            assert PA.bits(grid) == PA.bits(brute), (name, iterations, with_scale, grid, brute)
            assert 0 <= grid.steps <= iterations and 0 <= grid.matched_after <= len(p) and grid.scale > 0.0, (name, grid)
            assert np.isfinite(grid.rotation).all() and np.isfinite(grid.translation).all() and np.isfinite([grid.rms_before, grid.rms_after]).all()
            assert with_scale or grid.scale == 1.0, name
            if grid.steps == 0:
                assert (grid.scale, grid.rotation, grid.translation) == IDENTITY and grid.stopped == PA.TOO_FEW, (name, grid)
            stops.add(grid.stopped)
    assert stops == {PA.ITERATIONS, PA.CONVERGED, PA.TOO_FEW}


def umeyama(p, q, with_scale):
    """The least-squares rigid or similarity transform of the pairs (p_i, q_i) by a binary64 SVD."""
    p, q = p.astype(np.float64), q.astype(np.float64)
    pm, qm = p.mean(axis=0), q.mean(axis=0)
    u, w = p - pm, q - qm
    U, S, Vt = np.linalg.svd(w.T @ u)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    scale = float((S * np.diag(D)).sum() / (u * u).sum()) if with_scale else 1.0
    return scale, R, qm - scale * (R @ pm)


MEASURED = 7.771561172376096e-16      # see test_planted_transform_matches_numpy_after_one_step


@pytest.mark.parametrize("scale", [1.0, 1.03])
def test_planted_transform_matches_numpy_after_one_step(checker, scale):
    """Every first match is the point P was made from, so one step solves the true pairs: the checker's (scale, R, t) against
    numpy's SVD on them.  Measured here: the largest entry-wise difference is 4.7e-16 (R), 1.1e-16 (t), 0 (scale) in the rigid case
    and 7.8e-16 (R), 1.7e-16 (t), 0 (scale) in the scaled one -- MEASURED is the largest of them -- and four times that is
    allowed, for Jacobi against LAPACK in the order of their roundings.  The planted transform itself is met to what binary32
    positions allow."""
    p, q, chosen, scale, R, t = planted_case(scale)
    near = np.linalg.norm(p[:, None, :].astype(np.float64) - q[None].astype(np.float64), axis=2)
    assert np.array_equal(near.argmin(axis=1), chosen) and near.min(axis=1).max() < PLANTED_RADIUS
    with_scale = scale != 1.0
    a = PA.align(checker, p, q, PLANTED_RADIUS, iterations=1, with_scale=with_scale)
    assert (a.steps, a.stopped, a.matched_before, a.matched_after) == (1, PA.ITERATIONS, len(p), len(p))
    assert a.rms_after < 1e-6 < 0.3 < a.rms_before
    s, Rc, tc, quaternion, sweeps = PA.solve_pairs(checker, p, q[chosen], with_scale)
    assert (a.scale, a.rotation, a.translation) == (s, tuple(Rc.reshape(9)), tuple(tc))     # the search found exactly these pairs
    want = umeyama(p, q[chosen], with_scale)
    differences = (abs(s - want[0]), float(np.abs(Rc - want[1]).max()), float(np.abs(tc - want[2]).max()))
    print("scale", scale, "differences from numpy (scale, R, t)", differences, "sweeps", sweeps)
    assert max(differences) <= 4.0 * MEASURED, differences
    assert abs(s - scale) < 1e-8 and np.abs(Rc - R).max() < 1e-8 and np.abs(tc - t).max() < 1e-7
    assert 0 < sweeps < 16 and quaternion[0] >= 0.0 and abs(np.linalg.det(Rc) - 1.0) < 1e-14


def test_the_quaternion_has_w_not_below_zero_and_the_rotation_is_proper(checker):
    """Pairs under rotations of up to 180 degrees about random axes, noisy ones, and mirrored ones -- for which the best proper
    rotation is what comes out, never a reflection."""
    rng = np.random.default_rng(3)
    for trial in range(60):
        x = rng.normal(size=(40, 3))
        R = rotation([180.0, 179.999, 90.0, rng.uniform(0, 180)][trial % 4], rng.normal(size=3))
        y = x @ R.T + rng.normal(size=(40, 3)) * (0.05 if trial % 3 == 0 else 0.0)
        if trial % 5 == 0:
            y[:, 0] = -y[:, 0]
        s, Rc, tc, quaternion, sweeps = PA.solve_pairs(checker, x.astype(np.float32), y.astype(np.float32), trial % 2 == 1)
        assert quaternion[0] >= 0.0 and abs(np.linalg.norm(quaternion) - 1.0) < 1e-15, (trial, quaternion)
        assert abs(np.linalg.det(Rc) - 1.0) < 1e-14 and np.abs(Rc.T @ Rc - np.eye(3)).max() < 1e-14 and sweeps < 16, (trial, Rc, sweeps)
        assert s > 0.0
        if trial % 3 and trial % 5:
            assert np.abs(Rc - R).max() < 1e-6, trial


def test_a_far_start_converges_over_several_steps(checker):
    """iterations = 1, 2, 3, ..: the call with k iterations ends where the one with k + 1 stands after k steps, the rms distance
    never rises, and the call that is allowed enough steps ends CONVERGED at the planted transform."""
    p, q, radius, R, t = far_start_case()
    full, trace = PA.align(checker, p, q, radius, iterations=64, trace=True)
    assert full.stopped == PA.CONVERGED and 5 < full.steps < 20 and len(trace) == full.steps + 1
    assert all(b <= a for a, b in zip(trace, trace[1:])), trace
    assert full.rms_before == trace[0] and full.rms_after == trace[-1] and full.rms_after < 0.1 * full.rms_before
    assert np.abs(as_matrix(full) - R).max() < 1e-3 and np.abs(np.asarray(full.translation) - t).max() < 1e-2
    for iterations in range(1, full.steps + 3):
        a = PA.align(checker, p, q, radius, iterations=iterations)
        steps = min(iterations, full.steps)
        assert a.steps == steps and a.rms_after == trace[steps] and a.rms_before == trace[0], (iterations, a)
        assert a.stopped == (PA.ITERATIONS if iterations <= full.steps else PA.CONVERGED), (iterations, a)
    assert PA.bits(PA.align(checker, p, q, radius, iterations=full.steps + 1)) == PA.bits(full)


def test_tolerance_zero_ends_at_the_iteration_cap(checker):
    p, q, radius, _, _ = far_start_case()
    a, trace = PA.align(checker, p, q, radius, iterations=64, tolerance=0.0, trace=True)
    assert len(trace) == 65 or a.stopped == PA.CONVERGED        # an rms that repeats exactly is convergence at tolerance 0 too
    assert a.steps == len(trace) - 1 and a.stopped in (PA.ITERATIONS, PA.CONVERGED) and a.rms_after == trace[-1]


def test_too_few_matches_and_coincident_points(checker):
    for matched in range(3):
        p, q = few_matched_case(matched)
        a = PA.align(checker, p, q, PLANTED_RADIUS, iterations=5)
        assert (a.scale, a.rotation, a.translation) == IDENTITY and (a.steps, a.stopped) == (0, PA.TOO_FEW), a
        assert a.matched_before == a.matched_after == matched and a.rms_before == a.rms_after and (a.rms_before > 0.17) == (matched > 0)
    p, q = few_matched_case(3)
    a = PA.align(checker, p, q, PLANTED_RADIUS, iterations=5)
    assert a.steps > 0 and a.stopped != PA.TOO_FEW and a.matched_after == 3 and a.rms_after < 1e-6       # three are enough
    assert np.abs(np.asarray(a.translation) + 0.1).max() < 1e-6
    a = PA.align(checker, np.full((10, 3), 0.1, np.float32), FEW_TARGETS, PLANTED_RADIUS)
    assert (a.scale, a.rotation, a.translation) == IDENTITY and (a.steps, a.stopped, a.matched_before) == (0, PA.TOO_FEW, 10), a
    one, three, q = last_chunk_case()
    a = PA.align(checker, one, q, PLANTED_RADIUS)
    assert (a.steps, a.stopped, a.matched_before) == (0, PA.TOO_FEW, 1) and abs(a.rms_before - 0.05 * 3 ** 0.5) < 1e-6
    a = PA.align(checker, three, q, PLANTED_RADIUS)
    assert a.steps > 0 and a.matched_before == a.matched_after == 3 and a.rms_after < a.rms_before
    for n_p, n_q in ((0, 5), (5, 0), (0, 0)):
        a = PA.align(checker, np.ones((n_p, 3), np.float32), np.ones((n_q, 3), np.float32), 1.0)
        assert a == PA.Alignment(*IDENTITY, 0, 0, 0.0, 0.0, 0, PA.TOO_FEW)


def test_a_cloud_aligned_to_itself_is_the_identity(checker):
    """Every point finds itself at distance 0: one step that is exactly the identity, then an rms that repeats."""
    q = planted_case()[1]
    a = PA.align(checker, q, q, PLANTED_RADIUS)
    assert a == PA.Alignment(*IDENTITY, len(q), len(q), 0.0, 0.0, 1, PA.CONVERGED)


def test_transformed_is_numpy_in_binary64_rounded_once(checker):
    """scale * R x + t and R n in binary64, rounded to binary32: the checker's expression rounds the three products and the three
    sums one by one where numpy may order or fuse them otherwise, so a result may differ by the double rounding of a value that
    lies next to the middle between two binary32 numbers: at most 1 unit in the last place, and most are equal."""
    rng = np.random.default_rng(4)
    xyz = (rng.normal(size=(5000, 3)) * 3).astype(np.float32)
    normal = rng.normal(size=(5000, 3)).astype(np.float32)
    scale, R, t = 1.03, rotation(37.0, (3, -1, 2)), np.float64([0.5, -2.0, 11.0])
    got_xyz, got_normal = PA.transformed(checker, xyz, normal, scale, R, t)
    want_xyz = (scale * (xyz.astype(np.float64) @ R.T) + t).astype(np.float32)
    want_normal = (normal.astype(np.float64) @ R.T).astype(np.float32)
    for got, want in ((got_xyz, want_xyz), (got_normal, want_normal)):
        ulps = np.abs(bits32(got).astype(np.int64) - bits32(want).astype(np.int64))
        print("equal", float((ulps == 0).mean()), "largest difference in ulps", int(ulps.max()))
        assert ulps.max() <= 1 and (ulps == 0).mean() > 0.99
    same_xyz, same_normal = PA.transformed(checker, xyz, normal, 1.0, np.eye(3), np.zeros(3))
    assert np.array_equal(bits32(same_xyz), bits32(xyz)) and np.array_equal(same_normal, normal)


# --------------------------------------------------------------------------------------------------------------------
# the C ABI without a device
# --------------------------------------------------------------------------------------------------------------------

def test_header_declares_the_entry_points_as_ctypes_calls_them(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "apd_mi355x.h")).read(), flags=re.S)
    assert re.search(r"int\s+apd_points_align\s*\(\s*apd_points_t\s+\w+\s*,\s*apd_points_t\s+\w+\s*,\s*float\s+\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,"
                     r"\s*const\s+apd_points_align_options\s*\*\s*\w+\s*,\s*apd_points_alignment_t\s*\*\s*\w+\s*\)", text)
    assert re.search(r"int\s+apd_points_transformed\s*\(\s*apd_points_t\s+\w+\s*,\s*double\s+\w+\s*,\s*const\s+double\s*\*\s*\w+\s*,"
                     r"\s*const\s+double\s*\*\s*\w+\s*,\s*apd_points_t\s*\*\s*\w+\s*\)", text)
    assert re.search(r"typedef\s+struct\s*\{\s*unsigned\s+iterations\s*;\s*double\s+tolerance\s*;\s*int\s+with_scale\s*;\s*\}\s*apd_points_align_options\s*;",
                     text)
    assert re.search(r"typedef\s+struct\s*\{\s*double\s+scale\s*,\s*rotation\[9\]\s*,\s*translation\[3\]\s*;\s*long\s+long\s+matched_before\s*,"
                     r"\s*matched_after\s*;\s*double\s+rms_before\s*,\s*rms_after\s*;\s*int\s+steps\s*,\s*stopped\s*;\s*\}\s*apd_points_alignment_t\s*;", text)
    assert re.search(r"APD_ALIGN_ITERATIONS\s*=\s*0\s*,\s*APD_ALIGN_CONVERGED\s*=\s*1\s*,\s*APD_ALIGN_TOO_FEW\s*=\s*2", text)
    L = pkg.lib()
    assert L.apd_points_align.argtypes == [C.c_void_p, C.c_void_p, C.c_float, C.POINTER(C.c_float), C.POINTER(pkg.PointsAlignOptions),
                                           C.POINTER(pkg.PointsAlignment)]
    assert L.apd_points_transformed.argtypes == [C.c_void_p, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_void_p)]
    assert [n for n, _ in pkg.PointsAlignment._fields_] == list(PA.FIELDS) == list(pkg.Alignment._fields)
    assert C.sizeof(pkg.PointsAlignment) == 144 and C.sizeof(pkg.PointsAlignOptions) == 24
    assert (pkg.ALIGN_ITERATIONS, pkg.ALIGN_CONVERGED, pkg.ALIGN_TOO_FEW) == (PA.ITERATIONS, PA.CONVERGED, PA.TOO_FEW)


def test_library_exports_the_entry_points(pkg):
    for name in NEW_SYMBOLS:
        assert hasattr(pkg.lib(), name), name


def test_align_refusals_that_need_no_device(pkg):
    L = pkg.lib()
    pts = from_cloud(pkg, cloud([[0.5, 0, 0], [0.6, 0, 0]]), [4], [5], [[]])
    other = from_cloud(pkg, cloud([[0.5, 0, 0], [0.6, 0, 0], [0.7, 0, 0]]), [4], [5], [[]])
    out = pkg.PointsAlignment()
    out.scale, out.steps = -7.0, -7

    def refused(p, q, radius, origin, options, null_output, message, code=-1):
        org = None if origin is None else (C.c_float * 3)(*origin)
        opt = None if options is None else C.byref(pkg.PointsAlignOptions(*options))
        assert L.apd_points_align(p, q, radius, org, opt, None if null_output else C.byref(out)) == code
        assert L.apd_fusion_last_error().decode() == "apd_points_align: " + message
        assert out.scale == -7.0 and out.steps == -7

    refused(None, other._p, 1.0, None, None, False, "null argument")
    refused(pts._p, None, 1.0, None, None, False, "null argument")
    refused(pts._p, other._p, 1.0, None, None, True, "null argument")
    for (radius, origin), message in BAD_RADIUS:
        refused(pts._p, other._p, radius, origin, None, False, message)
    refused(pts._p, other._p, 1.0, None, (0, 1e-6, 0), False, "iterations = 0, not in 1 .. 64")
    refused(pts._p, other._p, 1.0, None, (65, 1e-6, 0), False, "iterations = 65, not in 1 .. 64")
    refused(pts._p, other._p, 1.0, None, (16, float("nan"), 0), False, "a tolerance of nan, not a finite number >= 0")
    refused(pts._p, other._p, 1.0, None, (16, float("inf"), 1), False, "a tolerance of inf, not a finite number >= 0")
    refused(pts._p, other._p, 1.0, None, (16, -1e-9, 0), False, "a tolerance of -1e-09, not a finite number >= 0")
    with pytest.raises(pkg.ApdError, match="apd_points_align: iterations = 0"):
        pts.align(other, 1.0, iterations=0)
    with pytest.raises(pkg.ApdError, match="apd_points_align: iterations = 65"):
        pts.align(other, 1.0, iterations=65)
    with pytest.raises(pkg.ApdError, match="apd_points_align: a tolerance of nan"):
        pts.align(other, 1.0, tolerance=float("nan"))
    with pytest.raises(pkg.ApdError, match="apd_points_align: a radius of 0"):
        pts.align(other, 0.0)
    with pytest.raises(pkg.ApdError, match="Points.align: the other points are closed or not a Points"):
        pts.align(None, 1.0)


def test_transformed_refusals_that_need_no_device(pkg):
    L = pkg.lib()
    pts = from_cloud(pkg, cloud([[0.5, 0, 0], [0.6, 0, 0]]), [4], [5], [[]])
    eye, zero = np.eye(3).reshape(9), np.zeros(3)

    def refused(p, scale, R, t, null_output, message):
        out = C.c_void_p(77)
        dp = lambda a: None if a is None else np.ascontiguousarray(a, np.float64).ctypes.data_as(C.POINTER(C.c_double))
        assert L.apd_points_transformed(p, scale, dp(R), dp(t), None if null_output else C.byref(out)) == -1
        assert L.apd_fusion_last_error().decode() == "apd_points_transformed: " + message
        assert out.value == 77

    refused(None, 1.0, eye, zero, False, "null argument")
    refused(pts._p, 1.0, None, zero, False, "null argument")
    refused(pts._p, 1.0, eye, None, False, "null argument")
    refused(pts._p, 1.0, eye, zero, True, "null argument")
    for scale, text in ((0.0, "0"), (-1.0, "-1"), (float("nan"), "nan"), (float("inf"), "inf")):
        refused(pts._p, scale, eye, zero, False, "a scale of %s, not a positive finite number" % text)
    bad = eye.copy()
    bad[4] = float("nan")
    refused(pts._p, 1.0, bad, zero, False, "rotation component 4 is nan")
    refused(pts._p, 1.0, eye, [0.0, float("inf"), 0.0], False, "translation component 1 is inf")
    refused(pts._p, 1.0, 2.0 * eye, zero, False, "not a rotation: entry (0, 0) of R^T R is 4")
    shear = eye.copy()
    shear[1] = 1e-5
    refused(pts._p, 1.0, shear, zero, False, "not a rotation: entry (0, 1) of R^T R is %.17g" % 1e-5)
    nearly = rotation(30.0).reshape(9) * (1.0 + 4e-7)            # R^T R - I is 8e-7 on the diagonal: within 1e-6
    assert np.abs(nearly.reshape(3, 3).T @ nearly.reshape(3, 3) - np.eye(3)).max() < 1e-6
    out = C.c_void_p()
    empty = from_cloud(pkg, cloud(np.zeros((0, 3), np.float32)), [4], [5], [[]])
    assert L.apd_points_transformed(empty._p, 1.0, nearly.ctypes.data_as(C.POINTER(C.c_double)), zero.ctypes.data_as(C.POINTER(C.c_double)), C.byref(out)) == 0
    pkg.Points(out, 0).close()
    with pytest.raises(pkg.ApdError, match="apd_points_transformed: a scale of -2"):
        pts.transformed(-2.0, np.eye(3), zero)
    with pytest.raises(pkg.ApdError, match="apd_points_transformed: not a rotation"):
        pts.transformed(1.0, np.ones((3, 3)), zero)
    with pytest.raises(TypeError):
        pts.transformed(1.0)
    with pytest.raises(ValueError):
        pts.transformed(1.0, np.eye(2), zero)


def test_objects_without_points_give_their_answers_without_a_device(pkg):
    c, (rows, cols, pairs) = dressed(np.random.default_rng(5), np.zeros((0, 3), np.float32))
    empty = from_cloud(pkg, c, rows, cols, pairs)
    some = from_cloud(pkg, cloud([[0.5, 0, 0], [0.6, 0, 0]]), [4], [5], [[]])
    for p, q in ((empty, some), (some, empty), (empty, empty)):
        a = p.align(q, 1.0, with_scale=True)
        assert a._fields == PA.FIELDS and PA.bits(a) == PA.bits(PA.Alignment(*IDENTITY, 0, 0, 0.0, 0.0, 0, PA.TOO_FEW)), a
        assert a.rotation.shape == (3, 3) and a.translation.shape == (3,) and isinstance(a.steps, int) and isinstance(a.matched_before, int)
    moved = empty.transformed(2.0, rotation(10.0), [1, 2, 3])
    assert moved.count == 0 and moved.on_device == empty.on_device and moved.visibility()[0].tolist() == [0]
    moved = empty.transformed(empty.align(some, 1.0))
    assert moved.count == 0


def test_no_gpu_means_the_alignment_fails_loudly(pkg):
    """There is no host implementation: without a device non-empty host objects are refused with a message."""
    if pkg.device_count() > 0:
        pytest.skip("a GPU is visible")
    pts = from_cloud(pkg, cloud([[0.5, 0, 0], [0.6, 0, 0]]), [4], [5], [[]])
    with pytest.raises(pkg.ApdError, match=r"apd_points_align: hipSetDevice\("):
        pts.align(pts, 1.0)
    with pytest.raises(pkg.ApdError, match=r"apd_points_transformed: hipSetDevice\("):
        pts.transformed(1.0, np.eye(3), np.zeros(3))


# --------------------------------------------------------------------------------------------------------------------
# the kernels' resources
# --------------------------------------------------------------------------------------------------------------------

def test_the_three_kernels_use_no_scratch_memory_and_spill_nothing(tmp_path):
    """k_align_sums1, k_align_sums2 and k_align_move keep their terms in registers: 0 bytes of scratch per lane and no spilled
    register; the two reductions hold 4 x 8 and 4 x 10 doubles of LDS, the move none.  The search compiled into the file
    (k_nearest_in and the sorts' helpers) uses no scratch either.  Registers, LDS and occupancy are printed."""
    found = kernel_resources("apd_points_align.hip", tmp_path)
    for kernel, lds in (("k_align_sums1", "256"), ("k_align_sums2", "320"), ("k_align_move", "0")):
        mine = [v for k, v in found.items() if kernel in k]
        assert len(mine) == 1, (kernel, sorted(found))
        print(kernel, "VGPRs", mine[0]["VGPRs"], "SGPRs", mine[0]["TotalSGPRs"], "LDS", mine[0]["LDS Size [bytes/block]"], "occupancy",
              mine[0]["Occupancy [waves/SIMD]"])
        assert mine[0]["ScratchSize [bytes/lane]"] == "0" and mine[0]["VGPRs Spill"] == "0" and mine[0]["SGPRs Spill"] == "0", (kernel, mine[0])
        assert mine[0]["LDS Size [bytes/block]"] == lds, (kernel, mine[0])
    for name, v in found.items():
        assert v["ScratchSize [bytes/lane]"] == "0", name
