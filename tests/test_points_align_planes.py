"""The alignment of one cloud to another cloud's tangent planes (arithmetic contract C20, DESIGN.md;
csrc/apd_align_plane_math.h), without a device: the sequential checker (tests/helpers/points_align_planes_ref.cpp) in its
brute-force and grid modes against each other, its 6 x 6 solve against numpy's least squares on the same rows, a planted
transform on a resampled surface against the point-to-point alignment of contract C18, the shapes that do not constrain a
motion, every way the iteration ends; what the C ABI refuses and answers without a device; the values of --ply-align-planes;
and the resources of the kernel as the compiler reports them.  The clouds are those of the device tests
(points_align_planes_cases.py)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from common import kernel_resources
import points_align_checker as PA
import points_align_planes_checker as PP
import points_align_planes_cases as K
from test_points_radius import BAD as BAD_RADIUS, dressed
from test_points_voxel import cloud, from_cloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "apd-mvs_amd", "_build", "libapd_host.so")
IDENTITY = (1.0, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0))
NOTHING = PP.PlaneAlignment(*IDENTITY, 0, 0, 0.0, 0.0, 0, PP.TOO_FEW, 0, 0, 0.0, 0.0)
SETTINGS = (1, 5)     # the iterations of every bitwise comparison
KAPPA = 2.0 ** -20


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return PP.build(tmp_path_factory.mktemp("points_align_planes_checker"))


@pytest.fixture(scope="module")
def point_checker(tmp_path_factory):
    return PA.build(tmp_path_factory.mktemp("points_align_checker"))


def errors(a, R, t):
    """(degrees between a's rotation and R, distance between a's translation and t)."""
    got = np.asarray(a.rotation, np.float64).reshape(3, 3)
    cosine = np.clip((np.trace(got @ R.T) - 1.0) / 2.0, -1.0, 1.0)
    return float(np.degrees(np.arccos(cosine))), float(np.linalg.norm(np.asarray(a.translation, np.float64) - t))


# --------------------------------------------------------------------------------------------------------------------
# the checker: its two modes, numpy, and how the iteration ends
# --------------------------------------------------------------------------------------------------------------------

def test_brute_force_and_grid_agree_on_every_device_case(pkg, checker):
    """The double loop over all pairs and the 27 lookups under every step's search: the same bits in every field, at 1 and 5
    iterations; and all four ways to end are among the cases."""
    stops = set()
    for name, (p, q, normal, radius, origin) in K.plane_cases(pkg).items():
        assert len(p) * len(q) <= 4e8, name
        for iterations in SETTINGS:
            grid = PP.align_planes(checker, p, q, normal, radius, origin, iterations)
            brute = PP.align_planes(checker, p, q, normal, radius, origin, iterations, mode=PP.BRUTE)
            assert PP.bits(grid) == PP.bits(brute), (name, iterations, grid, brute)
            assert 0 <= grid.steps <= iterations and 0 <= grid.planes_after <= grid.matched_after <= len(p) and grid.scale == 1.0, (name, grid)
            assert 0 <= grid.planes_before <= grid.matched_before, (name, grid)
            assert np.isfinite(grid.rotation).all() and np.isfinite(grid.translation).all(), (name, grid)
            assert np.isfinite([grid.rms_before, grid.rms_after, grid.plane_rms_before, grid.plane_rms_after]).all(), (name, grid)
            if grid.steps == 0:
                assert (grid.scale, grid.rotation, grid.translation) == IDENTITY and grid.stopped in (PP.TOO_FEW, PP.DEGENERATE), (name, grid)
                assert (grid.planes_before, grid.plane_rms_before) == (grid.planes_after, grid.plane_rms_after), (name, grid)
            stops.add(grid.stopped)
    assert stops == {PP.ITERATIONS, PP.CONVERGED, PP.TOO_FEW, PP.DEGENERATE}


def rows_of(p, q, normal, centre):
    """The rows g_i and the residuals r_i of contract C20 in binary64, as numpy words them."""
    n = normal.astype(np.float64)
    u = n / np.linalg.norm(n, axis=1, keepdims=True)
    x, y = p.astype(np.float64) - centre, q.astype(np.float64) - centre
    return np.concatenate([np.cross(x, u), u], axis=1), ((x - y) * u).sum(axis=1)


MEASURED = 7.632783294297951e-17      # see test_the_solve_matches_numpy_least_squares


def test_the_solve_matches_numpy_least_squares(checker):
    """One step's z = (omega, tau) from the thirty sums by LDL^T without pivoting against numpy.linalg.lstsq on the rows (g_i, -r_i)
    in binary64, the pairs those of the ellipsoid case as its first search matches them (found here by numpy).  Measured here: the
    largest difference of a component is 7.6e-17 -- MEASURED -- at |z| = 0.091 and a condition number of the rows of 4.2, which
    the normal equations square; four times the recorded value is allowed, for LDL^T against LAPACK in the order of their
    roundings.  The pivots are positive, each above kappa times its bound and at most the bound, and the sums are numpy's."""
    p, q, normal, radius = K.ellipsoid_case()[:4]
    near = np.linalg.norm(p[:, None, :].astype(np.float64) - q[None].astype(np.float64), axis=2)
    match = near.argmin(axis=1)
    assert near.min(axis=1).max() < radius
    centre, sums = PP.sums_of_pairs(checker, p, q[match], normal[match])
    assert np.abs(centre - q[match].astype(np.float64).mean(axis=0)).max() < 1e-14
    G, r = rows_of(p, q[match], normal[match], centre)
    A = G.T @ G
    assert np.allclose([sums[i * 6 - i * (i - 1) // 2 + j - i] for i in range(6) for j in range(i, 6)], A[np.triu_indices(6)], rtol=1e-12, atol=1e-12)
    assert np.allclose(sums[21:27], G.T @ r, rtol=1e-10, atol=1e-12) and np.isclose(sums[27], r @ r) and sums[28] == len(p)
    solved = PP.solve(checker, centre, sums)
    want = np.linalg.lstsq(G, -r, rcond=None)[0]
    difference = float(np.abs(solved.z - want).max())
    print("largest |z - lstsq|", difference, "|z|", float(np.linalg.norm(want)), "condition", float(np.linalg.cond(G)), "pivots", solved.d)
    assert not solved.degenerate and difference <= 4.0 * MEASURED, (solved, want)
    bound = np.r_[[sums[29]] * 3, [sums[28]] * 3]
    assert (solved.d > KAPPA * bound).all() and (solved.d <= bound).all()
    # the rotation is that of the quaternion (1, omega / 2) normalised: angle 2 atan(|omega| / 2) about omega, about the centre
    omega, tau = solved.z[:3], solved.z[3:]
    angle = 2.0 * np.arctan(np.linalg.norm(omega) / 2.0)
    assert np.abs(solved.rotation - K.rotation(np.degrees(angle), omega)).max() < 1e-15
    assert abs(np.linalg.det(solved.rotation) - 1.0) < 1e-14 and np.abs(solved.rotation.T @ solved.rotation - np.eye(3)).max() < 1e-14
    assert np.abs(solved.translation - (centre + tau - solved.rotation @ centre)).max() < 1e-15


def test_a_planted_transform_on_a_resampled_surface_beats_point_to_point(checker, point_checker):
    """Q and P are different samples of one curved, well-constrained surface, P moved by 2 degrees and 0.05 per axis.  From the same
    start and with the same cap the plane variant ends nearer to the planted transform than the point-to-point one, in rotation and
    in translation, at every cap tried; the plane rms falls.  Measured here (rotation error in degrees, translation error):
      cap  1: planes 0.250, 0.00144   points 1.850, 0.0539
      cap  5: planes 0.120, 0.00049   points 1.070, 0.0130
      cap 16: planes 0.120, 0.00049 (CONVERGED after 5 steps)   points 0.834, 0.0055
      cap 64: planes as at 16   points 0.840, 0.0055 (CONVERGED after 18 steps)
    The plane rms goes from 0.0522 to 0.0064; the point rms stays at 0.107, the sampling offset, under either."""
    p, q, normal, radius, R, t = K.ellipsoid_case()
    assert 600 <= len(q) <= 1000 and len(p) != len(q)
    for cap in (1, 5, 16, 64):
        planes = PP.align_planes(checker, p, q, normal, radius, iterations=cap)
        points = PA.align(point_checker, p, q, radius, iterations=cap)
        e_planes, e_points = errors(planes, R, t), errors(points, R, t)
        print("cap", cap, "planes", e_planes, planes.steps, planes.stopped, "points", e_points, points.steps, points.stopped,
              "plane rms", planes.plane_rms_before, planes.plane_rms_after, "point rms", planes.rms_after, points.rms_after)
        assert e_planes[0] < e_points[0] and e_planes[1] < e_points[1], (cap, e_planes, e_points)
        assert planes.plane_rms_after < planes.plane_rms_before and planes.stopped in (PP.ITERATIONS, PP.CONVERGED), (cap, planes)
        assert planes.matched_before == planes.planes_before == len(p) and planes.steps == min(cap, 5)
    assert planes.stopped == PP.CONVERGED and planes.steps < points.steps


def test_degenerate_geometry_is_refused(checker):
    """A sampled plane (three columns exactly zero), a sphere about its centre (the three rotations), a cylinder along its axis
    (the translation along it and, with every point on its match's normal, the spin about it): no step is invented -- the
    identity, DEGENERATE, 0 steps -- and the pivot that fails, the first dependent column in the order of elimination, is a
    rounding error's share of its bound, while the smallest pivot of the ellipsoid is above a hundredth of it."""
    for name, make in K.DEGENERATE_CASES.items():
        p, q, normal, radius = make()
        for iterations in SETTINGS:
            a = PP.align_planes(checker, p, q, normal, radius, iterations=iterations)
            assert (a.scale, a.rotation, a.translation) == IDENTITY and (a.steps, a.stopped) == (0, PP.DEGENERATE), (name, a)
            assert a.matched_before == a.planes_before == len(p) and a.plane_rms_before == a.plane_rms_after > 0.01, (name, a)
        centre, sums = PP.sums_of_pairs(checker, q, q, normal)
        solved = PP.solve(checker, centre, sums)
        share = solved.d / np.r_[[sums[29]] * 3, [sums[28]] * 3]
        failed = int(np.argmax(~(share > KAPPA)))
        print(name, "pivots over their bounds", share, "fails at column", failed)
        assert solved.degenerate and not solved.z.any() and share[failed] < 1e-12 and (share[:failed] > 1e-4).all(), (name, share)
        assert failed == {"plane": 2, "sphere": 0, "cylinder": 4}[name]
    p, q, normal, radius = K.ellipsoid_case()[:4]
    centre, sums = PP.sums_of_pairs(checker, q, q, normal)
    solved = PP.solve(checker, centre, sums)
    share = solved.d / np.r_[[sums[29]] * 3, [sums[28]] * 3]
    print("ellipsoid: pivots over their bounds", share)
    assert not solved.degenerate and share.min() > 0.01
    assert PP.align_planes(checker, p, q, normal, radius).stopped == PP.CONVERGED


def test_the_solve_refuses_an_emptied_column_and_sums_that_are_not_finite(checker):
    """The sums of the ellipsoid solve; the same sums with the column of the third translation emptied do not, and the pivots up
    to it are reported; a sum that overflowed makes z not finite, which is refused the same way."""
    p, q, normal = K.ellipsoid_case()[:3]
    centre, sums = PP.sums_of_pairs(checker, q, q, normal)
    emptied = sums.copy()
    for i in range(6):
        emptied[i * 6 - i * (i - 1) // 2 + 5 - i] = 0.0
    emptied[26] = 0.0
    assert not PP.solve(checker, centre, sums).degenerate
    solved = PP.solve(checker, centre, emptied)
    assert solved.degenerate and solved.d[5] == 0.0 and (solved.d[:5] > 0.0).all() and np.array_equal(solved.rotation, np.eye(3))
    bad = sums.copy()
    bad[21] = np.inf                                    # a sum that overflowed: z is not finite
    assert PP.solve(checker, centre, bad).degenerate


def test_few_usable_matches_on_either_side_of_six(checker):
    for count in range(9):
        p, q, normal, radius = K.few_usable_case(count)
        a = PP.align_planes(checker, p, q, normal, radius, iterations=5)
        assert (a.matched_before, a.planes_before) == (8, count), (count, a)
        assert abs(a.rms_before - 0.05) < 1e-6 and (count == 0 or abs(a.plane_rms_before - 0.05) < 1e-6), (count, a)
        if count < 6:
            assert a == PP.PlaneAlignment(*IDENTITY, 8, 8, a.rms_before, a.rms_before, 0, PP.TOO_FEW, count, count, a.plane_rms_before, a.plane_rms_before)
        else:
            assert a.steps >= 1 or a.stopped == PP.DEGENERATE, (count, a)       # six are enough to try
    for n_p, n_q in ((0, 5), (5, 0), (0, 0)):
        a = PP.align_planes(checker, np.ones((n_p, 3), np.float32), np.ones((n_q, 3), np.float32), np.ones((n_q, 3), np.float32), 1.0)
        assert a == NOTHING
    one, eight, q, normal = K.last_chunk_case()
    a = PP.align_planes(checker, one, q, normal, K.SURFACE_RADIUS)
    assert (a.steps, a.stopped, a.matched_before, a.planes_before) == (0, PP.TOO_FEW, 1, 1) and 0.0 < a.plane_rms_before <= a.rms_before
    a = PP.align_planes(checker, eight, q, normal, K.SURFACE_RADIUS, iterations=5)
    assert a.steps == 5 and a.matched_after == a.planes_after == 8 and a.plane_rms_after < 1e-6 < a.plane_rms_before
    # nothing matched: the plane figures are 0 and 0.0
    a = PP.align_planes(checker, one[:200], q, normal, K.SURFACE_RADIUS)
    assert a == NOTHING


def test_bad_normals_are_unusable_and_the_sign_plays_no_part(checker):
    p, q, normal, radius = K.bad_normals_case()
    good = K.usable(normal)
    assert 100 < (~good).sum() < 120 and good[4 * 5] and good[5 * 5]        # the tiny and the huge normal are usable
    a = PP.align_planes(checker, p, q, normal, radius, iterations=5)
    near = np.linalg.norm(p[:, None, :].astype(np.float64) - q[None].astype(np.float64), axis=2).argmin(axis=1)
    assert a.matched_before == len(p) and a.planes_before == int(good[near].sum()) < len(p) and a.steps == 5, a
    # zeroing the unusable ones changes nothing, and neither does negating any normal
    zeroed = normal.copy()
    zeroed[~good] = 0.0
    assert PP.bits(PP.align_planes(checker, p, q, zeroed, radius, iterations=5)) == PP.bits(a)
    flipped = normal.copy()
    flipped[::2] = -flipped[::2]
    assert PP.bits(PP.align_planes(checker, p, q, flipped, radius, iterations=5)) == PP.bits(a)
    assert PP.bits(PP.align_planes(checker, p, q, -normal, radius, iterations=5)) == PP.bits(a)
    # and their length plays none beyond rounding: the planted transform comes back as with the unit normals
    R, t = K.ellipsoid_case()[4:]
    assert errors(a, R, t)[0] < 0.2 and errors(a, R, t)[1] < 0.002


def test_a_cloud_aligned_to_itself_is_the_identity(checker):
    """Every point finds itself at distance 0: one step that is exactly the identity, then a point rms that repeats."""
    q, normal = K.surface_sample(800, 11)
    a = PP.align_planes(checker, q, q, normal, K.SURFACE_RADIUS)
    assert a == PP.PlaneAlignment(*IDENTITY, len(q), len(q), 0.0, 0.0, 1, PP.CONVERGED, len(q), len(q), 0.0, 0.0)


def test_tolerance_zero_ends_at_the_iteration_cap(checker):
    p, q, normal, radius = K.ellipsoid_case()[:4]
    a = PP.align_planes(checker, p, q, normal, radius, iterations=64, tolerance=0.0)
    assert a.stopped == PP.ITERATIONS and a.steps == 64 or a.stopped == PP.CONVERGED      # an rms that repeats exactly is convergence too
    assert a.steps > PP.align_planes(checker, p, q, normal, radius, iterations=64).steps
    for cap in (1, 2, 3):       # the call with k iterations ends where the one with more stands after k steps
        a = PP.align_planes(checker, p, q, normal, radius, iterations=cap, tolerance=0.0)
        assert (a.steps, a.stopped) == (cap, PP.ITERATIONS) and a.planes_after == len(p) and a.plane_rms_after < a.plane_rms_before


# --------------------------------------------------------------------------------------------------------------------
# the C ABI without a device
# --------------------------------------------------------------------------------------------------------------------

def test_header_declares_the_entry_point_as_ctypes_calls_it(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "apd_mi355x.h")).read(), flags=re.S)
    assert re.search(r"int\s+apd_points_align_planes\s*\(\s*apd_points_t\s+\w+\s*,\s*apd_points_t\s+\w+\s*,\s*float\s+\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,"
                     r"\s*const\s+apd_points_align_planes_options\s*\*\s*\w+\s*,\s*apd_points_plane_alignment_t\s*\*\s*\w+\s*\)", text)
    assert re.search(r"typedef\s+struct\s*\{\s*unsigned\s+iterations\s*;\s*double\s+tolerance\s*;\s*\}\s*apd_points_align_planes_options\s*;", text)
    assert re.search(r"typedef\s+struct\s*\{\s*double\s+scale\s*,\s*rotation\[9\]\s*,\s*translation\[3\]\s*;\s*long\s+long\s+matched_before\s*,"
                     r"\s*matched_after\s*;\s*double\s+rms_before\s*,\s*rms_after\s*;\s*int\s+steps\s*,\s*stopped\s*;\s*long\s+long\s+planes_before\s*,"
                     r"\s*planes_after\s*;\s*double\s+plane_rms_before\s*,\s*plane_rms_after\s*;\s*\}\s*apd_points_plane_alignment_t\s*;", text)
    assert re.search(r"enum\s*\{\s*APD_ALIGN_DEGENERATE\s*=\s*3\s*\}", text)
    L = pkg.lib()
    assert hasattr(L, "apd_points_align_planes")
    assert L.apd_points_align_planes.argtypes == [C.c_void_p, C.c_void_p, C.c_float, C.POINTER(C.c_float), C.POINTER(pkg.PointsAlignPlanesOptions),
                                                  C.POINTER(pkg.PointsPlaneAlignment)]
    assert [n for n, _ in pkg.PointsPlaneAlignment._fields_] == list(PP.FIELDS) == list(pkg.PlaneAlignment._fields)
    assert (pkg.ALIGN_ITERATIONS, pkg.ALIGN_CONVERGED, pkg.ALIGN_TOO_FEW, pkg.ALIGN_DEGENERATE) == (PP.ITERATIONS, PP.CONVERGED, PP.TOO_FEW, PP.DEGENERATE)
    assert C.sizeof(pkg.PointsAlignPlanesOptions) == 16


def test_the_struct_begins_as_the_alignment_struct(pkg):
    """Every field of apd_points_alignment_t at its offset and size, then the four new ones: code that reads an alignment reads
    this one."""
    old, new = pkg.PointsAlignment, pkg.PointsPlaneAlignment
    assert pkg.PlaneAlignment._fields[:len(pkg.Alignment._fields)] == pkg.Alignment._fields
    for name, _ in old._fields_:
        assert (getattr(new, name).offset, getattr(new, name).size) == (getattr(old, name).offset, getattr(old, name).size), name
    assert C.sizeof(old) == 144 and new.planes_before.offset == 144 and C.sizeof(new) == 176
    assert [getattr(new, n).offset for n in ("planes_before", "planes_after", "plane_rms_before", "plane_rms_after")] == [144, 152, 160, 168]


def test_refusals_that_need_no_device(pkg):
    L = pkg.lib()
    pts = from_cloud(pkg, cloud([[0.5, 0, 0], [0.6, 0, 0]]), [4], [5], [[]])
    other = from_cloud(pkg, cloud([[0.5, 0, 0], [0.6, 0, 0], [0.7, 0, 0]]), [4], [5], [[]])
    out = pkg.PointsPlaneAlignment()
    out.scale, out.steps, out.planes_after = -7.0, -7, -7

    def refused(p, q, radius, origin, options, null_output, message, code=-1):
        org = None if origin is None else (C.c_float * 3)(*origin)
        opt = None if options is None else C.byref(pkg.PointsAlignPlanesOptions(*options))
        assert L.apd_points_align_planes(p, q, radius, org, opt, None if null_output else C.byref(out)) == code
        assert L.apd_fusion_last_error().decode() == "apd_points_align_planes: " + message
        assert out.scale == -7.0 and out.steps == -7 and out.planes_after == -7

    refused(None, other._p, 1.0, None, None, False, "null argument")
    refused(pts._p, None, 1.0, None, None, False, "null argument")
    refused(pts._p, other._p, 1.0, None, None, True, "null argument")
    for (radius, origin), message in BAD_RADIUS:
        refused(pts._p, other._p, radius, origin, None, False, message)
    refused(pts._p, other._p, 1.0, None, (0, 1e-6), False, "iterations = 0, not in 1 .. 64")
    refused(pts._p, other._p, 1.0, None, (65, 1e-6), False, "iterations = 65, not in 1 .. 64")
    refused(pts._p, other._p, 1.0, None, (16, float("nan")), False, "a tolerance of nan, not a finite number >= 0")
    refused(pts._p, other._p, 1.0, None, (16, float("inf")), False, "a tolerance of inf, not a finite number >= 0")
    refused(pts._p, other._p, 1.0, None, (16, -1e-9), False, "a tolerance of -1e-09, not a finite number >= 0")
    with pytest.raises(pkg.ApdError, match="apd_points_align_planes: iterations = 0"):
        pts.align_planes(other, 1.0, iterations=0)
    with pytest.raises(pkg.ApdError, match="apd_points_align_planes: iterations = 65"):
        pts.align_planes(other, 1.0, iterations=65)
    with pytest.raises(pkg.ApdError, match="apd_points_align_planes: a tolerance of nan"):
        pts.align_planes(other, 1.0, tolerance=float("nan"))
    with pytest.raises(pkg.ApdError, match="apd_points_align_planes: a radius of 0"):
        pts.align_planes(other, 0.0)
    with pytest.raises(pkg.ApdError, match="Points.align_planes: the other points are closed or not a Points"):
        pts.align_planes(None, 1.0)
    with pytest.raises(ValueError, match="Points.align_planes: -1 iterations"):
        pts.align_planes(other, 1.0, iterations=-1)


def test_objects_without_points_give_their_answers_without_a_device(pkg):
    c, (rows, cols, pairs) = dressed(np.random.default_rng(5), np.zeros((0, 3), np.float32))
    empty = from_cloud(pkg, c, rows, cols, pairs)
    some = from_cloud(pkg, cloud([[0.5, 0, 0], [0.6, 0, 0]]), [4], [5], [[]])
    for p, q in ((empty, some), (some, empty), (empty, empty)):
        a = p.align_planes(q, 1.0)
        assert a._fields == PP.FIELDS and PP.bits(a) == PP.bits(NOTHING), a
        assert a.rotation.shape == (3, 3) and a.translation.shape == (3,) and isinstance(a.steps, int) and isinstance(a.planes_before, int)
    moved = empty.transformed(empty.align_planes(some, 1.0))        # transformed() takes a PlaneAlignment as it takes an Alignment
    assert moved.count == 0
    with pytest.raises(TypeError):
        empty.transformed(empty.align_planes(some, 1.0), np.eye(3))


def test_no_gpu_means_the_alignment_fails_loudly(pkg):
    """There is no host implementation: without a device non-empty host objects are refused with a message."""
    if pkg.device_count() > 0:
        pytest.skip("a GPU is visible")
    pts = from_cloud(pkg, cloud([[0.5, 0, 0], [0.6, 0, 0]]), [4], [5], [[]])
    with pytest.raises(pkg.ApdError, match=r"apd_points_align_planes: hipSetDevice\("):
        pts.align_planes(pts, 1.0)


# --------------------------------------------------------------------------------------------------------------------
# the values of --ply-align-planes
# --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def parse(pkg):
    assert os.path.exists(HOST_LIB), "run __graft_entry__.build() first"
    pkg.lib()  # libapd_host.so depends on libapd_mi355x.so
    L = C.CDLL(HOST_LIB)
    L.apdhost_parse_ply_option.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]

    def call(flag, value):
        fields, message = C.create_string_buffer(4096), C.create_string_buffer(1024)
        rc = L.apdhost_parse_ply_option(flag.encode(), value.encode(), fields, len(fields), message, len(message))
        return rc, dict(line.split(" ", 1) for line in fields.value.decode().splitlines()), message.value.decode()
    return call


BAD_VALUES = ("", "truth.ply", "truth.ply,", ",1", "truth.ply,0", "truth.ply,-1", "truth.ply,nan", "truth.ply,inf", "truth.ply,1e30", "truth.ply,1e-30",
              "truth.ply,1x", "truth.ply,1,0", "truth.ply,1,2,", "truth.ply,0.5,scale", "truth.ply,0.5,8,scale", "scale", ",8")
GOOD_VALUES = {"truth.ply,1": ("truth.ply", "1", "16"), "a,b.ply,0.5": ("a,b.ply", "0.5", "16"), "truth.ply,0.5,8": ("truth.ply", "0.5", "8"),
               "truth.ply,0.5,64": ("truth.ply", "0.5", "64"), "truth.ply,0.5,1": ("truth.ply", "0.5", "1"),
               "truth.ply,0.5,65": ("truth.ply,0.5", "65", "16"),      # no count: it reads as the radius, and the file's name grows
               "a,b,c.ply,0.25,7": ("a,b,c.ply", "0.25", "7"), "truth.ply,0.5,007": ("truth.ply", "0.5", "7"), "truth.ply,2,1.5": ("truth.ply,2", "1.5", "16"),
               ",0.5,8": (",0.5", "8", "16")}       # a file's name is not empty, so the first comma belongs to it
EXPECTS = "TRUTH.ply,RADIUS[,ITERATIONS], a file with nx ny nz, a positive number and a count of 1 .. 64"


def test_values_of_the_flag(parse):
    table = json.load(open(os.path.join(ROOT, "tests", "golden", "ply_option_values.json")))
    defaults = {**table["defaults"], "planes_radius": "0", "planes_iterations": "16", "planes_truth": ""}
    for bad in BAD_VALUES:
        rc, fields, message = parse("--ply-align-planes", bad)
        assert (rc, message) == (1, "bad value '%s' of --ply-align-planes: %s" % (bad, EXPECTS)) and fields == defaults, (bad, rc, message, fields)
    for good, (truth, radius, iterations) in GOOD_VALUES.items():
        rc, fields, message = parse("--ply-align-planes", good)
        assert (rc, message) == (0, "") and fields == {**defaults, "planes_truth": truth, "planes_radius": radius, "planes_iterations": iterations}, (good, fields)


def test_the_dump_of_every_other_flag_is_as_it_was(parse):
    """The new fields are reported for the new flag alone: every flag of the committed table answers with exactly its fields."""
    table = json.load(open(os.path.join(ROOT, "tests", "golden", "ply_option_values.json")))
    flags = sorted({r["flag"] for r in table["rows"]})
    assert len(flags) == 10 and "--ply-align-planes" not in flags
    for row in table["rows"]:
        if row["good"]:
            rc, fields, _ = parse(row["flag"], row["value"])
            assert rc == 0 and list(fields) == list(table["defaults"]) and fields == {**table["defaults"], **row["fields"]}, row
    for flag in flags:
        assert list(parse(flag, "no such value,,")[1]) == list(table["defaults"]), flag
    assert list(parse("--ply-align-planes", "t.ply,1")[1]) == list(table["defaults"]) + ["planes_radius", "planes_iterations", "planes_truth"]


# --------------------------------------------------------------------------------------------------------------------
# the kernel's resources
# --------------------------------------------------------------------------------------------------------------------

def test_the_kernel_uses_no_scratch_memory_and_spills_nothing(tmp_path):
    """k_align_plane_sums keeps its thirty terms in registers: 0 bytes of scratch per lane and no spilled register; the reduction
    holds 4 x 30 doubles of LDS.  Pass 1 and the move, compiled into the file too, are as in apd_points_align.hip, and nothing in
    the file uses scratch.  Registers, LDS and occupancy are printed."""
    found = kernel_resources("apd_points_align_planes.hip", tmp_path)
    for kernel, lds in (("k_align_plane_sums", "960"), ("k_align_sums1", "256"), ("k_align_move", "0")):
        mine = [v for k, v in found.items() if kernel in k]
        assert len(mine) == 1, (kernel, sorted(found))
        print(kernel, "VGPRs", mine[0]["VGPRs"], "SGPRs", mine[0]["TotalSGPRs"], "LDS", mine[0]["LDS Size [bytes/block]"], "occupancy",
              mine[0]["Occupancy [waves/SIMD]"])
        assert mine[0]["ScratchSize [bytes/lane]"] == "0" and mine[0]["VGPRs Spill"] == "0" and mine[0]["SGPRs Spill"] == "0", (kernel, mine[0])
        assert mine[0]["LDS Size [bytes/block]"] == lds, (kernel, mine[0])
    for name, v in found.items():
        assert v["ScratchSize [bytes/lane]"] == "0", name
