"""Normals and surface variation from each point's neighbourhood without a device: the two modes of the sequential checker
(tests/helpers/points_normals_ref.cpp) against each other on every cloud the device tests run; the cap on Jacobi sweeps, which
none of them reaches; numpy.linalg.eigh as an independent yardstick; planted truth (a plane, a sphere, a cube); the sign rule;
degenerate clouds; the order of the binary64 sums; the kernel's scratch size; the refusals of apd_points_estimate_normals and
apd_points_with_estimated_normals, which need no device; objects without points; the loud failure without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fusion_cases
from common import walk_kernel_resources
import points_normals_checker as PN
import points_radius_checker as PR
import points_voxel_checker as PV
import vis_checker as VC
from test_points_radius import (DENSE_ORIGIN, DENSE_RADIUS, MERGED_RADIUS, BAD as BAD_RADIUS, border_case, dense_case, determinism_case, dressed, grid_edge_case,
                                merged_many_views_case, outside_case, real_cloud_radius, size_case, size_list)
from test_points_voxel import REAL_CLOUDS, cloud, from_cloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("apd_points_estimate_normals", "apd_points_with_estimated_normals")
SIZE_MINS = (2, 7)
REAL_MIN = 5          # min_neighbours on the real clouds: at three times the median spacing some points have it and some do not
REAL_CLOUD = REAL_CLOUDS[1]
INF = float("inf")
f32 = np.float32


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return PN.build(tmp_path_factory.mktemp("points_normals_checker"))


@pytest.fixture(scope="module")
def radius_checker(tmp_path_factory):
    return PR.build(tmp_path_factory.mktemp("points_radius_checker"))


@pytest.fixture(scope="module")
def voxel_checker(tmp_path_factory):
    return PV.build(tmp_path_factory.mktemp("points_voxel_checker"))


@pytest.fixture(scope="module")
def vis(tmp_path_factory):
    return VC.build(tmp_path_factory.mktemp("vis_checker"))


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# --------------------------------------------------------------------------------------------------------------------
# the clouds of the device tests (test_gpu_points_normals.py) that test_points_radius.py does not make; radius 1, origin 0
# --------------------------------------------------------------------------------------------------------------------

PLANE_NORMAL = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
SPHERE_RADIUS = 20.0     # cells
CUBE_SIDE = 8.0


def with_normals(xyz, normal):
    return cloud(np.asarray(xyz, np.float32), normal=np.ascontiguousarray(normal, np.float32))


def plane_case(rng, side=12.0, per_area=12):
    """A tilted plane through the origin, side x side cells of it at about 12 points per unit of area -- a cell the plane cuts holds
    about that many -- with binary32 coordinates; every stored normal is the true normal with a random sign.  (cloud, signs)."""
    n = int(side * side * per_area)
    e1 = np.cross(PLANE_NORMAL, [0.0, 0.0, 1.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(PLANE_NORMAL, e1)
    uv = (rng.random((n, 2)) - 0.5) * side
    xyz = uv[:, :1] * e1 + uv[:, 1:] * e2
    signs = rng.integers(0, 2, n) * 2.0 - 1.0
    return with_normals(xyz, signs[:, None] * PLANE_NORMAL), signs


def sphere_case(rng, n=20000):
    """n points on a sphere of radius 20 cells around (0.3, 0.2, 0.1), about four per unit of area; the stored normals point outwards."""
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    return with_normals(d * SPHERE_RADIUS + [0.3, 0.2, 0.1], d)


def cube_case(rng, per_area=12):
    """The six faces of the cube [0, 8]^3 at about 12 points per unit of area, the face coordinate exact; the stored normals point
    outwards.  (cloud, the distance of every point to the nearest edge of the cube)."""
    per_face = int(CUBE_SIDE * CUBE_SIDE * per_area)
    xyz, normal = [], []
    for axis in range(3):
        for side in (0.0, CUBE_SIDE):
            p = rng.random((per_face, 3)) * CUBE_SIDE
            p[:, axis] = side
            nrm = np.zeros((per_face, 3))
            nrm[:, axis] = 1.0 if side else -1.0
            xyz.append(p)
            normal.append(nrm)
    xyz = np.concatenate(xyz).astype(np.float32)
    to_face = np.sort(np.minimum(xyz, CUBE_SIDE - xyz), axis=1)   # [:, 0] is 0: the point's own face; [:, 1]: the nearest edge
    return with_normals(xyz, np.concatenate(normal)), to_face[:, 1].astype(np.float64)


def lattice_plane(stored):
    """The 9 x 9 points at multiples of 1/4 in the plane z = 1/2: every term has d_z = 0 exactly, so the third row and column of the
    covariance are exact zeros, no rotation touches them and the estimate is (0, 0, +-1) exactly."""
    g = np.arange(9) * 0.25
    xyz = np.stack(np.meshgrid(g, g, [0.5], indexing="ij"), axis=-1).reshape(-1, 3)
    return with_normals(xyz, np.tile(np.asarray(stored, np.float64), (len(xyz), 1)))


def sign_cases(rng):
    """name -> cloud: the plane, and one point far from it, with zero stored normals and with NaN components; the lattice with an
    orthogonal stored normal."""
    plane, _ = plane_case(rng, side=6.0)
    xyz = np.concatenate([plane.xyz, [[100.5, 100.5, 100.5]]])        # and a point without neighbours
    nan = np.tile(np.float32([np.nan, 1.0, 0.0]), (len(xyz), 1))
    nan[::3] = [0.0, np.nan, np.nan]
    return {"zero": with_normals(xyz, np.zeros((len(xyz), 3))), "nan": with_normals(xyz, nan),
            "orthogonal": lattice_plane([1.0, 2.0, 0.0])}


def degenerate_cases():
    """name -> cloud: seven coincident points; forty points on a line."""
    t = np.arange(40)[:, None] * 0.03
    return {"coincident": with_normals(np.tile([0.5, 0.25, 0.75], (7, 1)), np.tile([0.0, 0.0, 1.0], (7, 1))),
            "collinear": with_normals(0.1 + t * [0.3, 0.5, 0.2], np.tile([0.0, 0.0, 1.0], (40, 1)))}


ORDER_LINE = np.array([0.3, 0.5, 0.2]) / np.linalg.norm([0.3, 0.5, 0.2])


def order_cases(rng, n=150):
    """The same n points of one cell in three input orders -- as made, reversed, shuffled: the cell's points are summed in input
    order, so the three clouds give every point the same terms in three orders.  The points stand on a line, up to the rounding
    of their binary32 coordinates: the two smallest eigenvalues are of the size of the rounding of the binary64 sums, so that
    the order of the sums decides bits that survive the conversion to binary32 (on a cloud with three distinct eigenvalues it
    moves the binary64 results by parts in 10^16 and the binary32 results almost never).  [(cloud, the position of made point j)]."""
    xyz = (0.05 + rng.random((n, 1)) * 0.9 * ORDER_LINE).astype(np.float32)
    normal = np.tile([0.0, 0.0, 1.0], (n, 1))
    out = []
    for order in (np.arange(n), np.arange(n)[::-1], rng.permutation(n)):
        out.append((with_normals(xyz[order], normal), np.argsort(order)))
    return out


def small_cases(pkg, voxel_checker):
    """name -> (cloud, radius, origin, the min_neighbours values) of every synthetic device case with at most 20 001 points."""
    out = {}
    for n in size_list(pkg):
        out["n=%d" % n] = (size_case(pkg, n)[0], 1.0, None, SIZE_MINS)
    out["borders"] = (dressed(np.random.default_rng(1), border_case()[0])[0], 1.0, None, (2,))
    out["grid edges"] = (dressed(np.random.default_rng(2), grid_edge_case()[0])[0], 1.0, None, (2,))
    out["outside"] = (dressed(np.random.default_rng(3), outside_case(np.random.default_rng(4))[0])[0], 1.0, None, (2, 3))
    out["dense"] = (dressed(np.random.default_rng(7), dense_case(np.random.default_rng(8)))[0], DENSE_RADIUS, DENSE_ORIGIN, (2,))
    out["merged"] = (merged_many_views_case(voxel_checker)[2], MERGED_RADIUS, None, (3,))
    out["determinism"] = (determinism_case()[0], 1.0, [0.25, -0.5, 0.125], (4,))
    out["plane"] = (plane_case(np.random.default_rng(31))[0], 1.0, None, (5,))
    out["sphere"] = (sphere_case(np.random.default_rng(32)), 1.0, None, (5,))
    out["cube"] = (cube_case(np.random.default_rng(33))[0], 1.0, None, (5,))
    for name, c in sign_cases(np.random.default_rng(34)).items():
        out["sign " + name] = (c, 1.0, None, (3,))
    for name, c in degenerate_cases().items():
        out[name] = (c, 1.0, None, (2,))
    for j, (c, _) in enumerate(order_cases(np.random.default_rng(35))):
        out["order %d" % j] = (c, 1.0, None, (2,))
    return out


PLANTED = ("plane", "sphere", "cube")


@pytest.fixture(scope="module")
def results(pkg, checker, voxel_checker):
    """name -> (cloud, radius, origin, {min_neighbours: the checker's grid-mode result}) of small_cases, computed once."""
    return {name: (c, radius, origin, {k: PN.run(checker, c, radius, k, origin) for k in mins})
            for name, (c, radius, origin, mins) in small_cases(pkg, voxel_checker).items()}


def same(a, b):
    return (np.array_equal(bits32(a.normal), bits32(b.normal)) and np.array_equal(bits32(a.variation), bits32(b.variation)) and
            np.array_equal(a.sweeps, b.sweeps) and np.array_equal(a.estimated, b.estimated) and a.count == b.count)


# --------------------------------------------------------------------------------------------------------------------
# the checker: its two modes, the cap
# --------------------------------------------------------------------------------------------------------------------

def test_brute_force_and_grid_agree_on_every_small_device_case(checker, results):
    """The double loop over all pairs with a sort of each point's terms and the 27 lookups in key order: the same bits of every
    normal and variation, the same sweeps."""
    for name, (c, radius, origin, by_min) in results.items():
        assert c.count <= 20001, name
        for k, grid in by_min.items():
            assert same(PN.run(checker, c, radius, k, origin, PN.BRUTE), grid), (name, k)
            assert not np.isnan(grid.variation).any(), name
            assert not np.isnan(grid.normal[grid.estimated]).any(), name
            assert np.isinf(grid.variation[~grid.estimated]).all() and np.array_equal(bits32(grid.normal[~grid.estimated]), bits32(c.normal[~grid.estimated]))


def test_the_cap_on_sweeps_is_never_reached_and_is_the_largest_count_seen(pkg, checker, results):
    """kNormalSweepCap is the smallest cap that stops no point of any test cloud: no point is capped, and some point takes
    exactly that many sweeps.  The large cloud of the device tests is held to it too; the real cloud, which takes fewer, in
    test_real_cloud_choice_is_not_vacuous, and the clouds only a device makes in test_gpu_points_normals.py."""
    from test_points_radius import large_case
    most = 0
    large = dressed(np.random.default_rng(9), large_case(np.random.default_rng(10)))[0]
    for name, by_min in list((n, r[3]) for n, r in results.items()) + [("large", {4: PN.run(checker, large, 1.0, 4)})]:
        for k, res in by_min.items():
            assert not res.capped.any(), (name, k)
            most = max(most, int(res.sweeps.max()) if res.count else 0)
    print("largest sweep count", most, "cap", PN.sweep_cap(checker))
    assert most == PN.sweep_cap(checker)


# --------------------------------------------------------------------------------------------------------------------
# numpy.linalg.eigh as the yardstick
# --------------------------------------------------------------------------------------------------------------------

def numpy_neighbourhoods(c, radius, origin=None):
    """(i, j): every pair with j a neighbour of i by contract C11 or j == i, both inside the grid, restated with numpy's binary32
    operations: the cell of C10 per axis, adjacent cells, (dx * dx + dy * dy) + dz * dz <= radius * radius."""
    xyz = c.xyz
    org = np.zeros(3, f32) if origin is None else np.asarray(origin, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        cell = np.floor((xyz - org) / f32(radius))
    inside = (np.isfinite(cell) & (cell >= -2.0 ** 20) & (cell < 2.0 ** 20)).all(axis=1)
    index = np.flatnonzero(inside)
    x, cl, r2 = xyz[index], cell[index], f32(radius) * f32(radius)
    pi, pj = [], []
    for first in range(0, len(index), 256):
        a = slice(first, first + 256)
        d = x[a, None, :] - x[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        near = (np.abs(cl[a, None, :] - cl[None, :, :]) <= 1).all(axis=2) & (d2 <= r2)
        i, j = np.nonzero(near)
        pi.append(index[i + first])
        pj.append(index[j])
    return np.concatenate(pi), np.concatenate(pj)


def numpy_estimates(c, radius, min_neighbours, origin=None):
    """Per point: whether it has an estimate, the eigenvalues (ascending) and the eigenvector of the smallest, by numpy.linalg.eigh on
    the binary64 covariance numpy forms from the neighbour set: the mean and the mean outer product of the centred terms."""
    n = c.count
    i, j = numpy_neighbourhoods(c, radius, origin)
    count = np.bincount(i, minlength=n)
    d = c.xyz[j].astype(np.float64) - c.xyz[i].astype(np.float64)
    mean = np.stack([np.bincount(i, d[:, a], n) for a in range(3)], axis=1) / np.maximum(count, 1)[:, None]
    d -= mean[i]
    cov = np.zeros((n, 3, 3))
    for a in range(3):
        for b in range(a, 3):
            cov[:, a, b] = cov[:, b, a] = np.bincount(i, d[:, a] * d[:, b], n) / np.maximum(count, 1)
    values, vectors = np.linalg.eigh(cov)
    return count - 1 >= min_neighbours, values, vectors[:, :, 0]


def against_numpy(c, res, radius, min_neighbours, origin=None):
    """(the largest angle between the checker's and numpy's normals, mod sign, the largest difference of the variations, both over
    the points above the gap bound; the share of the points with an estimate that are under it)."""
    have, values, vectors = numpy_estimates(c, radius, min_neighbours, origin)
    assert np.array_equal(have, res.estimated)
    values, vectors, mine = np.maximum(values[have], 0.0), vectors[have], res.normal[have].astype(np.float64)
    total = values.sum(axis=1)
    gap = np.where(total > 0, (values[:, 1] - values[:, 0]) / np.where(values[:, 2] > 0, values[:, 2], 1.0), 0.0)
    clear = gap > GAP_BOUND
    angle = np.arctan2(np.linalg.norm(np.cross(mine, vectors), axis=1), np.abs((mine * vectors).sum(axis=1)))
    variation = np.where(total > 0, values[:, 0] / np.where(total > 0, total, 1.0), 0.0)
    differ = np.abs(variation - res.variation[have].astype(np.float64))
    if not clear.any():
        return 0.0, 0.0, 1.0
    return float(angle[clear].max()), float(differ[clear].max()), 1.0 - float(clear.mean())


# Measured here, on the CPU, with numpy's eigh (LAPACK) against the checker, over the planted clouds and the other clouds named in the
# test below: the largest angle over the points above the gap bound was 9.21e-7 rad (on "determinism"; 5.9e-8 on the planted
# clouds) and the largest difference of the variations 2.54e-8 (on "order 2"; 7.9e-9 on the planted clouds).  The variation's
# figure is the rounding of the result to binary32 (a value below 1/3 carries 1.5e-8).  The angle's is more than the 6e-8 a
# binary32 unit vector carries: the contract's terms are binary32 differences, numpy's are exact, and on a sparse cloud near the
# origin that relative 6e-8 of a term is divided by the gap.  The assertions allow four times the measured values, for other
# libm and BLAS builds.  Below a relative gap (l1 - l0) / l2 of GAP_BOUND the direction is not determined and is not compared.
GAP_BOUND = 1e-3
MEASURED_ANGLE, MEASURED_VARIATION = 9.21e-7, 2.54e-8


def test_numpy_eigh_agrees_on_the_normals_and_the_variation(results):
    worst_angle = worst_variation = 0.0
    for name in PLANTED + ("n=257", "determinism", "order 2", "merged", "sign zero", "collinear", "coincident"):
        c, radius, origin, by_min = results[name]
        for k, res in by_min.items():
            angle, differ, under = against_numpy(c, res, radius, k, origin)
            print("%-12s min %d: %6d estimated, angle %.3g rad, variation %.3g, under the gap bound %.4f" % (name, k, res.count, angle, differ, under))
            worst_angle, worst_variation = max(worst_angle, angle), max(worst_variation, differ)
            assert angle <= 4 * MEASURED_ANGLE and differ <= 4 * MEASURED_VARIATION, name
            if name in PLANTED:   # the condition that makes the comparison mean something
                assert res.count > 1000 and under <= 0.05, (name, under)
    print("largest angle %.3g rad, largest variation difference %.3g" % (worst_angle, worst_variation))


# --------------------------------------------------------------------------------------------------------------------
# planted truth
# --------------------------------------------------------------------------------------------------------------------

def angle_to(normals, truth):
    normals = normals.astype(np.float64)
    return np.arctan2(np.linalg.norm(np.cross(normals, truth), axis=1), (normals * truth).sum(axis=1))


# Measured on the plane of plane_case: the coordinates are binary32, so a point stands up to 2^-24 * 6 off the plane; the largest
# angle of an estimate to the true normal was 1.65e-7 rad and the largest variation 6.27e-14.  Four times that is allowed.
PLANE_ANGLE, PLANE_VARIATION = 1.65e-7, 6.27e-14


def test_planted_plane(results):
    c, _, _, by_min = results["plane"]
    _, signs = plane_case(np.random.default_rng(31))
    res = by_min[5]
    assert res.count > 0.95 * c.count
    e = res.estimated
    assert ((res.normal[e].astype(np.float64) * PLANE_NORMAL).sum(axis=1) * signs[e] > 0).all()      # the stored normal's sign
    angle = angle_to(res.normal[e], signs[e, None] * PLANE_NORMAL)
    print("plane: largest angle %.3g rad, largest variation %.3g" % (angle.max(), res.variation[e].max()))
    assert angle.max() <= 4 * PLANE_ANGLE
    assert res.variation[e].max() <= 4 * PLANE_VARIATION


def test_planted_sphere(results):
    """Radius 20 cells: the neighbourhood of radius 1 is a cap whose sagitta is 1/40, so the normals are the radial directions within
    a few degrees of sampling noise and the variation is small but not 0."""
    c, _, _, by_min = results["sphere"]
    res = by_min[5]
    e = res.estimated
    assert res.count > 0.9 * c.count
    angle = angle_to(res.normal[e], c.normal[e].astype(np.float64))
    print("sphere: median angle %.3g rad, largest %.3g, median variation %.3g" % (np.median(angle), angle.max(), np.median(res.variation[e])))
    assert np.median(angle) < 0.02 and angle.max() < 0.5       # outwards, like the stored normals
    assert 0 < np.median(res.variation[e]) < 1e-2


def test_planted_cube_orders_faces_below_edges(results):
    """A point further than a radius from every edge sees one face: its variation is that of a plane.  Within a radius of an edge
    the other face comes into the neighbourhood and the variation is larger: the ordering is asserted, not a value."""
    c, _, _, by_min = results["cube"]
    _, to_edge = cube_case(np.random.default_rng(33))
    res = by_min[5]
    e = res.estimated
    face, edge, close = e & (to_edge > 1.0), e & (to_edge < 1.0), e & (to_edge < 0.5)
    assert face.sum() > 1000 and close.sum() > 300
    print("cube: face max %.3g, edge median %.3g, close min %.3g" % (res.variation[face].max(), np.median(res.variation[edge]), res.variation[close].min()))
    assert res.variation[face].max() < np.median(res.variation[edge])
    assert res.variation[face].max() < res.variation[close].min()
    assert angle_to(res.normal[face], c.normal[face].astype(np.float64)).max() < 1e-6


# --------------------------------------------------------------------------------------------------------------------
# the sign rule, degenerate clouds, the order of the sums
# --------------------------------------------------------------------------------------------------------------------

def first_nonzero_is_positive(normals):
    first = np.where(normals[:, 0] != 0, normals[:, 0], np.where(normals[:, 1] != 0, normals[:, 1], normals[:, 2]))
    return first > 0


def test_sign_rule(checker, results):
    """A zero stored normal and one with NaN components give the estimate whose first non-zero component is positive; that is the
    negation of what the true normal as the stored one gives, whose first component is negative.  A stored normal exactly
    orthogonal to the estimate, likewise; a stored normal along it decides."""
    for name in ("sign zero", "sign nan"):
        plane, res = results[name][0], results[name][3][3]
        e = res.estimated
        assert e.sum() > 300 and not e[-1] and first_nonzero_is_positive(res.normal[e]).all(), name
        assert not np.isnan(res.normal[e]).any()
        towards = PN.run(checker, with_normals(plane.xyz, np.tile(-PLANE_NORMAL, (plane.count, 1))), 1.0, 3)
        assert (towards.normal[e][:, 0] < 0).all()
        assert np.array_equal(bits32(res.normal[e]), bits32(-towards.normal[e])) and np.array_equal(bits32(res.variation), bits32(towards.variation))
    nan = results["sign nan"][0]
    res = results["sign nan"][3][3]
    assert np.isnan(nan.normal[-1]).any() and np.array_equal(bits32(res.normal[~res.estimated]), bits32(nan.normal[~res.estimated]))   # NaN copied where there is no estimate
    res = results["sign orthogonal"][3][3]
    assert res.estimated.all() and (res.normal == [0, 0, 1]).all() and (res.variation == 0).all()     # dot = 0 exactly
    for stored, want in (([0, 0, -1], [0, 0, -1]), ([5, 5, 0.001], [0, 0, 1]), ([1, -1, -0.0], [0, 0, 1])):
        got = PN.run(checker, lattice_plane(stored), 1.0, 3)
        assert (got.normal == want).all(), stored


def test_degenerate_clouds(results):
    """Coincident points: the covariance is zero, no rotation happens, the three eigenvalues tie and the lowest column, (1, 0, 0),
    is the vector; the stored normal (0, 0, 1) is orthogonal to it and the first component is positive already; variation 0.
    Collinear points: two eigenvalues are 0 up to rounding; whatever the vector, it is finite, of unit length, orthogonal to
    the line and the same in both modes (held by the test of the modes)."""
    res = results["coincident"][3][2]
    assert res.estimated.all() and (res.normal == [1, 0, 0]).all() and (bits32(res.variation) == 0).all() and (res.sweeps == 0).all()
    res = results["collinear"][3][2]
    assert res.estimated.all() and np.isfinite(res.normal).all() and np.isfinite(res.variation).all()
    assert np.allclose(np.linalg.norm(res.normal.astype(np.float64), axis=1), 1.0, atol=1e-6)
    line = np.array([0.3, 0.5, 0.2]) / np.linalg.norm([0.3, 0.5, 0.2])
    assert np.abs(res.normal.astype(np.float64) @ line).max() < 1e-5
    assert (res.variation < 1e-10).all()


def test_summation_order_shows_in_the_results(results):
    """The same 150 points of one cell, on a line, in three input orders: every point has the same terms in three orders, the
    binary64 sums round differently, and where the two smallest eigenvalues are rounding themselves that shows: every result is a
    unit vector orthogonal to the line with a variation of next to nothing, in every order, and they are not the same bits
    in every order -- the order is part of the contract.  (That the brute-force mode follows the order too is held by the test
    of the modes, and that the device does by test_gpu_points_normals.py.)"""
    made = []
    for j, (c, where) in enumerate(order_cases(np.random.default_rng(35))):
        res = results["order %d" % j][3][2]
        assert res.estimated.all() and np.isfinite(res.normal).all()
        assert np.allclose(np.linalg.norm(res.normal.astype(np.float64), axis=1), 1.0, atol=1e-6)
        assert np.abs(res.normal.astype(np.float64) @ ORDER_LINE).max() < 1e-5 and (res.variation < 1e-10).all()
        made.append((res.normal[where], res.variation[where]))
    assert any(not np.array_equal(bits32(normal), bits32(made[0][0])) or not np.array_equal(bits32(variation), bits32(made[0][1]))
               for normal, variation in made[1:])


# --------------------------------------------------------------------------------------------------------------------
# the C ABI without a device
# --------------------------------------------------------------------------------------------------------------------

def test_header_declares_the_entry_points_as_ctypes_calls_them(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "apd_mi355x.h")).read(), flags=re.S)
    assert re.search(r"int\s+apd_points_estimate_normals\s*\(\s*apd_points_t\s+\w+\s*,\s*float\s+\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,"
                     r"\s*unsigned\s+\w+\s*,\s*float\s*\*\s*\w+\s*,\s*float\s*\*\s*\w+\s*\)", text)
    assert re.search(r"int\s+apd_points_with_estimated_normals\s*\(\s*apd_points_t\s+\w+\s*,\s*float\s+\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,"
                     r"\s*unsigned\s+\w+\s*,\s*apd_points_t\s*\*\s*\w+\s*,\s*long\s+long\s*\*\s*\w+\s*\)", text)
    L = pkg.lib()
    fp, vpp, llp = C.POINTER(C.c_float), C.POINTER(C.c_void_p), C.POINTER(C.c_longlong)
    assert L.apd_points_estimate_normals.argtypes == [C.c_void_p, C.c_float, fp, C.c_uint, C.c_void_p, C.c_void_p]
    assert L.apd_points_with_estimated_normals.argtypes == [C.c_void_p, C.c_float, fp, C.c_uint, vpp, llp]


def test_library_exports_the_entry_points(pkg):
    for name in NEW_SYMBOLS:
        assert hasattr(pkg.lib(), name), name


def test_refusals_that_need_no_device(pkg):
    """Every bad argument answers APD_ERR_INVALID with its message and leaves the outputs as they were: no device is touched,
    so this passes on a machine without one."""
    L = pkg.lib()
    pts = from_cloud(pkg, cloud([[0.5, 0, 0], [0.6, 0, 0]]), [4], [5], [[]])
    normal, variation = np.full(6, 77, np.float32), np.full(2, 77, np.float32)
    out, estimated = C.c_void_p(1234), C.c_longlong(-7)

    def both(p, radius, origin, k, null_output, message):
        org = None if origin is None else (C.c_float * 3)(*origin)
        assert L.apd_points_estimate_normals(p, radius, org, k, None if null_output else C.c_void_p(normal.ctypes.data),
                                             None if null_output else C.c_void_p(variation.ctypes.data)) == -1
        assert L.apd_fusion_last_error().decode() == "apd_points_estimate_normals: " + message
        assert L.apd_points_with_estimated_normals(p, radius, org, k, None if null_output else C.byref(out), C.byref(estimated)) == -1
        assert L.apd_fusion_last_error().decode() == "apd_points_with_estimated_normals: " + message
        assert out.value == 1234 and estimated.value == -7 and normal.tolist() == [77] * 6 and variation.tolist() == [77, 77]

    both(None, 1.0, None, 3, False, "null argument")
    both(pts._p, 1.0, None, 3, True, "null argument")
    for (radius, origin), message in BAD_RADIUS:
        both(pts._p, radius, origin, 3, False, message)
    both(pts._p, 1.0, None, 0, False, "min_neighbours = 0, not in 2 .. 2147483647")
    both(pts._p, 1.0, None, 1, False, "min_neighbours = 1, not in 2 .. 2147483647")
    both(pts._p, 1.0, None, 0x80000000, False, "min_neighbours = 2147483648, not in 2 .. 2147483647")
    both(pts._p, 1.0, None, 0xFFFFFFFF, False, "min_neighbours = 4294967295, not in 2 .. 2147483647")
    # one of the two outputs may be NULL: then the radius is what is refused
    assert L.apd_points_estimate_normals(pts._p, 0.0, None, 3, None, C.c_void_p(variation.ctypes.data)) == -1
    assert L.apd_fusion_last_error().decode() == "apd_points_estimate_normals: a radius of 0, not a positive finite number"
    assert L.apd_points_estimate_normals(pts._p, 0.0, None, 3, C.c_void_p(normal.ctypes.data), None) == -1
    assert L.apd_fusion_last_error().decode() == "apd_points_estimate_normals: a radius of 0, not a positive finite number"
    with pytest.raises(pkg.ApdError, match="apd_points_estimate_normals: a radius of 0"):
        pts.estimate_normals(0.0, 3)
    with pytest.raises(pkg.ApdError, match="apd_points_with_estimated_normals: min_neighbours = 1, not in 2"):
        pts.with_estimated_normals(1.0, 1)
    with pytest.raises(pkg.ApdError, match="apd_points_with_estimated_normals: origin component 0 is inf"):
        pts.with_estimated_normals(1.0, 2, origin=[float("inf"), 0, 0])
    with pytest.raises(ValueError, match="a minimum of -1 neighbours"):   # the Python layer: a negative count does not wrap into an unsigned one
        pts.estimate_normals(1.0, -1)
    with pytest.raises(ValueError, match="a minimum of 4294967298 neighbours"):   # nor does a large one wrap into 2
        pts.with_estimated_normals(1.0, 2 ** 32 + 2)
    pts.close()


def test_objects_without_points_give_empty_results_without_a_device(pkg):
    empty = cloud(np.zeros((0, 3), np.float32))
    pts = from_cloud(pkg, empty, [4], [5], [[]])
    normals, variation = pts.estimate_normals(1.0, 3)
    assert normals.dtype == np.float32 and normals.shape == (0, 3) and variation.dtype == np.float32 and variation.shape == (0,)
    same_points, estimated = pts.with_estimated_normals(1.0, 2, origin=[1, 2, 3])
    assert same_points.count == 0 and estimated == 0 and not same_points.merged and not same_points.on_device
    assert same_points.visibility()[0].tolist() == [0]
    merged, _ = pts.merge_voxels(1.0)           # a merged object without points stays merged
    again, _ = merged.with_estimated_normals(1.0, 2)
    assert again.merged and again.count == 0
    # `estimated` may be NULL
    out = C.c_void_p()
    assert pkg.lib().apd_points_with_estimated_normals(pts._p, 1.0, None, 2, C.byref(out), None) == 0
    pkg.lib().apd_points_destroy(out)


def test_no_gpu_means_the_estimate_fails_loudly(pkg):
    """There is no host implementation: without a device a non-empty host object is refused with a message, and the outputs
    stay as they were."""
    if pkg.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = pkg.lib()
    pts = from_cloud(pkg, cloud([[0.5, 0, 0], [0.6, 0, 0], [0.6, 0.1, 0]]), [4], [5], [[]])
    out, estimated = C.c_void_p(1234), C.c_longlong(-7)
    assert L.apd_points_with_estimated_normals(pts._p, 1.0, None, 2, C.byref(out), C.byref(estimated)) != 0
    assert L.apd_fusion_last_error().startswith(b"apd_points_with_estimated_normals: hipSetDevice(")
    assert out.value == 1234 and estimated.value == -7
    with pytest.raises(pkg.ApdError, match=r"apd_points_estimate_normals: hipSetDevice\("):
        pts.estimate_normals(1.0, 2)
    pts.close()


# --------------------------------------------------------------------------------------------------------------------
# the real cloud of the device tests; the kernel's resources
# --------------------------------------------------------------------------------------------------------------------

def test_real_cloud_choice_is_not_vacuous(ob, vis, radius_checker, checker):
    """On the sequential fusion's points, at the radius of the radius filter's tests and REAL_MIN neighbours: some points get an
    estimate and some do not, no point is capped, and the brute-force mode gives what the grid mode gives."""
    name, variant, _ = REAL_CLOUD
    want = VC.fuse_case(vis, ob, variant, fusion_cases.case(name))
    c = PV.Cloud(*[getattr(want, f) for f in PV.FIELDS], want.offsets, want.views)
    radius = real_cloud_radius(radius_checker, c)
    res = PN.run(checker, c, radius, REAL_MIN)
    print(name, variant, c.count, radius, res.count, int(res.sweeps.max()))
    assert 0 < res.count < c.count and not res.capped.any()
    assert c.count > 20001 or same(PN.run(checker, c, radius, REAL_MIN, mode=PN.BRUTE), res)
    angle, differ, under = against_numpy(c, res, radius, REAL_MIN)
    print("angle %.3g rad, variation %.3g, under the gap bound %.4f" % (angle, differ, under))   # reported, not asserted: not a planted cloud


def test_the_normals_kernel_uses_no_scratch_memory(tmp_path):
    """k_point_normals keeps its ten sums, the matrix and the vectors in registers: the compiler reports 0 bytes of scratch per lane,
    no spilled register and no LDS for it, and no scratch for any kernel of the file."""
    found = walk_kernel_resources("k_point_normals", tmp_path)
    for name, v in found.items():
        assert v["ScratchSize [bytes/lane]"] == "0", name
