"""Neighbours within a radius and the removal of sparse points without a device: the two modes of the sequential checker
(tests/helpers/points_radius_ref.cpp) against each other and against hand-computed answers on every clause of contract C11; the
clouds the device tests run, made here; the refusals of apd_points_neighbour_counts and apd_points_remove_sparse, which need no
device; objects without points; the loud failure without a GPU; and the radius of the device tests' real clouds, chosen with the
checker alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fusion_cases
from common import walk_kernel_resources
import points_radius_checker as PR
import points_voxel_checker as PV
import vis_checker as VC
from test_points_voxel import REAL_CLOUDS, cloud, from_cloud, views_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("apd_points_neighbour_counts", "apd_points_remove_sparse")
EDGE = 2 ** 20
UP = float(np.nextafter(np.float32(1), np.float32(2)))   # the binary32 after 1


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return PR.build(tmp_path_factory.mktemp("points_radius_checker"))


@pytest.fixture(scope="module")
def voxel_checker(tmp_path_factory):
    return PV.build(tmp_path_factory.mktemp("points_voxel_checker"))


@pytest.fixture(scope="module")
def vis(tmp_path_factory):
    return VC.build(tmp_path_factory.mktemp("vis_checker"))


def sort_tile(pkg):
    t, s = C.c_int(), C.c_int()
    pkg.lib().apd_sort_tile_sizes(C.byref(t), C.byref(s))
    return t.value


# --------------------------------------------------------------------------------------------------------------------
# the clouds of the device tests (test_gpu_points_radius.py), all at radius 1 and origin 0 unless they say otherwise
# --------------------------------------------------------------------------------------------------------------------

def dressed(rng, xyz, num_views=3, nsrc=2):
    """(PV.Cloud, (rows, cols, pairs)) of points at xyz with random normals, colours, views and sources."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    rows, cols, pairs = views_of(num_views, nsrc)
    view = rng.integers(0, num_views, n).astype(np.int32)
    sources = rng.integers(0, 1 << nsrc, n).astype(np.uint32)
    c = cloud(xyz, normal=rng.normal(size=(n, 3)).astype(np.float32), bgr=rng.integers(0, 256, (n, 3)).astype(np.uint8), view=view, sources=sources,
              pairs=pairs)
    return c, (rows, cols, pairs)


def three_per_cell(rng, n, cells=None):
    """n points at about three per cell: half of them in cells drawn from the whole grid, which have no occupied cell beside them
    -- 1, 2, 3, 4, 5, 1, 2, ... points to a cell, so some of them have no neighbour and some have four, or with `cells` that many
    cells with random numbers of points; half of them anywhere in a block of about n / 6 cells around the origin, with
    neighbours across the borders of their cells."""
    far = n - n // 2
    if cells is None:
        member = np.repeat(np.arange(far), 1 + np.arange(far) % 5)[:far]
    else:
        member = rng.integers(0, cells, far)
    corner = rng.integers(-EDGE, EDGE, (int(member.max()) + 1 if far else 1, 3))
    a = corner[member] + rng.random((far, 3)) * 0.5 + 0.25
    side = max(int(round((n / 6.0) ** (1.0 / 3.0))), 1)
    b = (rng.random((n // 2, 3)) - 0.5) * side
    xyz = np.concatenate([a, b]).astype(np.float32)
    return xyz[rng.permutation(n)]


def size_case(pkg, n):
    return dressed(np.random.default_rng(100 + n), three_per_cell(np.random.default_rng(200 + n), n))


def size_list(pkg):
    T = sort_tile(pkg)
    return [0, 1, 2, 63, 64, 65, 255, 256, 257, 3 * T + 17, 5 * T + 17]


def border_case():
    """Every pair of points stands apart from the others (the groups are 10 cells apart along y).  The expected counts are
    hand-computed beside each group."""
    groups = [
        # at exact integers, on cell borders: (0,0,0)-(1,0,0) at distance exactly 1 count each other, (0,0,0)-(0,1,0) too; (1,0,0)-(0,1,0) are sqrt(2) apart
        ([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [2, 1, 1]),
        # distance exactly 1 counts, the next binary32 after 1 does not
        ([[0.25, 0, 0], [1.25, 0, 0]], [1, 1]),
        ([[0, 0, 0], [UP, 0, 0]], [0, 0]),
        # the same in negative cells
        ([[-3.75, 0, 0], [-2.75, 0, 0]], [1, 1]),
        ([[-0.5, 0, 0], [-0.5 - UP, 0, 0]], [0, 0]),
        ([[-7, 0, 0], [-8, 0, 0]], [1, 1]),
        # across a cell border, near; and two cells apart, at more than a radius
        ([[0.9, 0.5, 0.5], [1.1, 0.5, 0.5]], [1, 1]),
        ([[0.9, 0.5, 0.5], [2.1, 0.5, 0.5]], [0, 0]),
        # diagonal neighbours across an edge and a corner of the cell
        ([[0.9, 0.9, 0.5], [1.1, 1.1, 0.5]], [1, 1]),
        ([[0.9, 0.9, 0.9], [1.1, 1.1, 1.1], [-0.1 + 1, 0.9, 1.2]], [2, 2, 2]),
        # three coincident points: each counts the other two
        ([[0.5, 0.5, 0.5]] * 3, [2, 2, 2]),
    ]
    xyz, want = [], []
    for g, (pts, counts) in enumerate(groups):
        xyz += [[p[0], p[1] + 10 * g, p[2]] for p in pts]
        want += counts
    return np.float32(xyz), want


def grid_edge_case():
    """Points in the outermost cells.  x cells 2^20 - 1 of row y and -2^20 of row y + 1 have consecutive keys and are not
    neighbours; the outermost y and z cells have their own neighbours and nothing beyond them."""
    lo, hi = -float(EDGE), float(EDGE) - 1
    xyz = [[hi + 0.5, 0.5, 0.5], [lo + 0.5, 1.5, 0.5],        # consecutive keys, 2^21 cells apart: 0 each
           [hi + 0.5, 0.75, 0.5],                              # a neighbour of the first, in its cell
           [lo + 0.25, 1.5, 0.5], [lo + 1.0, 1.5, 0.5],        # neighbours of the second: same cell, and the next cell
           [0.5, hi + 0.5, 0.5], [0.5, hi - 0.25, 0.5],        # outermost y cell and the one below
           [0.5, lo + 0.5, 0.5], [0.5, lo + 0.5, 1.25],
           [0.5, 0.5, hi + 0.75], [0.5, 0.5, hi - 0.125],      # outermost z cells
           [0.5, 0.5, lo + 0.25], [1.25, 0.5, lo + 0.25],
           [hi + 0.5, hi + 0.5, hi + 0.5], [hi + 0.25, hi + 0.25, hi + 0.25],   # the last cell of the grid
           [lo, lo, lo], [lo + 0.5, lo + 0.5, lo + 0.5]]       # the first
    want = [1, 2, 1, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]
    return np.float32(xyz), want


def outside_case(rng, n=600):
    """Ordinary points with NaN, infinities and points 3 * 2^20 cells out among them: (xyz, the indices outside the grid)."""
    xyz = three_per_cell(rng, n)
    bad = [0, 1, 63, 64, 255, 256, 257, n - 2, n - 1]
    values = [np.nan, np.inf, -np.inf, 3.0 * EDGE, -3.0 * EDGE]
    for j, k in enumerate(bad):
        xyz[k, j % 3] = values[j % len(values)]
    return xyz, bad


def dense_case(rng, n=20001):
    """n points inside the one cell of a grid of cell size 1 at origin -0.5: the coordinates of the voxel test's one-cell case
    (magnitudes from 1e-2 to 1e8 and more) scaled by 4e-9 and clipped to [-0.49, 0.49]: a few hundred points lie on every face
    of the cell, and those on opposite faces are a radius or more apart when they differ on another axis too."""
    xyz = rng.normal(size=(n, 3)) * 10.0 ** rng.integers(-2, 9, (n, 3))
    return np.clip(xyz * 4e-9, -0.49, 0.49).astype(np.float32)


DENSE_RADIUS, DENSE_ORIGIN = 1.0, [-0.5] * 3


def large_case(rng, n=200000):
    """n points over n / 4 cells: a pool of that many cells drawn from [-64, 64)^3, where about one cell in forty is taken, so
    that many of them have a taken cell beside them; the points anywhere inside their cells."""
    cells = rng.integers(-64, 64, (n // 4, 3))
    return (cells[rng.integers(0, n // 4, n)] + rng.random((n, 3))).astype(np.float32)


def determinism_case():
    return dressed(np.random.default_rng(13), three_per_cell(np.random.default_rng(14), 20000))


MERGED_RADIUS, MERGED_MIN = 8.0, 2


def merged_many_views_case(voxel_checker):
    """(the input cloud, its views, its merge at cell size 1 by the voxel checker): 3000 points of 200 views in 300 cells, so the
    merged points have lists that no mask holds.  Filtered at MERGED_RADIUS with MERGED_MIN."""
    from test_gpu_points_voxel import many_views_cloud
    c, views = many_views_cloud(np.random.default_rng(12), 3000, 300)
    return c, views, PV.merge(voxel_checker, c, 1.0)


def modes_agree(checker, c, radius, mins, origin=None, caps=(0, 2), what=""):
    """The double loop over all pairs and the 27 lookups per point on one cloud: the same counts at every cap, the same points
    kept at every minimum, with the same arrays and lists.  Returns the uncapped counts."""
    assert c.count <= 20001, what
    full = None
    for cap in caps:
        brute, grid = PR.counts(checker, c, radius, cap, origin, PR.BRUTE), PR.counts(checker, c, radius, cap, origin, PR.GRID)
        assert np.array_equal(brute, grid), (what, cap)
        full = grid if cap == 0 else full
        assert cap == 0 or full is None or np.array_equal(grid, np.minimum(full, cap)), (what, cap)
    for k in mins:
        a, b = PR.remove(checker, c, radius, k, origin, PR.BRUTE), PR.remove(checker, c, radius, k, origin, PR.GRID)
        assert np.array_equal(a.index, b.index) and a.removed == b.removed, (what, k)
        PV.assert_equal(a, b, (what, k))
    return full


def small_cases(pkg, voxel_checker):
    """name -> (cloud, radius, origin, caps, minima) of every synthetic device case with at most 20 001 points, with the caps and
    the minima its device test runs.  The real clouds, which need a fusion, are held the same way where they are made:
    test_real_cloud_radius_removes_some_points_and_not_all here, and test_gpu_points_radius.py for those a device makes."""
    out = {}
    for n in size_list(pkg):
        out["n=%d" % n] = (size_case(pkg, n)[0], 1.0, None, (0, 2), (1, 3))
    out["borders"] = (dressed(np.random.default_rng(1), border_case()[0])[0], 1.0, None, (0, 2), (1, 3))
    out["grid edges"] = (dressed(np.random.default_rng(2), grid_edge_case()[0])[0], 1.0, None, (0, 2), (1, 2))
    out["outside"] = (dressed(np.random.default_rng(3), outside_case(np.random.default_rng(4))[0])[0], 1.0, None, (0, 2), (0, 1, 3))
    out["cap"] = (dressed(np.random.default_rng(5), three_per_cell(np.random.default_rng(6), 3000))[0], 1.0, [0.25, -0.5, 0.125], (0, 1, 3, 1000), (2,))
    out["dense"] = (dressed(np.random.default_rng(7), dense_case(np.random.default_rng(8)))[0], DENSE_RADIUS, DENSE_ORIGIN, (0,), ())
    out["merged"] = (merged_many_views_case(voxel_checker)[2], MERGED_RADIUS, None, (0, 5), (MERGED_MIN,))
    out["determinism"] = (determinism_case()[0], 1.0, None, (0,), (3,))
    return out


def real_cloud_radius(checker, c):
    """Three times the median distance from a point of `c` to its nearest other point, from the checker's counts alone: the median
    nearest distance is the radius at which half of the points have a neighbour, found by doubling up from 2^-20 of the extent
    (so that no radius tried holds many points) and eight steps of bisection."""
    finite = c.xyz[np.isfinite(c.xyz).all(axis=1)]
    half_have_one = lambda r: 2 * int((PR.counts(checker, c, r, cap=1) > 0).sum()) >= c.count
    hi = float(np.linalg.norm(finite.max(axis=0) - finite.min(axis=0))) * 2.0 ** -20
    while not half_have_one(hi):
        hi *= 2.0
    lo = 0.5 * hi
    for _ in range(8):
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if half_have_one(mid) else (mid, hi)
    return float(np.float32(3.0 * hi))


# --------------------------------------------------------------------------------------------------------------------
# the checker
# --------------------------------------------------------------------------------------------------------------------

def test_checker_counts_on_cell_borders(checker):
    xyz, want = border_case()
    for mode in (PR.BRUTE, PR.GRID):
        assert PR.counts(checker, cloud(xyz), 1.0, mode=mode).tolist() == want, mode
    # a radius that is no power of two, an origin: 0.3 apart at radius 0.3 + a little counts, at radius 0.29 it does not
    pair = cloud([[0.1, 0.2, 0.3], [0.4, 0.2, 0.3]])
    assert PR.counts(checker, pair, 0.31, origin=[0.05, 0, 0]).tolist() == [1, 1]
    assert PR.counts(checker, pair, 0.29, origin=[0.05, 0, 0]).tolist() == [0, 0]


def test_checker_counts_at_the_edges_of_the_grid(checker):
    xyz, want = grid_edge_case()
    for mode in (PR.BRUTE, PR.GRID):
        assert PR.counts(checker, cloud(xyz), 1.0, mode=mode).tolist() == want, mode


def test_checker_points_outside_the_grid_count_nothing_and_are_counted_by_nobody(checker):
    xyz, bad = outside_case(np.random.default_rng(4))
    c = cloud(xyz)
    inside = np.setdiff1d(np.arange(c.count), bad)
    got = PR.counts(checker, c, 1.0)
    assert (got[bad] == 0).all() and got[inside].sum() > 0
    assert np.array_equal(got[inside], PR.counts(checker, cloud(xyz[inside]), 1.0))   # as if they were not there
    at1, at0 = PR.remove(checker, c, 1.0, 1), PR.remove(checker, c, 1.0, 0)
    assert not np.isin(bad, at1.index).any() and 0 < at1.removed < c.count
    assert at0.removed == 0 and np.array_equal(at0.index, np.arange(c.count))
    PV.assert_equal(PV.Cloud(*[getattr(at0, f) for f in PV.FIELDS], at0.offsets, at0.views), c)


def test_checker_cap_and_removal(checker):
    """Five points in a row 0.4 apart at radius 1: the neighbours are those at most two steps away."""
    c = cloud([[0.4 * k, 0, 0] for k in range(5)], view=[0, 1, 2, 1, 0], sources=[1, 2, 3, 0, 1], pairs=views_of(3, 2)[2])
    for mode in (PR.BRUTE, PR.GRID):
        assert PR.counts(checker, c, 1.0, mode=mode).tolist() == [2, 3, 4, 3, 2]
        assert PR.counts(checker, c, 1.0, cap=3, mode=mode).tolist() == [2, 3, 3, 3, 2]
        kept = PR.remove(checker, c, 1.0, 3, mode=mode)
        assert kept.index.tolist() == [1, 2, 3] and kept.removed == 2
        assert np.array_equal(kept.xyz, c.xyz[1:4]) and kept.sources.tolist() == [2, 3, 0] and kept.view.tolist() == [1, 2, 1]
        assert kept.offsets.tolist() == [0, 2, 5, 6] and kept.views.tolist() == c.views[c.offsets[1]:c.offsets[4]].tolist()
        assert PR.remove(checker, c, 1.0, 5, mode=mode).count == 0


def test_brute_force_and_grid_agree_on_every_small_device_case(pkg, checker, voxel_checker):
    """The double loop over all pairs and the 27 lookups per point give the same integers, capped and not, and keep the same
    points: the cell condition is part of the relation.  Every synthetic cloud of the device tests with at most 20 001 points."""
    for name, (c, radius, origin, caps, mins) in small_cases(pkg, voxel_checker).items():
        full = modes_agree(checker, c, radius, mins, origin, caps, what=name)
        if name == "dense":
            assert 0 < full.min() < full.max() <= c.count - 1   # one cell, and the radius cuts through it
        for k in mins:
            if c.count >= 63 and k > 0:   # what the device tests rely on
                assert 0 < PR.remove(checker, c, radius, k, origin).removed < c.count, (name, k)


# --------------------------------------------------------------------------------------------------------------------
# the C ABI without a device
# --------------------------------------------------------------------------------------------------------------------

def test_header_declares_the_entry_points_as_ctypes_calls_them(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "apd_mi355x.h")).read(), flags=re.S)
    assert re.search(r"int\s+apd_points_neighbour_counts\s*\(\s*apd_points_t\s+\w+\s*,\s*float\s+\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,"
                     r"\s*unsigned\s+\w+\s*,\s*uint32_t\s*\*\s*\w+\s*\)", text)
    assert re.search(r"int\s+apd_points_remove_sparse\s*\(\s*apd_points_t\s+\w+\s*,\s*float\s+\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,"
                     r"\s*unsigned\s+\w+\s*,\s*apd_points_t\s*\*\s*\w+\s*,\s*long\s+long\s*\*\s*\w+\s*\)", text)
    L = pkg.lib()
    fp, vpp, llp = C.POINTER(C.c_float), C.POINTER(C.c_void_p), C.POINTER(C.c_longlong)
    assert L.apd_points_neighbour_counts.argtypes == [C.c_void_p, C.c_float, fp, C.c_uint, C.c_void_p]
    assert L.apd_points_remove_sparse.argtypes == [C.c_void_p, C.c_float, fp, C.c_uint, vpp, llp]


def test_library_exports_the_entry_points(pkg):
    for name in NEW_SYMBOLS:
        assert hasattr(pkg.lib(), name), name


BAD = [((0.0, None), "a radius of 0, not a positive finite number"),
       ((-1.0, None), "a radius of -1, not a positive finite number"),
       ((float("inf"), None), "a radius of inf, not a positive finite number"),
       ((float("nan"), None), "a radius of nan, not a positive finite number"),
       ((1e30, None), "a radius of 1e+30, whose square inf is not a positive finite number"),
       ((1e-30, None), "a radius of 1e-30, whose square 0 is not a positive finite number"),
       ((1.0, [0.0, float("nan"), 0.0]), "origin component 1 is nan"),
       ((1.0, [0.0, 0.0, float("-inf")]), "origin component 2 is -inf")]


def test_refusals_that_need_no_device(pkg):
    """Every bad argument answers APD_ERR_INVALID with its message and leaves the outputs as they were: no device is touched,
    so this passes on a machine without one."""
    L = pkg.lib()
    pts = from_cloud(pkg, cloud([[0.5, 0, 0], [0.6, 0, 0]]), [4], [5], [[]])
    counts = np.full(2, 77, np.uint32)
    out, removed = C.c_void_p(1234), C.c_longlong(-7)

    def both(p, radius, origin, null_output, message):
        org = None if origin is None else (C.c_float * 3)(*origin)
        assert L.apd_points_neighbour_counts(p, radius, org, 0, None if null_output else C.c_void_p(counts.ctypes.data)) == -1
        assert L.apd_fusion_last_error().decode() == "apd_points_neighbour_counts: " + message
        assert L.apd_points_remove_sparse(p, radius, org, 1, None if null_output else C.byref(out), C.byref(removed)) == -1
        assert L.apd_fusion_last_error().decode() == "apd_points_remove_sparse: " + message
        assert out.value == 1234 and removed.value == -7 and counts.tolist() == [77, 77]

    both(None, 1.0, None, False, "null argument")
    both(pts._p, 1.0, None, True, "null argument")
    for (radius, origin), message in BAD:
        both(pts._p, radius, origin, False, message)
    with pytest.raises(pkg.ApdError, match="apd_points_neighbour_counts: a radius of 0"):
        pts.neighbour_counts(0.0)
    with pytest.raises(pkg.ApdError, match="apd_points_remove_sparse: origin component 0 is inf"):
        pts.remove_sparse(1.0, 2, origin=[float("inf"), 0, 0])
    with pytest.raises(ValueError, match="a cap of -1"):   # the Python layer: a negative count does not wrap into an unsigned one
        pts.neighbour_counts(1.0, cap=-1)
    with pytest.raises(ValueError, match="a minimum of -2 neighbours"):
        pts.remove_sparse(1.0, -2)
    pts.close()


def test_objects_without_points_give_empty_results_without_a_device(pkg):
    empty = cloud(np.zeros((0, 3), np.float32))
    pts = from_cloud(pkg, empty, [4], [5], [[]])
    got = pts.neighbour_counts(1.0, cap=3)
    assert got.dtype == np.uint32 and got.shape == (0,)
    kept, removed = pts.remove_sparse(1.0, 2, origin=[1, 2, 3])
    assert kept.count == 0 and removed == 0 and not kept.merged and not kept.on_device
    assert kept.visibility()[0].tolist() == [0]
    again, removed = kept.remove_sparse(0.5, 0)
    assert again.count == 0 and removed == 0
    merged, _ = pts.merge_voxels(1.0)           # a merged object without points stays merged
    kept_merged, _ = merged.remove_sparse(1.0, 1)
    assert kept_merged.merged and kept_merged.count == 0
    # `removed` may be NULL
    out = C.c_void_p()
    assert pkg.lib().apd_points_remove_sparse(pts._p, 1.0, None, 1, C.byref(out), None) == 0
    pkg.lib().apd_points_destroy(out)


def test_no_gpu_means_the_counts_fail_loudly(pkg):
    """There is no host implementation: without a device a non-empty host object is refused with a message, and the outputs
    stay as they were."""
    if pkg.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = pkg.lib()
    pts = from_cloud(pkg, cloud([[0.5, 0, 0], [0.6, 0, 0]]), [4], [5], [[]])
    out, removed = C.c_void_p(1234), C.c_longlong(-7)
    assert L.apd_points_remove_sparse(pts._p, 1.0, None, 1, C.byref(out), C.byref(removed)) != 0
    assert L.apd_fusion_last_error().startswith(b"apd_points_remove_sparse: hipSetDevice(")
    assert out.value == 1234 and removed.value == -7
    with pytest.raises(pkg.ApdError, match=r"apd_points_neighbour_counts: hipSetDevice\("):
        pts.neighbour_counts(1.0)
    pts.close()


# --------------------------------------------------------------------------------------------------------------------
# the real clouds of the device tests; the kernel's resources
# --------------------------------------------------------------------------------------------------------------------

def test_the_count_kernel_uses_no_scratch_memory(tmp_path):
    """k_neighbour_count, the walk with the least around it: the compiler reports 0 bytes of scratch per lane, no spilled register,
    no LDS and 8 waves per SIMD for it, and no scratch for any kernel of the file."""
    found = walk_kernel_resources("k_neighbour_count", tmp_path)
    for name, v in found.items():
        assert v["ScratchSize [bytes/lane]"] == "0", name


@pytest.mark.parametrize("name,variant", [(n, v) for n, v, _ in REAL_CLOUDS])
def test_real_cloud_radius_removes_some_points_and_not_all(ob, vis, checker, name, variant):
    """At three times its median nearest-point spacing -- a radius that is no power of two, where the cell quotient rounds -- the
    checker alone, on the sequential fusion's points, finds a number of neighbours to ask for that removes some points and keeps
    some; and on the clouds with at most 20 001 points its brute-force mode gives what its grid mode gives."""
    want = VC.fuse_case(vis, ob, variant, fusion_cases.case(name))
    c = PV.Cloud(*[getattr(want, f) for f in PV.FIELDS], want.offsets, want.views)
    radius = real_cloud_radius(checker, c)
    counts = PR.counts(checker, c, radius)
    k = real_cloud_min_neighbours(counts)
    kept = PR.remove(checker, c, radius, k)
    print(name, variant, c.count, radius, k, kept.removed)
    assert 0 < kept.removed < c.count
    if c.count <= 20001:
        modes_agree(checker, c, radius, (k,), what=(name, variant))


def real_cloud_min_neighbours(counts):
    """One more than the tenth percentile of the uncapped counts: about a tenth of the points go, whatever the density."""
    return int(np.sort(counts)[len(counts) // 10]) + 1
