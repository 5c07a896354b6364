"""The k-nearest mean distances and the statistical removal without a device: the two modes of the sequential checker
(tests/helpers/points_knn_ref.cpp) against each other and against hand-computed answers on every clause of contract C12; the
threshold's chunked binary64 sums against a plain Python restatement; the clouds the device tests run, made here; the refusals of
apd_points_knn_mean_distances and apd_points_remove_statistical, which need no device; objects without points; the loud failure
without a GPU; the choices for the device tests' real clouds, made with the checkers alone; and the kernel's scratch size."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import fusion_cases
from common import walk_kernel_resources
import points_knn_checker as PK
import points_radius_checker as PR
import points_voxel_checker as PV
import vis_checker as VC
from test_points_radius import (DENSE_ORIGIN, DENSE_RADIUS, MERGED_RADIUS, BAD as BAD_RADIUS, border_case, dense_case, determinism_case, dressed, grid_edge_case,
                                merged_many_views_case, outside_case, real_cloud_radius, size_case, size_list)
from test_points_voxel import REAL_CLOUDS, cloud, from_cloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("apd_points_knn_mean_distances", "apd_points_remove_statistical")
SIZE_KS = (1, 2, 7, 33, 64)
INF = float("inf")
f32 = np.float32


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return PK.build(tmp_path_factory.mktemp("points_knn_checker"))


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


def bits64(x):
    return struct.pack("<d", x)


# --------------------------------------------------------------------------------------------------------------------
# the clouds of the device tests (test_gpu_points_knn.py) that test_points_radius.py does not make
# --------------------------------------------------------------------------------------------------------------------

ARRIVAL_KS = (1, 7, 33, 64)


def arrival_case(rng, per_copy=150):
    """Three copies of one cell's points, ten cells apart along x, around a first point at the cell's centre: the others stand on
    random directions at distances between 2^-10 and 0.45 that ascend with the input index in the first copy, descend in the
    second and are shuffled in the third.  The sort of the cells is stable, so in sorted order the centre's nearest candidates
    arrive first in the first copy (no replacement after the first k), last in the second (every candidate replaces) and in no
    order in the third; the other points of a copy see everything in between."""
    t = np.sort(rng.random(per_copy - 1) * (0.45 - 2.0 ** -10) + 2.0 ** -10)
    direction = rng.normal(size=(per_copy - 1, 3))
    direction /= np.linalg.norm(direction, axis=1)[:, None]
    out = []
    for copy, order in enumerate((np.arange(per_copy - 1), np.arange(per_copy - 1)[::-1], rng.permutation(per_copy - 1))):
        centre = np.array([0.5 + 10 * copy, 0.5, 0.5])
        out.append(np.concatenate([centre[None], centre + direction[order] * t[order, None]]))
    return np.concatenate(out).astype(np.float32)


LATTICE_KS = (6, 7, 18, 19, 33, 64)


def lattice_case():
    """The 8 x 8 x 8 points at multiples of 1/4 in [0, 2)^3 at radius 1: every squared distance is a multiple of 1/16 and exact, an
    inner point has 6 neighbours at 1/4, 12 at sqrt(2)/4, 8 at sqrt(3)/4, 6 at 1/2, ...: at most values of k many candidates tie
    at the k-th distance."""
    g = np.arange(8) * 0.25
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)


def small_cases(pkg, voxel_checker):
    """name -> (cloud, views, radius, origin, the k values, the ratios) of every synthetic device case with at most 20 001 points."""
    out = {}
    for n in size_list(pkg):
        out["n=%d" % n] = (*size_case(pkg, n), 1.0, None, SIZE_KS, (1.0,))
    out["borders"] = (*dressed(np.random.default_rng(1), border_case()[0]), 1.0, None, (1, 2), (0.0,))
    out["grid edges"] = (*dressed(np.random.default_rng(2), grid_edge_case()[0]), 1.0, None, (1, 2), (0.0,))
    out["outside"] = (*dressed(np.random.default_rng(3), outside_case(np.random.default_rng(4))[0]), 1.0, None, (1, 3), (0.5,))
    out["arrival"] = (*dressed(np.random.default_rng(21), arrival_case(np.random.default_rng(22))), 1.0, None, ARRIVAL_KS, (0.0, -0.5))
    out["lattice"] = (*dressed(np.random.default_rng(23), lattice_case()), 1.0, None, LATTICE_KS, (0.0, 1.0))
    out["dense"] = (*dressed(np.random.default_rng(7), dense_case(np.random.default_rng(8))), DENSE_RADIUS, DENSE_ORIGIN, (64,), (1.0,))
    c, views, first = merged_many_views_case(voxel_checker)
    out["merged"] = (first, views, MERGED_RADIUS, None, (3,), (0.5,))
    out["determinism"] = (*determinism_case(), 1.0, [0.25, -0.5, 0.125], (4,), (1.0,))
    return out


def modes_agree(checker, c, radius, ks, ratios, origin=None, what=""):
    """The double loop over all pairs with a full sort and the 27 lookups per point with a partial sort on one cloud: the same
    bits of every score, the same threshold, the same points kept with the same arrays and lists."""
    assert c.count <= 20001, what
    for k in ks:
        for ratio in ratios:
            sa, a = PK.run(checker, c, radius, k, ratio, origin, PK.BRUTE)
            sb, b = PK.run(checker, c, radius, k, ratio, origin, PK.GRID)
            assert np.array_equal(bits32(sa), bits32(sb)), (what, k)
            assert bits64(a.threshold) == bits64(b.threshold) and a.removed == b.removed and np.array_equal(a.index, b.index), (what, k, ratio)
            PV.assert_equal(a, b, (what, k, ratio))


def real_cloud_choice(radius_checker, checker, c):
    """(radius, k, ratio) for a real cloud from the checkers alone: the radius of the radius filter's tests, k the tenth percentile
    of the uncapped neighbour counts (1 .. 64), and the ratio that puts T at the 90th percentile of the finite scores: mu and
    sigma are read off the checker's own thresholds at ratios 0 and 1."""
    radius = real_cloud_radius(radius_checker, c)
    counts = PR.counts(radius_checker, c, radius)
    k = min(max(int(np.sort(counts)[len(counts) // 10]), 1), 64)
    scores = PK.scores(checker, c, radius, k)
    finite = np.sort(scores[np.isfinite(scores)])
    mu = PK.threshold(checker, scores, 0.0)[0]
    sigma = PK.threshold(checker, scores, 1.0)[0] - mu
    ratio = float(f32((float(finite[(9 * len(finite)) // 10]) - mu) / sigma))
    return radius, k, ratio


def assert_not_vacuous(checker, c, radius, k, ratio, what=""):
    """What a device test on a real cloud relies on: at least half of the points are full, a full point goes, a point stays."""
    scores, kept = PK.run(checker, c, radius, k, ratio)
    full = int(np.isfinite(scores).sum())
    print(what, c.count, radius, k, ratio, full, kept.removed, kept.threshold)
    assert 2 * full >= c.count, what
    assert kept.count < full, what
    assert kept.count >= 1, what
    return kept


# --------------------------------------------------------------------------------------------------------------------
# the checker: scores
# --------------------------------------------------------------------------------------------------------------------

def test_checker_scores_of_a_row_with_exactly_k_and_with_k_minus_one_neighbours(checker):
    """Four points 1/4 apart in one cell at radius 1: the first has neighbours at 1/4, 1/2, 3/4."""
    c = cloud([[0.25 * j, 0, 0] for j in range(4)])
    third = f32(1.0) / f32(3.0)
    for mode in (PK.BRUTE, PK.GRID):
        assert PK.scores(checker, c, 1.0, 1, mode=mode).tolist() == [0.25] * 4
        assert PK.scores(checker, c, 1.0, 2, mode=mode).tolist() == [0.375, 0.25, 0.25, 0.375]
        got = PK.scores(checker, c, 1.0, 3, mode=mode)                 # exactly k neighbours
        assert got.tolist() == [0.5, float(third), float(third), 0.5]   # (1/4 + 1/2 + 3/4) / 3, (1/4 + 1/4 + 1/2) / 3
        assert PK.scores(checker, c, 1.0, 4, mode=mode).tolist() == [INF] * 4   # k - 1 neighbours
    # a point beyond the radius is no neighbour however few there are: at radius 3/8 the end points have one neighbour, the others two
    assert PK.scores(checker, c, 0.375, 2).tolist() == [INF, 0.25, 0.25, INF]


def test_checker_scores_of_coincident_points(checker):
    c = cloud([[0.5, 0.5, 0.5]] * 3 + [[0.5, 0.5, 1.0]])
    for mode in (PK.BRUTE, PK.GRID):
        assert PK.scores(checker, c, 1.0, 2, mode=mode).tolist() == [0.0, 0.0, 0.0, 0.5]
        want = float((f32(0) + f32(0) + f32(0.5)) / f32(3))
        assert PK.scores(checker, c, 1.0, 3, mode=mode).tolist() == [want, want, want, 0.5]
        assert bits32(PK.scores(checker, c, 1.0, 1, mode=mode)).tolist() == bits32([0.0, 0.0, 0.0, 0.5]).tolist()   # +0, not -0


def test_checker_scores_on_the_tie_lattice(checker):
    """An inner point of the lattice: 6 neighbours at 1/4, then 12 tied at sqrt(1/8): k = 7 takes one of the twelve, whichever."""
    xyz = lattice_case()
    inner = int(np.flatnonzero((xyz == [1.0, 0.75, 0.5]).all(axis=1))[0])
    for mode in (PK.BRUTE, PK.GRID):
        assert PK.scores(checker, cloud(xyz), 1.0, 6, mode=mode)[inner] == 0.25
        for k in (7, 18, 19):
            terms = [f32(0.0625)] * 6 + [f32(0.125)] * 12 + [f32(0.1875)] * 8
            total = f32(0)
            for t in terms[:k]:
                total = f32(total + np.sqrt(t))   # numpy's binary32 sqrt is correctly rounded
            assert PK.scores(checker, cloud(xyz), 1.0, k, mode=mode)[inner] == f32(total / f32(k)), k


def test_checker_scores_at_exactly_the_radius_and_one_ulp_beyond(checker):
    xyz, counts = border_case()
    for mode in (PK.BRUTE, PK.GRID):
        got = PK.scores(checker, cloud(xyz), 1.0, 1, mode=mode)
        assert np.array_equal(np.isfinite(got), np.array(counts) >= 1)
        assert got[3] == got[4] == 1.0            # 0.25 and 1.25: exactly the radius
        assert got[5] == got[6] == INF            # 0 and the binary32 after 1
        assert got[7] == got[8] == 1.0 and got[9] == got[10] == INF   # the same in negative cells
        assert np.array_equal(np.isfinite(PK.scores(checker, cloud(xyz), 1.0, 2, mode=mode)), np.array(counts) >= 2)


def test_checker_points_outside_the_grid_score_infinity_and_are_nobodys_neighbour(checker):
    xyz, bad = outside_case(np.random.default_rng(4))
    c = cloud(xyz)
    inside = np.setdiff1d(np.arange(c.count), bad)
    got = PK.scores(checker, c, 1.0, 1)
    assert np.isinf(got[bad]).all() and np.isfinite(got[inside]).any()
    assert np.array_equal(bits32(got[inside]), bits32(PK.scores(checker, cloud(xyz[inside]), 1.0, 1)))   # as if they were not there
    kept = PK.remove(checker, c, 1.0, 1, 100.0)
    assert not np.isin(bad, kept.index).any() and kept.count == int(np.isfinite(got).sum())


def test_brute_force_and_grid_agree_on_every_small_device_case(pkg, checker, voxel_checker):
    for name, (c, _, radius, origin, ks, ratios) in small_cases(pkg, voxel_checker).items():
        modes_agree(checker, c, radius, ks, ratios, origin, what=name)


def test_the_arrival_and_lattice_cases_hold_what_they_are_for(checker):
    """Arrival: the three centres have the same scores (the same distances in three orders, up to the rounding of the positions
    far from the origin -- so compared loosely), every k up to 64 finds full points.  Lattice: full inner points at k = 64."""
    xyz = arrival_case(np.random.default_rng(22))
    for k in ARRIVAL_KS:
        got = PK.scores(checker, cloud(xyz), 1.0, k)
        assert np.isfinite(got).all(), k
        assert np.allclose(got[[0, 150, 300]], got[0], rtol=1e-4), k
    got = PK.scores(checker, cloud(lattice_case()), 1.0, 64)
    assert np.isfinite(got).sum() > 100 and np.isinf(got).sum() > 0


# --------------------------------------------------------------------------------------------------------------------
# the checker: threshold
# --------------------------------------------------------------------------------------------------------------------

def python_threshold(values, ratio, chunk=256):
    """Contract C12's threshold in plain Python floats (binary64): (T, n_f, S1, S2); chunk=None: one sequential sum."""
    values = [float(v) for v in np.asarray(values, np.float32)]
    chunk = chunk or max(len(values), 1)
    S1 = S2 = 0.0
    n_f = 0
    for first in range(0, len(values), chunk):
        a = b = 0.0
        for v in values[first:first + chunk]:
            if v != INF:
                a = a + v
                b = b + v * v
                n_f += 1
        S1 = S1 + a
        S2 = S2 + b
    if n_f == 0:
        return 0.0, 0, S1, S2
    mu = S1 / n_f
    var = max((S2 - S1 * S1 / n_f) / (n_f - 1), 0.0) if n_f >= 2 else 0.0
    return mu + float(f32(ratio)) * np.sqrt(var).item(), n_f, S1, S2


def same_threshold(got, want):
    return got[1] == want[1] and all(bits64(a) == bits64(b) for a, b in zip((got[0], got[2], got[3]), (want[0], want[2], want[3])))


def test_threshold_of_no_one_and_two_full_points(checker):
    assert PK.threshold(checker, [INF, INF, INF], 2.0) == (0.0, 0, 0.0, 0.0)
    assert PK.threshold(checker, [], 2.0) == (0.0, 0, 0.0, 0.0)
    assert PK.threshold(checker, [INF, 0.75, INF], 2.0) == (0.75, 1, 0.75, 0.5625)        # var = 0 for n_f < 2
    T, n_f, S1, S2 = PK.threshold(checker, [0.25, INF, 0.75], 2.0)
    assert (n_f, S1, S2) == (2, 1.0, 0.625)
    assert T == 0.5 + 2.0 * np.sqrt((0.625 - 1.0 * 1.0 / 2.0) / 1.0)                      # mu 1/2, var 1/8
    # through the clouds: nobody full -> nothing kept, T = 0; two points -> both full with the same score, var = 0, both kept at ratio 0
    lone = PK.remove(checker, cloud([[0.5, 0.5, 0.5], [5.5, 0.5, 0.5]]), 1.0, 1, 3.0)
    assert lone.count == 0 and lone.removed == 2 and lone.threshold == 0.0
    pair = PK.remove(checker, cloud([[0.5, 0.5, 0.5], [0.75, 0.5, 0.5], [5.5, 0.5, 0.5]]), 1.0, 1, 0.0)
    assert pair.index.tolist() == [0, 1] and pair.removed == 1 and pair.threshold == 0.25


def test_threshold_with_all_scores_equal_clamps_the_variance_and_keeps_every_full_point_at_ratio_zero(checker):
    """Pairs 1/4 apart, each pair far from the others, and a few lone points: every full score is 1/4, the sums are exact, the
    variance is 0, T = mu = 1/4 at ratio 0 and every full point stays; a negative ratio changes nothing at sigma = 0.  And the
    clamp itself: 1000 equal scores of 0.1f, where S2 - S1 * S1 / n_f comes out negative in binary64."""
    xyz = [[10.0 * j + 0.25 * h, 0.5, 0.5] for j in range(300) for h in (0, 1)] + [[10.0 * j, 20.5, 0.5] for j in range(5)]
    c = cloud(xyz)
    for ratio in (0.0, -1.0):
        kept = PK.remove(checker, c, 1.0, 1, ratio)
        assert kept.threshold == 0.25 and kept.index.tolist() == list(range(600)) and kept.removed == 5
    values = np.full(1000, 0.1, np.float32)
    T, n_f, S1, S2 = PK.threshold(checker, values, 5.0)
    assert S2 - S1 * S1 / n_f < 0.0 and T == S1 / n_f
    assert same_threshold((T, n_f, S1, S2), python_threshold(values, 5.0))


def test_threshold_with_a_negative_ratio(checker):
    values = [0.25, 0.5, 0.75, 1.0, INF]
    T, n_f, S1, S2 = PK.threshold(checker, values, -0.5)
    assert same_threshold((T, n_f, S1, S2), python_threshold(values, -0.5))
    assert T < S1 / n_f
    c = cloud([[0, 0, 0], [0.25, 0, 0], [0.25, 0.5, 0]])   # scores 1/4, 1/4, 1/2
    kept = PK.remove(checker, c, 1.0, 1, -0.5)
    assert PK.scores(checker, c, 1.0, 1).tolist() == [0.25, 0.25, 0.5]
    assert kept.index.tolist() == [0, 1] and kept.threshold == python_threshold([0.25, 0.25, 0.5], -0.5)[0]


@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_threshold_sums_in_chunks_of_256(checker, n):
    """Scores over sixty binades with infinities among them: the chunked binary64 sums are those of a plain Python loop in the same
    order, bit for bit; and at n = 513, where a full chunk follows the first, they are not those of one sequential sum (at n = 257 the
    second chunk is one score, and adding it to the first chunk's sum is what the sequential sum does too)."""
    rng = np.random.default_rng(n)
    values = (rng.random(n) * 2.0 ** rng.integers(-30, 31, n)).astype(np.float32)
    values[rng.integers(0, n, n // 10)] = INF
    got = PK.threshold(checker, values, 1.5)
    assert same_threshold(got, python_threshold(values, 1.5))
    assert got[1] == int(np.isfinite(values).sum())
    plain = python_threshold(values, 1.5, chunk=None)
    assert same_threshold(got, plain) == (n <= 257)


# --------------------------------------------------------------------------------------------------------------------
# the C ABI without a device
# --------------------------------------------------------------------------------------------------------------------

def test_header_declares_the_entry_points_as_ctypes_calls_them(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "apd_mi355x.h")).read(), flags=re.S)
    assert re.search(r"int\s+apd_points_knn_mean_distances\s*\(\s*apd_points_t\s+\w+\s*,\s*float\s+\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,"
                     r"\s*unsigned\s+\w+\s*,\s*float\s*\*\s*\w+\s*\)", text)
    assert re.search(r"int\s+apd_points_remove_statistical\s*\(\s*apd_points_t\s+\w+\s*,\s*float\s+\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,"
                     r"\s*unsigned\s+\w+\s*,\s*float\s+\w+\s*,\s*apd_points_t\s*\*\s*\w+\s*,\s*long\s+long\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*\)", text)
    L = pkg.lib()
    fp, vpp, llp, dp = C.POINTER(C.c_float), C.POINTER(C.c_void_p), C.POINTER(C.c_longlong), C.POINTER(C.c_double)
    assert L.apd_points_knn_mean_distances.argtypes == [C.c_void_p, C.c_float, fp, C.c_uint, C.c_void_p]
    assert L.apd_points_remove_statistical.argtypes == [C.c_void_p, C.c_float, fp, C.c_uint, C.c_float, vpp, llp, dp]


def test_library_exports_the_entry_points(pkg):
    for name in NEW_SYMBOLS:
        assert hasattr(pkg.lib(), name), name


def test_refusals_that_need_no_device(pkg):
    """Every bad argument answers APD_ERR_INVALID with its message and leaves the outputs as they were: no device is touched,
    so this passes on a machine without one."""
    L = pkg.lib()
    pts = from_cloud(pkg, cloud([[0.5, 0, 0], [0.6, 0, 0]]), [4], [5], [[]])
    mean = np.full(2, 77, np.float32)
    out, removed, threshold = C.c_void_p(1234), C.c_longlong(-7), C.c_double(-3.5)

    def both(p, radius, origin, k, null_output, message, ratio=1.0, scores_too=True):
        org = None if origin is None else (C.c_float * 3)(*origin)
        if scores_too:
            assert L.apd_points_knn_mean_distances(p, radius, org, k, None if null_output else C.c_void_p(mean.ctypes.data)) == -1
            assert L.apd_fusion_last_error().decode() == "apd_points_knn_mean_distances: " + message
        assert L.apd_points_remove_statistical(p, radius, org, k, ratio, None if null_output else C.byref(out), C.byref(removed), C.byref(threshold)) == -1
        assert L.apd_fusion_last_error().decode() == "apd_points_remove_statistical: " + message
        assert out.value == 1234 and removed.value == -7 and threshold.value == -3.5 and mean.tolist() == [77, 77]

    both(None, 1.0, None, 3, False, "null argument")
    both(pts._p, 1.0, None, 3, True, "null argument")
    for (radius, origin), message in BAD_RADIUS:
        both(pts._p, radius, origin, 3, False, message)
    both(pts._p, 1.0, None, 0, False, "k = 0, not in 1 .. 64")
    both(pts._p, 1.0, None, 65, False, "k = 65, not in 1 .. 64")
    both(pts._p, 1.0, None, 0xFFFFFFFF, False, "k = 4294967295, not in 1 .. 64")
    for ratio, text in ((float("nan"), "nan"), (float("inf"), "inf"), (float("-inf"), "-inf")):
        both(pts._p, 1.0, None, 3, False, "a ratio of %s, not a finite number" % text, ratio=ratio, scores_too=False)
    with pytest.raises(pkg.ApdError, match="apd_points_knn_mean_distances: a radius of 0"):
        pts.knn_mean_distances(0.0, 3)
    with pytest.raises(pkg.ApdError, match="apd_points_remove_statistical: k = 65, not in 1 .. 64"):
        pts.remove_statistical(1.0, 65, 1.0)
    with pytest.raises(pkg.ApdError, match="apd_points_remove_statistical: origin component 0 is inf"):
        pts.remove_statistical(1.0, 2, 1.0, origin=[float("inf"), 0, 0])
    with pytest.raises(ValueError, match="k = -1"):   # the Python layer: a negative count does not wrap into an unsigned one
        pts.knn_mean_distances(1.0, -1)
    with pytest.raises(ValueError, match="k = 4294967297"):   # nor does a large one wrap into 1
        pts.remove_statistical(1.0, 2 ** 32 + 1, 1.0)
    pts.close()


def test_objects_without_points_give_empty_results_without_a_device(pkg):
    empty = cloud(np.zeros((0, 3), np.float32))
    pts = from_cloud(pkg, empty, [4], [5], [[]])
    got = pts.knn_mean_distances(1.0, 3)
    assert got.dtype == np.float32 and got.shape == (0,)
    kept, removed, threshold = pts.remove_statistical(1.0, 2, -1.0, origin=[1, 2, 3])
    assert kept.count == 0 and removed == 0 and threshold == 0.0 and not kept.merged and not kept.on_device
    assert kept.visibility()[0].tolist() == [0]
    merged, _ = pts.merge_voxels(1.0)           # a merged object without points stays merged
    kept_merged, _, _ = merged.remove_statistical(1.0, 1, 0.0)
    assert kept_merged.merged and kept_merged.count == 0
    # `removed` and `threshold` may be NULL
    out = C.c_void_p()
    assert pkg.lib().apd_points_remove_statistical(pts._p, 1.0, None, 1, 1.0, C.byref(out), None, None) == 0
    pkg.lib().apd_points_destroy(out)


def test_no_gpu_means_the_scores_fail_loudly(pkg):
    """There is no host implementation: without a device a non-empty host object is refused with a message, and the outputs
    stay as they were."""
    if pkg.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = pkg.lib()
    pts = from_cloud(pkg, cloud([[0.5, 0, 0], [0.6, 0, 0]]), [4], [5], [[]])
    out, removed, threshold = C.c_void_p(1234), C.c_longlong(-7), C.c_double(-3.5)
    assert L.apd_points_remove_statistical(pts._p, 1.0, None, 1, 1.0, C.byref(out), C.byref(removed), C.byref(threshold)) != 0
    assert L.apd_fusion_last_error().startswith(b"apd_points_remove_statistical: hipSetDevice(")
    assert out.value == 1234 and removed.value == -7 and threshold.value == -3.5
    with pytest.raises(pkg.ApdError, match=r"apd_points_knn_mean_distances: hipSetDevice\("):
        pts.knn_mean_distances(1.0, 1)
    pts.close()


# --------------------------------------------------------------------------------------------------------------------
# the real clouds of the device tests; the kernel's resources
# --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,variant", [(n, v) for n, v, _ in REAL_CLOUDS])
def test_real_cloud_choice_is_not_vacuous(ob, vis, radius_checker, checker, name, variant):
    """On the sequential fusion's points, at the radius of the radius filter's tests, k the tenth percentile of the neighbour counts
    and the ratio that puts T at the 90th percentile of the finite scores: at least half of the points are full, a full point
    goes and a point stays; and on the clouds with at most 20 001 points the brute-force mode gives what the grid mode gives."""
    want = VC.fuse_case(vis, ob, variant, fusion_cases.case(name))
    c = PV.Cloud(*[getattr(want, f) for f in PV.FIELDS], want.offsets, want.views)
    radius, k, ratio = real_cloud_choice(radius_checker, checker, c)
    assert_not_vacuous(checker, c, radius, k, ratio, what=(name, variant))
    if c.count <= 20001:
        modes_agree(checker, c, radius, (k,), (ratio,), what=(name, variant))


def test_the_selection_kernel_uses_no_scratch_memory(tmp_path):
    """k_knn_mean keeps a lane's k values in LDS: the compiler reports 0 bytes of scratch per lane for it (k is a runtime argument
    of the one kernel, so this holds for every k), and no spilled register."""
    found = walk_kernel_resources("k_knn_mean", tmp_path)   # no static LDS: the k * 64 slots are the dynamic region
    for name, v in found.items():
        assert v["ScratchSize [bytes/lane]"] == "0", name
