"""The nearest point of another cloud and the score on it, without a device: the two modes of the sequential checker
(tests/helpers/points_nearest_ref.cpp) against each other and against a numpy all-pairs search on every pair of clouds the device
tests run; planted lattices with exact answers; ties; the border, grid-edge and outside-the-grid clouds of test_points_radius.py;
the refusals of apd_points_nearest and apd_points_score, which need no device; objects without points; the loud failure without
a GPU; apd_points_read_ply, which is host code; the kernels' resources."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from common import kernel_resources, walk_kernel_resources
import points_nearest_checker as PX
from test_points_radius import BAD as BAD_RADIUS, EDGE, UP, border_case, dressed, grid_edge_case, outside_case, size_list, three_per_cell
from test_points_voxel import cloud, from_cloud, ply_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("apd_points_nearest", "apd_points_score", "apd_points_read_ply")
INF = float("inf")
f32 = np.float32


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return PX.build(tmp_path_factory.mktemp("points_nearest_checker"))


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# --------------------------------------------------------------------------------------------------------------------
# the pairs of clouds of the device tests (test_gpu_points_nearest.py): name -> (P, Q, radius, origin)
# --------------------------------------------------------------------------------------------------------------------

def queries_near(rng, q, n):
    """n queries for the targets q: each a target drawn at random, moved by a Gaussian of half a radius per axis -- some stay within
    the radius, some leave it, many change cell; in the far cells, where a binary32 step is an eighth of a cell, many come to
    stand at equal distances.  Without targets: three to a cell on their own."""
    if len(q) == 0:
        return three_per_cell(rng, n)
    return (q[rng.integers(0, len(q), n)].astype(np.float64) + rng.normal(size=(n, 3)) * 0.5).astype(np.float32)


def size_pairs(pkg):
    """(n_P, n_Q): every size of size_list on either side, never the same on both."""
    sizes = size_list(pkg)
    return [(n, sizes[(k + 4) % len(sizes)]) for k, n in enumerate(sizes)]


def lattice(side=8, step=0.5):
    """side^3 points at multiples of `step` (a power of two), x fastest."""
    g = np.arange(side, dtype=np.float32) * f32(step)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    return np.stack([x, y, z], axis=-1).reshape(-1, 3)


def planted_case(moved=0):
    """Q: the 8 x 8 x 8 lattice of spacing 1/2; P: every third point of Q shifted by 1/4 along x, so that its nearest point of Q is
    the one it was made from at exactly 1/4 (the next one along x is also at 1/4: the smaller index wins, and that is the one it
    came from) -- and the first `moved` of them taken 40 cells away.  (P, Q, the planted indices)."""
    q = lattice()
    chosen = np.arange(0, len(q), 3)
    p = q[chosen] + f32([0.25, 0, 0])
    p[:moved] += f32([0, 40, 0])
    return p, q, chosen


def tie_case(shuffle_seed=None):
    """A query at the centre of the 8 lattice points of a unit cube whose corners stand in 8 different cells, among other points
    farther away; with a seed, Q in a shuffled order.  (P, Q, the expected index)."""
    corners = np.float32([[x, y, z] for z in (0.5, 1.5) for y in (0.5, 1.5) for x in (0.5, 1.5)])   # every corner in its own cell at radius 1
    q = np.concatenate([np.float32([[3.5, 3.5, 3.5], [-2, 1, 1]]), corners, np.float32([[1, 1, 2.25]])])
    order = np.arange(len(q)) if shuffle_seed is None else np.random.default_rng(shuffle_seed).permutation(len(q))
    q = q[order]
    is_corner = np.isin(order, np.arange(2, 10))
    return np.float32([[1, 1, 1]]), q, int(np.flatnonzero(is_corner)[0])


def crowded_case(rng, n=3000):
    """n targets in the one cell (0, 0, 0) of the grid of cell size 1; queries in it, in each of its 26 neighbours and one in a cell
    with an empty neighbourhood."""
    q = (rng.random((n, 3)) * 0.98 + 0.01).astype(np.float32)
    offsets = np.float32([[x, y, z] for z in (-1, 0, 1) for y in (-1, 0, 1) for x in (-1, 0, 1)])
    p = np.concatenate([(offsets[:, None, :] + rng.random((27, 20, 3)) * 0.98 + 0.01).reshape(-1, 3), [[30.5, 30.5, 30.5]]]).astype(np.float32)
    return p, q


def pair_cases(pkg):
    out = {}
    for n_p, n_q in size_pairs(pkg):
        q = three_per_cell(np.random.default_rng(300 + n_q), n_q)
        out["n=%d in %d" % (n_p, n_q)] = (queries_near(np.random.default_rng(400 + n_p), q, n_p), q, 1.0, None)
    border = border_case()[0]
    out["borders, halves"] = (border[0::2], border[1::2], 1.0, None)
    out["borders, other halves"] = (border[1::2], border[0::2], 1.0, None)
    out["borders, itself reversed"] = (border, border[::-1].copy(), 1.0, None)
    edge = grid_edge_case()[0]
    out["grid edges, halves"] = (edge[0::2], edge[1::2], 1.0, None)
    out["grid edges, itself"] = (edge, edge, 1.0, None)
    outside, _ = outside_case(np.random.default_rng(4))
    out["outside in both"] = (outside, queries_near(np.random.default_rng(5), outside, 500), 1.0, None)
    out["queries all outside"] = (np.full((70, 3), np.nan, np.float32), outside, 1.0, None)
    out["targets all outside"] = (outside, np.full((70, 3), 3.0 * EDGE, np.float32), 1.0, None)
    out["planted"] = planted_case()[:2] + (1.0, None)
    out["planted, some moved"] = planted_case(moved=19)[:2] + (1.0, None)
    out["tie"] = tie_case()[:2] + (1.0, None)
    out["tie, shuffled"] = tie_case(shuffle_seed=6)[:2] + (1.0, None)
    out["crowded"] = crowded_case(np.random.default_rng(7)) + (1.0, None)
    q = three_per_cell(np.random.default_rng(8), 3000)
    out["origin and radius"] = (queries_near(np.random.default_rng(9), q, 2500) * f32(0.3), q * f32(0.3), 0.3, [0.25, -0.5, 0.125])
    return out


@pytest.fixture(scope="module")
def results(pkg, checker):
    """name -> (P, Q, radius, origin, (distance, index) of the grid mode, the grid mode's score), computed once."""
    return {name: (p, q, radius, origin, PX.nearest(checker, p, q, radius, origin), PX.score(checker, p, q, radius, origin))
            for name, (p, q, radius, origin) in pair_cases(pkg).items()}


# --------------------------------------------------------------------------------------------------------------------
# the checker: its two modes, and numpy
# --------------------------------------------------------------------------------------------------------------------

def test_brute_force_and_grid_agree_on_every_device_case(checker, results):
    """The double loop over all pairs and the 27 lookups: the same bits of every distance, the same indices, the same nine fields
    of the score, in both directions."""
    for name, (p, q, radius, origin, (distance, index), score) in results.items():
        assert len(p) * len(q) <= 4e8, name
        d, i = PX.nearest(checker, p, q, radius, origin, PX.BRUTE)
        assert np.array_equal(bits32(d), bits32(distance)) and np.array_equal(i, index), name
        assert PX.score_bits(PX.score(checker, p, q, radius, origin, PX.BRUTE)) == PX.score_bits(score), name
        none = index < 0
        assert (index[none] == -1).all() and np.isposinf(distance[none]).all() and np.isfinite(distance[~none]).all(), name
        assert (distance[~none] <= f32(radius)).all() and (index[~none] < len(q)).all(), name
        assert score.p_within == int((~none).sum()) and score.n_p == len(p) and score.n_q == len(q), name


def numpy_nearest(p, q, radius, origin=None):
    """All pairs in numpy binary32, the operations of the contract in their order: the cells by floor((x - origin) / radius), the
    squared distance (dx * dx + dy * dy) + dz * dz, argmin (the first of equal minima: the smallest index), sqrt."""
    p, q = np.asarray(p, f32).reshape(-1, 3), np.asarray(q, f32).reshape(-1, 3)
    org = np.zeros(3, f32) if origin is None else np.asarray(origin, f32)
    distance, index = np.full(len(p), np.inf, f32), np.full(len(p), -1, np.int32)
    if len(p) == 0 or len(q) == 0:
        return distance, index
    with np.errstate(invalid="ignore", over="ignore"):
        cell = lambda x: np.floor((x - org) / f32(radius))
        cp, cq = cell(p), cell(q)
        inside = lambda c: ((c >= -float(EDGE)) & (c < float(EDGE))).all(axis=1)
        r2 = f32(radius) * f32(radius)
        for first in range(0, len(p), 512):
            a, ca = p[first:first + 512], cp[first:first + 512]
            d = a[:, None, :] - q[None, :, :]
            sq = d * d
            d2 = (sq[..., 0] + sq[..., 1]) + sq[..., 2]
            assert d2.dtype == f32
            ok = inside(ca)[:, None] & inside(cq)[None, :] & (np.abs(ca[:, None, :] - cq[None, :, :]) <= 1).all(axis=2) & (d2 <= r2)
            d2 = np.where(ok, d2, f32(np.inf))
            j = d2.argmin(axis=1)
            best = d2[np.arange(len(a)), j]
            have = np.isfinite(best)
            distance[first:first + 512] = np.where(have, np.sqrt(best), f32(np.inf))
            index[first:first + 512] = np.where(have, j, -1)
    return distance, index


def test_numpy_all_pairs_agrees_in_bits(results):
    """numpy's binary32 subtraction, multiplication, addition, division, floor and square root are the IEEE operations of the
    contract, taken in its order, so the distances agree in every bit and no tolerance is needed; argmin returns the first of
    equal minima, which is the smallest index.  The score's integers are those of the numpy search in both directions."""
    for name, (p, q, radius, origin, (distance, index), score) in results.items():
        if len(p) * len(q) > 3e7:
            continue   # held by the brute-force mode above
        d, i = numpy_nearest(p, q, radius, origin)
        assert np.array_equal(i, index), name
        assert np.array_equal(bits32(d), bits32(distance)), name
        back, _ = numpy_nearest(q, p, radius, origin)
        a, b = int(np.isfinite(d).sum()), int(np.isfinite(back).sum())
        assert (score.p_within, score.q_within) == (a, b), name
        assert score.precision == (a / len(p) if len(p) else 0.0) and score.recall == (b / len(q) if len(q) else 0.0), name
        # the means: numpy adds pairwise, the contract in chunks, both in binary64 over binary32 values
        assert score.mean_p == pytest.approx(float(d[np.isfinite(d)].astype(np.float64).mean()) if a else 0.0, rel=1e-12), name
        assert score.mean_q == pytest.approx(float(back[np.isfinite(back)].astype(np.float64).mean()) if b else 0.0, rel=1e-12), name


# --------------------------------------------------------------------------------------------------------------------
# planted answers
# --------------------------------------------------------------------------------------------------------------------

def test_planted_lattice_gives_exact_distances_and_indices(checker):
    """Every coordinate is a multiple of 1/4: differences, squares and the root are exact."""
    p, q, chosen = planted_case()
    for mode in (PX.BRUTE, PX.GRID):
        distance, index = PX.nearest(checker, p, q, 1.0, mode=mode)
        assert (distance == f32(0.25)).all() and np.array_equal(index, chosen)
        back, back_index = PX.nearest(checker, q, p, 1.0, mode=mode)
        assert np.array_equal(back[chosen], np.full(len(chosen), 0.25, f32)) and np.array_equal(back_index[chosen], np.arange(len(chosen)))


def test_planted_share_gives_exact_rationals(checker):
    """171 queries, 19 of them 40 cells away.  At threshold 1/4 (a lattice point 1/4 away counts: <=) every query left has its
    lattice point and the one after it along x, and a lattice point has a query within 1/4 when it or the one before it along x
    was chosen: counted here from the planted indices, not by a search."""
    p, q, chosen = planted_case(moved=19)
    near = chosen[19:]
    covered = set(near.tolist()) | {int(j) + 1 for j in near if (j + 1) % 8 != 0}
    a, n_p, b, n_q = len(p) - 19, len(p), len(covered), len(q)
    assert (a, n_p, n_q) == (152, 171, 512)
    for mode in (PX.BRUTE, PX.GRID):
        s = PX.score(checker, p, q, 0.25, mode=mode)
        assert (s.n_p, s.n_q, s.p_within, s.q_within) == (n_p, n_q, a, b)
        assert s.precision == a / n_p and s.recall == b / n_q
        assert s.fscore == 2.0 * (a / n_p) * (b / n_q) / (a / n_p + b / n_q)
        assert s.mean_p == 0.25 and s.mean_q == 0.25
    # below the spacing of the shift nothing is within reach
    assert PX.score(checker, p, q, 0.125)[2:] == (0, 0, 0.0, 0.0, 0.0, 0.0, 0.0)
    # no points on either side, or on both
    assert PX.score(checker, p[:0], q, 0.25) == (0, 512, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0)
    assert PX.score(checker, p, q[:0], 0.25) == (171, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0)
    assert PX.score(checker, p[:0], q[:0], 0.25) == (0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0)


def test_ties_go_to_the_smallest_input_index(checker):
    """Eight targets at the same distance in eight different cells: the cell order would give the one in the lowest cell, the
    contract gives the smallest input index -- before and after a shuffle of the targets that changes which cell that is in."""
    seen = set()
    for seed in (None, 6, 7, 8):
        p, q, want = tie_case(seed)
        for mode in (PX.BRUTE, PX.GRID):
            distance, index = PX.nearest(checker, p, q, 1.0, mode=mode)
            assert index.tolist() == [want] and distance[0] == np.sqrt(f32(0.75))
        seen.add(tuple(q[want]))
    assert len(seen) > 1   # the winner is not always the corner of the lowest cell
    # a cloud against itself: distance 0 and, among coincident points, the first
    xyz = border_case()[0]
    distance, index = PX.nearest(checker, xyz, xyz, 1.0)
    assert (distance == 0).all() and index[-3:].tolist() == [len(xyz) - 3] * 3 and np.array_equal(index[:-3], np.arange(len(xyz) - 3))


def test_exactly_the_radius_counts_and_the_next_binary32_does_not(checker):
    p = f32([[0.25, 0, 0], [0, 10, 0], [-3.75, 20, 0], [-0.5, 30, 0], [0.9, 40.5, 0.5], [0.9, 50.5, 0.5]])
    q = f32([[1.25, 0, 0], [UP, 10, 0], [-2.75, 20, 0], [-0.5 - UP, 30, 0], [1.1, 40.5, 0.5], [2.1, 50.5, 0.5]])
    for mode in (PX.BRUTE, PX.GRID):
        distance, index = PX.nearest(checker, p, q, 1.0, mode=mode)
        assert index.tolist() == [0, -1, 2, -1, 4, -1]
        assert distance[[0, 2]].tolist() == [1.0, 1.0] and np.isposinf(distance[[1, 3, 5]]).all()


def test_the_last_cells_of_the_grid_and_points_outside_it(checker, results):
    """The outermost cells have their neighbours and nothing beyond: cells 2^20 - 1 of one row and -2^20 of the next have
    consecutive keys and are no neighbours.  A point outside the grid finds nothing and is found by nobody."""
    edge = grid_edge_case()[0]
    distance, index = PX.nearest(checker, edge[:1], edge[1:], 1.0)      # the first point: its neighbour is edge[2], not edge[1]
    assert index.tolist() == [1] and distance[0] == f32(0.25)
    distance, index = PX.nearest(checker, edge[1:2], edge[:1], 1.0)
    assert index.tolist() == [-1]
    p, q, _, _, (distance, index), _ = results["outside in both"]
    _, bad = outside_case(np.random.default_rng(4))
    assert (index[bad] == -1).all() and np.isposinf(distance[bad]).all() and (index >= 0).sum() > 100
    back, back_index = PX.nearest(checker, q, p, 1.0)
    assert not np.isin(back_index, bad).any() and (back_index >= 0).sum() > 100
    for name in ("queries all outside", "targets all outside"):
        assert (results[name][4][1] == -1).all() and results[name][5].fscore == 0.0


# --------------------------------------------------------------------------------------------------------------------
# the C ABI without a device
# --------------------------------------------------------------------------------------------------------------------

def test_header_declares_the_entry_points_as_ctypes_calls_them(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "apd_mi355x.h")).read(), flags=re.S)
    assert re.search(r"int\s+apd_points_nearest\s*\(\s*apd_points_t\s+\w+\s*,\s*apd_points_t\s+\w+\s*,\s*float\s+\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,"
                     r"\s*float\s*\*\s*\w+\s*,\s*int32_t\s*\*\s*\w+\s*\)", text)
    assert re.search(r"int\s+apd_points_score\s*\(\s*apd_points_t\s+\w+\s*,\s*apd_points_t\s+\w+\s*,\s*float\s+\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,"
                     r"\s*apd_points_score_t\s*\*\s*\w+\s*\)", text)
    assert re.search(r"int\s+apd_points_read_ply\s*\(\s*const\s+char\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*apd_points_t\s*\*\s*\w+\s*\)", text)
    assert re.search(r"typedef\s+struct\s*\{\s*long\s+long\s+n_p\s*,\s*n_q\s*,\s*p_within\s*,\s*q_within\s*;\s*double\s+precision\s*,\s*recall\s*,"
                     r"\s*fscore\s*,\s*mean_p\s*,\s*mean_q\s*;\s*\}\s*apd_points_score_t\s*;", text)
    L = pkg.lib()
    fp = C.POINTER(C.c_float)
    assert L.apd_points_nearest.argtypes == [C.c_void_p, C.c_void_p, C.c_float, fp, C.c_void_p, C.c_void_p]
    assert L.apd_points_score.argtypes == [C.c_void_p, C.c_void_p, C.c_float, fp, C.POINTER(pkg.PointsScore)]
    assert L.apd_points_read_ply.argtypes == [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    assert [n for n, _ in pkg.PointsScore._fields_] == list(PX.FIELDS) == list(pkg.Score._fields) and C.sizeof(pkg.PointsScore) == 72


def test_library_exports_the_entry_points(pkg):
    for name in NEW_SYMBOLS:
        assert hasattr(pkg.lib(), name), name


class _ElsewherePoints(C.Structure):
    """The first two fields of the library's points object (csrc/apd_points_host.h): where it lives."""
    _fields_ = [("device", C.c_int), ("on_device", C.c_int)]


def test_refusals_that_need_no_device(pkg):
    """Every bad argument answers with its message and leaves the outputs as they were: no device is touched, so this passes on a
    machine without one."""
    L = pkg.lib()
    pts = from_cloud(pkg, cloud([[0.5, 0, 0], [0.6, 0, 0]]), [4], [5], [[]])
    other = from_cloud(pkg, cloud([[0.5, 0, 0], [0.6, 0, 0], [0.7, 0, 0]]), [4], [5], [[]])
    distance, index = np.full(2, 77, np.float32), np.full(2, 77, np.int32)
    out = pkg.PointsScore(*([-7] * 4 + [-7.0] * 5))

    def untouched():
        return distance.tolist() == [77, 77] and index.tolist() == [77, 77] and out.n_p == -7 and out.fscore == -7.0

    def both(p, q, radius, origin, null_output, message, code=-1):
        org = None if origin is None else (C.c_float * 3)(*origin)
        assert L.apd_points_nearest(p, q, radius, org, None if null_output else C.c_void_p(distance.ctypes.data),
                                    None if null_output else C.c_void_p(index.ctypes.data)) == code
        assert L.apd_fusion_last_error().decode() == "apd_points_nearest: " + message
        assert L.apd_points_score(p, q, radius, org, None if null_output else C.byref(out)) == code
        assert L.apd_fusion_last_error().decode() == "apd_points_score: " + message
        assert untouched()

    both(None, other._p, 1.0, None, False, "null argument")
    both(pts._p, None, 1.0, None, False, "null argument")
    both(pts._p, other._p, 1.0, None, True, "null argument")      # both outputs NULL; no *out
    for (radius, origin), message in BAD_RADIUS:
        both(pts._p, other._p, radius, origin, False, message)
    # one of the two outputs may be NULL: then the radius is what is refused
    assert L.apd_points_nearest(pts._p, other._p, 0.0, None, None, C.c_void_p(index.ctypes.data)) == -1
    assert L.apd_fusion_last_error().decode() == "apd_points_nearest: a radius of 0, not a positive finite number"
    assert L.apd_points_nearest(pts._p, other._p, 0.0, None, C.c_void_p(distance.ctypes.data), None) == -1
    assert L.apd_fusion_last_error().decode() == "apd_points_nearest: a radius of 0, not a positive finite number"
    # the other points on another device than the one the computation runs on: refused before hipSetDevice, which would fail here
    # with its own message on a machine without a device.  The object is host memory; only where it says it lives is changed
    where = _ElsewherePoints.from_address(other._p.value if hasattr(other._p, "value") else other._p)
    assert (where.device, where.on_device) == (0, 0)
    where.device, where.on_device = 5, 1
    try:
        both(pts._p, other._p, 1.0, None, False, "the other points live on device 5, the computation runs on device 0", code=-5)
        with pytest.raises(pkg.ApdError, match="apd_points_nearest: the other points live on device 5"):
            pts.nearest(other, 1.0)
    finally:
        where.device, where.on_device = 0, 0
    with pytest.raises(pkg.ApdError, match="apd_points_nearest: a radius of 0"):
        pts.nearest(other, 0.0)
    with pytest.raises(pkg.ApdError, match="apd_points_score: origin component 0 is inf"):
        pts.score(other, 1.0, origin=[float("inf"), 0, 0])
    with pytest.raises(pkg.ApdError, match="Points.nearest: the other points are closed or not a Points"):
        pts.nearest(None, 1.0)
    other.close()
    with pytest.raises(pkg.ApdError, match="Points.score: the other points are closed or not a Points"):
        pts.score(other, 1.0)
    pts.close()


def test_objects_without_points_give_empty_results_without_a_device(pkg):
    empty = from_cloud(pkg, cloud(np.zeros((0, 3), np.float32)), [4], [5], [[]])
    some = from_cloud(pkg, cloud([[0.5, 0, 0], [0.6, 0, 0]]), [4], [5], [[]])
    distance, index = empty.nearest(some, 1.0)
    assert distance.dtype == np.float32 and distance.shape == (0,) and index.dtype == np.int32 and index.shape == (0,)
    assert empty.nearest(empty, 1.0, origin=[1, 2, 3])[1].shape == (0,)
    assert empty.score(empty, 1.0) == (0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0)
    assert empty.score(some, 1.0) == (0, 2, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0)
    assert some.score(empty, 1.0) == (2, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0)
    assert some.score(empty, 1.0)._fields == PX.FIELDS


def test_no_gpu_means_the_search_fails_loudly(pkg):
    """There is no host implementation: without a device non-empty host objects are refused with a message, and the outputs
    stay as they were."""
    if pkg.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = pkg.lib()
    pts = from_cloud(pkg, cloud([[0.5, 0, 0], [0.6, 0, 0]]), [4], [5], [[]])
    empty = from_cloud(pkg, cloud(np.zeros((0, 3), np.float32)), [4], [5], [[]])
    out = pkg.PointsScore(*([-7] * 4 + [-7.0] * 5))
    assert L.apd_points_score(pts._p, pts._p, 1.0, None, C.byref(out)) != 0
    assert L.apd_fusion_last_error().startswith(b"apd_points_score: hipSetDevice(")
    assert out.n_p == -7 and out.mean_q == -7.0
    with pytest.raises(pkg.ApdError, match=r"apd_points_nearest: hipSetDevice\("):
        pts.nearest(pts, 1.0)
    with pytest.raises(pkg.ApdError, match=r"apd_points_nearest: hipSetDevice\("):
        pts.nearest(empty, 1.0)     # the fill is the device's too
    pts.close()


# --------------------------------------------------------------------------------------------------------------------
# apd_points_read_ply: host code
# --------------------------------------------------------------------------------------------------------------------

def test_read_ply_returns_what_write_ply_wrote(pkg, tmp_path):
    """With and without normals: the same bits of xyz (a NaN, an infinity and -0 among them), normal and colour; one view of
    1 x 1 without sources."""
    c, views = dressed(np.random.default_rng(1), outside_case(np.random.default_rng(2), 700)[0])
    c.xyz[5] = [-0.0, 1e-42, -1e38]
    pts = from_cloud(pkg, c, *views)
    for normals in (False, True):
        path = tmp_path / ("n%d.ply" % normals)
        pts.write_ply(path, normals=normals)
        assert path.read_bytes() == ply_bytes(c, normals)
        back = pkg.Points.read_ply(path)
        assert back.count == c.count and not back.on_device and not back.merged
        assert np.array_equal(bits32(back.xyz), bits32(c.xyz)) and np.array_equal(back.bgr, c.bgr)
        assert np.array_equal(bits32(back.normal), bits32(c.normal) if normals else np.zeros((c.count, 3), np.uint32))
        assert not back.support.any() and not back.view.any() and not back.pixel.any() and not back.sources.any()
        offsets, listed = back.visibility()
        assert np.array_equal(offsets, np.arange(c.count + 1)) and not np.asarray(listed).any()    # each point: its own view, 0
        back.write_ply(tmp_path / "again.ply", normals=normals)
        assert (tmp_path / "again.ply").read_bytes() == path.read_bytes()
    empty = tmp_path / "empty.ply"
    from_cloud(pkg, cloud(np.zeros((0, 3), np.float32)), [4], [5], [[]]).write_ply(empty)
    assert pkg.Points.read_ply(str(empty)).count == 0


def ply_file(path, header, body=b""):
    path.write_bytes(("\n".join(header) + "\n").encode() + body)
    return path


def test_read_ply_skips_what_it_does_not_keep(pkg, tmp_path):
    """A ground-truth style file: comments, properties in another order and of every scalar size, red green blue, CR LF line ends,
    and a face element with a list after the vertices."""
    rng = np.random.default_rng(3)
    n = 41
    rec = np.zeros(n, np.dtype([("scalar_a", "<f8"), ("z", "<f4"), ("red", "u1"), ("flag", "<i2"), ("x", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("blue", "u1"),
                                ("id", "<u4"), ("y", "<f4"), ("nz", "<f4"), ("green", "u1"), ("c", "i1")]))
    for name in rec.dtype.names:
        rec[name] = rng.normal(size=n) * 50 if rec.dtype[name].kind == "f" else rng.integers(0, 100, n)
    header = ["ply", "format binary_little_endian 1.0", "comment made by a scanner", "obj_info whatever 3", "element vertex %d" % n,
              "property double scalar_a", "property float32 z", "property uint8 red", "property short flag", "property float x", "property float nx",
              "property float ny", "property uchar blue", "property uint id", "property float y", "property float nz", "property uchar green",
              "property char c", "element face 2", "property list uchar int vertex_indices", "property float quality", "end_header"]
    faces = b"\x03" + np.int32([0, 1, 2]).tobytes() + np.float32([1]).tobytes() + b"\x03" + np.int32([2, 1, 0]).tobytes() + np.float32([2]).tobytes()
    for ending in ("\n", "\r\n"):
        path = tmp_path / "truth.ply"
        path.write_bytes((ending.join(header) + ending).encode() + rec.tobytes() + faces)
        back = pkg.Points.read_ply(path)
        assert back.count == n
        assert np.array_equal(bits32(back.xyz), bits32(np.stack([rec["x"], rec["y"], rec["z"]], axis=1)))
        assert np.array_equal(bits32(back.normal), bits32(np.stack([rec["nx"], rec["ny"], rec["nz"]], axis=1)))
        assert np.array_equal(back.bgr, np.stack([rec["blue"], rec["green"], rec["red"]], axis=1))
    # coordinates alone: normals and colours are zeros; two of three normal components are not a normal
    xyz = rng.normal(size=(5, 3)).astype(np.float32)
    back = pkg.Points.read_ply(ply_file(tmp_path / "bare.ply", ["ply", "format binary_little_endian 1.0", "element vertex 5", "property float x",
                                                                "property float y", "property float z", "end_header"], xyz.tobytes()))
    assert np.array_equal(back.xyz, xyz) and not back.normal.any() and not back.bgr.any()
    four = np.concatenate([xyz, xyz[:, :2]], axis=1).astype(np.float32)
    back = pkg.Points.read_ply(ply_file(tmp_path / "part.ply", ["ply", "format binary_little_endian 1.0", "element vertex 5", "property float x",
                                                                "property float y", "property float z", "property float nx", "property float ny",
                                                                "end_header"], four.tobytes()))
    assert np.array_equal(back.xyz, xyz) and not back.normal.any()


def test_read_ply_refuses_by_name(pkg, tmp_path):
    """Every refused form, with the file and the reason in the message; *out stays as it was."""
    L = pkg.lib()
    head = ["ply", "format binary_little_endian 1.0", "element vertex 2"]
    xyz = ["property float x", "property float y", "property float z"]
    body = np.arange(6, dtype=np.float32).tobytes()
    cases = [
        ("ascii", ["ply", "format ascii 1.0", "element vertex 2"] + xyz + ["end_header"], b"0 1 2\n3 4 5\n", -1, "format ascii, not binary_little_endian 1.0"),
        ("big", ["ply", "format binary_big_endian 1.0", "element vertex 2"] + xyz + ["end_header"], body, -1,
         "format binary_big_endian, not binary_little_endian 1.0"),
        ("list", head + xyz + ["property list uchar int seen_by", "end_header"], body, -1, "a list property in element vertex"),
        ("no_z", head + xyz[:2] + ["end_header"], body, -1, "no float coordinate z in element vertex"),
        ("double_x", head + ["property double x"] + xyz[1:] + ["end_header"], body, -1, "coordinate x is double, not float"),
        ("short", head + xyz + ["end_header"], body[:-1], -6, "the file ends before its 2 vertices of 12 bytes do"),
        ("no_end", head + xyz, b"", -6, "the file ends inside the header"),
        ("not_ply", ["plx"] + head[1:] + xyz + ["end_header"], body, -1, "not a PLY file"),
        ("no_vertex", ["ply", "format binary_little_endian 1.0", "end_header"], b"", -1, "no element vertex"),
        ("face_first", ["ply", "format binary_little_endian 1.0", "element face 0", "property list uchar int vertex_indices", "element vertex 2"] + xyz +
         ["end_header"], body, -1, "element face before element vertex"),
        ("bad_type", head + xyz + ["property quad w", "end_header"], body, -1, "a malformed property line: property quad w"),
        ("bad_count", ["ply", "format binary_little_endian 1.0", "element vertex -2"] + xyz + ["end_header"], body, -1,
         "element vertex -2, not one count of vertices"),
    ]
    for name, header, data, code, reason in cases:
        path = ply_file(tmp_path / (name + ".ply"), header, data)
        out = C.c_void_p(1234)
        assert L.apd_points_read_ply(str(path).encode(), 0, 0, C.byref(out)) == code, name
        assert L.apd_fusion_last_error().decode() == "apd_points_read_ply: %s: %s" % (path, reason), name
        assert out.value == 1234
    missing = tmp_path / "none.ply"
    with pytest.raises(pkg.ApdError, match=re.escape("apd error -6: apd_points_read_ply: %s: cannot read the file" % missing)):
        pkg.Points.read_ply(missing)
    out = C.c_void_p(1234)
    assert L.apd_points_read_ply(None, 0, 0, C.byref(out)) == -1 and L.apd_fusion_last_error() == b"apd_points_read_ply: null argument"
    assert L.apd_points_read_ply(b"x.ply", 0, 0, None) == -1 and out.value == 1234


# --------------------------------------------------------------------------------------------------------------------
# the kernels' resources
# --------------------------------------------------------------------------------------------------------------------

def test_the_nearest_kernel_uses_no_scratch_memory(tmp_path):
    """k_nearest_in keeps the best distance and index in registers: the compiler reports 0 bytes of scratch per lane, no spilled
    register and no LDS for it, and no scratch for any kernel of the file.  Registers and occupancy are printed."""
    found = kernel_resources("apd_points_nearest.hip", tmp_path)
    mine = [v for k, v in found.items() if "k_nearest_in" in k]
    assert len(mine) == 1, sorted(found)
    print("k_nearest_in VGPRs", mine[0]["VGPRs"], "SGPRs", mine[0]["TotalSGPRs"], "occupancy", mine[0]["Occupancy [waves/SIMD]"])
    assert mine[0]["ScratchSize [bytes/lane]"] == "0" and mine[0]["VGPRs Spill"] == "0" and mine[0]["SGPRs Spill"] == "0", mine[0]
    assert mine[0]["LDS Size [bytes/block]"] == "0", mine[0]
    for name, v in found.items():
        assert v["ScratchSize [bytes/lane]"] == "0", name


@pytest.mark.parametrize("kernel", ["k_neighbour_count", "k_knn_mean", "k_point_normals", "k_cluster_link"])
def test_the_walks_that_became_a_call_of_the_walk_around_a_cell_keep_their_resources(tmp_path, kernel):
    """for_each_candidate is now for_each_candidate_around with the cell of keys[i]: the kernels built on it keep what
    walk_kernel_resources asserts of them -- no scratch, no spill, no static LDS, 8 waves per SIMD."""
    walk_kernel_resources(kernel, tmp_path)


def test_the_smoothing_walk_keeps_its_resources(tmp_path):
    """k_point_smooth, the fifth walk, had 7 waves per SIMD before and is held to what its own test holds it to."""
    found = kernel_resources("apd_points_smooth.hip", tmp_path)
    mine = [v for k, v in found.items() if "k_point_smooth" in k]
    assert len(mine) == 1 and mine[0]["ScratchSize [bytes/lane]"] == "0" and mine[0]["VGPRs Spill"] == "0" and mine[0]["LDS Size [bytes/block]"] == "0"
    print("k_point_smooth VGPRs", mine[0]["VGPRs"], "occupancy", mine[0]["Occupancy [waves/SIMD]"])
