"""Contract C27 on the CPU: the sequential checker of apd_mesh_nearest, apd_mesh_sample_points and apd_mesh_score
(tests/mesh_nearest_checker.py) shares csrc/apd_mesh_nearest_math.h with the kernels, so it is itself checked here against answers
that do not: closed forms, a numpy float64 brute force, the tie rule, the counting rule of the samples.  And what the Python classes
and the C entry points refuse without a GPU."""
import ctypes as C

import numpy as np
import pytest

import mesh_nearest_checker as NC

F = np.float32


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return NC.build(tmp_path_factory.mktemp("mesh_nearest_ref"))


TRIANGLE = (np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], F), np.array([[0, 1, 2]], np.int32))
# query, closest point, squared distance: one above each of the seven regions; small integers and halves, so every step is exact
REGIONS = [("a", (-1, -1, 2), (0, 0, 0), 6.0), ("b", (6, -1, 0.5), (4, 0, 0), 5.25), ("c", (-1, 6, 0.5), (0, 4, 0), 5.25),
           ("ab", (2, -1, 1), (2, 0, 0), 2.0), ("ac", (-1, 2, 1), (0, 2, 0), 2.0), ("bc", (3, 3, 1), (2, 2, 0), 3.0),
           ("interior", (1, 1, 3), (1, 1, 0), 9.0)]


@pytest.mark.parametrize("name,query,closest,d2", REGIONS, ids=[r[0] for r in REGIONS])
def test_the_seven_regions_of_one_triangle_in_closed_form(ref, name, query, closest, d2):
    d, f, x, got = NC.nearest(ref, *TRIANGLE, [query], 4.0)
    assert got[0] == d2 and d[0] == F(np.sqrt(d2)) and f[0] == 0 and x[0].tolist() == list(closest)
    # every rotation of the corners gives the same point: the region's name changes, the surface does not
    for roll in (1, 2):
        d, f, x, got = NC.nearest(ref, TRIANGLE[0], np.roll(TRIANGLE[1], roll, 1), [query], 4.0)
        assert got[0] == d2 and x[0].tolist() == list(closest)
    # just out of reach: the radius is part of the definition
    d, f, x, got = NC.nearest(ref, *TRIANGLE, [query], float(np.nextafter(F(np.sqrt(d2)), F(0))) * 0.999)
    assert np.isinf(d[0]) and f[0] == -1 and np.isnan(x[0]).all()


def brute_force(vertices, faces, points):
    """float64 [queries, faces] squared distances by another method than the header's: the foot of the perpendicular where it is
    inside the triangle, the nearest of the three edges otherwise."""
    v = vertices.astype(np.float64)
    a, b, c = v[faces[:, 0]][None], v[faces[:, 1]][None], v[faces[:, 2]][None]
    p = points.astype(np.float64)[:, None, :]

    def segment(s, e):
        t = np.clip(((p - s) * (e - s)).sum(-1) / ((e - s) * (e - s)).sum(-1), 0.0, 1.0)
        off = p - (s + t[..., None] * (e - s))
        return (off * off).sum(-1)

    n = np.cross(b - a, c - a)
    n = n / np.linalg.norm(n, axis=-1, keepdims=True)
    h = ((p - a) * n).sum(-1)
    foot = p - h[..., None] * n
    inside = np.ones(h.shape, bool)
    for s, e in ((a, b), (b, c), (c, a)):
        inside &= (np.cross(e - s, foot - s) * n).sum(-1) >= 0.0
    edges = np.minimum(np.minimum(segment(a, b), segment(b, c)), segment(c, a))
    return np.where(inside, h * h, edges)


def test_a_random_soup_against_a_float64_brute_force(ref):
    rng = np.random.default_rng(27)
    vertices = rng.uniform(-2.0, 2.0, (600, 3)).astype(F)
    vertices[1::3] = vertices[0::3] + rng.uniform(-0.6, 0.6, (200, 3)).astype(F)
    vertices[2::3] = vertices[0::3] + rng.uniform(-0.6, 0.6, (200, 3)).astype(F)
    faces = np.arange(600, dtype=np.int32).reshape(200, 3)
    points = rng.uniform(-2.2, 2.2, (500, 3)).astype(F)
    radius = 0.4
    d, f, x, d2 = NC.nearest(ref, vertices, faces, points, radius)
    want = brute_force(vertices, faces, points)
    best = want.min(1)
    found = best <= radius * radius * (1 - 1e-9)
    assert found.sum() > 200 and (~found).sum() > 10, (found.sum(), len(found))
    assert (f[found] >= 0).all() and (f[best > radius * radius * (1 + 1e-9)] == -1).all()
    k = np.flatnonzero(found)
    assert np.allclose(np.sqrt(d2[k]), np.sqrt(best[k]), rtol=1e-12, atol=1e-15)
    assert np.allclose(d[k], np.sqrt(best[k]), rtol=1e-6)
    # where the two name different faces their squared distances differ by less than that
    other = want.argmin(1)
    for i in k[f[k] != other[k]]:
        assert abs(want[i, f[i]] - want[i, other[i]]) <= 1e-12 * max(want[i, other[i]], 1e-30)
    # the closest point is on the face and at the distance
    assert np.allclose(np.linalg.norm(points[k].astype(np.float64) - x[k], axis=1), np.sqrt(best[k]), rtol=1e-5, atol=1e-6)
    assert np.allclose(np.sqrt(want[k, f[k]]), np.sqrt(best[k]), rtol=1e-12, atol=1e-15)


def test_ties_go_to_the_smallest_face_index(ref):
    # the shared edge of two faces
    v, f = NC.sheet(1, 1)
    d, face, x, _ = NC.nearest(ref, v, f, [[0.5, 0.5, 0.25]], 1.0)
    assert face[0] == 0 and d[0] == F(0.25) and x[0].tolist() == [0.5, 0.5, 0.0]
    d, face, x, _ = NC.nearest(ref, v, f[::-1], [[0.5, 0.5, 0.25]], 1.0)
    assert face[0] == 0
    # a vertex shared by six faces, the centre standing at every corner position in turn
    ring = [[np.cos(k * np.pi / 3), np.sin(k * np.pi / 3), 0.0] for k in range(6)]
    v = np.array([[0, 0, 0]] + ring, F)
    fan = np.array([np.roll([0, 1 + k, 1 + (k + 1) % 6], k % 3) for k in range(6)], np.int32)
    for order in (np.arange(6), np.arange(6)[::-1], np.array([3, 1, 5, 0, 2, 4])):
        d, face, x, d2 = NC.nearest(ref, v, fan[order], [[0.0, 0.0, 0.5], [0.0, 0.0, -0.5]], 1.0)
        assert face.tolist() == [0, 0] and d2.tolist() == [0.25, 0.25] and x.tolist() == [[0, 0, 0], [0, 0, 0]]
    # two identical faces among others
    v, f = NC.sheet(2, 1)
    f = np.concatenate([f[:1], f[2:3], f[1:2], f[2:3], f[3:]])
    d, face, x, _ = NC.nearest(ref, v, f, [[1.75, 0.25, 0.125]], 1.0)
    assert face[0] == 1 and (f[3] == f[1]).all()


def test_faces_and_queries_that_are_never_candidates(ref):
    v, f = NC.sheet(2, 2)
    bad = np.array([[np.nan, 0, 0], [3, 3, 0], [3, 4, 0], [0, 0, 1], [1, 1, 2], [2, 2, 3], [3e7, 0, 0], [3e7, 1, 0], [3e7, 0, 1]], F)
    vertices = np.concatenate([v, bad])
    n = len(v)
    extra = np.array([[n, n + 1, n + 2], [0, 0, 1], [n + 3, n + 4, n + 5], [n + 6, n + 7, n + 8]], np.int32)  # NaN, repeated, collinear, off the grid
    queries = np.array([[0.5, 0.5, 0.1], [3, 3.5, 0.1], [1, 1, 2], [3e7, 0.2, 0.2], [np.nan, 0, 0], [0.5, 3e7, 0], [np.inf, 0, 0]], F)
    d, face, x, _ = NC.nearest(ref, vertices, extra, queries, 1.0)
    assert np.isinf(d).all() and (face == -1).all() and np.isnan(x).all()
    d, face, x, _ = NC.nearest(ref, vertices, np.concatenate([extra, f]), queries, 1.0)
    assert np.isfinite(d).tolist() == [True, False, False, False, False, False, False] and face[0] >= 4
    assert NC.pairs(ref, vertices, extra, 1.0) == 0


@pytest.mark.parametrize("origin,radius,triangle,query", NC.ROUNDING_CASES)
def test_cells_two_apart_within_the_radius_are_still_reached(ref, origin, radius, triangle, query):
    """The binary32 cells of a face and of a query less than a radius away can differ by two; the face is binned one cell wider there."""
    cell = lambda x, o: int(np.floor((F(x) - F(o)) / F(radius)))
    v = np.array(triangle, F)
    gaps = [min(abs(cell(query[a], origin[a]) - cell(x, origin[a])) for x in v[:, a]) for a in range(3)]
    assert max(gaps) == 2, gaps
    d, f, x, d2 = NC.nearest(ref, v, [[0, 1, 2]], [query], radius, origin)
    assert f[0] == 0 and d2[0] <= float(F(radius)) ** 2
    assert NC.reached(ref, v, query, radius, origin)


def test_every_candidate_on_a_lattice_is_reached_from_the_27_cells(ref):
    """Vertices and queries on a regular lattice with origins off it: the distances that are exactly one radius and the corners that
    stand on cell boundaries, which random queries never meet."""
    rng = np.random.default_rng(3)
    met = 0
    for origin, radius, step in (((0.3, -0.7, 0.1), 0.4, 0.1), ((3 * 2.0 ** -25, 0.0, -(2.0 ** -24)), 1.0, 0.5), ((0.0, 0.0, 0.0), 0.25, 0.125),
                                 ((1e3 + 0.3, -2e3, 0.7), 0.4, 0.2), ((-0.1, 0.2, 0.3), 0.3, 0.1)):
        for _ in range(4000):
            base = rng.integers(-400, 400, 3)
            tri = (base + rng.integers(0, 4, (3, 3))) * step
            if np.linalg.matrix_rank(tri[1:] - tri[0]) < 2:
                continue
            axis = rng.integers(0, 3)
            query = (base + rng.integers(0, 4, 3)) * step
            query[axis] = tri[:, axis].max() + radius if rng.integers(0, 2) else tri[:, axis].min() - radius
            d, f, x, d2 = NC.nearest(ref, tri.astype(F), [[0, 1, 2]], [query], radius, origin)
            if f[0] == 0:
                met += 1
                assert NC.reached(ref, tri.astype(F), query, radius, origin), (origin, radius, tri, query)
    assert met > 1000, met


def barycentrics(a, b, c, p):
    m = np.stack([b - a, c - a], 1).astype(np.float64)
    r = np.linalg.lstsq(m, (p - a).astype(np.float64), rcond=None)[0]
    return np.array([1.0 - r.sum(), r[0], r[1]])


@pytest.mark.parametrize("which", ["triangle", "square"])
def test_samples_lie_on_their_faces_in_face_order_and_follow_the_counting_rule(ref, which):
    v, f = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F), np.array([[0, 1, 2]], np.int32)) if which == "triangle" else NC.sheet(1, 1)
    density = 400.0
    xyz, normal, bgr, face = NC.sample_points(ref, v, f, density, seed=7)
    assert (np.diff(face) >= 0).all() and set(face.tolist()) == set(range(len(f)))
    for s in range(len(xyz)):
        a, b, c = v[f[face[s]]]
        w = barycentrics(a, b, c, xyz[s])
        assert (w >= -1e-6).all() and abs(w.sum() - 1) < 1e-9 and xyz[s][2] == 0
    assert (normal == np.array([0, 0, 1], F)).all() and (bgr == 0).all()
    for k in range(len(f)):
        assert (face == k).sum() == int(np.floor(0.5 * density + NC.number(ref, 7, k, 0, 0)))
    again = NC.sample_points(ref, v, f, density, seed=7)
    assert all(np.array_equal(p, q) for p, q in zip((xyz, normal, bgr, face), again))
    other = NC.sample_points(ref, v, f, density, seed=8)
    assert len(other[0]) != len(xyz) or not np.array_equal(other[0], xyz)
    # spread over the face: the mean is the centroid within four standard errors
    for k in range(len(f)):
        mine = xyz[face == k].astype(np.float64)
        centroid = v[f[k]].astype(np.float64).mean(0)
        assert np.abs(mine.mean(0) - centroid)[:2].max() < 4 * 0.24 / np.sqrt(len(mine))


def test_sample_colours_mix_the_corners_and_round_half_up(ref):
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F)
    f = np.array([[0, 1, 2]], np.int32)
    colours = np.array([[0, 10, 200], [255, 10, 100], [0, 10, 0]], np.uint8)
    xyz, _, bgr, _ = NC.sample_points(ref, v, f, 300.0, seed=1, colours=colours)
    x, y = xyz[:, 0].astype(np.float64), xyz[:, 1].astype(np.float64)
    assert (bgr[:, 1] == 10).all()
    assert np.abs(bgr[:, 0] - 255.0 * x).max() <= 0.51 and np.abs(bgr[:, 2] - (200.0 * (1 - x - y) + 100.0 * x)).max() <= 0.51


def test_the_sample_count_of_a_sheet_is_within_five_deviations_of_density_times_area(ref):
    v, f = NC.sheet(10, 10)
    density, seed = 50.0, 0
    total = len(NC.sample_points(ref, v, f, density, seed)[0])
    # every face rounds 25 up or down by one Bernoulli draw: a deviation of at most sqrt(faces) / 2
    assert abs(total - density * 100.0) <= 5 * np.sqrt(len(f)) / 2, total
    # faces far smaller than 1 / density are still sampled
    small = NC.sample_points(ref, v * F(0.01), f, density * 100.0, seed)
    assert 20 <= len(small[0]) <= 80


def test_a_mesh_against_its_own_samples_scores_one(ref):
    v, f = NC.sheet(4, 4)
    truth = NC.sample_points(ref, v, f, 30.0, seed=3)[0]
    s = NC.score(ref, v, f, truth, 0.5, seed=4)
    assert s.n_q == len(truth) and s.n_p == len(NC.sample_points(ref, v, f, 16.0, seed=4)[0])
    assert s.p_within == s.n_p and s.q_within == s.n_q and s.precision == 1.0 and s.recall == 1.0 and s.fscore == 1.0
    assert s.mean_q < 1e-6 and 0 < s.mean_p < 0.5
    far = NC.score(ref, v, f, truth + F([0, 0, 2]), 0.5, seed=4)
    assert far.precision == 0.0 and far.recall == 0.0 and far.fscore == 0.0 and far.mean_p == 0.0 and far.n_p == s.n_p


def _host_points(pkg, xyz):
    xyz = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    n = len(xyz)
    return pkg.Points.from_arrays(xyz, np.zeros((n, 3), F), np.zeros((n, 3), np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros(n, np.int32),
                                  np.zeros(n, np.uint32), [1], [1], [[]])


def test_the_python_classes_and_the_entry_points_refuse_bad_arguments_without_a_gpu(pkg):
    L = pkg.lib()
    points = _host_points(pkg, [[0, 0, 0]])
    closed = pkg.Mesh.__new__(pkg.Mesh)
    closed._m = None
    for call in (lambda: closed.nearest(points, 1.0), lambda: closed.sample_points(1.0), lambda: closed.score(points, 1.0)):
        with pytest.raises(pkg.ApdError, match="the mesh is closed"):
            call()
    stand_in = pkg.Mesh.__new__(pkg.Mesh)   # the arguments are checked before the library sees the handle
    stand_in._m, stand_in.vertices, stand_in.faces = 1, np.zeros((0, 3), F), np.zeros((0, 3), np.int32)
    try:
        for density in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="density"):
                stand_in.sample_points(density)
        for call in (lambda: stand_in.sample_points(1.0, seed=-1), lambda: stand_in.score(points, 1.0, seed=2 ** 64)):
            with pytest.raises(ValueError, match="seed"):
                call()
        for call in (lambda: stand_in.nearest(np.zeros((1, 3), F), 1.0), lambda: stand_in.score(None, 1.0)):
            with pytest.raises(pkg.ApdError, match="not a Points"):
                call()
    finally:
        stand_in._m = None
    out = (C.c_float * 3)()
    score = pkg.PointsScore()
    made = C.c_void_p()
    assert L.apd_mesh_nearest(None, points._p, 1.0, None, out, None, None) == -1 and b"apd_mesh_nearest: null argument" in L.apd_fusion_last_error()
    assert L.apd_mesh_nearest(None, None, 1.0, None, out, None, None) == -1
    assert L.apd_mesh_nearest(None, points._p, 1.0, None, None, None, None) == -1 and b"apd_mesh_nearest: null argument" in L.apd_fusion_last_error()
    assert L.apd_mesh_nearest(None, points._p, -1.0, None, out, None, None) == -1 and b"apd_mesh_nearest: a radius of -1" in L.apd_fusion_last_error()
    assert L.apd_mesh_sample_points(None, 1.0, 0, 0, C.byref(made), None) == -1 and b"apd_mesh_sample_points: null argument" in L.apd_fusion_last_error()
    assert L.apd_mesh_score(None, points._p, 1.0, None, 0.0, 0, C.byref(score)) == -1 and b"apd_mesh_score: null argument" in L.apd_fusion_last_error()
    assert L.apd_mesh_score(None, points._p, 0.0, None, 0.0, 0, C.byref(score)) == -1 and b"apd_mesh_score: a radius of 0" in L.apd_fusion_last_error()
    assert made.value is None and L.apd_mesh_device(None) == -1
    points.close()
