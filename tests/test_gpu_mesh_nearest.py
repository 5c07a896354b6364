"""apd_mesh_nearest, apd_mesh_sample_points and apd_mesh_score on the device (csrc/apd_mesh_nearest.hip, contract C27), bitwise against the
sequential checker (tests/helpers/mesh_nearest_ref.cpp, brute force over all faces): distance, face, closest point, the sampled arrays
and every field of the score, each call run twice for the same bytes, with the mesh and the points read back unchanged; host- and
device-resident points; and the chain through pipeline.mesh and the drop-in binary.  The checker's own tests: test_mesh_nearest.py."""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest

import fusion_cases
import mesh_nearest_checker as NC
from test_gpu_dropin_binary import APD_BIN, _write_dense_folder
from test_gpu_fusion_options import _read_dmb, _scene
from test_gpu_mesh_render import last_timing, sort_tile
from test_mesh_nearest import REGIONS, TRIANGLE, _host_points

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return NC.build(tmp_path_factory.mktemp("mesh_nearest_checker"))


def points_of(pkg, xyz, on_device):
    xyz = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    n = len(xyz)
    return pkg.Points.from_arrays(xyz, np.zeros((n, 3), F), np.zeros((n, 3), np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros(n, np.int32),
                                  np.zeros(n, np.uint32), [1], [1], [[]], on_device=on_device)


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def bits(a):
    return np.ascontiguousarray(host(a)).view(np.uint32)


def check_nearest(pkg, ref, vertices, faces, queries, radius, origin=None, places=("host", "device"), what=""):
    """The device call against the checker, twice per place of the points; returns the checker's (distance, face, closest)."""
    vertices, faces = np.ascontiguousarray(vertices, F).reshape(-1, 3), np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    queries = np.ascontiguousarray(queries, F).reshape(-1, 3)
    d, f, x, _ = NC.nearest(ref, vertices, faces, queries, radius, origin)
    m = pkg.Mesh.from_arrays(vertices, faces)
    for place in places:
        p = points_of(pkg, queries, place == "device")
        for again in (0, 1):
            gd, gf, gx = m.nearest(p, radius, origin)
            assert host(gd).dtype == F and host(gf).dtype == np.int32 and host(gx).shape == (len(queries), 3)
            assert np.array_equal(host(gf), f), (what, place, again, np.flatnonzero(host(gf) != f)[:5], host(gf)[host(gf) != f][:5], f[host(gf) != f][:5])
            assert np.array_equal(bits(gd), bits(d)), (what, place, again, np.flatnonzero(bits(gd) != bits(d))[:5])
            assert np.array_equal(bits(gx), bits(x)), (what, place, again, np.argwhere(bits(gx) != bits(x))[:5])
        assert np.array_equal(bits(p.xyz), bits(queries)), (what, place, "the points")
        p.close()
    m.refresh()
    assert np.array_equal(bits(m.vertices), bits(vertices)) and np.array_equal(m.faces, faces), (what, "the mesh")
    m.close()
    return d, f, x


def queries_over(rng, lo, hi, n, height=0.6):
    q = rng.uniform(lo, hi, (n, 3))
    q[:, 2] = rng.uniform(-height, height, n)
    return q.astype(F)


def small_faces(n):
    """n separate faces of a quarter cell each at radius 1, one to a cell along x: n pairs."""
    v = np.zeros((3 * n, 3), F)
    v[:, 0] = np.repeat(np.arange(n), 3) + np.tile([0.25, 0.5, 0.25], n)
    v[:, 1] = np.tile([0.25, 0.25, 0.5], n)
    v[:, 2] = 0.25
    return v, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def test_every_cpu_case_on_the_device(gpu_pkg, ref):
    queries = [r[1] for r in REGIONS]
    d, f, x = check_nearest(gpu_pkg, ref, *TRIANGLE, queries, 4.0, what="regions")
    assert [float(v) for v in d] == [float(F(np.sqrt(r[3]))) for r in REGIONS] and x.tolist() == [list(map(float, r[2])) for r in REGIONS]
    for roll in (1, 2):
        check_nearest(gpu_pkg, ref, TRIANGLE[0], np.roll(TRIANGLE[1], roll, 1), queries, 4.0, what="regions rolled")
    # the soup of test_mesh_nearest.py
    rng = np.random.default_rng(27)
    vertices = rng.uniform(-2.0, 2.0, (600, 3)).astype(F)
    vertices[1::3] = vertices[0::3] + rng.uniform(-0.6, 0.6, (200, 3)).astype(F)
    vertices[2::3] = vertices[0::3] + rng.uniform(-0.6, 0.6, (200, 3)).astype(F)   # negative coordinates: cells straddle 0
    faces = np.arange(600, dtype=np.int32).reshape(200, 3)
    d, f, x = check_nearest(gpu_pkg, ref, vertices, faces, rng.uniform(-2.2, 2.2, (500, 3)).astype(F), 0.4, what="soup")
    assert (f >= 0).sum() > 200 and (f < 0).sum() > 10
    # ties: a shared edge, a vertex shared by six faces, two identical faces
    v, f2 = NC.sheet(1, 1)
    assert check_nearest(gpu_pkg, ref, v, f2, [[0.5, 0.5, 0.25]], 1.0, what="edge")[1][0] == 0
    ring = [[np.cos(k * np.pi / 3), np.sin(k * np.pi / 3), 0.0] for k in range(6)]
    fan = np.array([np.roll([0, 1 + k, 1 + (k + 1) % 6], k % 3) for k in range(6)], np.int32)
    for order in (np.arange(6), np.array([3, 1, 5, 0, 2, 4])):
        got = check_nearest(gpu_pkg, ref, np.array([[0, 0, 0]] + ring, F), fan[order], [[0, 0, 0.5], [0, 0, -0.5]], 1.0, what="fan")
        assert got[1].tolist() == [0, 0]
    v, f2 = NC.sheet(2, 1)
    f2 = np.concatenate([f2[:1], f2[2:3], f2[1:2], f2[2:3], f2[3:]])
    assert check_nearest(gpu_pkg, ref, v, f2, [[1.75, 0.25, 0.125]], 1.0, what="identical")[1][0] == 1


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_query_counts_at_the_wave_and_block_edges(gpu_pkg, ref, n):
    v, f = NC.strip(40)
    rng = np.random.default_rng(n)
    q = queries_over(rng, -1.0, 22.0, n)
    q[:, 1] = rng.uniform(-0.5, 1.5, n)
    d, face, x = check_nearest(gpu_pkg, ref, v, f, q, 0.75, what="queries %d" % n)
    assert n < 63 or ((face >= 0).any() and (face < 0).any())


def test_face_counts_at_the_wave_block_and_sort_tile_edges(gpu_pkg, ref):
    rng = np.random.default_rng(5)
    for n in (1, 2, 63, 64, 65):
        v, f = NC.strip(n)
        q = queries_over(rng, -1.0, n / 2 + 2.0, 200)
        q[:, 1] = rng.uniform(-0.5, 1.5, 200)
        check_nearest(gpu_pkg, ref, v, f, q, 0.75, places=("device",), what="faces %d" % n)
    n = sort_tile(gpu_pkg) + 1
    v, f = small_faces(n)
    assert NC.pairs(ref, v, f, 1.0) == n
    q = queries_over(rng, -1.0, n + 1.0, 300)
    q[:, 1] = rng.uniform(-0.5, 1.0, 300)
    d, face, x = check_nearest(gpu_pkg, ref, v, f, q, 1.0, places=("device",), what="pairs = sort tile + 1")
    assert (face >= 0).sum() > 100 and face.max() > n - 200


def test_a_face_over_81_cells_is_found_from_each_and_the_pairs_are_counted(gpu_pkg, ref):
    big = np.array([[0.25, 0.25, 0.5], [8.75, 0.25, 0.5], [0.25, 8.75, 0.5]], F)   # its box: cells 0 .. 8 x 0 .. 8 x 0
    v, f = small_faces(50)
    v = v + F([20, 0, 0])
    vertices, faces = np.concatenate([big, v]), np.concatenate([[[0, 1, 2]], f + 3]).astype(np.int32)
    want = 81 + 50
    assert NC.pairs(ref, vertices, faces, 1.0) == want
    # one query in every cell of the box, at the cell's centre: each reaches the face or is farther than the radius from it by the checker too
    cells = np.array([[i + 0.5, j + 0.5, 0.5] for j in range(9) for i in range(9)], F)
    d, face, x = check_nearest(gpu_pkg, ref, vertices, faces, np.concatenate([cells, v[::3] + F([0, 0, 0.5])]), 1.0, what="large face")
    inside = np.array([i + j <= 8 for j in range(9) for i in range(9)])
    assert (face[:81][inside] == 0).all() and (d[:81][inside] == 0).all() and (face[81:] == np.arange(1, 51)).all()
    # the device counts the same pairs: a limit of exactly that many refuses, one more passes
    m = gpu_pkg.Mesh.from_arrays(vertices, faces)
    p = points_of(gpu_pkg, cells, False)
    L = gpu_pkg.lib()
    try:
        L.apd_mesh_nearest_pair_limit(want)
        with pytest.raises(gpu_pkg.ApdError, match="apd_mesh_nearest: %d \\(cell, face\\) pairs at a radius of 1" % want):
            m.nearest(p, 1.0)
        L.apd_mesh_nearest_pair_limit(want + 1)
        assert np.array_equal(m.nearest(p, 1.0)[1], face[:81])
    finally:
        L.apd_mesh_nearest_pair_limit(0)
    m.close()
    p.close()


def test_the_pair_limit_hook_refuses_and_is_restored(gpu_pkg, ref):
    v, f = NC.strip(12)
    assert NC.pairs(ref, v, f, 0.5) > 10
    m = gpu_pkg.Mesh.from_arrays(v, f)
    p = points_of(gpu_pkg, [[1.0, 0.5, 0.1]], False)
    L = gpu_pkg.lib()
    try:
        L.apd_mesh_nearest_pair_limit(10)
        with pytest.raises(gpu_pkg.ApdError) as e:
            m.nearest(p, 0.5)
        assert "apd error -5" in str(e.value) and "%d (cell, face) pairs" % NC.pairs(ref, v, f, 0.5) in str(e.value) and "larger radius" in str(e.value)
    finally:
        L.apd_mesh_nearest_pair_limit(0)
    want = NC.nearest(ref, v, f, [[1.0, 0.5, 0.1]], 0.5)
    got = m.nearest(p, 0.5)
    assert np.array_equal(got[1], want[1]) and np.array_equal(bits(got[0]), bits(want[0]))
    m.close()
    p.close()


def test_a_squared_distance_of_exactly_the_squared_radius_is_kept(gpu_pkg, ref):
    v, f = NC.sheet(1, 1)
    q = [[0.25, 0.5, 1.0], [0.25, 0.5, -1.0]]
    d, face, x = check_nearest(gpu_pkg, ref, v, f, q, 1.0, what="d2 == r2")
    assert d.tolist() == [1.0, 1.0] and (face >= 0).all()
    d, face, x = check_nearest(gpu_pkg, ref, v, f, q, float(np.nextafter(F(1), F(0))), what="d2 > r2")
    assert np.isinf(d).all() and (face == -1).all() and np.isnan(x).all()


def test_what_is_never_a_candidate_alone_and_mixed_with_good_faces(gpu_pkg, ref):
    v, f = NC.sheet(2, 2)
    bad = np.array([[np.nan, 0, 0], [3, 3, 0], [3, 4, 0], [0, 0, 1], [1, 1, 2], [2, 2, 3], [3e7, 0, 0], [3e7, 1, 0], [3e7, 0, 1]], F)
    vertices = np.concatenate([v, bad])
    n = len(v)
    extra = np.array([[n, n + 1, n + 2], [0, 0, 1], [n + 3, n + 4, n + 5], [n + 6, n + 7, n + 8]], np.int32)   # NaN, repeated, collinear, off the grid
    queries = np.array([[0.5, 0.5, 0.1], [3, 3.5, 0.1], [1, 1, 2], [3e7, 0.2, 0.2], [np.nan, 0, 0], [0.5, 3e7, 0], [np.inf, 0, 0], [1.5, 1.2, -0.3]], F)
    for k in range(4):
        d, face, x = check_nearest(gpu_pkg, ref, vertices, extra[k:k + 1], queries, 1.0, what="bad face %d" % k)
        assert (face == -1).all() and np.isinf(d).all() and np.isnan(x).all()
    d, face, x = check_nearest(gpu_pkg, ref, vertices, np.concatenate([extra[:2], f, extra[2:]]), queries, 1.0, what="mixed")
    assert (face >= 0).tolist() == [True, False, False, False, False, False, False, True] and (face[face >= 0] >= 2).all()


@pytest.mark.parametrize("origin,radius,triangle,query", NC.ROUNDING_CASES)
def test_cells_two_apart_within_the_radius_are_still_reached(gpu_pkg, ref, origin, radius, triangle, query):
    """A face and a query less than a radius apart whose binary32 cells differ by two (test_mesh_nearest.py): the brute force finds
    the face, and so does the walk of the 27 cells, because the face is binned one cell wider on that side."""
    d, face, x = check_nearest(gpu_pkg, ref, triangle, [[0, 1, 2]], [query], radius, origin=origin, what="cells two apart")
    assert face[0] == 0 and np.isfinite(d[0])


def test_a_lattice_mesh_with_queries_exactly_one_radius_away(gpu_pkg, ref):
    """Vertices on a regular lattice, origins off it, queries on the lattice at exactly one radius from the surface and from its border:
    the coincidences of cell boundaries that random queries never meet."""
    for origin, radius, step in (((0.3, -0.7, 0.1), 0.4, 0.2), ((3 * 2.0 ** -25, 0.0, -(2.0 ** -24)), 1.0, 0.5), ((1e3 + 0.3, -2e3, 0.7), 0.4, 0.2),
                                 (None, 0.25, 0.125)):
        v, f = NC.sheet(16, 16, step=step, origin=(-8 * step, -8 * step))
        r = float(F(radius))
        grid = np.arange(-10, 11) * step
        xs, ys = np.meshgrid(grid, grid)
        over = np.stack([xs.ravel(), ys.ravel(), np.full(xs.size, r)], 1)
        beside = np.stack([np.full(len(grid), 8 * step + r), grid, np.zeros(len(grid))], 1)
        queries = np.concatenate([over, over * [1, 1, -1], beside, beside * [-1, 1, 1], beside[:, [1, 0, 2]], beside[:, [1, 0, 2]] * [1, -1, 1]]).astype(F)
        d, face, x = check_nearest(gpu_pkg, ref, v, f, queries, radius, origin=origin, places=("device",), what="lattice %r" % (origin,))
        assert (face >= 0).sum() > 500 and (face < 0).sum() > 50, ((face >= 0).sum(), (face < 0).sum())


def test_an_origin_and_cells_on_both_sides_of_zero(gpu_pkg, ref):
    v, f = NC.sheet(6, 6, step=0.5, z=-0.25, origin=(-1.5, -1.5))
    rng = np.random.default_rng(11)
    q = queries_over(rng, -2.0, 2.0, 400, height=0.7)
    for origin in (None, (0.3, -0.2, 0.1), (-100.0, 50.0, 7.0)):
        d, face, x = check_nearest(gpu_pkg, ref, v, f, q, 0.4, origin=origin, what="origin %r" % (origin,))
        assert (face >= 0).sum() > 50 and (face < 0).sum() > 50


def test_every_choice_of_outputs_an_empty_mesh_and_no_points(gpu_pkg, ref):
    v, f = NC.strip(9)
    rng = np.random.default_rng(2)
    q = queries_over(rng, -1.0, 6.0, 70)
    want = NC.nearest(ref, v, f, q, 0.75)
    m = gpu_pkg.Mesh.from_arrays(v, f)
    p = points_of(gpu_pkg, q, False)
    L = gpu_pkg.lib()
    for mask in range(1, 8):
        out = [np.full(70, 7, F), np.full(70, 7, np.int32), np.full((70, 3), 7, F)]
        args = [C.c_void_p(a.ctypes.data) if mask >> k & 1 else None for k, a in enumerate(out)]
        assert L.apd_mesh_nearest(m._m, p._p, 0.75, None, *args) == 0, L.apd_fusion_last_error()
        for k in range(3):
            assert np.array_equal(bits(out[k]), bits(want[k])) if mask >> k & 1 else (out[k] == 7).all(), (mask, k)
    assert L.apd_mesh_nearest(m._m, p._p, 0.75, None, None, None, None) == -1 and b"apd_mesh_nearest: null argument" in L.apd_fusion_last_error()
    empty = gpu_pkg.Mesh.from_arrays(np.zeros((0, 3), F), np.zeros((0, 3), np.int32))
    bare = gpu_pkg.Mesh.from_arrays(v, np.zeros((0, 3), np.int32))
    for mesh in (empty, bare):
        for place in (False, True):
            pts = points_of(gpu_pkg, q, place)
            d, face, x = mesh.nearest(pts, 0.75)
            assert np.isinf(host(d)).all() and (host(face) == -1).all() and np.isnan(host(x)).all()
            pts.close()
        assert len(mesh.sample_points(10.0)) == 0
    for place in (False, True):
        none = points_of(gpu_pkg, np.zeros((0, 3), F), place)
        d, face, x = m.nearest(none, 0.75)
        assert host(d).shape == (0,) and host(face).shape == (0,) and host(x).shape == (0, 3)
        none.close()
    for mesh in (m, empty, bare):
        mesh.close()
    p.close()


def test_last_timing_reports_the_pair_build_the_sorts_and_the_search(gpu_pkg):
    v, f = NC.sheet(8, 8)
    m = gpu_pkg.Mesh.from_arrays(v, f)
    p = points_of(gpu_pkg, queries_over(np.random.default_rng(1), 0.0, 8.0, 500), True)
    m.nearest(p, 0.5)
    build, sorts, search = last_timing(gpu_pkg)
    assert build > 0.0 and sorts > 0.0 and search > 0.0
    m.close()
    p.close()


def check_samples(pkg, ref, vertices, faces, colours, density, seed, count=None):
    xyz, normal, bgr, face = NC.sample_points(ref, vertices, faces, density, seed, colours)
    assert count is None or len(xyz) == count, len(xyz)
    m = pkg.Mesh.from_arrays(vertices, faces, colours)
    for on_device in (True, False):
        for again in (0, 1):
            s = m.sample_points(density, seed, on_device=on_device)
            what = (density, seed, on_device, again)
            assert s.on_device == on_device and s.count == len(xyz) and len(s) == len(xyz), what
            assert np.array_equal(bits(s.xyz), bits(xyz)) and np.array_equal(bits(s.normal), bits(normal)), what
            assert np.array_equal(host(s.bgr), bgr) and np.array_equal(s.face, face) and s.face.dtype == np.int32, what
            for name in ("support", "view", "pixel", "sources"):
                assert not host(getattr(s, name)).any(), (what, name)
            s.close()
    m.refresh()
    assert np.array_equal(bits(m.vertices), bits(np.ascontiguousarray(vertices, F))) and np.array_equal(m.faces, faces)
    m.close()
    return xyz


def test_sample_points_in_both_places_with_and_without_colours(gpu_pkg, ref):
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F)
    f = np.array([[0, 1, 2]], np.int32)
    colours = np.array([[0, 10, 200], [255, 10, 100], [0, 10, 0]], np.uint8)
    for density, count in ((1e-9, 0), (2.0, 1), (514.0, 257)):   # floor(0.5 * density + u), u in [0, 1)
        for c in (None, colours):
            check_samples(gpu_pkg, ref, v, f, c, density, 3, count)
    v, f = NC.sheet(10, 10)
    rng = np.random.default_rng(4)
    v[:, 2] = rng.uniform(-0.3, 0.3, len(v)).astype(F)
    colours = rng.integers(0, 256, (len(v), 3)).astype(np.uint8)
    f = np.concatenate([f, [[0, 0, 5], [3, 4, 5]]]).astype(np.int32)   # a repeated index and a collinear face: no samples
    f[7] = f[-1]
    f[-1] = [0, 1, 12]
    for c in (None, colours):
        xyz = check_samples(gpu_pkg, ref, v, f, c, 50.0, 0)
        assert 4500 < len(xyz) < 5800
    bad = np.concatenate([v, [[np.nan, 0, 0]]]).astype(F)
    check_samples(gpu_pkg, ref, bad, np.concatenate([f[:20], [[0, 1, len(v)]]]).astype(np.int32), None, 20.0, 1)
    m = gpu_pkg.Mesh.from_arrays(v, f)
    drawn = m.sample_points(5.0, seed=2)
    d, face, x = m.nearest(drawn, 0.25)
    assert np.isfinite(host(d)).all() and host(d).max() < 1e-6     # the samples lie on the surface; every downstream call works on them
    m.close()
    drawn.close()


def test_score_against_the_surfaces_own_samples_moved_along_the_normal(gpu_pkg, ref):
    v, f = NC.sheet(4, 4)
    tau = 0.25
    m = gpu_pkg.Mesh.from_arrays(v, f)
    base = NC.sample_points(ref, v, f, 400.0, 9)[0]   # dense enough that every sample of the surface has one within the threshold
    for shift, expect in ((0.5 * tau, 1.0), (2.0 * tau, 0.0)):
        truth = base + F([0, 0, shift])
        for place in (False, True):
            t = points_of(gpu_pkg, truth, place)
            for kw in ({}, {"seed": 5}, {"density": 30.0, "seed": 1}, {"origin": (0.1, 0.2, 0.3)}):
                want = NC.score(ref, v, f, truth, tau, kw.get("density"), kw.get("seed", 0), kw.get("origin"))
                for again in (0, 1):
                    got = m.score(t, tau, **kw)
                    assert tuple(got) == tuple(want), (shift, place, kw, got, want)
                assert want.precision == expect and want.recall == expect and want.n_q == len(truth) and want.n_p > 400, want
            assert np.array_equal(bits(t.xyz), bits(truth))
            t.close()
    none = points_of(gpu_pkg, np.zeros((0, 3), F), False)
    got = m.score(none, tau)
    assert got.n_q == 0 and got.n_p == NC.score(ref, v, f, np.zeros((0, 3), F), tau).n_p and got.fscore == 0.0
    none.close()
    m.refresh()
    assert np.array_equal(bits(m.vertices), bits(v)) and np.array_equal(m.faces, f)
    m.close()


def test_through_the_pipeline(gpu_pkg, ref, tmp_path):
    from apd_mvs_amd import pipeline
    case = fusion_cases.case("mixed_sizes")
    scene, results = _scene(gpu_pkg, pipeline, case)
    voxel = 0.05
    options = gpu_pkg.default_fusion_options(factor_strong=0.0, factor_weak=0.0)
    _, points = pipeline.fuse(scene, results, None, options=options, return_points=True)
    pipeline.mesh(scene, results, tmp_path / "plain.ply", voxel, bounds=points, options=options)
    for score in ((points, 0.05), (points, 0.05, 900.0), (points, 0.05, 900.0, 6)):
        nv, nf, mesh, got = pipeline.mesh(scene, results, tmp_path / "scored.ply", voxel, bounds=points, options=options, return_mesh=True, score=score)
        assert (tmp_path / "scored.ply").read_bytes() == (tmp_path / "plain.ply").read_bytes()
        assert tuple(got) == tuple(mesh.score(*score)) and got.n_q == len(points) and got.n_p > 0 and 0.0 < got.fscore <= 1.0, got
        if len(score) == 3:   # the brute force over every (sample, point) and (point, face) pair: once
            want = NC.score(ref, mesh.vertices, mesh.faces, host(points.xyz), *score[1:])
            assert tuple(got) == tuple(want), (got, want)
        mesh.close()
    counted = pipeline.mesh(scene, results, None, voxel, bounds=points, options=options, score=(points, 0.05))
    assert len(counted) == 3 and counted[2].n_q == len(points)
    with pytest.raises(ValueError, match="score"):
        pipeline.mesh(scene, results, None, voxel, bounds=points, options=options, score=(points,))
    points.close()


def test_binary_scores_the_mesh(gpu_pkg, synth, tmp_path):
    """--mesh 0.05 --mesh-score TRUTH.ply,TAU[,DENSITY[,SEED]]: the line holds the numbers of pipeline.mesh(score=...) on the run's own
    maps, APD.ply.mesh keeps its bytes; the flag without --mesh and a malformed value end with the usage line."""
    from apd_mvs_amd import pipeline
    folder = tmp_path / "dense"
    folder.mkdir()
    _write_dense_folder(folder, synth, 96, 72, 4)
    base = [APD_BIN, str(folder), "0", "--seed", "21", "--iters", "1", "--keep-maps", "--mesh", "0.05"]
    r = subprocess.run(base, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "All done" in r.stdout and "Mesh score" not in r.stdout, r.stdout[-2000:]
    plain = (folder / "APD" / "APD.ply.mesh").read_bytes()
    truth_file = tmp_path / "truth.ply"
    shutil.copy(folder / "APD" / "APD.ply", truth_file)
    scene = pipeline.load_dense_folder(str(folder), gpu_pkg.Camera)
    results = {}
    for v in range(scene.num_views):
        d = folder / "APD" / ("%08d" % scene.ids[v])
        results[v] = pipeline.ViewState(_read_dmb(d / "depths.dmb"), _read_dmb(d / "normals.dmb"), _read_dmb(d / "weak.bin"), _read_dmb(d / "selected_views.bin"))
    colour = pipeline.load_colour_images(str(folder), scene.ids[:scene.num_views])
    truth = gpu_pkg.Points.read_ply(truth_file)
    for value, score in (("%s,0.05" % truth_file, (truth, 0.05)), ("%s,0.05,700,3" % truth_file, (truth, 0.05, 700.0, 3))):
        r = subprocess.run(base + ["--mesh-score", value], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert r.returncode == 0 and "All done" in r.stdout, r.stdout[-2000:]
        assert (folder / "APD" / "APD.ply.mesh").read_bytes() == plain
        line = [x for x in r.stdout.splitlines() if x.startswith("Mesh score against %s at 0.05:" % truth_file)]
        assert len(line) == 1, r.stdout[-2000:]
        words = line[0].split(": ", 1)[1].split()
        told = dict(zip(words[0::2], words[1::2]))
        want = pipeline.mesh(scene, results, None, 0.05, colour_images=colour, score=score)[2]
        assert list(told) == list(want._fields)
        assert tuple(float(told[n]) for n in want._fields) == tuple(float(x) for x in want), (told, want)
        assert (folder / "APD" / "APD.ply.mesh.score").read_text().split() == words and want.n_p > 0 and want.fscore > 0.0
    for value in ("x", "%s,0" % truth_file, "%s,0.05,-1" % truth_file, "%s,0.05,10,x" % truth_file):
        bad = subprocess.run(base + ["--mesh-score", value], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
        assert bad.returncode != 0 and "bad value '%s' of --mesh-score" % value in bad.stdout and "USAGE" in bad.stdout, bad.stdout[-800:]
    alone = subprocess.run([APD_BIN, str(folder), "0", "--mesh-score", "%s,0.05" % truth_file], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert alone.returncode != 0 and "--mesh-score changes the mesh of --mesh VOXEL[,TRUNC]: not without it" in alone.stdout and "USAGE" in alone.stdout
    truth.close()
