"""The vertex adjacency of a mesh and Laplacian / Taubin smoothing over it (contract C24): the sequential checker
(tests/helpers/mesh_smooth_ref.cpp) against known answers and against what smoothing is for, and what apd_mesh_adjacency and
apd_mesh_smooth refuse, which needs no device.  The device side against this checker: test_gpu_mesh_smooth.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mesh_checker as MC
import mesh_smooth_checker as KC
import volume_checker as VC
from test_mesh import APD_BIN, F, ROOT, fan, islands, joined, moved, octahedron, sheet, soup, strip
from test_mesh_simplify import sphere_rms
from test_volume import sphere_field

MODES = ("fixed", "along", "free")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return KC.build(tmp_path_factory.mktemp("mesh_smooth_checker"))


@pytest.fixture(scope="module")
def sphere(tmp_path_factory):
    """(mesh, centre, radius): the marching-tetrahedra mesh of sphere_field, from the volume's own checker; its vertices are shared."""
    g, tsdf, weight = sphere_field((24, 22, 20), 7.0)
    m = VC.extract(VC.build(tmp_path_factory.mktemp("volume_checker")), g, tsdf, weight)
    centre = (np.array((24, 22, 20)) - 1) * 0.25 + np.array([0.11, -0.07, 0.05])
    return MC.Mesh(m.vertices, m.faces), centre, 7.0 * 0.5


def noisy_sphere(mesh, centre, radius, sigma=0.05, seed=5):
    """The mesh with every vertex moved along its radius by a normal deviate of `sigma`."""
    d = mesh.vertices.astype(np.float64) - centre
    scale = 1.0 + np.random.default_rng(seed).normal(0.0, sigma, len(d))[:, None] / radius
    return MC.Mesh((centre + d * scale).astype(F), mesh.faces)


def border_of(nx, ny):
    j, i = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    return ((i == 0) | (i == nx - 1) | (j == 0) | (j == ny - 1)).ravel()


def quality(smooth, mesh, centre, radius, what):
    """The two inequalities of the issue, for any smooth(mesh, iterations, lam, mu) that answers with vertices."""
    rms_in = sphere_rms(mesh.vertices, centre, radius)
    taubin, laplace = smooth(mesh, 10, 0.5, -0.53), smooth(mesh, 10, 0.5, 0.0)
    mean_radius = lambda v: float(np.linalg.norm(v.astype(np.float64) - centre, axis=1).mean())
    rms_out = sphere_rms(taubin, centre, radius)
    print("%s: rms distance to the sphere %.4g -> %.4g after 10 Taubin iterations; mean radius %.5f (true %.5f), Taubin %.5f, Laplacian %.5f" % (
        what, rms_in, rms_out, mean_radius(mesh.vertices), radius, mean_radius(taubin), mean_radius(laplace)))
    assert rms_out < rms_in, what
    assert abs(mean_radius(taubin) - radius) < abs(mean_radius(laplace) - radius), what


# --------------------------------------------------------------------------------------------------------------------
# adjacency
# --------------------------------------------------------------------------------------------------------------------

def test_an_octahedron_is_closed_and_manifold(checker):
    valence, boundary, edges, open_edges, many = KC.adjacency(checker, octahedron())
    assert (valence == 4).all() and not boundary.any() and (edges, open_edges, many) == (12, 0, 0)


def test_a_sheet_has_the_edges_and_the_border_of_its_grid(checker):
    for nx, ny in ((2, 2), (3, 3), (7, 4), (12, 11)):
        valence, boundary, edges, open_edges, many = KC.adjacency(checker, sheet(nx, ny, 0.2))
        assert edges == (nx - 1) * ny + nx * (ny - 1) + (nx - 1) * (ny - 1), (nx, ny)
        assert open_edges == 2 * (nx - 1) + 2 * (ny - 1) and many == 0, (nx, ny)
        assert np.array_equal(boundary, border_of(nx, ny)), (nx, ny)
        assert valence.sum() == 2 * edges
        if nx > 2 and ny > 2:
            assert (valence[~boundary] == 6).all()


def test_a_third_face_on_an_edge_makes_it_non_manifold_and_a_duplicate_closes_a_border(checker):
    base = sheet(2, 2)   # faces (0, 1, 3) and (0, 3, 2): the edge {0, 3} has two sides
    third = MC.Mesh(np.concatenate([base.vertices, [[0.5, 0.5, 1.0]]]).astype(F), np.concatenate([base.faces, [[0, 3, 4]]]).astype(np.int32))
    valence, boundary, edges, open_edges, many = KC.adjacency(checker, third)
    assert (edges, open_edges, many) == (7, 6, 1) and list(valence) == [4, 2, 2, 4, 2] and boundary.all()
    # a single triangle is all border; the same face twice gives every edge multiplicity 2: that is the rule
    one = MC.Mesh(base.vertices[:3], np.array([[0, 1, 2]], np.int32))
    assert KC.adjacency(checker, one)[2:] == (3, 3, 0) and KC.adjacency(checker, one)[1].all()
    twice = MC.Mesh(one.vertices, np.array([[0, 1, 2], [0, 1, 2]], np.int32))
    assert KC.adjacency(checker, twice)[2:] == (3, 0, 0) and not KC.adjacency(checker, twice)[1].any()
    thrice = MC.Mesh(one.vertices, np.array([[0, 1, 2], [0, 1, 2], [2, 1, 0]], np.int32))
    assert KC.adjacency(checker, thrice)[2:] == (3, 0, 3)


def test_a_repeated_index_adds_no_self_pair_and_an_unreferenced_vertex_has_no_neighbour(checker):
    mesh = MC.Mesh(np.arange(12).reshape(4, 3).astype(F), np.array([[0, 0, 1]], np.int32))
    valence, boundary, edges, open_edges, many = KC.adjacency(checker, mesh)
    assert list(valence) == [1, 1, 0, 0] and (edges, open_edges, many) == (1, 0, 0) and not boundary.any()   # the pair (0, 1) occurs twice
    mesh = MC.Mesh(mesh.vertices, np.array([[2, 2, 2]], np.int32))
    assert KC.adjacency(checker, mesh)[2:] == (0, 0, 0) and not KC.adjacency(checker, mesh)[0].any()
    mesh = MC.Mesh(mesh.vertices, np.zeros((0, 3), np.int32))
    assert KC.adjacency(checker, mesh)[2:] == (0, 0, 0)
    got, n = KC.smooth(checker, mesh, 3)
    assert n == 0 and np.array_equal(MC.bits(got.vertices), MC.bits(mesh.vertices))


# --------------------------------------------------------------------------------------------------------------------
# the step
# --------------------------------------------------------------------------------------------------------------------

# sheet(3, 3): faces (0,1,4) (0,4,3) (1,2,5) (1,5,4) (3,4,7) (3,7,6) (4,5,8) (4,8,7)
NEIGHBOURS_3X3 = {0: (1, 3, 4), 1: (0, 2, 4, 5), 2: (1, 5), 3: (0, 4, 6, 7), 4: (0, 1, 3, 5, 7, 8), 5: (1, 2, 4, 8), 6: (3, 7), 7: (3, 4, 6, 8), 8: (4, 5, 7)}
BORDER_NEIGHBOURS_3X3 = {0: (1, 3), 1: (0, 2), 2: (1, 5), 3: (0, 6), 5: (2, 8), 6: (3, 7), 7: (6, 8), 8: (5, 7)}


def test_one_laplacian_iteration_on_a_three_by_three_sheet_by_hand(checker):
    mesh = sheet(3, 3)
    mesh.vertices[:, 2] = np.arange(9) ** 2   # small integers: every sum below is exact, so the order does not matter here
    for lam in (0.5, 1.0, 0.25):
        for mode in MODES:
            want = mesh.vertices.copy()
            for v in range(9):
                if mode == "fixed" and v != 4:
                    continue
                ws = BORDER_NEIGHBOURS_3X3[v] if mode == "along" and v != 4 else NEIGHBOURS_3X3[v]
                for a in range(3):
                    p = float(mesh.vertices[v, a])
                    m = sum(float(mesh.vertices[w, a]) for w in ws) / len(ws)
                    want[v, a] = F(p + lam * (m - p))
            got, n = KC.smooth(checker, mesh, 1, lam, 0.0, mode)
            assert np.array_equal(MC.bits(got.vertices), MC.bits(want)), (lam, mode)
            assert n == (1 if mode == "fixed" else 9) and np.array_equal(got.faces, mesh.faces)
    # the centre: (0 + 1 + 9 + 25 + 49 + 64) / 6 = 24.666..., half way from 16
    assert KC.smooth(checker, mesh, 1, 0.5, 0.0, "free")[0].vertices[4, 2] == F(16 + 0.5 * (148 / 6 - 16))


def test_taubin_is_a_step_with_lambda_then_a_step_with_mu(checker):
    mesh = sheet(9, 8, 0.3)
    for mode in MODES:
        one, _ = KC.smooth(checker, mesh, 1, 0.5, 0.0, mode)
        two, _ = KC.smooth(checker, one, 1, 0.53, 0.0, mode)   # a step with +0.53 ...
        back = MC.Mesh(one.vertices.astype(np.float64) - (two.vertices.astype(np.float64) - one.vertices), mesh.faces)   # ... mirrored
        got, _ = KC.smooth(checker, mesh, 1, 0.5, -0.53, mode)
        assert np.abs(got.vertices - back.vertices).max() < 1e-5, mode
        twice, _ = KC.smooth(checker, KC.smooth(checker, mesh, 1, 0.5, -0.53, mode)[0], 1, 0.5, -0.53, mode)
        assert np.array_equal(MC.bits(KC.smooth(checker, mesh, 2, 0.5, -0.53, mode)[0].vertices), MC.bits(twice.vertices)), mode


def test_a_flat_sheet_stays_in_its_plane(checker):
    mesh = sheet(11, 9, 0.3)
    mesh.vertices[:, 2] = 0.75
    for mode in MODES:
        for mu in (0.0, -0.53):
            got, _ = KC.smooth(checker, mesh, 7, 0.5, mu, mode)
            assert (got.vertices[:, 2] == F(0.75)).all(), (mode, mu)
            assert not np.array_equal(got.vertices, mesh.vertices)


def test_fixed_holds_the_border_along_keeps_it_on_its_lines_and_free_shrinks(checker):
    n = 16
    mesh = sheet(n, n, 0.3)
    border = border_of(n, n)
    j, i = [a.ravel() for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij")]
    mesh.vertices[(i == 0) | (i == n - 1), 0] = i[(i == 0) | (i == n - 1)]   # the border back on its four lines, jittered along them
    mesh.vertices[(j == 0) | (j == n - 1), 1] = j[(j == 0) | (j == n - 1)]
    mesh.vertices[border, 2] = 0
    corner = ((i == 0) | (i == n - 1)) & ((j == 0) | (j == n - 1))
    fixed, moved_fixed = KC.smooth(checker, mesh, 5, 0.5, -0.53, "fixed")
    assert np.array_equal(MC.bits(fixed.vertices[border]), MC.bits(mesh.vertices[border])) and moved_fixed == (~border).sum()
    assert (fixed.vertices[~border] != mesh.vertices[~border]).any(1).all()
    along, moved_along = KC.smooth(checker, mesh, 5, 0.5, 0.0, "along")
    assert moved_along == n * n
    # a border vertex that is no corner takes its two neighbours on the same line: while they are on the line it stays there, exactly.
    # A corner's two neighbours lie on two lines: the rule moves it towards their middle, off both, and what is off a line pulls its
    # neighbour off in the next step: after 5 steps the 5 vertices next to each end of a line have left it, the others have not
    steps = 5
    far = lambda k: (k >= steps) & (k <= n - 1 - steps)
    for line, axis, value, k in ((i == 0, 0, 0, j), (i == n - 1, 0, n - 1, j), (j == 0, 1, 0, i), (j == n - 1, 1, n - 1, i)):
        assert (along.vertices[line & far(k), axis] == F(value)).all()
        assert (along.vertices[line & ~far(k), axis] != F(value)).all()
    once = KC.smooth(checker, mesh, 1, 0.5, 0.0, "along")[0]
    for line, axis, value in ((i == 0, 0, 0), (i == n - 1, 0, n - 1), (j == 0, 1, 0), (j == n - 1, 1, n - 1)):
        assert (once.vertices[line & ~corner, axis] == F(value)).all()
    inside = lambda v: (v[:, :2] > 0).all(1) & (v[:, :2] < n - 1).all(1)
    assert inside(along.vertices[corner]).all()
    free, _ = KC.smooth(checker, mesh, 5, 0.5, 0.0, "free")
    extent = lambda v: v[:, :2].max(0) - v[:, :2].min(0)
    assert (extent(free.vertices) < extent(mesh.vertices)).all() and (extent(free.vertices) < extent(along.vertices)).all()
    assert inside(free.vertices[border & ~corner]).all()


def test_a_vertex_that_is_not_finite_stays_and_poisons_no_neighbour(checker):
    mesh = sheet(7, 7, 0.2)
    mesh.vertices[17, 1] = np.nan
    mesh.vertices[30] = [np.inf, 0, -np.inf]
    mesh.vertices[3, 0] = 5e6   # finite: it counts, and pulls
    before = mesh.vertices.copy()
    for mode in MODES:
        got, n = KC.smooth(checker, mesh, 3, 0.5, -0.53, mode)
        assert np.array_equal(MC.bits(got.vertices[[17, 30]]), MC.bits(before[[17, 30]])), mode
        rest = np.delete(np.arange(49), [17, 30])
        assert np.isfinite(got.vertices[rest]).all(), mode
        assert n == {"fixed": 25 - 2, "along": 49 - 2, "free": 49 - 2}[mode]
    assert np.array_equal(MC.bits(mesh.vertices), MC.bits(before))
    # every neighbour not finite: the vertex does not move
    lone = MC.Mesh(np.array([[0, 0, 0], [np.nan, 0, 0], [0, np.inf, 0]], F), np.array([[0, 1, 2]], np.int32))
    got, n = KC.smooth(checker, lone, 2, 1.0, 0.0, "free")
    assert n == 0 and np.array_equal(MC.bits(got.vertices), MC.bits(lone.vertices))


def test_lambda_one_puts_a_vertex_on_the_mean_and_colours_stay(checker):
    mesh = joined(fan(12), moved(soup(strip(6)), [5, 0, 0]), colour=True)
    got, _ = KC.smooth(checker, mesh, 1, 1.0, 0.0, "free")
    rim = mesh.vertices[1:14].astype(np.float64)
    assert np.allclose(got.vertices[0], rim.mean(0), atol=1e-6) and np.array_equal(got.colours, mesh.colours) and got.normals is None
    for name, m in (("islands", islands(5, 40)), ("shuffled strip", strip(50, True))):
        a, b = KC.smooth(checker, m, 4)[0], KC.smooth(checker, m, 4)[0]
        assert np.array_equal(MC.bits(a.vertices), MC.bits(b.vertices)), name


# --------------------------------------------------------------------------------------------------------------------
# what it is for
# --------------------------------------------------------------------------------------------------------------------

def test_taubin_brings_a_sphere_nearer_and_keeps_its_radius_where_laplacian_shrinks_it(checker, sphere):
    mesh, centre, radius = sphere
    assert KC.adjacency(checker, mesh)[3:] == (0, 0)   # closed and manifold
    smooth = lambda m, n, lam, mu: KC.smooth(checker, m, n, lam, mu, "along")[0].vertices
    quality(smooth, mesh, centre, radius, "the marching-tetrahedra sphere")
    quality(smooth, noisy_sphere(mesh, centre, radius), centre, radius, "the sphere with radial noise")


# --------------------------------------------------------------------------------------------------------------------
# the C ABI without a device, the documents, the binary
# --------------------------------------------------------------------------------------------------------------------

def test_header_library_and_documents_name_the_calls(pkg):
    header = open(os.path.join(ROOT, "include", "apd_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = pkg.lib()
    for name in ("apd_mesh_adjacency", "apd_mesh_smooth"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(L, name) and getattr(L, name).argtypes is not None, name
    assert "APD_SMOOTH_BOUNDARY_FIXED = 0, APD_SMOOTH_BOUNDARY_ALONG = 1, APD_SMOOTH_BOUNDARY_FREE = 2" in text
    for name in ("DESIGN.md", "INTEGRATION.md", "README.md", os.path.join("apd-mvs_amd", "csrc", "apd_mesh_smooth_math.h")):
        assert "C24" in open(os.path.join(ROOT, name)).read(), name
    assert "contract C24" in header and "Smoothing the mesh" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


class MeshFields(C.Structure):
    """struct apd_mesh of csrc/apd_mesh_host.h: what a call reads of a mesh before it touches a device."""
    _fields_ = [("device", C.c_int), ("vertices", C.c_longlong), ("faces", C.c_longlong), ("colour", C.c_int), ("normals", C.c_int),
                ("xyz", C.c_void_p), ("bgr", C.c_void_p), ("normal", C.c_void_p), ("index", C.c_void_p)]


def test_refusals_and_an_empty_mesh(pkg):
    L = pkg.lib()
    m = C.c_void_p()
    assert L.apd_mesh_create(0, 0, None, None, 0, None, 0, C.byref(m)) == 0
    out, n = C.c_void_p(1234), C.c_longlong(-7)
    last = lambda: L.apd_fusion_last_error().decode()
    for bad in (0, -1, 1001, 2 ** 31 - 1):
        assert L.apd_mesh_smooth(m, bad, 0.5, -0.53, 1, C.byref(out), C.byref(n)) == -1
        assert last() == "apd_mesh_smooth: %d iterations, outside 1 .. 1000" % bad
    for bad in (0.0, -0.5, 1.0000001, 2.0, float("nan"), float("inf")):
        assert L.apd_mesh_smooth(m, 1, bad, -0.53, 1, C.byref(out), C.byref(n)) == -1
        assert last() == "apd_mesh_smooth: a lambda of %g, not in (0, 1]" % F(bad)
    for bad in (0.01, -2.0000002, 1.0, float("nan"), float("inf"), -float("inf")):
        assert L.apd_mesh_smooth(m, 1, 0.5, bad, 1, C.byref(out), C.byref(n)) == -1
        assert last() == "apd_mesh_smooth: a mu of %g, not in [-2, 0]" % F(bad)
    for bad in (-1, 3, 7):
        assert L.apd_mesh_smooth(m, 1, 0.5, -0.53, bad, C.byref(out), C.byref(n)) == -1
        assert last() == "apd_mesh_smooth: boundary mode %d, none of APD_SMOOTH_BOUNDARY_FIXED, _ALONG and _FREE" % bad
    assert L.apd_mesh_smooth(None, 1, 0.5, -0.53, 1, C.byref(out), None) == -1 and last() == "apd_mesh_smooth: null argument"
    assert L.apd_mesh_smooth(m, 1, 0.5, -0.53, 1, None, None) == -1 and last() == "apd_mesh_smooth: null argument"
    assert L.apd_mesh_adjacency(None, None, None, C.byref(n), None, None) == -1 and last() == "apd_mesh_adjacency: null argument"
    assert L.apd_mesh_adjacency(m, None, None, None, None, None) == -1 and last() == "apd_mesh_adjacency: every output is null"
    # 6 * faces at 2^32, on the fields of a mesh alone: refused before its arrays or a device are looked at
    for faces in (715827883, 2 ** 31 - 1):
        assert 6 * faces >= 2 ** 32 > 6 * 715827882
        huge = MeshFields(0, 3, faces, 0, 0, None, None, None, None)
        assert L.apd_mesh_smooth(C.byref(huge), 1, 0.5, -0.53, 1, C.byref(out), C.byref(n)) == -5
        assert last().startswith("apd_mesh_smooth: %d faces, whose 6 directed pairs each are 2^32 or more" % faces)
        assert L.apd_mesh_adjacency(C.byref(huge), None, None, C.byref(n), None, None) == -5
        assert last().startswith("apd_mesh_adjacency: %d faces, whose 6 directed pairs each are 2^32 or more" % faces)
    assert out.value == 1234 and n.value == -7
    # the limits themselves are taken, and an empty mesh gives an empty mesh and touches no device
    for lam, mu, mode, iterations in ((1.0, 0.0, 0, 1), (1e-6, -2.0, 2, 1000), (0.5, -0.0, 1, 3)):
        assert L.apd_mesh_smooth(m, iterations, lam, mu, mode, C.byref(out), C.byref(n)) == 0 and out.value != 1234 and n.value == 0
        assert L.apd_mesh_has_normals(out) == 0
        L.apd_mesh_destroy(out)
        out, n = C.c_void_p(1234), C.c_longlong(-7)
    counts = [C.c_longlong(-7) for _ in range(3)]
    assert L.apd_mesh_adjacency(m, None, None, *[C.byref(c) for c in counts]) == 0 and [c.value for c in counts] == [0, 0, 0]
    L.apd_mesh_destroy(m)
    mesh = pkg.Mesh.from_arrays(np.zeros((0, 3), F), np.zeros((0, 3), np.int32))
    got = mesh.smooth(3)
    assert got.vertices.shape == (0, 3) and got.faces.shape == (0, 3) and got.normals is None and mesh.moved == 0 and got.moved == 0
    valence, boundary, edges, open_edges, many = mesh.adjacency()
    assert valence.shape == (0,) and valence.dtype == np.uint32 and boundary.dtype == bool and (edges, open_edges, many) == (0, 0, 0)
    with pytest.raises(pkg.ApdError, match="apd_mesh_smooth: 0 iterations"):
        mesh.smooth(0)
    with pytest.raises(ValueError, match="boundary"):
        mesh.smooth(1, boundary="open")
    mesh.close()
    with pytest.raises(pkg.ApdError, match="the mesh is closed"):
        mesh.smooth(1)
    with pytest.raises(pkg.ApdError, match="the mesh is closed"):
        mesh.adjacency()


def _apd(tmp_path, *flags):
    r = subprocess.run([APD_BIN, str(tmp_path / "no_such_folder"), "0"] + list(flags), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode != 0 and not (tmp_path / "no_such_folder").exists()
    return r.stdout


def test_binary_refuses_mesh_smooth_without_mesh_and_bad_values_before_anything_is_read(tmp_path):
    for flags in (("--mesh-smooth", "3"), ("--mesh-smooth", "3,0.5,-0.53,fixed", "--mesh-normals")):
        out = _apd(tmp_path, *flags)
        assert "changes the mesh of --mesh VOXEL[,TRUNC]: not without it" in out and "USAGE" in out, (flags, out[-500:])
    for bad in ("", "0", "-1", "x", "1001", "3.5", "3,", "3,0", "3,1.5", "3,nan", "3,0.5,", "3,0.5,0.1", "3,0.5,-2.5", "3,0.5,nan", "3,0.5,-0.53,",
                "3,0.5,-0.53,open", "3,0.5,-0.53,along,free", "3,0.5,-0.53x", ",0.5", "along"):
        out = _apd(tmp_path, "--mesh", "0.1", "--mesh-smooth", bad)
        assert "bad value '%s' of --mesh-smooth" % bad in out and "USAGE" in out, (bad, out[-500:])
    for good in (("--mesh-smooth", "1"), ("--mesh-smooth", "1000,1"), ("--mesh-smooth", "3,0.5,0"), ("--mesh-smooth", "3,0.5,-2,free"),
                 ("--mesh-smooth", "10,0.33,-0.34,fixed", "--mesh-weld", "1e-5", "--mesh-simplify", "0.2", "--mesh-normals")):
        for order in (("--mesh", "0.1") + good, good + ("--mesh", "0.1")):
            out = _apd(tmp_path, *order)
            assert "bad value" not in out and "USAGE" not in out, (order, out[-500:])
    assert "--mesh-smooth ITERATIONS[,LAMBDA[,MU[,fixed|along|free]]]" in _apd(tmp_path, "--mesh-smooth")
