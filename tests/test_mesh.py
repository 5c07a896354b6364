"""Cleaning a mesh (contract C22: weld, face components, removal of small components, vertex normals) without a GPU: the sequential
checker (tests/helpers/mesh_ref.cpp) against an independent numpy restatement and against known answers, the refusals of the C ABI
and of the binary, and the file of a mesh with normals.  The meshes of test_gpu_mesh.py are made here.  The checker's own bits are
only ever compared with the device (test_gpu_mesh.py); here its integers must equal numpy's, and its normals must equal numpy's where
every sum is exact and lie within a written bound where it is not."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mesh_checker as MC

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APD_BIN = os.path.join(ROOT, "apd-mvs_amd", "_build", "APD")
NEW_SYMBOLS = ("apd_mesh_create", "apd_mesh_weld", "apd_mesh_components", "apd_mesh_remove_small_components", "apd_mesh_with_vertex_normals",
               "apd_mesh_has_normals", "apd_mesh_download_normals")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return MC.build(tmp_path_factory.mktemp("mesh_checker"))


# --------------------------------------------------------------------------------------------------------------------
# meshes
# --------------------------------------------------------------------------------------------------------------------

def colours_of(n, seed=3):
    return np.random.default_rng(seed).integers(0, 256, (n, 3), dtype=np.uint8)


def sheet(nx, ny, jitter=0.0, seed=1, spacing=1.0):
    """A triangulated nx x ny grid of vertices in the plane z = 0, `spacing` apart, each moved by up to `jitter` along every axis:
    2 (nx - 1) (ny - 1) faces, counter-clockwise seen from +z."""
    j, i = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    V = np.stack([i.ravel() * spacing, j.ravel() * spacing, np.zeros(nx * ny)], 1)
    if jitter:
        V = V + np.random.default_rng(seed).uniform(-jitter, jitter, V.shape)
    a = (j[:-1, :-1] * nx + i[:-1, :-1]).ravel()
    faces = np.concatenate([np.stack([a, a + 1, a + nx + 1], 1), np.stack([a, a + nx + 1, a + nx], 1)], 1).reshape(-1, 3)
    return MC.Mesh(V.astype(F), faces.astype(np.int32))


def soup(mesh, colour=False):
    """Every face with three vertices of its own: what welding at a small tolerance undoes."""
    V = mesh.vertices[mesh.faces.ravel()]
    return MC.Mesh(V, np.arange(len(V), dtype=np.int32).reshape(-1, 3), colours_of(len(V)) if colour else None)


def cube_soup():
    """A unit cube as 12 faces of 36 unshared vertices."""
    corners = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], F)
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    faces = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    return soup(MC.Mesh(corners, faces))


def octahedron():
    V = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F)
    faces = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    return MC.Mesh(V, faces)


def tetrahedra(shared):
    """Two tetrahedra that share one vertex, or none."""
    T = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F)
    faces = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
    if shared:
        V = np.concatenate([T, -T[1:]])
        second = np.array([0, 4, 5, 6], np.int32)[faces]
    else:
        V = np.concatenate([T, T + 5])
        second = faces + 4
    return MC.Mesh(V, np.concatenate([faces, second]))


def fan(n):
    """n faces around vertex 0, on a cone so that no normal vanishes."""
    t = 2 * np.pi * np.arange(n + 1) / (n + 1)
    V = np.concatenate([[[0, 0, 0.5]], np.stack([np.cos(t), np.sin(t), 0 * t], 1)])
    k = np.arange(1, n + 1)
    return MC.Mesh(V.astype(F), np.stack([0 * k, k, k + 1], 1).astype(np.int32))


def strip(n, shuffled=False, seed=9):
    """n faces (k, k + 1, k + 2) on n + 2 vertices in a zig-zag; shuffled: the same surface with vertices and faces in a fixed random
    order."""
    k = np.arange(n + 2)
    V = np.stack([k * 0.5, k % 2, 0.01 * (k % 7)], 1).astype(F)
    f = np.arange(n)
    faces = np.where((f % 2 == 0)[:, None], np.stack([f, f + 1, f + 2], 1), np.stack([f + 1, f, f + 2], 1))
    if shuffled:
        rng = np.random.default_rng(seed)
        order = rng.permutation(n + 2)   # new vertex k is old vertex order[k]
        where = np.argsort(order)
        V, faces = V[order], where[faces][rng.permutation(n)]
    return MC.Mesh(V, faces.astype(np.int32))


def joined(*meshes, colour=False):
    """The meshes side by side in one, in order."""
    V, faces, base = [], [], 0
    for m in meshes:
        V.append(m.vertices)
        faces.append(m.faces + base)
        base += len(m.vertices)
    V = np.concatenate(V)
    return MC.Mesh(V, np.concatenate(faces), colours_of(len(V)) if colour else None)


def moved(mesh, offset):
    return MC.Mesh(mesh.vertices + F(offset), mesh.faces, mesh.colours)


def islands(count, big):
    """`count` disjoint triangles far from each other and from one sheet of `big` faces or more, interleaved with it in face order."""
    tri = MC.Mesh(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F), np.array([[0, 1, 2]], np.int32))
    side = int(np.ceil(np.sqrt(big / 2))) + 1
    m = joined(sheet(side, side, 0.2), *[moved(tri, [0, 0, 10.0 * (k + 1)]) for k in range(count)])
    order = np.random.default_rng(4).permutation(len(m.faces))
    return MC.Mesh(m.vertices, m.faces[order])


def with_count(n, what):
    """A strip mesh with exactly n vertices (what = 0) or n faces (what = 1), n >= 0; 0 and 1 vertices have no faces."""
    if what == 1:
        return strip(n) if n > 0 else MC.Mesh(np.zeros((3, 3), F), np.zeros((0, 3), np.int32))
    if n < 3:
        return MC.Mesh(np.arange(3 * n).reshape(n, 3).astype(F), np.zeros((0, 3), np.int32))
    return strip(n - 2)


def weldable(n):
    """A mesh of exactly n >= 3 vertices in which welding at a small tolerance merges all along: the unshared triangles of a strip of
    n // 3 faces, then n % 3 more vertices at the positions of vertices 0 and 1, which one more face names with vertex 2 (or 1 and 2):
    it welds to a second copy of face 0, which stays."""
    m = soup(strip(n // 3), colour=True)
    r = n % 3
    if r == 0:
        return m
    V = np.concatenate([m.vertices, m.vertices[:r]])
    extra = [[3 * (n // 3), 1, 2]] if r == 1 else [[3 * (n // 3), 3 * (n // 3) + 1, 2]]
    return MC.Mesh(V, np.concatenate([m.faces, np.array(extra, np.int32)]), colours_of(len(V)))


EDGE_COUNTS = (0, 1, 63, 64, 65, 2047, 2048, 2049)


# --------------------------------------------------------------------------------------------------------------------
# numpy restatement
# --------------------------------------------------------------------------------------------------------------------

def propagate(n, a, b):
    """label[k]: the smallest index connected to k by the edges (a[e], b[e]); by repeated minimum over the edges."""
    label = np.arange(n)
    while True:
        new = label.copy()
        np.minimum.at(new, a, label[b])
        np.minimum.at(new, b, label[a])
        new = np.minimum(new, new[new])
        if np.array_equal(new, label):
            return label
        label = new


def np_compact(mesh, faces, keep):
    used = np.zeros(len(mesh.vertices), bool)
    used[faces[keep].ravel()] = True
    renumber = np.cumsum(used) - 1
    pick = lambda a: None if a is None else a[used]
    return MC.Mesh(mesh.vertices[used], renumber[faces[keep]], pick(mesh.colours), pick(mesh.normals))


def np_weld(mesh, tolerance, origin=(0, 0, 0)):
    V, tol, org = mesh.vertices, F(tolerance), np.array(origin, F)
    with np.errstate(invalid="ignore", over="ignore"):
        cell = np.floor(((V - org).astype(F) / tol).astype(F))
        inside = ((cell >= -2.0 ** 20) & (cell < 2.0 ** 20)).all(1)
        d = (V[:, None, :] - V[None, :, :]).astype(F)
        q = (d * d).astype(F)
        d2 = ((q[..., 0] + q[..., 1]).astype(F) + q[..., 2]).astype(F)
        adjacent = (np.abs(np.where(inside[:, None], cell, 0)[:, None, :] - np.where(inside[:, None], cell, 0)[None, :, :]) <= 1).all(2)
        edge = (d2 <= F(tol * tol)) & adjacent & inside[:, None] & inside[None, :]
    np.fill_diagonal(edge, False)
    a, b = np.nonzero(edge)
    rep = propagate(len(V), a, b)
    faces = rep[mesh.faces]
    keep = (faces[:, 0] != faces[:, 1]) & (faces[:, 0] != faces[:, 2]) & (faces[:, 1] != faces[:, 2])
    return np_compact(mesh, faces, keep)


def np_components(mesh):
    f = mesh.faces
    group = propagate(len(mesh.vertices), np.concatenate([f[:, 0], f[:, 0]]), np.concatenate([f[:, 1], f[:, 2]]))[f[:, 0]] if len(f) else np.zeros(0, int)
    label, size = np.zeros(len(f), np.uint32), np.zeros(len(f), np.uint32)
    for g in np.unique(group):
        members = np.nonzero(group == g)[0]
        label[members], size[members] = members.min(), len(members)
    return label, size, len(np.unique(group))


def np_remove_small(mesh, min_faces):
    return np_compact(mesh, mesh.faces, np_components(mesh)[1] >= min_faces)


def np_face_normals(mesh):
    P = mesh.vertices.astype(np.float64)[mesh.faces]
    u, w = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    return np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)


def np_normals(mesh):
    """(normals float32, sums float64, sum of |g| per vertex and component, corners per vertex); the sums in np.add.at's order, corner
    by corner, which is not the contract's."""
    g = np_face_normals(mesh)
    n = len(mesh.vertices)
    s, a, k = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, int)
    for c in range(3):
        np.add.at(s, mesh.faces[:, c], g)
        np.add.at(a, mesh.faces[:, c], np.abs(g))
        np.add.at(k, mesh.faces[:, c], 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        length = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        ok = np.isfinite(length) & (length > 0)
        normals = np.where(ok[:, None], s / length[:, None], 0.0).astype(F)
    return normals, s, a, k


def weld_cases():
    yield "cube soup", cube_soup(), 1e-4, None
    yield "sheet soup with colour", soup(sheet(9, 7, 0.2), colour=True), 1e-3, None
    yield "sheet soup, origin off the lattice", soup(sheet(6, 5, 0.1)), 1e-3, (0.3, -0.7, 0.11)
    yield "jittered sheet at a tolerance that joins neighbours", sheet(12, 9, 0.3, spacing=0.5), 0.35, None
    bad = soup(sheet(5, 5, 0.1))
    bad.vertices[7, 1] = np.nan
    bad.vertices[20, 0] = np.inf
    yield "a NaN and an infinite coordinate", bad, 1e-3, None
    yield "islands", islands(20, 60), 0.9, None


def component_cases():
    yield "octahedron", octahedron()
    yield "tetrahedra, one shared vertex", tetrahedra(True)
    yield "tetrahedra, none shared", tetrahedra(False)
    yield "islands", islands(30, 100)
    yield "strip, shuffled", strip(300, shuffled=True)
    yield "soup", soup(sheet(5, 4))
    rep = sheet(4, 4)
    rep.faces[3] = [5, 5, 9]
    rep.faces[7] = [2, 2, 2]
    yield "faces that repeat an index", rep


# --------------------------------------------------------------------------------------------------------------------
# the checker against numpy
# --------------------------------------------------------------------------------------------------------------------

def test_checker_welds_like_the_numpy_restatement(checker):
    for name, mesh, tol, origin in weld_cases():
        got, want = MC.weld(checker, mesh, tol, origin), np_weld(mesh, tol, origin or (0, 0, 0))
        MC.assert_mesh_equal(got, want, name)
        assert len(got.vertices) < len(mesh.vertices), name


def test_checker_labels_and_removes_like_the_numpy_restatement(checker):
    for name, mesh in component_cases():
        label, size, count = MC.components(checker, mesh)
        want = np_components(mesh)
        assert np.array_equal(label, want[0]) and np.array_equal(size, want[1]) and count == want[2], name
        for min_faces in (0, 1, 2, 4, 9, 1000):
            MC.assert_mesh_equal(MC.remove_small(checker, mesh, min_faces), np_remove_small(mesh, min_faces), (name, min_faces))


def test_checker_normals_equal_numpy_where_every_sum_is_exact(checker):
    """Small integer coordinates: every cross product and every partial sum is an integer far below 2^53, so no order can change a
    sum, and sqrt and the division are correctly rounded on both sides."""
    rng = np.random.default_rng(11)
    for name, mesh in (("octahedron", octahedron()), ("tetrahedra", tetrahedra(True)), ("cube", MC.weld(checker, cube_soup(), 0.5)),
                       ("integer sheet", MC.Mesh(sheet(9, 8).vertices + rng.integers(-3, 4, (72, 3)).astype(F), sheet(9, 8).faces))):
        got = MC.with_normals(checker, mesh)
        want = np_normals(mesh)[0]
        assert np.array_equal(MC.bits(got.normals), MC.bits(want)), name
        assert np.any(want != 0), name


def test_checker_normals_on_a_general_mesh_within_the_bound_of_the_valence(checker):
    """A vertex of k corners: either order of summation errs by at most (k - 1) u sum|g| per component to first order (u = 2^-53), so
    the two sums differ by at most d_c = 2 k u sum|g_c|.  A unit vector s / |s| moves by at most 2 |d| / |s| when s moves by d; the
    square root and the division add a few u, taken as 8 u; and two binary64 values e apart round to binary32 values at most e + 2^-24
    apart below magnitude 1."""
    for mesh in (sheet(23, 17, 0.3, spacing=0.5), fan(700), islands(10, 300)):
        got = MC.with_normals(checker, mesh).normals
        want, s, a, k = np_normals(mesh)
        u = 2.0 ** -53
        d = np.linalg.norm(2 * k[:, None] * u * a, axis=1)
        length = np.linalg.norm(s, axis=1)
        assert (length > 1e6 * d).all()   # general position: no sum near zero, so the bound means something
        bound = 2 * d / length + 8 * u + 2.0 ** -24
        assert (np.abs(got.astype(np.float64) - want.astype(np.float64)).max(1) <= bound).all()
        assert np.allclose(np.linalg.norm(got, axis=1), 1, atol=1e-6)


# --------------------------------------------------------------------------------------------------------------------
# known answers
# --------------------------------------------------------------------------------------------------------------------

def test_cube_of_unshared_vertices_welds_to_eight(checker):
    got = MC.weld(checker, cube_soup(), 1e-4)
    assert got.vertices.shape == (8, 3) and got.faces.shape == (12, 3)
    assert {tuple(v) for v in got.vertices} == {(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)}
    assert MC.components(checker, got)[2] == 1 and MC.components(checker, cube_soup())[2] == 12


def test_weld_known_answers(checker):
    tri = lambda V: MC.Mesh(np.array(V, F), np.arange(len(V), dtype=np.int32).reshape(-1, 3))
    # -0.0 and +0.0 are one position: the two faces share the vertex afterwards, and it keeps the bits of the smaller index
    m = tri([[-0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0.0, -0.0, 0], [-1, 0, 0], [0, -1, 0]])
    got = MC.weld(checker, m, 1e-3)
    assert len(got.vertices) == 5 and got.faces.tolist() == [[0, 1, 2], [0, 3, 4]] and MC.bits(got.vertices[0]).tolist() == [0x80000000, 0, 0]
    # a chain at 0.6 tolerances welds to its first vertex: every face that names two of them goes, and their vertices with it
    tol = 0.25
    chain = np.stack([0.6 * tol * np.arange(7), np.zeros(7), np.zeros(7)], 1)
    far = np.array([[0, 5, 0], [0, 9, 0], [3, 5, 0], [3, 9, 0]])
    V = np.concatenate([chain, far]).astype(F)
    m = MC.Mesh(V, np.array([[6, 7, 8], [3, 9, 10], [0, 6, 7], [2, 5, 9]], np.int32))
    got = MC.weld(checker, m, tol)
    assert got.faces.tolist() == [[0, 1, 2], [0, 3, 4]] and np.array_equal(got.vertices, V[[0, 7, 8, 9, 10]])
    # 1.5 tolerances apart: nothing welds
    m = tri([[0, 0, 0], [1.5 * tol, 0, 0], [0, 1.5 * tol, 0]])
    MC.assert_mesh_equal(MC.weld(checker, m, tol), m)
    # a face that collapses to two equal indices goes, and the vertex only it named with it; colours stay with their vertices
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1e-5, 0, 0], [5, 5, 5]], F)
    m = MC.Mesh(V, np.array([[0, 1, 2], [0, 3, 4]], np.int32), colours_of(5))
    got = MC.weld(checker, m, 1e-3)
    assert got.faces.tolist() == [[0, 1, 2]] and np.array_equal(got.vertices, V[:3]) and np.array_equal(got.colours, m.colours[:3])
    # a vertex no face names goes, welded or not
    m = MC.Mesh(np.array([[0, 0, 0], [9, 9, 9], [1, 0, 0], [0, 1, 0]], F), np.array([[0, 2, 3]], np.int32))
    got = MC.weld(checker, m, 1e-3)
    assert got.faces.tolist() == [[0, 1, 2]] and len(got.vertices) == 3


def test_octahedron_normals_point_along_the_axes_exactly(checker):
    m = octahedron()
    got = MC.with_normals(checker, m)
    assert np.array_equal(MC.bits(got.normals), MC.bits(m.vertices))
    flipped = MC.with_normals(checker, MC.Mesh(m.vertices, m.faces[:, ::-1]))
    assert np.array_equal(flipped.normals, -m.vertices)


def test_normals_of_vertices_nobody_names_of_repeated_indices_and_of_a_nan(checker):
    V = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [7, 7, 7], [0, 0, 3]], F)
    m = MC.Mesh(V, np.array([[0, 1, 2], [1, 1, 2], [0, 4, 4]], np.int32))
    got = MC.with_normals(checker, m).normals
    assert np.array_equal(MC.bits(got), MC.bits(np.array([[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 0], [0, 0, 0]], F)))
    V[1, 2] = np.nan
    got = MC.with_normals(checker, MC.Mesh(V, np.array([[0, 1, 2], [0, 2, 4]], np.int32))).normals
    assert np.array_equal(MC.bits(got[[1, 3]]), np.zeros((2, 3), np.uint32)) and not got[[0, 2]].any() and not np.isnan(got).any()


def test_tetrahedra_components_and_min_faces(checker):
    label, size, count = MC.components(checker, tetrahedra(True))
    assert count == 1 and (label == 0).all() and (size == 8).all()
    label, size, count = MC.components(checker, tetrahedra(False))
    assert count == 2 and label.tolist() == [0] * 4 + [4] * 4 and (size == 4).all()
    m = islands(5, 40)
    for keep_all in (0, 1):
        MC.assert_mesh_equal(MC.remove_small(checker, m, keep_all), m, keep_all)
    got = MC.remove_small(checker, m, 2)
    assert len(got.faces) == len(m.faces) - 5 and len(got.vertices) == len(m.vertices) - 15 and MC.components(checker, got)[2] == 1
    assert len(MC.remove_small(checker, m, 10 ** 6).vertices) == 0
    spare = MC.Mesh(np.concatenate([m.vertices, [[1, 2, 3]]]).astype(F), m.faces)   # an unreferenced vertex goes whatever min_faces is
    MC.assert_mesh_equal(MC.remove_small(checker, spare, 0), m)


def test_checker_on_the_meshes_of_every_edge_count(checker):
    """The meshes test_gpu_mesh.py takes to the wave and tile edges have the counts they are named for, and the checker gives on them
    what their construction says: a strip is one component, and the unshared triangles of a strip of k faces weld back to its k + 2
    vertices, the duplicate face the extra vertices make included."""
    for n in EDGE_COUNTS:
        by_vertices, by_faces = with_count(n, 0), with_count(n, 1)
        assert len(by_vertices.vertices) == n and len(by_faces.faces) == n
        for mesh in (by_vertices, by_faces):
            label, size, count = MC.components(checker, mesh)
            assert count == min(len(mesh.faces), 1) and (label == 0).all() and (size == len(mesh.faces)).all(), n
        if n >= 3:
            mesh = weldable(n)
            got = MC.weld(checker, mesh, 1e-3)
            assert len(mesh.vertices) == n and len(got.vertices) == n // 3 + 2 and len(got.faces) == n // 3 + (1 if n % 3 else 0), n
            if n < 100:
                MC.assert_mesh_equal(got, np_weld(mesh, 1e-3), n)
    a, b = strip(50), strip(50, shuffled=True)
    assert not np.array_equal(a.faces, b.faces) and np.array_equal(np.sort(a.vertices, 0), np.sort(b.vertices, 0))
    assert np.array_equal(MC.components(checker, b)[1], MC.components(checker, a)[1])


# --------------------------------------------------------------------------------------------------------------------
# the file
# --------------------------------------------------------------------------------------------------------------------

def test_ply_bytes_of_a_mesh_with_normals_read_back(checker):
    m = MC.with_normals(checker, MC.Mesh(octahedron().vertices, octahedron().faces, colours_of(6)))
    data = MC.ply_bytes(m)
    head, body = data.split(b"end_header\n")
    props = re.findall(rb"property (\w+) (\w+)\n", head)
    assert [p[1] for p in props] == [b"x", b"y", b"z", b"nx", b"ny", b"nz", b"red", b"green", b"blue"]
    rec = np.frombuffer(body[:6 * 27], np.dtype([("xyz", "<f4", 3), ("n", "<f4", 3), ("rgb", "u1", 3)]))
    assert np.array_equal(rec["xyz"], m.vertices) and np.array_equal(rec["n"], m.normals) and np.array_equal(rec["rgb"], m.colours[:, ::-1])
    faces = np.frombuffer(body[6 * 27:], np.dtype([("n", "u1"), ("v", "<i4", 3)]))
    assert (faces["n"] == 3).all() and np.array_equal(faces["v"], m.faces)
    plain = MC.ply_bytes(MC.Mesh(m.vertices, m.faces, m.colours))
    assert b"nx" not in plain and len(plain) == len(data) - 6 * 12 - len(b"property float nx\n") * 3


def test_points_read_the_file_of_a_mesh_with_normals(pkg, checker, tmp_path):
    m = MC.with_normals(checker, MC.Mesh(octahedron().vertices, octahedron().faces, colours_of(6)))
    for mesh in (m, MC.Mesh(m.vertices, m.faces, None, m.normals), MC.Mesh(m.vertices, m.faces)):
        (tmp_path / "m.ply").write_bytes(MC.ply_bytes(mesh))
        pts = pkg.Points.read_ply(tmp_path / "m.ply")
        assert pts.count == 6 and np.array_equal(MC.bits(np.asarray(pts.xyz)), MC.bits(m.vertices))
        if mesh.normals is not None:
            assert np.array_equal(MC.bits(np.asarray(pts.normal)), MC.bits(m.normals))
        if mesh.colours is not None:
            assert np.array_equal(np.asarray(pts.bgr), m.colours)


# --------------------------------------------------------------------------------------------------------------------
# the C ABI without a device
# --------------------------------------------------------------------------------------------------------------------

def test_header_library_and_documents_name_every_entry_point(pkg):
    header = open(os.path.join(ROOT, "include", "apd_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = pkg.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(L, name) and getattr(L, name).argtypes is not None, name
    assert "contract C22" in header and "C22" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "contract C22" in open(os.path.join(ROOT, "apd-mvs_amd", "csrc", "apd_mesh_math.h")).read()


def empty_mesh(L):
    out = C.c_void_p()
    assert L.apd_mesh_create(0, 0, None, None, 0, None, 0, C.byref(out)) == 0
    return out


def test_create_refusals(pkg):
    L = pkg.lib()
    out = C.c_void_p(1234)
    xyz, idx = np.zeros((3, 3), F), np.array([[0, 1, 2]], np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)

    def refused(message, nv=3, v=p(xyz), nf=1, f=p(idx), outp=C.byref(out), device=0, on_device=0):
        assert L.apd_mesh_create(device, nv, v, None, nf, f, on_device, outp) == -1
        assert L.apd_fusion_last_error().decode() == "apd_mesh_create: " + message
        assert out.value == 1234

    refused("null argument", outp=None)
    refused("-1 vertices and 1 faces", nv=-1)
    refused("3 vertices and -5 faces", nf=-5)
    refused("2147483648 vertices and 1 faces, 2^31 or more", nv=2 ** 31)
    refused("3 vertices and 2147483648 faces, 2^31 or more", nf=2 ** 31)
    refused("a null array with a count that is not 0", v=None)
    refused("a null array with a count that is not 0", f=None)
    refused("a null array with a count that is not 0", v=None, on_device=1)
    refused("device -1", device=-1)
    for bad, at in ((3, 1), (-1, 2), (2 ** 31 - 1, 0)):
        wrong = idx.copy()
        wrong[0, at] = bad
        refused("face 0 names vertex %d, outside 0 .. 3" % bad, f=p(wrong))
    refused("face 0 names vertex 0, outside 0 .. 0", nv=0, v=None)
    with pytest.raises(pkg.ApdError, match="apd_mesh_create: face 1 names vertex 3"):
        pkg.Mesh.from_arrays(xyz, [[0, 1, 2], [0, 1, 3]])
    with pytest.raises(ValueError):
        pkg.Mesh.from_arrays(xyz, idx, colours=np.zeros((2, 3), np.uint8))


def test_refusals_of_the_calls_on_a_mesh_and_an_empty_mesh_through_every_call(pkg):
    """An empty mesh is made without a device, so everything a call refuses is refused on any machine; and every call on it gives an
    empty answer, again without a device."""
    L = pkg.lib()
    m = empty_mesh(L)
    out, n = C.c_void_p(1234), C.c_longlong(-7)
    last = lambda: L.apd_fusion_last_error().decode()
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert L.apd_mesh_weld(m, bad, None, C.byref(out), C.byref(n), C.byref(n)) == -1
        assert last() == "apd_mesh_weld: a tolerance of %g, not a positive finite number" % bad
    assert L.apd_mesh_weld(m, 1e-30, None, C.byref(out), None, None) == -1 and "whose square" in last()
    assert L.apd_mesh_weld(m, 0.1, (C.c_float * 3)(0, float("inf"), 0), C.byref(out), None, None) == -1 and last() == "apd_mesh_weld: origin component 1 is inf"
    assert L.apd_mesh_weld(None, 0.1, None, C.byref(out), None, None) == -1 and last() == "apd_mesh_weld: null argument"
    assert L.apd_mesh_weld(m, 0.1, None, None, None, None) == -1 and last() == "apd_mesh_weld: null argument"
    label = np.full(4, 9, np.uint32)
    lp = C.c_void_p(label.ctypes.data)
    assert L.apd_mesh_components(None, lp, None, C.byref(n)) == -1 and last() == "apd_mesh_components: null argument"
    assert L.apd_mesh_components(m, None, lp, C.byref(n)) == -1 and last() == "apd_mesh_components: null argument"
    assert L.apd_mesh_remove_small_components(None, 2, C.byref(out), None, None) == -1 and last() == "apd_mesh_remove_small_components: null argument"
    assert L.apd_mesh_remove_small_components(m, 2, None, None, None) == -1
    assert L.apd_mesh_with_vertex_normals(None, C.byref(out)) == -1 and last() == "apd_mesh_with_vertex_normals: null argument"
    assert L.apd_mesh_with_vertex_normals(m, None) == -1
    assert L.apd_mesh_download_normals(None, lp) == -1 and last() == "apd_mesh_download_normals: null argument"
    assert L.apd_mesh_download_normals(m, None) == -1
    assert L.apd_mesh_download_normals(m, lp) == -1 and last() == "apd_mesh_download_normals: a mesh without normals"
    assert out.value == 1234 and n.value == -7 and (label == 9).all()
    assert L.apd_mesh_has_normals(None) == 0 and L.apd_mesh_has_normals(m) == 0
    L.apd_mesh_destroy(m)

    mesh = pkg.Mesh.from_arrays(np.zeros((0, 3), F), np.zeros((0, 3), np.int32))
    assert mesh.normals is None and mesh.colours is None
    for got in (mesh.weld(0.5), mesh.weld(0.5, origin=(1, 2, 3)), mesh.remove_small_components(3), mesh.with_vertex_normals()):
        assert got.vertices.shape == (0, 3) and got.faces.shape == (0, 3)
    assert mesh.with_vertex_normals().normals.shape == (0, 3)
    label, size, count = mesh.components()
    assert len(label) == 0 and len(size) == 0 and count == 0
    with pytest.raises(pkg.ApdError, match="apd_mesh_weld: a tolerance of 0"):
        mesh.weld(0)
    mesh.close()
    with pytest.raises(pkg.ApdError, match="the mesh is closed"):
        mesh.weld(1.0)


def test_no_gpu_means_the_calls_fail_loudly(pkg):
    if pkg.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(pkg.ApdError, match="apd_mesh_create: "):
        pkg.Mesh.from_arrays(octahedron().vertices, octahedron().faces)


# --------------------------------------------------------------------------------------------------------------------
# the binary
# --------------------------------------------------------------------------------------------------------------------

def _apd(tmp_path, *flags):
    r = subprocess.run([APD_BIN, str(tmp_path / "no_such_folder"), "0"] + list(flags), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode != 0 and not (tmp_path / "no_such_folder").exists()
    return r.stdout


def test_binary_refuses_the_mesh_options_without_mesh_and_bad_values_before_anything_is_read(tmp_path):
    for flags in (("--mesh-weld", "1e-5"), ("--mesh-min-component", "10"), ("--mesh-normals",), ("--mesh-normals", "--mesh-weld", "0.1")):
        out = _apd(tmp_path, *flags)
        assert "changes the mesh of --mesh VOXEL[,TRUNC]: not without it" in out and "USAGE" in out, (flags, out[-500:])
    for bad in ("", "0", "-1", "x", "nan", "inf", "1e-30", "0.1,0.2", "0.1x"):
        out = _apd(tmp_path, "--mesh", "0.1", "--mesh-weld", bad)
        assert "bad value '%s' of --mesh-weld" % bad in out and "USAGE" in out, (bad, out[-500:])
    for bad in ("", "-1", "x", "1.5", "2147483648", "10,", "+3"):
        out = _apd(tmp_path, "--mesh", "0.1", "--mesh-min-component", bad)
        assert "bad value '%s' of --mesh-min-component" % bad in out and "USAGE" in out, (bad, out[-500:])
    for good in (("--mesh-weld", "1e-5"), ("--mesh-min-component", "0"), ("--mesh-min-component", "2147483647"), ("--mesh-normals",),
                 ("--mesh-normals", "--mesh-min-component", "12", "--mesh-weld", "0.001")):
        for order in (("--mesh", "0.1") + good, good + ("--mesh", "0.1")):
            out = _apd(tmp_path, *order)
            assert "bad value" not in out and "USAGE" not in out, (order, out[-500:])
