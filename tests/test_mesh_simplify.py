"""Simplification of a mesh by vertex clustering (apd_mesh_simplify, arithmetic contract C23): the sequential checker
(tests/helpers/mesh_simplify_ref.cpp) against a numpy restatement, against answers known exactly (a plane, a crease, a corner), and in
its edge cases; what the library refuses before any device is touched; the binary's flag.  No test here needs a GPU: the device is
held against the checker in test_gpu_mesh_simplify.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mesh_checker as MC
import mesh_simplify_checker as SC
import volume_checker as VC
from test_mesh import APD_BIN, F, ROOT, colours_of, fan, islands, joined, moved, octahedron, sheet, soup, strip
from test_volume import sphere_field

HALF = 1 << 20
PLACEMENTS = ("mean", "quadric")

# The largest difference between a QUADRIC position of the checker (cyclic Jacobi, sums in corner order) and of np_simplify below
# (numpy.linalg.eigh, sums in np.add.at's and np.sum's order) over restatement_cases(), measured with this file: 1.55e-15, on the
# shuffled strip, at a coordinate near zero; every other coordinate of every case came out with the same binary32 bits, the two
# binary64 solves differing far below half a unit in the last place of a binary32 position.  The margin is four times the figure.
QUADRIC_MARGIN = 4 * 1.55e-15


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return SC.build(tmp_path_factory.mktemp("mesh_simplify_checker"))


# --------------------------------------------------------------------------------------------------------------------
# the numpy restatement
# --------------------------------------------------------------------------------------------------------------------

def np_keys(V, cell, origin=(0, 0, 0)):
    """(inside bool [n], key int64 [n]): contract C10's key of every vertex."""
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor((V - np.array(origin, F)) / F(cell))
        inside = ((f >= -HALF) & (f < HALF)).all(1)
    c = np.where(inside[:, None], f, 0).astype(np.int64) + HALF
    return inside, (c[:, 2] << 42) | (c[:, 1] << 21) | c[:, 0]


def np_rotated(t):
    """Every row rotated so that its smallest entry comes first."""
    first = np.argmin(t, axis=1)
    return np.take_along_axis(t, (first[:, None] + np.arange(3)) % 3, axis=1)


def np_simplify(mesh, cell, origin=(0, 0, 0), placement="quadric", details=False):
    V, faces = mesh.vertices, mesh.faces.astype(np.int64)
    org, size = np.array(origin, F), F(cell)
    inside, key = np_keys(V, size, org)
    keys, cluster_of_inside = np.unique(key[inside], return_inverse=True)
    cluster_of = np.full(len(V), -1, np.int64)
    cluster_of[inside] = cluster_of_inside
    K = len(keys)
    whole = inside[faces].all(1) if len(faces) else np.zeros(0, bool)
    mapped = cluster_of[faces]
    alive = whole & (mapped[:, 0] != mapped[:, 1]) & (mapped[:, 0] != mapped[:, 2]) & (mapped[:, 1] != mapped[:, 2])
    keep = np.zeros(len(faces), bool)
    ids = np.flatnonzero(alive)
    if len(ids):
        _, firsts = np.unique(np_rotated(mapped[ids]), axis=0, return_index=True)   # the first occurrence of every triple
        keep[ids[firsts]] = True
    used = np.zeros(K, bool)
    used[mapped[keep].ravel()] = True
    members = [np.flatnonzero(cluster_of == c) for c in range(K)]   # ascending vertex index
    cells = np.stack([(keys >> (21 * a)) & (2 * HALF - 1) for a in range(3)], 1).astype(np.int64) - HALF if K else np.zeros((0, 3), np.int64)
    centre = org.astype(np.float64) + (cells.astype(np.float64) + 0.5) * np.float64(size)
    out = np.zeros((K, 3), F)
    free = np.zeros((K, 3))
    if placement == "mean":
        for c in range(K):
            s = V[members[c][0]].copy()
            for v in members[c][1:]:
                s = s + V[v]
            out[c] = s / F(len(members[c]))
    else:
        P = V.astype(np.float64)
        S, t = np.zeros((K, 3, 3)), np.zeros((K, 3))
        wf = np.flatnonzero(whole)
        if len(wf):
            A, B, Cc = P[faces[wf, 0]], P[faces[wf, 1]], P[faces[wf, 2]]
            g = np.cross(B - A, Cc - A)
            for k in range(3):
                c = mapped[wf, k]
                d = -np.einsum("ij,ij->i", g, A - centre[c])
                np.add.at(S, c, g[:, :, None] * g[:, None, :])
                np.add.at(t, c, g * d[:, None])
        cut = 1e-3
        for c in range(K):
            mu = (P[members[c]] - centre[c]).sum(0) / len(members[c])
            x = mu.copy()
            if np.isfinite(S[c]).all() and np.isfinite(t[c]).all():
                w, E = np.linalg.eigh(S[c])
                if w.max() > 0:
                    r = -t[c] - S[c] @ mu
                    for k in range(3):
                        if w[k] > 0 and w[k] > cut * w.max():
                            x = x + E[:, k] * (E[:, k] @ r) / w[k]
            free[c] = x
            if not (np.isfinite(x).all() and (np.abs(x) <= np.float64(size)).all()):
                x = mu
            out[c] = (centre[c] + x).astype(F)
    colours = None
    if mesh.colours is not None:
        colours = np.zeros((K, 3), np.uint8)
        for c in range(K):
            m = len(members[c])
            colours[c] = (mesh.colours[members[c]].astype(np.uint64).sum(0) + np.uint64(m // 2)) // np.uint64(m)
    renumber = np.cumsum(used) - 1
    result = MC.Mesh(out[used], renumber[mapped[keep]].astype(np.int32), None if colours is None else colours[used])
    if details:
        return result, {"keys": keys[used], "free": free[used], "centre": centre[used], "members": [m for m, u in zip(members, used) if u]}
    return result


@pytest.fixture(scope="module")
def sphere(tmp_path_factory):
    """(mesh, grid, centre, radius): the marching-tetrahedra mesh of sphere_field, from the volume's own checker."""
    g, tsdf, weight = sphere_field((24, 22, 20), 7.0)
    m = VC.extract(VC.build(tmp_path_factory.mktemp("volume_checker")), g, tsdf, weight)
    centre = (np.array((24, 22, 20)) - 1) * 0.25 + np.array([0.11, -0.07, 0.05])
    return MC.Mesh(m.vertices, m.faces), g, centre, 7.0 * 0.5


def restatement_cases(sphere):
    yield "sheet", sheet(30, 28, 0.2), 2.5, None
    yield "sheet with colour at an origin with negative cells", MC.Mesh(sheet(21, 19, 0.3).vertices, sheet(21, 19, 0.3).faces, colours_of(21 * 19)), 3.0, (40.5, 7.25, 1.0)
    yield "shuffled strip", strip(300, True), 1.7, (0.1, 0.2, 0.3)
    yield "islands", islands(12, 200), 2.0, None
    yield "octahedron, every vertex its own cell", octahedron(), 0.5, (0.25, 0.25, 0.25)
    yield "fan", fan(40), 0.4, None
    yield "two sheets", joined(sheet(12, 12, 0.1), moved(sheet(12, 12, 0.1, seed=2), [0, 0, 0.3]), colour=True), 2.0, None
    yield "sphere", sphere[0], 2.0, None
    bad = sheet(10, 10, 0.2)
    bad.vertices[17, 1] = np.nan
    bad.vertices[55, 0] = 3e6
    yield "a nan and a vertex far out", bad, 2.0, None


def structure(mesh, result, cell, origin, removed=None):
    """What holds of every result."""
    f = result.faces
    assert f.size == 0 or (f.min() >= 0 and f.max() < len(result.vertices))
    assert not ((f[:, 0] == f[:, 1]) | (f[:, 0] == f[:, 2]) | (f[:, 1] == f[:, 2])).any()
    assert len(np.unique(np_rotated(f), axis=0)) == len(f)
    assert len(np.unique(f)) == len(result.vertices)
    assert result.normals is None
    assert len(result.faces) <= len(mesh.faces) and len(result.vertices) <= len(mesh.vertices)


def test_checker_simplifies_like_the_numpy_restatement(checker, sphere):
    worst = 0.0
    for name, mesh, cell, origin in restatement_cases(sphere):
        org = (0, 0, 0) if origin is None else origin
        mean, want = SC.simplify(checker, mesh, cell, origin, "mean"), np_simplify(mesh, cell, org, "mean")
        MC.assert_mesh_equal(mean, want, (name, "mean"))
        got, (want, more) = SC.simplify(checker, mesh, cell, origin, "quadric"), np_simplify(mesh, cell, org, "quadric", details=True)
        assert np.array_equal(got.faces, want.faces) and np.array_equal(got.faces, mean.faces), name
        assert (got.colours is None) == (mesh.colours is None) and (got.colours is None or np.array_equal(got.colours, want.colours)), name
        difference = float(np.abs(got.vertices.astype(np.float64) - want.vertices.astype(np.float64)).max()) if len(want.vertices) else 0.0
        print("%-50s %6d -> %5d faces, quadric against numpy: %.3g" % (name, len(mesh.faces), len(got.faces), difference))
        worst = max(worst, difference)
        assert difference <= QUADRIC_MARGIN, (name, difference)
        for result in (mean, got):
            structure(mesh, result, cell, org)
            # ascending key order: a QUADRIC vertex may leave its cell, so the order is that of the clusters' keys
            assert (np.diff(more["keys"].astype(np.int64)) > 0).all() and len(more["keys"]) == len(result.vertices), name
    print("largest difference: %.3g" % worst)


def plane_sheet(at, du, dv, nu, nv):
    """nu x nv vertices at + i du + j dv, triangulated."""
    m = sheet(nu, nv)
    V = np.array(at, np.float64) + m.vertices[:, :1].astype(np.float64) * np.array(du) + m.vertices[:, 1:2].astype(np.float64) * np.array(dv)
    assert np.array_equal(V.astype(F).astype(np.float64), V)
    return MC.Mesh(V.astype(F), m.faces)


STEP = 1.0 / 64


def clusters_of(mesh, result_details, want):
    keys = result_details["keys"]
    cells = np.stack([(keys >> (21 * a)) & (2 * HALF - 1) for a in range(3)], 1).astype(np.int64) - HALF
    pick = np.ones(len(keys), bool)
    for a, w in enumerate(want):
        if w is not None:
            pick &= cells[:, a] == w
    return pick


def test_a_flat_sheet_of_dyadic_coordinates_stays_on_its_plane_exactly(checker):
    mesh = plane_sheet((0, 0, 0.375), (STEP, 0, 0), (0, STEP, 0), 40, 37)
    got = SC.simplify(checker, mesh, 0.25, None, "quadric")
    assert len(got.vertices) >= 6 and len(got.faces) >= 4
    assert np.array_equal(MC.bits(got.vertices[:, 2]), MC.bits(np.full(len(got.vertices), 0.375, F)))
    structure(mesh, got, 0.25, (0, 0, 0))


def crease():
    floor = plane_sheet((0, 0, 0.375), (STEP, 0, 0), (0, STEP, 0), 33, 40)     # x 0 .. 0.5
    wall = plane_sheet((0.5, 0, 0.375), (0, 0, STEP), (0, STEP, 0), 33, 40)    # z 0.375 .. 0.875
    return joined(floor, wall)


def test_a_crease_keeps_its_line_under_quadric_and_not_under_mean(checker):
    """The floor z = 0.375 meets the wall x = 0.5; the cells with ix = 2 (x in [0.5, 0.75)) and iz = 1 (z in [0.25, 0.5)) hold the
    crease.  S is diagonal: no rotation."""
    mesh = crease()
    quadric, mean = SC.simplify(checker, mesh, 0.25, None, "quadric"), SC.simplify(checker, mesh, 0.25, None, "mean")
    _, more = np_simplify(mesh, 0.25, (0, 0, 0), "mean", details=True)
    on = clusters_of(mesh, more, (2, None, 1))
    assert on.sum() >= 2 and np.array_equal(quadric.faces, mean.faces) and len(quadric.vertices) == len(on)
    q, m = quadric.vertices[on], mean.vertices[on]
    assert (q[:, 0] == F(0.5)).all() and (q[:, 2] == F(0.375)).all(), q
    assert not ((m[:, 0] == F(0.5)) & (m[:, 2] == F(0.375))).all(), m
    assert (np.abs(m[:, 2] - 0.375) > 0.01).any()
    # the flat parts stay on their planes too
    floor_only = clusters_of(mesh, more, (1, None, 1)) | clusters_of(mesh, more, (0, None, 1))
    assert floor_only.any() and (quadric.vertices[floor_only][:, 2] == F(0.375)).all()
    wall_only = clusters_of(mesh, more, (2, None, 2))
    assert wall_only.any() and (quadric.vertices[wall_only][:, 0] == F(0.5)).all()


def test_a_box_corner_is_kept_exactly(checker):
    floor = plane_sheet((0, 0, 0.375), (STEP, 0, 0), (0, STEP, 0), 33, 33)       # x, y 0 .. 0.5
    wall_x = plane_sheet((0.5, 0, 0.375), (0, 0, STEP), (0, STEP, 0), 33, 33)    # x = 0.5
    wall_y = plane_sheet((0, 0.5, 0.375), (STEP, 0, 0), (0, 0, STEP), 33, 33)    # y = 0.5
    mesh = joined(floor, wall_x, wall_y)
    quadric, mean = SC.simplify(checker, mesh, 0.25, None, "quadric"), SC.simplify(checker, mesh, 0.25, None, "mean")
    _, more = np_simplify(mesh, 0.25, (0, 0, 0), "mean", details=True)
    corner = clusters_of(mesh, more, (2, 2, 1))
    assert corner.sum() == 1
    assert np.array_equal(MC.bits(quadric.vertices[corner][0]), MC.bits(np.array([0.5, 0.5, 0.375], F)))
    assert not np.array_equal(mean.vertices[corner][0], np.array([0.5, 0.5, 0.375], F))


def test_duplicates_collapse_and_reflected_faces_stay(checker):
    a = moved(sheet(9, 9, 0.05), [0.3, 0.3, 0.5])
    same = joined(a, moved(a, [0, 0, 0.1]))
    one = SC.simplify(checker, a, 2.0, None, "mean")
    got = SC.simplify(checker, same, 2.0, None, "mean")
    assert np.array_equal(got.faces, one.faces) and len(got.vertices) == len(one.vertices)
    flipped = MC.Mesh(a.vertices + F([0, 0, 0.1]), a.faces[:, ::-1].copy())
    both = SC.simplify(checker, joined(a, flipped), 2.0, None, "quadric")
    assert len(both.faces) == 2 * len(one.faces) and len(both.vertices) == len(one.vertices)
    assert np.array_equal(both.faces[:len(one.faces)], one.faces)
    assert np.array_equal(np.sort(np_rotated(both.faces[len(one.faces):][:, ::-1]), axis=0), np.sort(np_rotated(one.faces), axis=0))
    # the survivor of a set of duplicates is the smallest input face: its corner order is the one that is kept
    V = np.array([[0.5, 0.5, 0], [1.5, 0.5, 0], [0.5, 1.5, 0], [0.6, 0.6, 0], [1.6, 0.6, 0], [0.6, 1.6, 0]], F)
    for faces, want in (([[1, 2, 0], [3, 4, 5]], [1, 2, 0]), ([[3, 4, 5], [1, 2, 0]], [0, 1, 2]), ([[5, 3, 4], [0, 1, 2], [2, 0, 1]], [2, 0, 1])):
        got = SC.simplify(checker, MC.Mesh(V, np.array(faces, np.int32)), 1.0, None, "mean")
        assert got.faces.tolist() == [want], (faces, got.faces)   # clusters in key order: x, then y: the input's 0, 1, 2


def test_edge_inputs(checker):
    for placement in PLACEMENTS:
        got = SC.simplify(checker, moved(sheet(5, 5, 0.0, spacing=0.1), [0.05, 0.05, 0.05]), 1.0, None, placement)
        assert got.vertices.shape == (0, 3) and got.faces.shape == (0, 3)     # all in one cell
        base = sheet(8, 8, 0.1)
        ref = SC.simplify(checker, base, 2.0, None, placement)
        bad = MC.Mesh(base.vertices.copy(), base.faces)
        bad.vertices[27, 2] = np.nan
        bad.vertices[3, 0] = -2.0 * HALF * 2.0 - 1.0
        bad.vertices[60, 1] = np.inf
        got = SC.simplify(checker, bad, 2.0, None, placement)
        assert np.isfinite(got.vertices).all() and 0 < len(got.faces) <= len(ref.faces)
        MC.assert_mesh_equal(got, np_simplify(bad, 2.0, (0, 0, 0), placement) if placement == "mean" else MC.Mesh(got.vertices, np_simplify(bad, 2.0).faces))
        lone = MC.Mesh(np.concatenate([base.vertices, [[100, 100, 100]]]).astype(F), base.faces)     # a vertex no face names
        MC.assert_mesh_equal(SC.simplify(checker, lone, 2.0, None, placement), ref, "unreferenced")
        with_normals = MC.Mesh(base.vertices, base.faces, None, np.ones((64, 3), F))
        assert SC.simplify(checker, with_normals, 2.0, None, placement).normals is None
        shifted = SC.simplify(checker, moved(base, [-50, -60, -70]), 2.0, (0.5, 0.25, 0.125), placement)
        assert len(shifted.faces) > 0 and (shifted.vertices < 0).all()
    # colour rounding: m = 2 members (1, 2) -> (3 + 1) / 2 = 2; m = 3 members (1, 1, 2) -> (4 + 1) / 3 = 1, (2, 2, 3) -> (7 + 1) / 3 = 2
    V = np.array([[0.2, 0.2, 0], [0.4, 0.4, 0], [1.2, 0.2, 0], [1.4, 0.2, 0], [1.6, 0.4, 0], [0.5, 1.5, 0]], F)
    colours = np.array([[1, 0, 255], [2, 1, 254], [1, 2, 0], [1, 2, 0], [2, 3, 1], [9, 9, 9]], np.uint8)
    got = SC.simplify(checker, MC.Mesh(V, np.array([[0, 2, 5], [1, 3, 5], [1, 4, 5]], np.int32), colours), 1.0, None, "mean")
    assert got.faces.tolist() == [[0, 1, 2]] and got.colours.tolist() == [[2, 1, 255], [1, 2, 0], [9, 9, 9]]


def test_an_optimum_far_outside_the_cell_falls_back_to_the_mean(checker):
    """Two triangles with one vertex each in the cell [0, 1)^3, on the planes z = 0.45 and z = 0.75 + 0.1 (x - 0.5), which meet at
    x = -2.5: three cells from the centre (the other four vertices pair up in two more cells, so one face of three clusters is
    left, and the cluster in question is the first in key order).  Their normals are 0.1 rad apart, so the second eigenvalue passes the rank cut and the
    solve goes there; step 7 refuses it."""
    V = np.array([[0.5, 0.5, 0.45], [1.5, 0.5, 0.45], [0.5, 1.5, 0.45], [0.5, 0.4, 0.75], [1.5, 0.4, 0.85], [0.5, 1.4, 0.75]], F)
    mesh = MC.Mesh(V, np.array([[0, 1, 2], [3, 4, 5]], np.int32))
    got = SC.simplify(checker, mesh, 1.0, None, "quadric")
    want, more = np_simplify(mesh, 1.0, (0, 0, 0), "quadric", details=True)
    assert len(got.vertices) == 3 and np.abs(more["free"][0, 0]) > 2.0, more["free"][0]
    mu = ((V[0].astype(np.float64) - 0.5) + (V[3].astype(np.float64) - 0.5)) / 2.0
    assert np.array_equal(MC.bits(got.vertices[0]), MC.bits((0.5 + mu).astype(F)))
    # with a cell bound that reaches the optimum the same sums give it: the fallback is what kept it away
    P = V.astype(np.float64)
    S, t = np.zeros((3, 3)), np.zeros(3)
    for a, b, c in mesh.faces:
        g = np.cross(P[b] - P[a], P[c] - P[a])
        S += np.outer(g, g)
        t += g * -(g @ (P[a] - 0.5))
    sums = [S[0, 0], S[0, 1], S[0, 2], S[1, 1], S[1, 2], S[2, 2], t[0], t[1], t[2]]
    assert np.array_equal(SC.place(checker, sums, mu, 1.0), mu)
    assert np.abs(SC.place(checker, sums, mu, 8.0)[0] + 3.0) < 1e-3
    assert np.array_equal(SC.place(checker, [np.inf] + sums[1:], mu, 8.0), mu) and np.array_equal(SC.place(checker, [0.0] * 9, mu, 8.0), mu)


def sphere_rms(vertices, centre, radius):
    return float(np.sqrt(np.mean((np.linalg.norm(vertices.astype(np.float64) - centre, axis=1) - radius) ** 2)))


def test_quadric_vertices_lie_nearer_the_sphere_than_mean_vertices(checker, sphere):
    mesh, grid, centre, radius = sphere
    cell = 4 * float(grid.voxel)
    rms = {}
    for placement in PLACEMENTS:
        got = SC.simplify(checker, mesh, cell, None, placement)
        assert 0 < len(got.faces) < len(mesh.faces)
        structure(mesh, got, cell, (0, 0, 0))
        rms[placement] = sphere_rms(got.vertices, centre, radius)
        print("sphere of %d faces at cell = 4 voxels, %s: %d faces, rms distance to the sphere %.4g" % (len(mesh.faces), placement, len(got.faces), rms[placement]))
    assert rms["quadric"] < rms["mean"]


# --------------------------------------------------------------------------------------------------------------------
# the C ABI without a device, the documents, the binary
# --------------------------------------------------------------------------------------------------------------------

def test_header_library_and_documents_name_the_call(pkg):
    header = open(os.path.join(ROOT, "include", "apd_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = pkg.lib()
    assert re.search(r"\bint\s+apd_mesh_simplify\s*\(", text) and "APD_SIMPLIFY_QUADRIC = 1" in text and "APD_SIMPLIFY_MEAN = 0" in text
    assert hasattr(L, "apd_mesh_simplify") and L.apd_mesh_simplify.argtypes is not None
    for name in ("DESIGN.md", "INTEGRATION.md", "README.md", os.path.join("apd-mvs_amd", "csrc", "apd_simplify_math.h")):
        assert "C23" in open(os.path.join(ROOT, name)).read(), name
    assert "contract C23" in header and "Simplifying the mesh" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_refusals_and_an_empty_mesh(pkg):
    L = pkg.lib()
    m = C.c_void_p()
    assert L.apd_mesh_create(0, 0, None, None, 0, None, 0, C.byref(m)) == 0
    out, n = C.c_void_p(1234), C.c_longlong(-7)
    last = lambda: L.apd_fusion_last_error().decode()
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert L.apd_mesh_simplify(m, bad, None, 1, C.byref(out), C.byref(n), C.byref(n)) == -1
        assert last() == "apd_mesh_simplify: a cell of %g, not a positive finite number" % bad
    for k, bad in enumerate((float("inf"), float("nan"), -float("inf"))):
        org = [0.0, 0.0, 0.0]
        org[k] = bad
        assert L.apd_mesh_simplify(m, 0.5, (C.c_float * 3)(*org), 0, C.byref(out), C.byref(n), C.byref(n)) == -1
        assert last() == "apd_mesh_simplify: origin component %d is %g" % (k, bad)
    for bad in (-1, 2, 7):
        assert L.apd_mesh_simplify(m, 0.5, None, bad, C.byref(out), C.byref(n), C.byref(n)) == -1
        assert last() == "apd_mesh_simplify: placement %d, neither APD_SIMPLIFY_MEAN nor APD_SIMPLIFY_QUADRIC" % bad
    assert L.apd_mesh_simplify(None, 0.5, None, 1, C.byref(out), None, None) == -1 and last() == "apd_mesh_simplify: null argument"
    assert L.apd_mesh_simplify(m, 0.5, None, 1, None, None, None) == -1 and last() == "apd_mesh_simplify: null argument"
    assert out.value == 1234 and n.value == -7
    # an empty mesh gives an empty mesh, with or without the counts, and touches no device
    for counts in ((None, None), (C.byref(n), C.byref(n))):
        assert L.apd_mesh_simplify(m, 0.5, None, 1, C.byref(out), *counts) == 0 and out.value != 1234
        L.apd_mesh_destroy(out)
        out = C.c_void_p(1234)
    assert n.value == 0
    L.apd_mesh_destroy(m)
    mesh = pkg.Mesh.from_arrays(np.zeros((0, 3), F), np.zeros((0, 3), np.int32))
    for got in (mesh.simplify(0.5), mesh.simplify(0.5, origin=(1, 2, 3), placement="mean")):
        assert got.vertices.shape == (0, 3) and got.faces.shape == (0, 3) and got.normals is None
    with pytest.raises(pkg.ApdError, match="apd_mesh_simplify: a cell of 0"):
        mesh.simplify(0)
    with pytest.raises(ValueError, match="placement"):
        mesh.simplify(1.0, placement="median")
    mesh.close()
    with pytest.raises(pkg.ApdError, match="the mesh is closed"):
        mesh.simplify(1.0)


def _apd(tmp_path, *flags):
    r = subprocess.run([APD_BIN, str(tmp_path / "no_such_folder"), "0"] + list(flags), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode != 0 and not (tmp_path / "no_such_folder").exists()
    return r.stdout


def test_binary_refuses_mesh_simplify_without_mesh_and_bad_values_before_anything_is_read(tmp_path):
    for flags in (("--mesh-simplify", "0.2"), ("--mesh-simplify", "0.2,mean", "--mesh-normals")):
        out = _apd(tmp_path, *flags)
        assert "changes the mesh of --mesh VOXEL[,TRUNC]: not without it" in out and "USAGE" in out, (flags, out[-500:])
    for bad in ("", "0", "-1", "x", "nan", "inf", "0.1,", "0.1,median", "0.1,mean,quadric", ",mean", "0.1x", "mean"):
        out = _apd(tmp_path, "--mesh", "0.1", "--mesh-simplify", bad)
        assert "bad value '%s' of --mesh-simplify" % bad in out and "USAGE" in out, (bad, out[-500:])
    for good in (("--mesh-simplify", "0.2"), ("--mesh-simplify", "0.2,mean"), ("--mesh-simplify", "1e-3,quadric", "--mesh-weld", "1e-5", "--mesh-normals")):
        for order in (("--mesh", "0.1") + good, good + ("--mesh", "0.1")):
            out = _apd(tmp_path, *order)
            assert "bad value" not in out and "USAGE" not in out, (order, out[-500:])
    assert "--mesh-simplify CELL[,mean|quadric]" in _apd(tmp_path, "--mesh-simplify")
