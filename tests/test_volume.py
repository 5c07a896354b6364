"""The signed distance volume and its marching-tetrahedra mesh without a device: the sequential checker (tests/helpers/volume_ref.cpp)
held against an independent numpy restatement of contract C21 (binary32 operations written out, its own construction of the 6 x 16
table of cases from the rule) on the views and fields of the device tests; every pattern of one cell; an analytic sphere; a planted
plane whose answer is known exactly; the refusals of the apd_volume_* and apd_mesh_* calls; the entry points in the header and in the
library; and the loud failure without a GPU.  The grids, views and fields of test_gpu_volume.py are made here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import volume_checker as VC
from test_points_render import bits32, np_draw, ring_cameras, unit_camera

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("apd_volume_create", "apd_volume_destroy", "apd_volume_integrate", "apd_volume_download", "apd_volume_upload",
               "apd_volume_extract_mesh", "apd_volume_view_chunk", "apd_mesh_counts", "apd_mesh_has_colour", "apd_mesh_download",
               "apd_mesh_write_ply", "apd_mesh_destroy")
F = np.float32
# rows of samples around a wave, around a workgroup of 256 lanes, and off every multiple
INTEGRATE_DIMS = [(2, 2, 2), (3, 2, 2), (2, 65, 2), (65, 3, 2), (9, 5, 3), (17, 9, 6), (64, 4, 2)]
DIRS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]
PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return VC.build(tmp_path_factory.mktemp("volume_checker"))


# --------------------------------------------------------------------------------------------------------------------
# grids, views and fields
# --------------------------------------------------------------------------------------------------------------------

def box_grid(dims, half=1.25, trunc_voxels=3.0, max_weight=64.0):
    """A grid of `dims` samples centred on the origin whose longest axis spans 2 * half: the unit sphere fits inside."""
    voxel = F(2 * half / (max(dims) - 1))
    origin = [-float(voxel) * (d - 1) / 2 for d in dims]
    return VC.Grid(dims, origin, voxel, F(trunc_voxels) * voxel, max_weight)


def sphere_depth(cam, radius=1.0):
    """The depth map (K[8]-scaled z of the camera frame, as the projection gives it) of the sphere of `radius` about the origin; 0 where
    a pixel's ray misses it.  binary64, rounded once."""
    K, R, t = [np.array(list(a), np.float64) for a in (cam.K, cam.R, cam.t)]
    K, R = K.reshape(3, 3), R.reshape(3, 3)
    W, H = int(cam.width), int(cam.height)
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    rays = np.linalg.solve(K, np.stack([u.ravel(), v.ravel(), np.ones(W * H)]))   # camera frame, third component K[8] * z = 1
    centre = -R.T @ t
    dirs = R.T @ rays
    a, b, c = (dirs * dirs).sum(0), 2 * (dirs * centre[:, None]).sum(0), centre @ centre - radius * radius
    disc = b * b - 4 * a * c
    s = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), 0.0)
    return np.where((disc > 0) & (s > 0), s, 0.0).reshape(H, W).astype(F)


def plane_depth(cam, z0=4.0):
    return np.full((int(cam.height), int(cam.width)), z0, F)


def view_images(cams, channels, seed=5):
    rng = np.random.default_rng(seed)
    shape = lambda c: (int(c.height), int(c.width)) + ((3,) if channels == 3 else ())
    return [rng.integers(0, 256, shape(c)).astype(F) for c in cams]


def mixed_weights(V):
    return [F(w) for w in np.resize([1.0, 0.5, 2.25, 3.0], V)]


def planted_plane():
    """(grid, camera, z0): K = I, R = I, t = 0 and an image of 2 x 2 pixels, so a sample (x, y, z) has u = x / z and w = y / z; voxel,
    trunc and z0 are powers of two.  x runs from -1.5 to 3.5: at z = 2 the sample at x = -1 has u + 0.5 == 0 (pixel 0) and the one at
    x = 3 has u + 0.5 == 2, the width (outside).  z runs from -0.5 (behind the camera) to 3; the plane z0 = 2.125 lies midway between two
    layers of samples, so every crossing has t = 0.5 exactly (a plane through a layer would give t = 0 and triangles without area)."""
    return VC.Grid((21, 9, 15), (-1.5, -1.5, -0.5), 0.25, 0.5, 4.0), (2, 2), F(2.125)


def bad_depth_row():
    """A 5 x 1 depth map over the planted grid's camera model: a good depth, then 0, negative, +inf and NaN."""
    return (5, 1), np.array([[2.125, 0.0, -1.0, np.inf, np.nan]], F)


def long_axis_case(pkg, W, H):
    """unit_camera(W, H) and a map of W x H distinct depths between 1 and 2, for a 16384 x 2 or a 2 x 16384 image: the row stride."""
    cam = unit_camera(pkg, W, H)
    depth = (1.0 + np.arange(W * H, dtype=np.float64).reshape(H, W) / (W * H)).astype(F)
    return cam, depth


def corner_grids(W, H):
    """Two grids of 2 x 2 x 2 samples from (0, 0, 1) with a voxel of W - 1 and of H - 1: under unit_camera(W, H) the layer at z = 1 lands
    on pixel (0, 0) and, along the axis the voxel was taken from, on the last pixel of that axis; what lands outside stays untouched."""
    return [VC.Grid((2, 2, 2), (0.0, 0.0, 1.0), float(n - 1), 4.0 * (n - 1)) for n in (W, H)]


def sphere_field(dims, radius_voxels=5.0, shell=None):
    """(grid, tsdf, weight): the distance to a sphere about the grid's middle (off the samples), in units of trunc = 2 voxels, clamped
    to 1; every sample known, or with `shell` only those within that many trunc of the surface."""
    g = VC.Grid(dims, (0.0, 0.0, 0.0), 0.5, 1.0)
    P = g.positions().astype(np.float64)
    centre = (np.array(dims) - 1) * 0.25 + np.array([0.11, -0.07, 0.05])
    d = np.linalg.norm(P - centre, axis=1) - radius_voxels * 0.5
    tsdf = np.minimum(d / 1.0, 1.0).astype(F)
    weight = np.ones(len(P), F) if shell is None else (np.abs(d) <= shell).astype(F)
    return g, tsdf, weight


def random_field(dims, seed, unknown=0.2, colour=False):
    rng = np.random.default_rng(seed)
    g = VC.Grid(dims, (-1.0, 0.5, 2.0), 0.125, 0.5)
    tsdf = rng.uniform(-1, 1, g.samples).astype(F)
    weight = np.where(rng.random(g.samples) < unknown, 0, rng.integers(1, 5, g.samples)).astype(F)
    col = None
    if colour:
        col = np.concatenate([rng.uniform(0, 255, (g.samples, 3)), np.where(rng.random((g.samples, 1)) < 0.3, 0, 2.0)], 1).astype(F)
    return g, tsdf, weight, col


def one_cell(signs, known=0xFF):
    """(grid, tsdf, weight) of one unit cell: corner b (bit 0: x, 1: y, 2: z) is inside when bit b of `signs` is set and known when bit b
    of `known` is; magnitudes differ per corner and keep t away from 0 and 1."""
    g = VC.Grid((2, 2, 2), (0.0, 0.0, 0.0), 1.0, 1.0)
    b = np.arange(8)
    mag = (0.3 + 0.07 * b).astype(F)
    return g, np.where((signs >> b) & 1, -mag, mag).astype(F), ((known >> b) & 1).astype(F)


def slab_field(rows, known_rows=None, partial=0):
    """(grid, tsdf, weight): 2 x rows x 2 samples with x = 0 inside and x = 1 outside in every row: the zero level is the plane
    x = 0.5, crossed by the edges in the directions (1,0,0), (1,1,0), (1,0,1) and (1,1,1).  The first `known_rows` rows (default:
    all) are known, and of the two rows after them the samples (i, k) whose bit i + 2 * k (+ 4 for the second row) of `partial` is set."""
    g = VC.Grid((2, rows, 2), (0.0, 0.0, 0.0), 1.0, 1.0)
    tsdf = np.tile(np.array([-0.5, 0.5], F), rows * 2)
    w = np.ones((2, rows, 2), F)
    if known_rows is not None:
        w[:, known_rows:, :] = 0
        for bit in range(8):
            if (partial >> bit) & 1:
                w[(bit >> 1) & 1, known_rows + (bit >> 2), bit & 1] = 1
    return g, tsdf, w.ravel()


def slab_counts(known_rows):
    """(vertices, faces) of slab_field with that many fully known rows (>= 1) and no partial one: per row the edges (1,0,0) of both
    layers and (1,0,1) across them, between consecutive rows (1,1,0) of both layers and (1,1,1); per cell between two rows one
    triangle in each of the four tetrahedra whose permutation has x first or last, two in each of the two that have it in the middle."""
    r = known_rows
    return 3 * r + 3 * (r - 1), 8 * (r - 1)


def field_with_count(checker, target, what):
    """A slab_field whose mesh has exactly `target` vertices (what = 0) or faces (what = 1): the number of known rows that comes
    closest from below, and the two partial rows after them that make up the rest, found by asking the checker."""
    per_row = (6, 8)[what]
    for r in range(max(1, target // per_row - 1), target // per_row + 3):
        for partial in range(256):
            field = slab_field(r + 3, r, partial)
            mesh = VC.extract(checker, *field)
            if (len(mesh.vertices), len(mesh.faces))[what] == target:
                return field, mesh
    raise AssertionError("no slab with %d %s" % (target, ("vertices", "faces")[what]))


# --------------------------------------------------------------------------------------------------------------------
# the numpy restatement
# --------------------------------------------------------------------------------------------------------------------

def np_integrate(grid, state, cams, depths, images=None, weights=None):
    """Contract C21's update in place, every operation a binary32 one in the contract's order."""
    P = grid.positions()
    D, W, Cc = state.tsdf, state.weight, state.colour
    trunc, top = F(grid.trunc), F(grid.max_weight)
    for s, cam in enumerate(cams):
        w = F(1.0) if weights is None else F(weights[s])
        ok, c, r, d = np_draw(P, cam)
        px = np.where(ok, r * int(cam.width) + c, 0)
        with np.errstate(all="ignore"):
            z = np.ascontiguousarray(depths[s], F).ravel()[px]
            ok = ok & (z > 0) & (bits32(z) < 0x7f800000)
            sdf = z - d
            ok = ok & (sdf >= -trunc)
            v = sdf / trunc
            v = np.where(v > F(1), F(1), v)
            new_D = (D * W + v * w) / (W + w)
            total = W + w
            assert new_D.dtype == F and total.dtype == F and sdf.dtype == F
            if Cc is not None and images is not None:
                img = np.ascontiguousarray(images[s], F).reshape(int(cam.height) * int(cam.width), -1)
                paint = ok & (sdf <= trunc)
                for ch in range(3):
                    col = img[px, ch if img.shape[1] == 3 else 0]
                    mixed = (Cc[:, ch] * Cc[:, 3] + col * w) / (Cc[:, 3] + w)
                    Cc[:, ch] = np.where(paint, mixed, Cc[:, ch])
                ctotal = Cc[:, 3] + w
                Cc[:, 3] = np.where(paint, np.where(ctotal > top, top, ctotal), Cc[:, 3])
            D[:] = np.where(ok, new_D, D)
            W[:] = np.where(ok, np.where(total > top, top, total), W)
    return state


def corner_of(q, c):
    """Corner c of tetrahedron q as a 0/1 vector: the path along the axis permutation."""
    v = np.zeros(3, int)
    for axis in PERMS[q][:c] if c < 3 else (0, 1, 2):
        v[axis] = 1
    return v


def np_cases():
    """{(q, mask): [((lo, hi), (lo, hi), (lo, hi)), ..]}: the rule of the contract, restated with numpy vectors."""
    table = {}
    for q in range(6):
        X = [corner_of(q, c).astype(float) for c in range(4)]
        for mask in range(1, 15):
            ins = [c for c in range(4) if (mask >> c) & 1]
            outs = [c for c in range(4) if not (mask >> c) & 1]
            if len(ins) == 2:
                (a, b), (c, d) = ins, outs
                tris = [[(a, c), (a, d), (b, d)], [(a, c), (b, d), (b, c)]]
            else:
                a, rest = (ins[0], outs) if len(ins) == 1 else (outs[0], ins)
                tris = [[(a, x) for x in rest]]
            g = len(ins) * sum(X[c] for c in outs) - len(outs) * sum(X[c] for c in ins)
            out = []
            for tri in tris:
                mid = [(X[x] + X[y]) / 2 for x, y in tri]
                side = np.cross(mid[1] - mid[0], mid[2] - mid[0]) @ g
                assert side != 0
                tri = tri if side > 0 else [tri[0], tri[2], tri[1]]
                out.append(tuple((min(e), max(e)) for e in tri))
            table[(q, mask)] = out
    return table


def np_extract(grid, tsdf, weight, colour=None):
    """Contract C21's extraction, vectorised: flags per (sample, direction), their running count as ids, the faces of every (cell, q)
    from np_cases(), sorted by (cell, q, order)."""
    nx, ny, nz = grid.dims
    D, W = np.asarray(tsdf, F).reshape(nz, ny, nx), np.asarray(weight, F).reshape(nz, ny, nx)
    known = W > 0
    inside = known & (D < 0)
    P = grid.positions().reshape(nz, ny, nx, 3)
    Cc = None if colour is None else np.asarray(colour, F).reshape(nz, ny, nx, 4)
    flags = np.zeros((nz, ny, nx, 7), bool)
    xyz = np.zeros((nz, ny, nx, 7, 3), F)
    bgr = np.zeros((nz, ny, nx, 7, 3), np.uint8)
    for dir_, (dx, dy, dz) in enumerate(DIRS):
        lo = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx))
        up = (slice(dz, nz), slice(dy, ny), slice(dx, nx))
        flags[lo + (dir_,)] = known[lo] & known[up] & (inside[lo] != inside[up])
        with np.errstate(all="ignore"):
            t = D[lo] / (D[lo] - D[up])
            xyz[lo + (dir_,)] = P[lo] + t[..., None] * (P[up] - P[lo])
            if Cc is not None:
                ha, hb = Cc[lo][..., 3] > 0, Cc[up][..., 3] > 0
                for ch in range(3):
                    ca, cb = Cc[lo][..., ch], Cc[up][..., ch]
                    x = np.where(ha & hb, ca + t * (cb - ca), np.where(ha, ca, np.where(hb, cb, F(0))))
                    x = np.where(x > 0, np.where(x > F(255), F(255), x), F(0)).astype(F)
                    bgr[lo + (dir_, ch)] = np.trunc(x + F(0.5)).astype(np.uint8)
    flat = flags.ravel()
    ids = (np.cumsum(flat) - 1).reshape(flags.shape)
    vertices = xyz.reshape(-1, 3)[flat]
    colours = None if colour is None else bgr.reshape(-1, 3)[flat]
    cells = np.arange((nx - 1) * (ny - 1) * (nz - 1)).reshape(nz - 1, ny - 1, nx - 1)
    at = lambda a, b: a[b[2]:nz - 1 + b[2], b[1]:ny - 1 + b[1], b[0]:nx - 1 + b[0]]
    table = np_cases()
    rows = []
    for q in range(6):
        X = [corner_of(q, c) for c in range(4)]
        all_known = np.logical_and.reduce([at(known, x) for x in X])
        mask = sum(at(inside, x).astype(int) << c for c, x in enumerate(X))
        for m in range(1, 15):
            sel = all_known & (mask == m)
            if not sel.any():
                continue
            for order, tri in enumerate(table[(q, m)]):
                v = [at(ids[..., DIRS.index(tuple(X[hi] - X[lo]))], X[lo])[sel] for lo, hi in tri]
                rows.append(np.stack([cells[sel], np.full(sel.sum(), q), np.full(sel.sum(), order)] + v, 1))
    if rows:
        rows = np.concatenate(rows)
        rows = rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]
        faces = rows[:, 3:].astype(np.int32)
    else:
        faces = np.zeros((0, 3), np.int32)
    return VC.MeshArrays(vertices, colours, faces)


# --------------------------------------------------------------------------------------------------------------------
# the cases the device tests run, and the checker against the restatement on them
# --------------------------------------------------------------------------------------------------------------------

def integrate_cases(pkg, chunk=16):
    """(name, grid, cameras, depths, images or None, weights or None)"""
    for V in (1, 3, chunk + 1):
        cams = ring_cameras(pkg, V)
        for dims in INTEGRATE_DIMS if V == 3 else [(9, 5, 3), (17, 9, 6)]:
            g = box_grid(dims)
            yield "sphere %d views %r" % (V, dims), g, cams, [sphere_depth(c) for c in cams], None, None
        g = box_grid((17, 9, 6), max_weight=2.0)
        yield "plane %d views, 3 channels, mixed weights" % V, g, cams, [plane_depth(c) for c in cams], view_images(cams, 3), mixed_weights(V)
        yield "sphere %d views, 1 channel" % V, g, cams, [sphere_depth(c) for c in cams], view_images(cams, 1), None
    g, size, z0 = planted_plane()
    cam = unit_camera(pkg, *size)
    for n in (1, 2, 7):
        yield "planted plane %d views" % n, g, [cam] * n, [np.full(size[::-1], z0, F)] * n, [np.full(size[::-1], 77.0, F)] * n, None
    size, row = bad_depth_row()
    yield "depths 0, negative, inf, nan", g, [unit_camera(pkg, *size)], [row], [np.full((1, 5), 9.0, F)], None
    for W, H in ((16384, 2), (2, 16384)):
        cam, depth = long_axis_case(pkg, W, H)
        for grid in corner_grids(W, H):
            yield "map %d x %d, voxel %g" % (W, H, grid.voxel), grid, [cam], [depth], [depth * F(100)], None


def run_integrate(fn, grid, cams, depths, images, weights):
    state = VC.State(grid, colour=images is not None)
    return fn(grid, state, cams, depths, images, weights)


def extract_cases():
    """(name, grid, tsdf, weight, colour or None)"""
    for dims, seed in (((3, 3, 3), 1), ((9, 5, 3), 2), ((17, 9, 6), 3)):
        yield ("random %r" % (dims,),) + random_field(dims, seed)
        yield ("random with colour %r" % (dims,),) + random_field(dims, seed + 10, colour=True)
    g, tsdf, weight, _ = random_field((9, 5, 3), 4, unknown=0.0)
    zeros = tsdf.copy()
    zeros[::3], zeros[1::7] = 0.0, -0.0
    yield "zeros and negative zeros", g, zeros, weight, None
    yield "nothing known", g, tsdf, np.zeros_like(weight), None
    yield "nothing inside", g, np.abs(tsdf), weight, None
    yield ("sphere",) + sphere_field((17, 16, 15)) + (None,)
    yield ("sphere in a shell",) + sphere_field((17, 16, 15), shell=1.0) + (None,)


def test_checker_equals_the_numpy_restatement_on_every_integration(pkg, checker):
    for name, grid, cams, depths, images, weights in integrate_cases(pkg):
        want = run_integrate(np_integrate, grid, cams, depths, images, weights)
        got = run_integrate(lambda *a: VC.integrate(checker, *a), grid, cams, depths, images, weights)
        VC.assert_state_equal(got, want, name)
        assert (want.weight > 0).any(), name


def test_checker_equals_the_numpy_restatement_on_every_field(pkg, checker):
    with_faces = 0
    for name, grid, tsdf, weight, colour in extract_cases():
        want = np_extract(grid, tsdf, weight, colour)
        VC.assert_mesh_equal(VC.extract(checker, grid, tsdf, weight, colour), want, name)
        with_faces += int(len(want.faces) > 0)
    assert with_faces >= 8
    for signs in range(256):
        for g, tsdf, weight in (one_cell(signs), one_cell(0b10010110, known=signs)):
            VC.assert_mesh_equal(VC.extract(checker, g, tsdf, weight), np_extract(g, tsdf, weight), signs)
    state = run_integrate(lambda *a: VC.integrate(checker, *a), *list(integrate_cases(pkg))[3][1:])
    VC.assert_mesh_equal(VC.extract(checker, box_grid((17, 9, 6)), state.tsdf, state.weight), np_extract(box_grid((17, 9, 6)), state.tsdf, state.weight))


def test_the_table_of_the_header_is_the_rule(checker):
    table, want = VC.cases(checker), np_cases()
    for q in range(6):
        for mask in range(16):
            tris = want.get((q, mask), [])
            assert table[q, mask, 0] == len(tris), (q, mask)
            edges = [(lo << 2) | hi for tri in tris for lo, hi in tri]
            assert table[q, mask, 1:1 + len(edges)].tolist() == edges, (q, mask)


# --------------------------------------------------------------------------------------------------------------------
# one cell, exhaustively
# --------------------------------------------------------------------------------------------------------------------

def directed_edges(faces):
    return np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])


def tet_of_faces(known, inside):
    """The tetrahedron of every face of a one-cell mesh, in the mesh's order, with its inside and outside corners."""
    out = []
    for q in range(6):
        X = [corner_of(q, c) for c in range(4)]
        bit = [int(x[0] + 2 * x[1] + 4 * x[2]) for x in X]
        if not all((known >> b) & 1 for b in bit):
            continue
        ins = [X[c] for c in range(4) if (inside >> bit[c]) & 1]
        outs = [X[c] for c in range(4) if not (inside >> bit[c]) & 1]
        count = {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[len(ins)]
        out += [(ins, outs)] * count
    return out


def test_every_sign_pattern_of_one_cell(checker):
    for signs in range(256):
        g, tsdf, weight = one_cell(signs)
        mesh = VC.extract(checker, g, tsdf, weight)
        tets = tet_of_faces(0xFF, signs)
        assert len(mesh.faces) == len(tets), signs
        assert (len(mesh.faces) == 0) == (signs in (0, 255))
        V = mesh.vertices.astype(np.float64)
        for face, (ins, outs) in zip(mesh.faces, tets):
            normal = np.cross(V[face[1]] - V[face[0]], V[face[2]] - V[face[0]])
            gradient = len(ins) * np.sum(outs, 0) - len(outs) * np.sum(ins, 0)
            assert normal @ gradient > 0, (signs, face)
        # an edge of a triangle lies on the cell's boundary when both ends share a coordinate of exactly 0 or 1
        edges = directed_edges(mesh.faces)
        on_boundary = np.array([any(V[a, k] == V[b, k] and V[a, k] in (0.0, 1.0) for k in range(3)) for a, b in edges], bool)
        interior = [tuple(e) for e in edges[~on_boundary]]
        for a, b in interior:
            assert interior.count((a, b)) == 1 and interior.count((b, a)) == 1, (signs, a, b)
        assert ((V > 0) & (V < 1)).any(1).all()   # t stays away from 0 and 1


def test_every_known_pattern_of_one_cell(checker):
    signs = 0b10010110
    whole = len(VC.extract(checker, *one_cell(signs)).faces)
    for known in range(256):
        g, tsdf, weight = one_cell(signs, known)
        mesh = VC.extract(checker, g, tsdf, weight)
        assert len(mesh.faces) == len(tet_of_faces(known, signs)), known
        assert len(mesh.faces) <= whole and (known == 255) == (len(mesh.faces) == whole)
        # a vertex exists wherever two known corners of different sign share one of the seven edges, used by a face or not
        b = np.arange(8)
        crossing = sum(1 for lo in b for d in DIRS if lo & (d[0] + 2 * d[1] + 4 * d[2]) == 0 and (known >> lo) & 1 and
                       (known >> (lo + d[0] + 2 * d[1] + 4 * d[2])) & 1 and ((signs >> lo) ^ (signs >> (lo + d[0] + 2 * d[1] + 4 * d[2]))) & 1)
        assert len(mesh.vertices) == crossing, known
        assert mesh.faces.size == 0 or mesh.faces.max() < len(mesh.vertices)


# --------------------------------------------------------------------------------------------------------------------
# the sphere
# --------------------------------------------------------------------------------------------------------------------

def assert_closed(faces):
    edges = directed_edges(faces)
    both = np.concatenate([edges, edges[:, ::-1]])
    pairs, counts = np.unique(edges, axis=0, return_counts=True)
    assert (counts == 1).all()                                                # no edge twice the same way
    assert len(np.unique(both, axis=0)) == len(edges)                         # and each once the other way
    return len(edges) // 2


def test_sphere_is_closed_and_near_the_surface(checker):
    g, tsdf, weight = sphere_field((17, 16, 15))
    mesh = VC.extract(checker, g, tsdf, weight)
    assert len(mesh.faces) > 500
    E = assert_closed(mesh.faces)
    used = np.unique(mesh.faces)
    assert len(used) == len(mesh.vertices)           # every vertex of an all-known field is a face's
    assert len(mesh.vertices) - E + len(mesh.faces) == 2
    centre = (np.array(g.dims) - 1) * 0.25 + np.array([0.11, -0.07, 0.05])
    off = np.abs(np.linalg.norm(mesh.vertices.astype(np.float64) - centre, axis=1) - 2.5)
    # a vertex lies on an edge of at most sqrt(3) voxels whose ends bracket the surface
    assert off.max() <= np.sqrt(3) * 0.5
    _, _, shell = sphere_field((17, 16, 15), shell=1.0)
    assert 0 < (shell == 0).sum() < g.samples
    inner = VC.extract(checker, g, tsdf, shell)
    VC.assert_mesh_equal(inner, mesh, "the shell")


# --------------------------------------------------------------------------------------------------------------------
# the planted plane
# --------------------------------------------------------------------------------------------------------------------

def test_planted_plane(pkg, checker):
    g, size, z0 = planted_plane()
    cam = unit_camera(pkg, *size)
    P = g.positions().astype(np.float64)
    x, y, z = P.T
    with np.errstate(all="ignore"):
        u, w = x / z, y / z
        # int(v + 0.5f) truncates toward zero: a centre down to v + 0.5 > -1 still lands on pixel 0, as in the fusion
        in_view = (z > 0) & (u + 0.5 > -1) & (u + 0.5 < size[0]) & (w + 0.5 > -1) & (w + 0.5 < size[1])
    observed = in_view & (z0 - z >= -0.5)
    assert 300 < observed.sum() < in_view.sum() < g.samples
    at = lambda X, Y, Z: int(np.flatnonzero((x == X) & (y == Y) & (z == Z))[0])
    assert observed[at(-1.0, 0.0, 2.0)] and not observed[at(3.0, 0.0, 2.0)]      # u + 0.5 == 0 is pixel 0; u + 0.5 == width is outside
    assert observed[at(-1.25, 0.0, 2.0)] and not observed[at(-1.5, 0.0, 1.0)]   # u + 0.5 == -0.125 truncates to pixel 0; -1 is outside
    assert not observed[at(0.0, 0.0, -0.5)] and not observed[at(0.0, 0.0, 0.0)] and not observed[at(0.0, 0.0, 2.75)]
    want = np.where(observed, np.minimum(1.0, (z0 - z) / 0.5), 1.0).astype(F)
    for n in (1, 2, 7):
        state = VC.integrate(checker, g, VC.State(g, colour=True), [cam] * n, [np.full(size[::-1], z0, F)] * n, [np.full(size[::-1], 77.0, F)] * n)
        assert np.array_equal(bits32(state.tsdf), bits32(want)), n
        assert np.array_equal(state.weight, np.where(observed, min(n, 4), 0).astype(F)), n   # saturates at max_weight = 4
        painted = observed & (z0 - z <= 0.5)
        assert np.array_equal(state.colour, np.where(painted[:, None], F([77, 77, 77, min(n, 4)]), F(0))), n
        mesh = VC.extract(checker, g, state.tsdf, state.weight, state.colour)
        assert len(mesh.faces) > 50
        assert (np.abs(mesh.vertices[:, 2].astype(np.float64) - float(z0)) <= 2 * np.spacing(z0)).all()
        V = mesh.vertices.astype(np.float64)
        normals = np.cross(V[mesh.faces[:, 1]] - V[mesh.faces[:, 0]], V[mesh.faces[:, 2]] - V[mesh.faces[:, 0]])
        assert (normals[:, 2] < 0).all() and (normals[:, :2] == 0).all()
        assert (mesh.colours == 77).all()
    size, row = bad_depth_row()
    state = VC.integrate(checker, g, VC.State(g), [unit_camera(pkg, *size)], [row])
    ok, c, _, _ = np_draw(g.positions(), unit_camera(pkg, *size))
    assert all((ok & (c == k)).sum() > 20 for k in range(5))
    assert (state.weight[ok & (c > 0)] == 0).all() and (bits32(state.tsdf[ok & (c > 0)]) == bits32(F(1))).all()
    assert (state.weight[ok & (c == 0)] > 0).any()


def test_slab_counts(checker):
    for rows in (1, 2, 5):
        mesh = VC.extract(checker, *slab_field(7, rows))
        assert (len(mesh.vertices), len(mesh.faces)) == slab_counts(rows), rows
    for target in (2047, 2048, 2049):
        for what in (0, 1):
            _, mesh = field_with_count(checker, target, what)
            assert (len(mesh.vertices), len(mesh.faces))[what] == target


def test_empty_mesh_and_its_file(checker):
    g, tsdf, weight, _ = random_field((3, 3, 3), 1)
    mesh = VC.extract(checker, g, np.abs(tsdf), weight)
    assert mesh.vertices.shape == (0, 3) and mesh.faces.shape == (0, 3)
    assert VC.ply_bytes(mesh) == (b"ply\nformat binary_little_endian 1.0\nelement vertex 0\nproperty float x\nproperty float y\nproperty float z\n"
                                  b"element face 0\nproperty list uchar int vertex_indices\nend_header\n")


# --------------------------------------------------------------------------------------------------------------------
# the C ABI without a device
# --------------------------------------------------------------------------------------------------------------------

def test_header_and_library_name_every_entry_point(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "apd_mi355x.h")).read(), flags=re.S)
    L = pkg.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(L, name), name
    assert re.search(r"int\s+apd_volume_create\s*\(\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,\s*float\s+\w+\s*,"
                     r"\s*float\s+\w+\s*,\s*float\s+\w+\s*,\s*int\s+\w+\s*,\s*apd_volume_t\s*\*\s*\w+\s*\)", text)
    assert re.search(r"int\s+apd_volume_integrate\s*\(\s*apd_volume_t\s+\w+\s*,\s*int\s+\w+\s*,\s*const\s+apd_camera\s*\*\s*\w+\s*,\s*const\s+float\s*\*\s*const\s*\*\s*\w+\s*,"
                     r"\s*const\s+float\s*\*\s*const\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)", text)
    assert len(L.apd_volume_create.argtypes) == 10 and len(L.apd_volume_integrate.argtypes) == 8 and len(L.apd_mesh_download.argtypes) == 4
    assert 1 <= L.apd_volume_view_chunk() <= 24   # 128 bytes a view in 4 KiB of kernel arguments, with room for the rest
    contract = open(os.path.join(ROOT, "include", "apd_mi355x.h")).read()
    assert "contract C21" in contract and "C21" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_create_refusals(pkg):
    L = pkg.lib()
    out = C.c_void_p(1234)
    origin = (C.c_float * 3)(0, 0, 0)

    def refused(message, dims=(4, 4, 4), org=origin, voxel=0.5, trunc=1.0, top=64.0, outp=C.byref(out), device=0):
        assert L.apd_volume_create(device, *dims, org, voxel, trunc, top, 0, outp) == -1
        assert L.apd_fusion_last_error().decode() == "apd_volume_create: " + message
        assert out.value == 1234

    refused("null argument", org=None)
    refused("null argument", outp=None)
    refused("1 x 4 x 4 samples, fewer than 2 along an axis", dims=(1, 4, 4))
    refused("4 x 0 x 4 samples, fewer than 2 along an axis", dims=(4, 0, 4))
    refused("4 x 4 x -3 samples, fewer than 2 along an axis", dims=(4, 4, -3))
    refused("2048 x 1024 x 1024 samples, 2^31 or more", dims=(2048, 1024, 1024))
    refused("65536 x 65536 x 2 samples, 2^31 or more", dims=(65536, 65536, 2))
    refused("device -1", device=-1)
    refused("an origin of 0, nan, 0", org=(C.c_float * 3)(0, float("nan"), 0))
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        refused("a voxel size of %g, not a positive finite number" % bad, voxel=bad)
        refused("a truncation distance of %g, not a positive finite number" % bad, trunc=bad)
        refused("a maximal weight of %g, not a finite number of at least 1" % bad, top=bad)
    refused("a maximal weight of 0.5, not a finite number of at least 1", top=0.5)
    with pytest.raises(pkg.ApdError, match="apd_volume_create: 1 x 2 x 2 samples"):
        pkg.Volume((1, 2, 2), (0, 0, 0), 1.0, 1.0)
    assert L.apd_volume_destroy(None) == 0 and L.apd_mesh_destroy(None) == 0


def test_refusals_of_the_calls_on_a_volume(pkg):
    """A volume is made without a device, so everything a call refuses is refused on any machine, before a device is touched."""
    L = pkg.lib()
    plain, coloured = pkg.Volume((3, 2, 2), (0, 0, 0), 0.5, 1.0), pkg.Volume((3, 2, 2), (0, 0, 0), 0.5, 1.0, colour=True)
    assert plain.samples == 12 and coloured.colour
    good = unit_camera(pkg, 5, 4)
    depth, image = np.ones((4, 5), F), np.ones((4, 5, 3), F)
    table = lambda *arrays: (C.c_void_p * len(arrays))(*[None if a is None else a.ctypes.data for a in arrays])

    def sized(W, H):
        cam = pkg.Camera.from_buffer_copy(good)
        cam.width, cam.height = W, H
        return cam

    def refused(message, v=coloured, V=1, cams=(good,), deps=table(depth), imgs=table(image), channels=3, weights=None):
        cameras = None if cams is None else (pkg.Camera * len(cams))(*cams)
        w = None if weights is None else (C.c_float * len(weights))(*weights)
        assert L.apd_volume_integrate(None if v is None else v._v, V, cameras, deps, imgs, channels, w, 0) == -1
        assert L.apd_fusion_last_error().decode() == "apd_volume_integrate: " + message

    refused("null argument", v=None)
    refused("null argument", cams=None)
    refused("null argument", deps=None)
    refused("0 views", V=0)
    refused("-1 views", V=-1)
    refused("images for a volume without colour", v=plain)
    for channels in (0, 2, 4):
        refused("images of %d channels, not 1 or 3" % channels, channels=channels)
    refused("camera 0 has 0 x 4 pixels", cams=(sized(0, 4),))
    refused("camera 1 has 5 x -2 pixels", V=2, cams=(good, sized(5, -2)), deps=table(depth, depth), imgs=table(image, image))
    refused("camera 0 has 65536 x 32768 pixels, 2^31 or more", cams=(sized(65536, 32768),))
    refused("view 0 has a null map", deps=table(None))
    refused("view 0 has a null map", imgs=table(None))
    for bad in (0.0, -2.0, float("inf"), float("nan")):
        refused("view 0 has a weight of %g, not a positive finite number" % bad, weights=[bad])
    with pytest.raises(pkg.ApdError, match="apd_volume_integrate: 0 views"):
        coloured.integrate([], [])
    with pytest.raises(pkg.ApdError, match="apd_volume_integrate: images for a volume without colour"):
        plain.integrate([good], [depth], [image])
    with pytest.raises(ValueError, match="depth map of"):
        plain.integrate([good], [np.ones((5, 4), F)])

    buf = np.full(12 * 4, 7.0, F)
    ptr = C.c_void_p(buf.ctypes.data)
    for call, name in ((L.apd_volume_download, "apd_volume_download"), (L.apd_volume_upload, "apd_volume_upload")):
        for args, message in (((None, ptr, None, None), "null argument"), ((plain._v, None, None, None), "null argument"),
                              ((plain._v, None, None, ptr), "a colour array for a volume without colour")):
            assert call(*args) == -1 and L.apd_fusion_last_error().decode() == name + ": " + message
    assert (buf == 7.0).all()
    out = C.c_void_p(1234)
    assert L.apd_volume_extract_mesh(None, C.byref(out)) == -1 and L.apd_fusion_last_error().decode() == "apd_volume_extract_mesh: null argument"
    assert L.apd_volume_extract_mesh(plain._v, None) == -1 and out.value == 1234
    n = C.c_longlong(-7)
    assert L.apd_mesh_counts(None, C.byref(n), C.byref(n)) == -1 and L.apd_fusion_last_error().decode() == "apd_mesh_counts: null argument" and n.value == -7
    assert L.apd_mesh_download(None, ptr, None, None) == -1 and L.apd_fusion_last_error().decode() == "apd_mesh_download: null argument"
    assert L.apd_mesh_write_ply(None, b"x.ply") == -1 and L.apd_fusion_last_error().decode() == "apd_mesh_write_ply: null argument"
    plain.close()
    coloured.close()
    with pytest.raises(pkg.ApdError, match="the volume is closed"):
        plain.integrate([good], [depth])


def test_volume_around_a_box(pkg):
    v = pkg.Volume.around([0, 0, 0], [1, 2, 0.1], 0.25, 0.5)
    assert np.array_equal(v.origin, F([-0.5, -0.5, -0.5])) and v.dims == (9, 13, 6) and v.trunc == F(0.5)
    last = v.origin + (np.array(v.dims) - 1) * v.voxel
    assert (last >= F([1.5, 2.5, 0.6])).all() and (last - v.voxel < F([1.5, 2.5, 0.6])).all()
    tight = pkg.Volume.around([0, 0, 0], [0, 0, 0], 1.0, 0.5, margin=0.0, colour=True, max_weight=8)
    assert tight.dims == (2, 2, 2) and tight.colour and tight.max_weight == 8
    with pytest.raises(ValueError):
        pkg.Volume.around([0, 0, 0], [-1, 0, 0], 1.0, 0.5)


def test_no_gpu_means_the_calls_fail_loudly(pkg):
    """There is no host implementation: without a device every call that needs one is refused with a message, and outputs stay as they
    were."""
    if pkg.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = pkg.lib()
    v = pkg.Volume((3, 2, 2), (0, 0, 0), 0.5, 1.0)
    cam = unit_camera(pkg, 5, 4)
    with pytest.raises(pkg.ApdError, match="apd_volume_integrate: "):
        v.integrate([cam], [np.ones((4, 5), F)])
    with pytest.raises(pkg.ApdError, match="apd_volume_download: "):
        v.state()
    with pytest.raises(pkg.ApdError, match="apd_volume_upload: "):
        v.set_state(np.ones(12, F), np.ones(12, F))
    out = C.c_void_p(1234)
    assert L.apd_volume_extract_mesh(v._v, C.byref(out)) != 0 and L.apd_fusion_last_error().startswith(b"apd_volume_extract_mesh: ") and out.value == 1234
    with pytest.raises(pkg.ApdError):
        v.extract_mesh()
    v.close()
