"""The rasterised maps, the face visibility and the removal of unseen faces without a device: the sequential checker
(tests/helpers/mesh_render_ref.cpp) held against an independent numpy restatement of contract C25 (binary32 projection written out,
int64 edge functions, binary64 depth, np.minimum on uint64 keys), bit for bit; the properties of the coverage rule and of the z-buffer
on planted meshes whose answer is known; an oblique plane against the analytic ray-plane depth; the refusals and the empty meshes
through the library.  The meshes and cameras of test_gpu_mesh_render.py are made here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mesh_checker as MC
import mesh_render_checker as RC
from test_mesh import colours_of, joined, sheet, strip
from test_points_render import bits32, look_at, np_draw, pinhole, ring_cameras, unit_camera

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("apd_mesh_render", "apd_mesh_face_visibility", "apd_mesh_remove_unseen", "apd_mesh_render_split")
F = np.float32
NO = RC.NO_FACE
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
NAN = float("nan")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return RC.build(tmp_path_factory.mktemp("mesh_render_checker"))


# --------------------------------------------------------------------------------------------------------------------
# meshes and cameras
# --------------------------------------------------------------------------------------------------------------------

def flat(points, faces, depth=2.0):
    """A mesh whose vertex (x, y) lands on pixel coordinates (x, y) of unit_camera exactly: (x, y, 1) * depth, depth a power of two."""
    P = np.asarray(points, np.float64)
    z = np.broadcast_to(np.asarray(depth, np.float64), (len(P),))
    return MC.Mesh(np.stack([P[:, 0] * z, P[:, 1] * z, z], 1).astype(F), np.asarray(faces, np.int32).reshape(-1, 3))


def rectangle(x0, y0, x1, y1, diagonal=0, depth=2.0):
    corners = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    return flat(corners, [[0, 1, 2], [0, 2, 3]] if diagonal == 0 else [[0, 1, 3], [1, 2, 3]], depth)


def pixel_fan(cx=3, cy=2, radius=2.0):
    """8 faces around a vertex that sits on the centre of pixel (cx, cy)."""
    ring = [(cx + radius * np.cos(a), cy + radius * np.sin(a)) for a in 2 * np.pi * np.arange(8) / 8]
    return flat([(cx, cy)] + ring, [[0, 1 + k, 1 + (k + 1) % 8] for k in range(8)])


def sliver():
    return flat([(2.25, -1), (2.75, -1), (2.5, 6)], [[0, 1, 2]])


def reversed_winding(mesh):
    return MC.Mesh(mesh.vertices, mesh.faces[:, [0, 2, 1]], mesh.colours)


def not_drawn():
    """(mesh, the faces that are drawn): a good rectangle among faces with a corner behind the camera, at NaN, beyond the guard band,
    and with a repeated index."""
    good = rectangle(1, 1, 5, 4)
    V = np.concatenate([good.vertices, np.array([[1, 1, -2], [NAN, 1, 2], [2.0 ** 21, 0, 2], [-2.0 ** 21, 0, 2], [6, 0, 1], [6, 4, 1]], F)])
    faces = np.array([[8, 9, 4], [0, 1, 2], [8, 9, 5], [8, 6, 9], [0, 2, 3], [7, 9, 8], [8, 8, 9], [9, 8, 9]], np.int32)
    return MC.Mesh(V, faces), [1, 4]


def huge():
    """One face far larger than any frame here, at depth 4."""
    return flat([(-1000, -1000), (3000, -1000), (-1000, 3000)], [[0, 1, 2]], 4.0)


def coplanar_copies():
    a = rectangle(0, 0, 6, 4)
    return MC.Mesh(a.vertices, np.concatenate([a.faces[::-1], a.faces, a.faces]))


def small_in_front():
    """Faces 0, 1: a rectangle over the frame at depth 4; faces 2, 3: one over [2, 4) x [1, 3) at depth 2."""
    return joined(rectangle(-1, -1, 8, 6, 0, 4.0), rectangle(2, 1, 4, 3, 1, 2.0))


def oblique_sheet(n=24, jitter=0.0):
    """A sheet of 2 (n - 1)^2 faces in the world plane z = 0, centred on the origin, 4 units wide."""
    m = sheet(n, n, jitter, spacing=4.0 / (n - 1))
    return MC.Mesh(m.vertices - F([2, 2, 0]), m.faces, colours_of(len(m.vertices)))


def oblique_camera(pkg, W=65, H=63, f=40.0):
    return look_at(pkg, [1.5, -2.0, -4.0], W, H, f, roll=0.2)


def mixed(pkg):
    """(mesh, camera 256 x 192): a sheet of sub-pixel faces, a sheet of faces of about 20 pixels and one face that fills the frame behind
    them."""
    tiny = MC.Mesh(sheet(40, 40, 0.002, spacing=0.01).vertices + F([-0.77, -0.257, 7.0]), sheet(40, 40).faces)   # 0.2-pixel faces, half of them behind `middle`
    middle = MC.Mesh(sheet(12, 10, 0.05, spacing=0.25).vertices + F([-0.5, -1.0, 6.0]), sheet(12, 10).faces)     # about 6 x 6 pixels a square
    back = MC.Mesh(np.array([[-40, -40, 8], [80, -40, 8], [-40, 80, 8]], F), np.array([[0, 1, 2]], np.int32))
    m = joined(tiny, back, middle, colour=True)
    order = np.random.default_rng(12).permutation(len(m.faces))
    return MC.Mesh(m.vertices, m.faces[order], m.colours), pinhole(pkg, 256, 192, 150.0)


def occluded_sheets():
    """Faces 0, 1: a sheet over the frame at depth 2; faces 2, 3: one behind it at depth 4, all front-facing (A2 < 0)."""
    return joined(reversed_winding(rectangle(-1, -1, 8, 6, 0, 2.0)), reversed_winding(rectangle(0, 0, 6, 4, 1, 4.0)))


def render_cases(pkg):
    """(name, mesh, camera): every mesh of the device tests that the numpy restatement is run on."""
    cam = unit_camera(pkg, 7, 5)
    for diagonal in (0, 1):
        yield "rectangle, diagonal %d" % diagonal, rectangle(1, 1, 5, 4, diagonal), cam
    yield "fan", pixel_fan(), cam
    yield "sliver", sliver(), cam
    yield "reversed", reversed_winding(rectangle(1, 1, 5, 4)), cam
    yield "not drawn", not_drawn()[0], cam
    yield "huge", huge(), cam
    yield "coplanar copies", coplanar_copies(), cam
    yield "small in front", small_in_front(), cam
    yield "occluded sheets", occluded_sheets(), cam
    for W, H in ((1, 1), (7, 5), (65, 63)):
        yield "oblique sheet in %d x %d" % (W, H), oblique_sheet(24, 0.02), oblique_camera(pkg, W, H, 0.6 * W + 1)
    for s, c in enumerate(ring_cameras(pkg, 3)):
        yield "jittered sheet from ring camera %d" % s, oblique_sheet(9, 0.05), c
    yield "mixed", *mixed(pkg)


# --------------------------------------------------------------------------------------------------------------------
# the numpy restatement
# --------------------------------------------------------------------------------------------------------------------

def np_vertices(mesh, cam):
    """(X, Y int64 [n], d float32 [n], usable bool [n]): every operation a binary32 one in the header's order."""
    K, R, t = [np.array(list(a), F) for a in (cam.K, cam.R, cam.t)]
    P = mesh.vertices
    with np.errstate(all="ignore"):
        x = [((R[3 * i] * P[:, 0] + R[3 * i + 1] * P[:, 1]) + R[3 * i + 2] * P[:, 2]) + t[i] for i in range(3)]
        d = (K[6] * x[0] + K[7] * x[1]) + K[8] * x[2]
        u = ((K[0] * x[0] + K[1] * x[1]) + K[2] * x[2]) / d
        w = ((K[3] * x[0] + K[4] * x[1]) + K[5] * x[2]) / d
        su, sw = u * F(256) + F(0.5), w * F(256) + F(0.5)
        assert su.dtype == F and sw.dtype == F and d.dtype == F
        fu, fw = np.floor(su), np.floor(sw)
        usable = (d > 0) & np.isfinite(d) & (np.abs(fu) <= F(2.0 ** 27)) & (np.abs(fw) <= F(2.0 ** 27))   # NaN compares false
    X = np.where(usable, fu, 0).astype(np.int64)
    Y = np.where(usable, fw, 0).astype(np.int64)
    return X, Y, d, usable


def np_keys(mesh, cam, cull):
    W, H = int(cam.width), int(cam.height)
    X, Y, d, usable = np_vertices(mesh, cam)
    keys = np.full((H, W), EMPTY, np.uint64)
    drawn = np.zeros(len(mesh.faces), bool)
    for f, (a, b, c) in enumerate(mesh.faces.tolist()):
        if not (usable[a] and usable[b] and usable[c]):
            continue
        A2 = (int(X[b]) - int(X[a])) * (int(Y[c]) - int(Y[a])) - (int(Y[b]) - int(Y[a])) * (int(X[c]) - int(X[a]))
        if A2 == 0 or (cull == "back" and A2 > 0):
            continue
        drawn[f] = True
        if A2 < 0:
            b, c = c, b
        v = (a, b, c)
        xs, ys = [int(X[i]) for i in v], [int(Y[i]) for i in v]
        c0, c1 = max(-((-min(xs)) // 256), 0), min(max(xs) // 256, W - 1)
        r0, r1 = max(-((-min(ys)) // 256), 0), min(max(ys) // 256, H - 1)
        if c0 > c1 or r0 > r1:
            continue
        py, px = np.meshgrid(256 * np.arange(r0, r1 + 1, dtype=np.int64), 256 * np.arange(c0, c1 + 1, dtype=np.int64), indexing="ij")
        inside = np.ones(px.shape, bool)
        E = {}
        for i, j in ((0, 1), (1, 2), (2, 0)):
            dx, dy = xs[j] - xs[i], ys[j] - ys[i]
            E[i] = dx * (py - ys[i]) - dy * (px - xs[i])
            inside &= (E[i] > 0) | ((E[i] == 0) & (dy < 0 or (dy == 0 and dx > 0)))
        w0, w1, w2 = E[1], E[2], E[0]
        S = w0 + w1 + w2
        with np.errstate(all="ignore"):
            q = (w0.astype(np.float64) / np.float64(d[v[0]]) + w1.astype(np.float64) / np.float64(d[v[1]])) + w2.astype(np.float64) / np.float64(d[v[2]])
            z = (S.astype(np.float64) / q).astype(F)
            inside &= (z > 0) & np.isfinite(z)
        key = (bits32(z).astype(np.uint64) << np.uint64(32)) | np.uint64(f)
        box = keys[r0:r1 + 1, c0:c1 + 1]
        box[inside] = np.minimum(box[inside], key[inside])
    return keys, drawn


def maps_of(keys):
    empty = keys == EMPTY
    depth = np.where(empty, np.uint32(0), (keys >> np.uint64(32)).astype(np.uint32)).astype(np.uint32).view(F)
    return depth, (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def np_render(mesh, cam, cull="none"):
    return maps_of(np_keys(mesh, cam, cull)[0])


def np_visibility(mesh, cams, cull="back", min_pixels=1, tol=0.01):
    nf = len(mesh.faces)
    views, pixels = np.zeros(nf, np.uint32), np.zeros(nf, np.uint64)
    for cam in cams:
        keys, drawn = np_keys(mesh, cam, cull)
        depth, face = maps_of(keys)
        owned = np.bincount(face[face != NO].astype(np.int64), minlength=nf)
        ok, c, r, d = np_draw(mesh.vertices, cam)   # the points' rule: d > 0 and finite, the nearest pixel inside the image
        z = np.where(ok, depth[np.where(ok, r, 0), np.where(ok, c, 0)], F(0))
        with np.errstate(all="ignore"):
            corner = ok & (z > 0) & ((d - z) <= F(tol) * z)
        seen = drawn & ((owned >= min_pixels) | corner[mesh.faces].all(1))
        views += seen.astype(np.uint32)
        pixels += owned.astype(np.uint64)
    return views, pixels, int((views == 0).sum())


def assert_maps(got, want, what):
    for name, a, b in (("depth", bits32(got[0]), bits32(want[0])), ("face", np.asarray(got[1], np.uint32), np.asarray(want[1], np.uint32))):
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        differ = np.argwhere(a != b)
        assert differ.size == 0, (what, name, differ[:5], a[a != b][:5], b[a != b][:5])


# --------------------------------------------------------------------------------------------------------------------
# the checker against the restatement and against known answers
# --------------------------------------------------------------------------------------------------------------------

def test_checker_equals_the_numpy_restatement_on_every_case(pkg, checker):
    covered = 0
    for name, mesh, cam in render_cases(pkg):
        X, Y, d, usable = np_vertices(mesh, cam)
        gX, gY, gd, gu = RC.vertices(checker, mesh, cam)
        assert np.array_equal(gu, usable), name
        assert np.array_equal(gX[usable], X[usable]) and np.array_equal(gY[usable], Y[usable]) and np.array_equal(bits32(gd[usable]), bits32(d[usable])), name
        for cull in ("none", "back"):
            got = RC.render(checker, mesh, cam, cull)
            assert_maps(got, np_render(mesh, cam, cull), (name, cull))
            covered += int((got[1] != NO).sum())
    assert covered > 20000


def test_a_rectangle_on_pixel_centres_covers_its_half_open_box_once(pkg, checker):
    cam = unit_camera(pkg, 7, 5)
    want = np.zeros((5, 7), bool)
    want[1:4, 1:5] = True
    faces = []
    for diagonal in (0, 1):
        m = rectangle(1, 1, 5, 4, diagonal)
        depth, face = RC.render(checker, m, cam)
        assert np.array_equal(face != NO, want) and np.array_equal(bits32(depth), bits32(np.where(want, F(2), F(0)))), diagonal
        assert set(face[want].tolist()) == {0, 1}
        swapped = RC.render(checker, MC.Mesh(m.vertices, m.faces[::-1]), cam)[1]
        assert np.array_equal(swapped != NO, want) and np.array_equal(swapped[want], 1 - face[want]), diagonal   # a shared edge is owned once
        faces.append(face)
    # each triangle alone covers what it owns in the pair: nothing of the diagonal is drawn twice
    for diagonal in (0, 1):
        m = rectangle(1, 1, 5, 4, diagonal)
        alone = [RC.render(checker, MC.Mesh(m.vertices, m.faces[k:k + 1]), cam)[1] != NO for k in (0, 1)]
        assert not (alone[0] & alone[1]).any() and np.array_equal(alone[0], faces[diagonal] == 0) and np.array_equal(alone[1], faces[diagonal] == 1)


def test_a_fan_owns_its_hub_pixel_once_and_a_sliver_covers_nothing(pkg, checker):
    cam = unit_camera(pkg, 7, 5)
    m = pixel_fan()
    owners = sum((RC.render(checker, MC.Mesh(m.vertices, m.faces[k:k + 1]), cam)[1] != NO).astype(int) for k in range(8))
    assert owners[2, 3] == 1 and owners.max() == 1 and owners.sum() > 8
    assert (RC.render(checker, sliver(), cam)[1] == NO).all()


def test_facing_follows_the_right_hand_normal(pkg, checker):
    cam = unit_camera(pkg, 7, 5)
    back = rectangle(1, 1, 5, 4)         # (1,1) -> (5,1) -> (5,4): its normal (b - a) x (c - a) points along +z, away from the camera
    n = np.cross(back.vertices[1] - back.vertices[0], back.vertices[2] - back.vertices[0])
    assert n[2] > 0
    front = reversed_winding(back)
    assert_maps(RC.render(checker, front, cam, "none"), RC.render(checker, back, cam, "none"), "winding")
    assert (RC.render(checker, back, cam, "back")[1] == NO).all()
    assert_maps(RC.render(checker, front, cam, "back"), RC.render(checker, front, cam, "none"), "front")
    assert (RC.render(checker, front, cam, "back")[1] != NO).sum() == 12


def test_faces_that_are_not_drawn_leave_the_rest_alone(pkg, checker):
    cam = unit_camera(pkg, 7, 5)
    m, drawn = not_drawn()
    depth, face = RC.render(checker, m, cam)
    alone = RC.render(checker, MC.Mesh(m.vertices, m.faces[drawn]), cam)
    assert np.array_equal(bits32(depth), bits32(alone[0])) and np.array_equal(face != NO, alone[1] != NO)
    assert set(face[face != NO].tolist()) == set(drawn)
    for f in range(len(m.faces)):
        if f not in drawn:
            assert (RC.render(checker, MC.Mesh(m.vertices, m.faces[f:f + 1]), cam)[1] == NO).all(), f


def test_depth_order_ties_and_a_face_larger_than_the_frame(pkg, checker):
    cam = unit_camera(pkg, 7, 5)
    depth, face = RC.render(checker, huge(), cam)
    assert (face == 0).all() and (depth == 4).all()
    face = RC.render(checker, coplanar_copies(), cam)[1]
    assert set(face[face != NO].tolist()) == {0, 1} and (face != NO).sum() == 24
    depth, face = RC.render(checker, small_in_front(), cam)
    near = np.zeros((5, 7), bool)
    near[1:3, 2:4] = True
    assert np.isin(face[near], (2, 3)).all() and np.isin(face[~near], (0, 1)).all()
    assert (depth[near] == 2).all() and (depth[~near] == 4).all()


def test_an_oblique_plane_has_the_ray_plane_depth(pkg, checker):
    """The rendered depth of the plane z = 0 against the depth at which the ray through the pixel centre meets it.  The rasteriser's
    own error is the snapping of the corners to 1/256 pixel; the largest relative error measured on the checker here is 3.74e-5, and
    the bound is four times that."""
    cam = oblique_camera(pkg, 65, 63, 40.0)
    depth, face = RC.render(checker, oblique_sheet(24), cam)
    K, R, t = np.array(list(cam.K)).reshape(3, 3), np.array(list(cam.R)).reshape(3, 3), np.array(list(cam.t))
    r, c = np.mgrid[0:63, 0:65]
    rays = np.linalg.solve(K, np.stack([c.ravel(), r.ravel(), np.ones(c.size)]).astype(np.float64))   # camera frame, z = 1
    eye, world = -R.T @ t, R.T @ rays
    want = (-eye[2] / world[2]).reshape(63, 65)
    on = face != NO
    assert on.sum() > 1000
    err = np.abs(depth[on].astype(np.float64) - want[on]) / want[on]
    print("largest relative error against the ray-plane depth: %.3g over %d pixels" % (err.max(), on.sum()))
    assert err.max() < 4 * 3.74e-5


# --------------------------------------------------------------------------------------------------------------------
# visibility and removal
# --------------------------------------------------------------------------------------------------------------------

def visibility_cases(pkg):
    cam = unit_camera(pkg, 7, 5)
    yield "occluded sheets", occluded_sheets(), [cam]
    yield "not drawn", not_drawn()[0], [cam, cam]
    yield "jittered sheet in a ring", oblique_sheet(9, 0.05), ring_cameras(pkg, 5)
    yield "mixed", mixed(pkg)[0], [mixed(pkg)[1], pinhole(pkg, 64, 48, 30.0)]


def test_checker_visibility_equals_the_numpy_restatement(pkg, checker):
    for name, mesh, cams in visibility_cases(pkg):
        for cull, min_pixels, tol in (("back", 1, 0.01), ("none", 3, 0.0), ("none", 1, 0.5)):
            got = RC.face_visibility(checker, mesh, cams, cull, min_pixels, tol)
            want = np_visibility(mesh, cams, cull, min_pixels, tol)
            assert np.array_equal(got[0], want[0]), (name, cull, min_pixels, tol, np.argwhere(got[0] != want[0])[:5])
            assert np.array_equal(got[1], want[1]) and got[2] == want[2], (name, cull, min_pixels, tol)


def test_an_occluded_sheet_is_unseen(pkg, checker):
    cam = unit_camera(pkg, 7, 5)
    views, pixels, unseen = RC.face_visibility(checker, occluded_sheets(), [cam, cam], "back", 1, 0.01)
    assert views.tolist() == [2, 2, 0, 0] and unseen == 2 and pixels[2:].tolist() == [0, 0] and pixels[:2].sum() == 70
    # with the back faces of the same sheets nothing is drawn under cull = back
    views, _, unseen = RC.face_visibility(checker, reversed_winding(occluded_sheets()), [cam], "back", 1, 0.01)
    assert views.tolist() == [0, 0, 0, 0] and unseen == 4


def test_rule_b_sees_a_sub_pixel_face_and_rule_a_a_face_with_its_corners_outside(pkg, checker):
    cam = unit_camera(pkg, 7, 5)
    speck = flat([(3.2, 2.2), (3.2, 2.4), (3.4, 2.2)], [[0, 1, 2]])          # front-facing, between the pixel centres, over a back sheet
    m = joined(reversed_winding(rectangle(-1, -1, 8, 6, 0, 2.0)), speck)
    assert (RC.render(checker, m, cam, "back")[1] != 2).all()
    views, pixels, _ = RC.face_visibility(checker, m, [cam], "back", 1, 0.01)
    assert views.tolist() == [1, 1, 1] and pixels[2] == 0                       # (b): its corners lie on the sheet's depth
    behind = joined(reversed_winding(rectangle(-1, -1, 8, 6, 0, 2.0)), flat([(3.2, 2.2), (3.2, 2.4), (3.4, 2.2)], [[0, 1, 2]], 4.0))
    assert RC.face_visibility(checker, behind, [cam], "back", 1, 0.01)[0].tolist() == [1, 1, 0]
    views, pixels, _ = RC.face_visibility(checker, reversed_winding(huge()), [cam], "back", 35, 0.01)
    assert views.tolist() == [1] and pixels.tolist() == [35]                    # (a): every corner is far outside the frame
    assert RC.face_visibility(checker, reversed_winding(huge()), [cam], "back", 36, 0.01)[0].tolist() == [0]


def test_thresholds_at_their_boundary_values(pkg, checker):
    cam = unit_camera(pkg, 7, 5)
    # corners outside the frame, so that only rule (a) counts; the face owns every pixel of the frame
    m = reversed_winding(flat([(-3, -3), (40, -3), (-3, 40)], [[0, 1, 2]]))
    owned = int(RC.face_visibility(checker, m, [cam], "back", 1, 0.0)[1][0])
    assert owned == 35
    assert RC.face_visibility(checker, m, [cam], "back", owned, 0.0)[0].tolist() == [1]
    assert RC.face_visibility(checker, m, [cam], "back", owned + 1, 0.0)[0].tolist() == [0]
    cams = ring_cameras(pkg, 5)
    mesh = oblique_sheet(9, 0.05)
    views = RC.face_visibility(checker, mesh, cams, "back")[0]
    assert views.min() < views.max() and views.max() >= 2   # the cameras on one side of the sheet see its front
    k = int(views.max())
    at, removed = RC.remove_unseen(checker, mesh, cams, k)
    assert len(at.faces) == (views >= k).sum() > 0 and removed == (views < k).sum()
    assert len(RC.remove_unseen(checker, mesh, cams, k + 1)[0].faces) == 0
    assert len(RC.remove_unseen(checker, mesh, cams, 0)[0].faces) == len(mesh.faces)


def test_removal_is_a_filter_followed_by_renumbering(pkg, checker):
    mesh, cam = mixed(pkg)
    views = RC.face_visibility(checker, mesh, [cam], "none")[0]
    out, removed = RC.remove_unseen(checker, mesh, [cam], 1, "none")
    keep = views >= 1
    assert 0 < removed == (~keep).sum() < len(mesh.faces)
    # the positions of the kept faces' corners, and their colours, are those of the input, face by face in order
    assert np.array_equal(bits32(out.vertices[out.faces]), bits32(mesh.vertices[mesh.faces[keep]]))
    assert np.array_equal(out.colours[out.faces], mesh.colours[mesh.faces[keep]])
    assert len(out.vertices) == len(np.unique(mesh.faces[keep])) and np.array_equal(np.unique(out.faces), np.arange(len(out.vertices)))
    assert (np.diff(np.unique(mesh.faces[keep])) > 0).all() and np.array_equal(bits32(out.vertices), bits32(mesh.vertices[np.unique(mesh.faces[keep])]))


# --------------------------------------------------------------------------------------------------------------------
# the C ABI without a device
# --------------------------------------------------------------------------------------------------------------------

def test_header_and_library_have_the_entry_points(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "apd_mi355x.h")).read(), flags=re.S)
    assert re.search(r"int\s+apd_mesh_render\s*\(\s*apd_mesh_t\s+\w+\s*,\s*const\s+apd_camera\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*float\s*\*\s*\w+\s*,"
                     r"\s*uint32_t\s*\*\s*\w+\s*\)", text)
    assert re.search(r"int\s+apd_mesh_face_visibility\s*\(\s*apd_mesh_t\s+\w+\s*,\s*int\s+\w+\s*,\s*const\s+apd_camera\s*\*\s*\w+\s*,\s*int\s+\w+\s*,"
                     r"\s*unsigned\s+\w+\s*,\s*float\s+\w+\s*,\s*uint32_t\s*\*\s*\w+\s*,\s*uint64_t\s*\*\s*\w+\s*,\s*long\s+long\s*\*\s*\w+\s*\)", text)
    assert re.search(r"int\s+apd_mesh_remove_unseen\s*\(\s*apd_mesh_t\s+\w+\s*,\s*int\s+\w+\s*,\s*const\s+apd_camera\s*\*\s*\w+\s*,\s*int\s+\w+\s*,"
                     r"\s*unsigned\s+\w+\s*,\s*float\s+\w+\s*,\s*unsigned\s+\w+\s*,\s*apd_mesh_t\s*\*\s*\w+\s*,\s*long\s+long\s*\*\s*\w+\s*,"
                     r"\s*long\s+long\s*\*\s*\w+\s*\)", text)
    assert re.search(r"void\s+apd_mesh_render_split\s*\(\s*int\s+\w+\s*\)", text)
    assert re.search(r"APD_RENDER_CULL_NONE\s*=\s*0\s*,\s*APD_RENDER_CULL_BACK\s*=\s*1", text)
    L = pkg.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    assert len(L.apd_mesh_render.argtypes) == 5 and len(L.apd_mesh_face_visibility.argtypes) == 9 and len(L.apd_mesh_remove_unseen.argtypes) == 10


def empty_mesh(pkg):
    return pkg.Mesh.from_arrays(np.zeros((0, 3), F), np.zeros((0, 3), np.int32))


def test_refusals_that_need_no_device(pkg):
    L = pkg.lib()
    m = empty_mesh(pkg)
    good = unit_camera(pkg, 5, 4)
    depth, face = np.full(20, 7.0, F), np.full(20, 7, np.uint32)
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)

    def sized(W, H):
        cam = pkg.Camera.from_buffer_copy(good)
        cam.width, cam.height = W, H
        return cam

    def refused(message, mesh=m._m, cam=good, cull=0, d=depth, i=face):
        assert L.apd_mesh_render(mesh, None if cam is None else C.byref(cam), cull, ptr(d), ptr(i)) == -1
        assert L.apd_fusion_last_error().decode() == "apd_mesh_render: " + message
        assert (depth == 7.0).all() and (face == 7).all()

    refused("null argument", mesh=None)
    refused("null argument", cam=None)
    refused("every output is null", d=None, i=None)
    refused("cull mode 2, neither APD_RENDER_CULL_NONE nor APD_RENDER_CULL_BACK", cull=2)
    refused("cull mode -1, neither APD_RENDER_CULL_NONE nor APD_RENDER_CULL_BACK", cull=-1)
    refused("camera 0 has 0 x 4 pixels", cam=sized(0, 4))
    refused("camera 0 has 5 x -1 pixels", cam=sized(5, -1))
    refused("camera 0 has 65536 x 32768 pixels, 2^31 or more", cam=sized(65536, 32768))

    cams = (pkg.Camera * 2)(good, good)
    views, pixels, unseen = np.full(1, 7, np.uint32), np.full(1, 7, np.uint64), C.c_longlong(-7)
    out, gone = C.c_void_p(1234), C.c_longlong(-7)

    def both(message, mesh=m._m, cameras=cams, V=2, cull=1, min_pixels=1, tol=0.01):
        cp = None if cameras is None else C.byref(cameras)
        assert L.apd_mesh_face_visibility(mesh, V, cp, cull, min_pixels, tol, ptr(views), ptr(pixels), C.byref(unseen)) == -1
        assert L.apd_fusion_last_error().decode() == "apd_mesh_face_visibility: " + message
        assert L.apd_mesh_remove_unseen(mesh, V, cp, cull, min_pixels, tol, 1, C.byref(out), C.byref(gone), None) == -1
        assert L.apd_fusion_last_error().decode() == "apd_mesh_remove_unseen: " + message
        assert views[0] == 7 and pixels[0] == 7 and unseen.value == -7 and out.value == 1234 and gone.value == -7

    both("null argument", mesh=None)
    both("null argument", cameras=None)
    both("cull mode 5, neither APD_RENDER_CULL_NONE nor APD_RENDER_CULL_BACK", cull=5)
    both("min_pixels = 0, not at least 1", min_pixels=0)
    both("a relative tolerance of -0.5, not a non-negative finite number", tol=-0.5)
    both("a relative tolerance of inf, not a non-negative finite number", tol=float("inf"))
    both("a relative tolerance of nan, not a non-negative finite number", tol=float("nan"))
    both("0 views", V=0)
    both("-2 views", V=-2)
    both("camera 1 has 0 x 4 pixels", cameras=(pkg.Camera * 2)(good, sized(0, 4)))
    both("camera 1 has 65536 x 32768 pixels, 2^31 or more", cameras=(pkg.Camera * 2)(good, sized(65536, 32768)))
    assert L.apd_mesh_face_visibility(m._m, 2, C.byref(cams), 1, 1, 0.01, None, None, None) == -1
    assert L.apd_fusion_last_error().decode() == "apd_mesh_face_visibility: every output is null"
    assert L.apd_mesh_remove_unseen(m._m, 2, C.byref(cams), 1, 1, 0.01, 1, None, None, None) == -1
    assert L.apd_fusion_last_error().decode() == "apd_mesh_remove_unseen: null argument"
    with pytest.raises(pkg.ApdError, match="apd_mesh_render: camera 0 has 0 x 4 pixels"):
        m.render(sized(0, 4))
    with pytest.raises(ValueError, match="cull"):
        m.render(good, "front")
    with pytest.raises(pkg.ApdError, match="apd_mesh_face_visibility: 0 views"):
        m.face_visibility([])
    with pytest.raises(pkg.ApdError, match="apd_mesh_remove_unseen: min_pixels = 0"):
        m.remove_unseen([good], min_pixels=0)
    m.close()


def test_a_mesh_without_faces_gives_empty_results_without_a_device(pkg):
    m = empty_mesh(pkg)
    depth, face = m.render(unit_camera(pkg, 5, 4))
    assert depth.shape == (4, 5) and depth.dtype == F and (bits32(depth) == 0).all()
    assert face.shape == (4, 5) and face.dtype == np.uint32 and (face == NO).all()
    views, pixels = m.face_visibility(ring_cameras(pkg, 3))
    assert views.shape == (0,) and views.dtype == np.uint32 and pixels.shape == (0,) and pixels.dtype == np.uint64 and m.unseen == 0
    out = m.remove_unseen(ring_cameras(pkg, 33), 2)
    assert len(out.vertices) == 0 and len(out.faces) == 0 and out.removed_faces == 0 and m.removed_faces == 0
    pkg.lib().apd_mesh_render_split(1)
    pkg.lib().apd_mesh_render_split(0)
    out.close()
    m.close()


def test_pipeline_mesh_checks_trim_before_anything_runs(pkg):
    import inspect

    from apd_mvs_amd import pipeline
    sig = inspect.signature(pipeline.mesh)
    assert sig.parameters["trim"].default is None and sig.parameters["depth_maps"].default is False
    with pytest.raises(ValueError, match="trim"):
        pipeline.mesh(None, None, None, 0.1, trim=(1, 2))
