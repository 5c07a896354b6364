"""The rendered maps and the rendered visibility without a device: the sequential checker (tests/helpers/points_render_ref.cpp) held
against an independent numpy restatement of contract C15 (binary32 operations written out, np.minimum.at on uint64 keys) on the small
clouds of the device tests; a planted scene of two planes whose answer is known; the refusals of apd_points_render and
apd_points_rendered_visibility; objects without points; the entry points in the header and in the library; and the loud failure
without a GPU.  The clouds and cameras of test_gpu_points_render.py are made here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import points_render_checker as PRC
from test_points_radius import dressed
from test_points_voxel import arrays_of, cloud, from_cloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("apd_points_render", "apd_points_rendered_visibility")
F = np.float32
W0, H0 = 64, 48          # the image of the size cases
SIZES = [0, 1, 63, 64, 65, 255, 256, 257]   # around a wave and around a workgroup of 256 lanes, the block of every kernel
SPLATS = (0, 1, 2, 8)
SMALL_IMAGES = [(1, 1), (1, 7), (7, 1), (5, 4)]   # width, height


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return PRC.build(tmp_path_factory.mktemp("points_render_checker"))


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# --------------------------------------------------------------------------------------------------------------------
# cameras and clouds
# --------------------------------------------------------------------------------------------------------------------

def pinhole(pkg, W, H, f=None, R=None, t=None, skew=0.0, fy=None, cx=None, cy=None):
    f = float(W) / 2 if f is None else f
    K = [f, skew, (W - 1) / 2.0 if cx is None else cx, 0, f if fy is None else fy, (H - 1) / 2.0 if cy is None else cy, 0, 0, 1]
    return pkg.make_camera(K, np.eye(3).reshape(9) if R is None else R, [0, 0, 0] if t is None else t, W, H, 0.1, 100.0)


def unit_camera(pkg, W, H):
    """K = I, R = I, t = 0: a point (x, y, 1) has u = x and w = y exactly."""
    return pkg.make_camera(np.eye(3).reshape(9), np.eye(3).reshape(9), [0, 0, 0], W, H, 0.1, 100.0)


def look_at(pkg, eye, W, H, f, skew=0.0, fy=None, roll=0.0):
    """A camera at `eye` that looks at the origin."""
    eye = np.asarray(eye, np.float64)
    z = -eye / np.linalg.norm(eye)
    x = np.cross([0.0, 1.0, 0.1], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    c, s = np.cos(roll), np.sin(roll)
    R = np.stack([c * x + s * y, -s * x + c * y, z])
    return pinhole(pkg, W, H, f, R.reshape(9), -R @ eye, skew, fy)


def ring_cameras(pkg, V, W=40, H=30):
    """V cameras on a tilted ring of radius 4 around the origin, each looking at it; every third one with skew, every second one with
    fx != fy, all with some roll."""
    cams = []
    for s in range(V):
        a = 2 * np.pi * s / V
        cams.append(look_at(pkg, [4 * np.cos(a), 1.5 * np.sin(2 * a), 4 * np.sin(a)], W, H, 28.0, skew=0.7 if s % 3 == 1 else 0.0,
                            fy=33.0 if s % 2 else None, roll=0.1 * s))
    return cams


def sphere_points(rng, n=1500):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


def frustum_points(rng, n, W=W0, H=H0, f=W0 / 2.0):
    """n points in front of pinhole(pkg, W, H): pixel coordinates from 3 outside the image to 3 outside, depths 2 .. 6 in layers."""
    u, w = rng.uniform(-3, W + 3, n), rng.uniform(-3, H + 3, n)
    d = rng.choice([2.0, 3.5, 6.0], n) + rng.uniform(0, 0.2, n)
    return np.stack([(u - (W - 1) / 2.0) / f * d, (w - (H - 1) / 2.0) / f * d, d], 1).astype(F)


def size_case(n):
    return dressed(np.random.default_rng(500 + n), frustum_points(np.random.default_rng(600 + n), n))


def pixel_points(rng, W, H, pixels=None, layers=3):
    """`layers` points at distinct depths on each pixel of a W x H image of unit_camera (or on the given (c, r) pixels), shuffled."""
    if pixels is None:
        pixels = [(c, r) for r in range(H) for c in range(W)]
    pts = []
    for c, r in pixels:
        for d in rng.uniform(1.0, 4.0, layers):
            pts.append([c * d, r * d, d])
    pts = np.array(pts, F)
    return pts[rng.permutation(len(pts))]


def long_axis_case(rng, W, H):
    """A few hundred pixels of a 16384 x 2 or 2 x 16384 image, the corners among them: the row stride."""
    pixels = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)] + [(int(rng.integers(0, W)), int(rng.integers(0, H))) for _ in range(300)]
    return pixel_points(rng, W, H, pixels, layers=2)


def contention_cases(rng, n=4096):
    """n points on pixel (2, 1) of unit_camera(5, 4): distinct depths in random order; one depth (the winner is index 0); two depths
    that are adjacent binary32 values."""
    distinct = (2.0 + rng.permutation(n) * 2.0 ** -10).astype(F)
    same = np.full(n, 3.0, F)
    adjacent = np.where(rng.integers(0, 2, n) == 1, np.nextafter(F(3), F(4)), F(3)).astype(F)
    adjacent[0] = np.nextafter(F(3), F(4))   # the first point is not the winner
    out = {}
    for name, d in (("distinct", distinct), ("same", same), ("adjacent", adjacent)):
        out[name] = np.stack([2 * d, 1 * d, d], 1).astype(F)   # 2 * d / d == 2 exactly
    return out


def not_drawn_case():
    """(xyz, drawn) for unit_camera(5, 4): depths 0, -0, negative, +inf, NaN; u or w at +-2^31 and beyond; centres outside each border;
    u + 0.5 exactly 0 and exactly the width; among points that are drawn.  int(v + 0.5f) truncates toward zero, so a centre down to
    v + 0.5 > -1 still lands on pixel 0, as in the fusion."""
    W, H = 5, 4
    big = F(2.0 ** 31)
    below = np.nextafter(big, F(0))          # the largest binary32 below 2^31: convertible, and outside the image
    rows = [  # x, y, z, drawn
        (1, 1, 0.0, False), (1, 1, -0.0, False), (1, 1, -1.0, False), (1, 1, np.inf, False), (1, 1, np.nan, False), (np.nan, 1, 1, False),
        (big, 1, 1, False), (-big, 1, 1, False), (2 * big, 1, 1, False), (1, -2 * big, 1, False), (1e20, 1, 1, False), (1, below, 1, False),
        (below, 1, 1, False), (1, big, 1, False), (1, -big, 1, False), (np.inf, 1, 1, False),
        (-1.5, 1, 1, False), (-1.0, 1, 1, True), (-0.5, 1, 1, True), (-0.25, 1, 1, True), (1, -1.5, 1, False), (1, -0.5, 1, True),
        (W - 0.5, 1, 1, False), (np.nextafter(F(W - 0.5), F(0)), 1, 1, True), (1, H - 0.5, 1, False), (1, np.nextafter(F(H - 0.5), F(0)), 1, True),
        (W, 1, 1, False), (1, H, 1, False), (W - 1, H - 1, 1, True), (0, 0, 1, True), (2, 2, 1, True), (1, 1, 0.5, True), (3e-30, 1e-30, 1e-30, True),
    ]
    a = np.array(rows, np.float64)
    return a[:, :3].astype(F), a[:, 3].astype(bool)


def two_planes(pkg, step=1):
    """(xyz, cameras, front, behind): a fronto-parallel plane at depth 5, one point on every `step`-th pixel of columns 20 .. 44 and
    rows 14 .. 34 of pinhole(64, 48), in front of a plane at depth 10 with one point on every pixel; `front`: the indices of the front
    points; `behind`: those of the back points whose pixel lies within the front plane's extent.  Three cameras: the one the planes
    face, and two to its sides that look at the planes' middle."""
    cam = pinhole(pkg, W0, H0, 32.0, cx=32.0, cy=24.0)
    pts, front, behind = [], [], []
    for r in range(14, 35, step):
        for c in range(20, 45, step):
            front.append(len(pts))
            pts.append([(c - 32) * 5 / 32.0, (r - 24) * 5 / 32.0, 5.0])
    for r in range(H0):
        for c in range(W0):
            if 20 <= c <= 44 and 14 <= r <= 34:
                behind.append(len(pts))
            pts.append([(c - 32) * 10 / 32.0, (r - 24) * 10 / 32.0, 10.0])
    cams = [cam]
    for side in (-6.0, 6.0):
        eye = np.array([side, 0.5, 0.0])
        z = np.array([0, 0, 7.5]) - eye
        z /= np.linalg.norm(z)
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        cams.append(pinhole(pkg, W0, H0, 32.0, R.reshape(9), -R @ eye))
    return np.array(pts, F), cams, np.array(front), np.array(behind)


def small_render_cases(pkg):
    """(name, xyz, camera, splats): every cloud of the device tests that the numpy restatement is run on."""
    rng = np.random.default_rng(71)
    for n in SIZES:
        yield "size %d" % n, size_case(n)[0].xyz, pinhole(pkg, W0, H0), (0, 1)
    for W, H in SMALL_IMAGES:
        yield "image %d x %d" % (W, H), pixel_points(rng, W, H), unit_camera(pkg, W, H), SPLATS
    for W, H in ((16384, 2), (2, 16384)):
        yield "image %d x %d" % (W, H), long_axis_case(rng, W, H), unit_camera(pkg, W, H), (0, 2)
    for name, xyz in contention_cases(rng).items():
        yield "contention " + name, xyz, unit_camera(pkg, 5, 4), (0, 2)
    yield "not drawn", not_drawn_case()[0], unit_camera(pkg, 5, 4), (0, 1)
    sphere = sphere_points(rng)
    for s, cam in enumerate(ring_cameras(pkg, 5)):
        yield "sphere from camera %d" % s, sphere, cam, (0, 1)
    yield "camera behind the cloud", sphere + F([0, 0, 5]), pinhole(pkg, W0, H0, R=np.diag([-1.0, 1.0, -1.0]).reshape(9)), (1,)
    xyz, cams, _, _ = two_planes(pkg, 2)
    for s, cam in enumerate(cams):
        yield "two planes from camera %d" % s, xyz, cam, (0, 1)


# --------------------------------------------------------------------------------------------------------------------
# the numpy restatement
# --------------------------------------------------------------------------------------------------------------------

def np_draw(xyz, cam):
    """(drawn bool [n], c, r int64 [n], d float32 [n]): contract C15's draw rule, every operation a binary32 one in the header's order."""
    K, R, t = [np.array(list(a), F) for a in (cam.K, cam.R, cam.t)]
    P = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        x = [((R[3 * i] * P[:, 0] + R[3 * i + 1] * P[:, 1]) + R[3 * i + 2] * P[:, 2]) + t[i] for i in range(3)]
        d = (K[6] * x[0] + K[7] * x[1]) + K[8] * x[2]
        u = ((K[0] * x[0] + K[1] * x[1]) + K[2] * x[2]) / d
        w = ((K[3] * x[0] + K[4] * x[1]) + K[5] * x[2]) / d
        assert d.dtype == F and u.dtype == F and w.dtype == F
        su, sw = u + F(0.5), w + F(0.5)
        ok = (d > 0) & (bits32(d) < 0x7f800000) & (su > F(-2.0 ** 31)) & (su < F(2.0 ** 31)) & (sw > F(-2.0 ** 31)) & (sw < F(2.0 ** 31))
        c = np.where(ok, np.trunc(np.where(ok, su, 0)), -1).astype(np.int64)
        r = np.where(ok, np.trunc(np.where(ok, sw, 0)), -1).astype(np.int64)
    ok &= (c >= 0) & (c < cam.width) & (r >= 0) & (r < cam.height)
    return ok, c, r, d


def np_keys(xyz, cam, splat):
    ok, c, r, d = np_draw(xyz, cam)
    W, H = int(cam.width), int(cam.height)
    keys = np.full(W * H, 0xFFFFFFFFFFFFFFFF, np.uint64)
    k = np.flatnonzero(ok)
    key = (bits32(d[k]).astype(np.uint64) << np.uint64(32)) | k.astype(np.uint64)
    for dr in range(-splat, splat + 1):
        for dc in range(-splat, splat + 1):
            x, y = c[k] + dc, r[k] + dr
            inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
            np.minimum.at(keys, (y * W + x)[inside], key[inside])
    return keys, (ok, c, r, d)


def np_render(xyz, cam, splat):
    keys, _ = np_keys(xyz, cam, splat)
    empty = keys == np.uint64(0xFFFFFFFFFFFFFFFF)
    depth = np.where(empty, np.uint32(0), (keys >> np.uint64(32)).astype(np.uint32)).astype(np.uint32).view(F)
    index = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    shape = (int(cam.height), int(cam.width))
    return depth.reshape(shape), index.reshape(shape)


def np_seen(xyz, cams, splat, tol):
    """bool [n, len(cams)]"""
    out = np.zeros((len(xyz), len(cams)), bool)
    for s, cam in enumerate(cams):
        keys, (ok, c, r, d) = np_keys(xyz, cam, splat)
        k = np.flatnonzero(ok)
        z = (keys[r[k] * int(cam.width) + c[k]] >> np.uint64(32)).astype(np.uint32).view(F)
        with np.errstate(all="ignore"):
            out[k, s] = (d[k] - z) <= F(tol) * z
    return out


def lists_of(seen):
    offsets = np.concatenate([[0], np.cumsum(seen.sum(1))]).astype(np.int64)
    views = np.nonzero(seen)[1].astype(np.int32)
    length = seen.sum(1)
    support = np.where(length == 0, 0, np.minimum(255, length - 1)).astype(np.uint8)
    return offsets, views, support


def assert_maps(got, want, what):
    for name, a, b in (("depth", bits32(got[0]), bits32(want[0])), ("index", np.asarray(got[1], np.uint32), np.asarray(want[1], np.uint32))):
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        differ = np.argwhere(a != b)
        assert differ.size == 0, (what, name, differ[:5], a[a != b][:5], b[a != b][:5])


def test_checker_equals_the_numpy_restatement_on_every_small_case(pkg, checker):
    drawn_somewhere = 0
    for name, xyz, cam, splats in small_render_cases(pkg):
        for splat in splats:
            want = np_render(xyz, cam, splat)
            assert_maps(PRC.render(checker, xyz, cam, splat), want, (name, splat))
            drawn_somewhere += int((want[1] != PRC.NO_INDEX).any())
            if name == "camera behind the cloud":
                assert (want[1] == PRC.NO_INDEX).all() and (bits32(want[0]) == 0).all()
    assert drawn_somewhere > 30


def test_checker_draws_what_the_not_drawn_case_says(pkg, checker):
    xyz, drawn = not_drawn_case()
    ok, _, _, _ = np_draw(xyz, unit_camera(pkg, 5, 4))
    assert np.array_equal(ok, drawn), np.flatnonzero(ok != drawn)
    lists = PRC.visibility(checker, xyz, [unit_camera(pkg, 5, 4)], 0, 1e30)
    assert np.array_equal(np.diff(lists.offsets) == 1, drawn) and lists.unseen == int((~drawn).sum())


def test_checker_contention_winners(pkg, checker):
    cam = unit_camera(pkg, 5, 4)
    cases = contention_cases(np.random.default_rng(71))
    depth, index = PRC.render(checker, cases["distinct"], cam, 0)
    assert index[1, 2] == int(np.argmin(cases["distinct"][:, 2])) and depth[1, 2] == 2.0 and (np.delete(index.ravel(), 7) == PRC.NO_INDEX).all()
    depth, index = PRC.render(checker, cases["same"], cam, 0)
    assert index[1, 2] == 0 and depth[1, 2] == 3.0
    depth, index = PRC.render(checker, cases["adjacent"], cam, 0)
    first = int(np.flatnonzero(cases["adjacent"][:, 2] == 3.0)[0])
    assert index[1, 2] == first > 0 and depth[1, 2] == 3.0
    # with a tolerance of 0 only the winner and its exact ties are seen; one binary32 step behind is not
    lists = PRC.visibility(checker, cases["adjacent"], [cam], 0, 0.0)
    assert np.array_equal(np.diff(lists.offsets) == 1, cases["adjacent"][:, 2] == 3.0)
    assert PRC.visibility(checker, cases["same"], [cam], 0, 0.0).unseen == 0


@pytest.mark.parametrize("V", [1, 32, 33, 40])
def test_checker_lists_equal_the_numpy_restatement(pkg, checker, V):
    xyz = sphere_points(np.random.default_rng(72))
    cams = ring_cameras(pkg, V)
    for splat, tol in ((1, 0.0), (1, 0.01), (0, 1e30)):
        want = lists_of(np_seen(xyz, cams, splat, tol))
        got = PRC.visibility(checker, xyz, cams, splat, tol)
        assert np.array_equal(got.offsets, want[0]) and np.array_equal(got.views, want[1]) and np.array_equal(got.support, want[2]), (V, splat, tol)
        assert got.unseen == int((np.diff(want[0]) == 0).sum())
    assert 0 < len(got.views) <= V * len(xyz)


def test_planted_two_planes(pkg, checker):
    """Drawn with footprints of 3 x 3 pixels the front plane hides every back point behind its extent from the camera the planes face,
    whether it has a point on every pixel or on every second one; drawn with single pixels the sparse front plane lets the back points
    between its samples through.  Every front point is seen."""
    for step in (1, 2):
        xyz, cams, front, behind = two_planes(pkg, step)
        closed = PRC.visibility(checker, xyz, cams[:1], 1, 0.01)
        seen = np.diff(closed.offsets) == 1
        assert seen[front].all() and not seen[behind].any(), step
        outside = np.setdiff1d(np.arange(len(xyz)), np.concatenate([front, behind]))
        assert seen[outside].sum() > 0.8 * len(outside)   # past the border of a footprint the back plane shows
        open_ = np.diff(PRC.visibility(checker, xyz, cams[:1], 0, 0.01).offsets) == 1
        assert open_[front].all()
        assert (open_[behind].sum() == 0) if step == 1 else (0.5 * len(behind) < open_[behind].sum() < len(behind))
        three = PRC.visibility(checker, xyz, cams, 1, 0.01)
        assert three.unseen < len(xyz) and len(three.views) > len(closed.views)
        assert np.array_equal(three.support, np.where(np.diff(three.offsets) == 0, 0, np.diff(three.offsets) - 1))


# --------------------------------------------------------------------------------------------------------------------
# the C ABI without a device
# --------------------------------------------------------------------------------------------------------------------

def test_header_declares_the_entry_points_as_ctypes_calls_them(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "apd_mi355x.h")).read(), flags=re.S)
    assert re.search(r"int\s+apd_points_render\s*\(\s*apd_points_t\s+\w+\s*,\s*const\s+apd_camera\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*float\s*\*\s*\w+\s*,"
                     r"\s*uint32_t\s*\*\s*\w+\s*\)", text)
    assert re.search(r"int\s+apd_points_rendered_visibility\s*\(\s*apd_points_t\s+\w+\s*,\s*int\s+\w+\s*,\s*const\s+apd_camera\s*\*\s*\w+\s*,\s*int\s+\w+\s*,"
                     r"\s*float\s+\w+\s*,\s*apd_points_t\s*\*\s*\w+\s*,\s*long\s+long\s*\*\s*\w+\s*\)", text)
    L = pkg.lib()
    assert len(L.apd_points_render.argtypes) == 5 and len(L.apd_points_rendered_visibility.argtypes) == 7


def test_library_exports_the_entry_points(pkg):
    L = pkg.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name


def one_point(pkg):
    return from_cloud(pkg, cloud([[0.5, 0.5, 5.0]]), [4], [5], [[]])


def test_refusals_that_need_no_device(pkg):
    L = pkg.lib()
    pts = one_point(pkg)
    good = unit_camera(pkg, 5, 4)
    depth, index = np.full(20, 7.0, F), np.full(20, 7, np.uint32)
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)

    def sized(W, H):
        cam = pkg.Camera.from_buffer_copy(good)
        cam.width, cam.height = W, H
        return cam

    def refused(code, message, p=pts._p, cam=good, splat=0, d=depth, i=index):
        assert L.apd_points_render(p, None if cam is None else C.byref(cam), splat, ptr(d), ptr(i)) == code
        assert L.apd_fusion_last_error().decode() == "apd_points_render: " + message
        assert (depth == 7.0).all() and (index == 7).all()

    refused(-1, "null argument", p=None)
    refused(-1, "null argument", cam=None)
    refused(-1, "null argument", d=None, i=None)
    refused(-1, "splat = -1, not in 0 .. 8", splat=-1)
    refused(-1, "splat = 9, not in 0 .. 8", splat=9)
    refused(-1, "camera 0 has 0 x 4 pixels", cam=sized(0, 4))
    refused(-1, "camera 0 has 5 x -1 pixels", cam=sized(5, -1))
    refused(-1, "camera 0 has 65536 x 32768 pixels, 2^31 or more", cam=sized(65536, 32768))

    out, unseen = C.c_void_p(1234), C.c_longlong(-7)
    cams = (pkg.Camera * 2)(good, good)

    def refused_vis(code, message, p=pts._p, cameras=cams, V=2, splat=1, tol=0.01, outp=C.byref(out)):
        assert L.apd_points_rendered_visibility(p, V, None if cameras is None else C.byref(cameras), splat, tol, outp, C.byref(unseen)) == code
        assert L.apd_fusion_last_error().decode() == "apd_points_rendered_visibility: " + message
        assert out.value == 1234 and unseen.value == -7

    refused_vis(-1, "null argument", p=None)
    refused_vis(-1, "null argument", cameras=None)
    refused_vis(-1, "null argument", outp=None)
    refused_vis(-1, "splat = 9, not in 0 .. 8", splat=9)
    refused_vis(-1, "splat = -3, not in 0 .. 8", splat=-3)
    refused_vis(-1, "0 views", V=0)
    refused_vis(-1, "-2 views", V=-2)
    refused_vis(-1, "a relative tolerance of -0.5, not a non-negative finite number", tol=-0.5)
    refused_vis(-1, "a relative tolerance of inf, not a non-negative finite number", tol=float("inf"))
    refused_vis(-1, "a relative tolerance of nan, not a non-negative finite number", tol=float("nan"))
    refused_vis(-1, "camera 1 has 0 x 4 pixels", cameras=(pkg.Camera * 2)(good, sized(0, 4)))
    refused_vis(-1, "camera 1 has 65536 x 32768 pixels, 2^31 or more", cameras=(pkg.Camera * 2)(good, sized(65536, 32768)))
    with pytest.raises(pkg.ApdError, match="apd_points_render: splat = 9"):
        pts.render(good, 9)
    with pytest.raises(pkg.ApdError, match="apd_points_rendered_visibility: 0 views"):
        pts.with_rendered_visibility([])
    pts.close()


def test_objects_without_points_give_empty_results_without_a_device(pkg, tmp_path):
    pts = from_cloud(pkg, cloud(np.zeros((0, 3), F)), [4, 4], [5, 5], [[1], [0]])
    depth, index = pts.render(unit_camera(pkg, 5, 4), 2)
    assert depth.shape == (4, 5) and depth.dtype == F and (bits32(depth) == 0).all()
    assert index.shape == (4, 5) and index.dtype == np.uint32 and (index == PRC.NO_INDEX).all()
    new, unseen = pts.with_rendered_visibility(ring_cameras(pkg, 3))
    assert new.count == 0 and unseen == 0 and new.merged and not new.on_device
    offsets, views = new.visibility()
    assert offsets.tolist() == [0] and len(views) == 0
    new.write_vis(tmp_path / "none.vis")
    assert (tmp_path / "none.vis").read_bytes() == bytes(8)
    new.close()
    pts.close()


def test_no_gpu_means_the_calls_fail_loudly(pkg):
    """There is no host implementation: without a device a non-empty host object is refused with a message, and the maps, *out and
    *unseen stay as they were."""
    if pkg.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = pkg.lib()
    pts = one_point(pkg)
    cam = unit_camera(pkg, 5, 4)
    depth, index = np.full(20, 7.0, F), np.full(20, 7, np.uint32)
    assert L.apd_points_render(pts._p, C.byref(cam), 0, C.c_void_p(depth.ctypes.data), C.c_void_p(index.ctypes.data)) != 0
    assert L.apd_fusion_last_error().startswith(b"apd_points_render: ")
    assert (depth == 7.0).all() and (index == 7).all()
    out, unseen = C.c_void_p(1234), C.c_longlong(-7)
    assert L.apd_points_rendered_visibility(pts._p, 1, C.byref(cam), 1, F(0.01), C.byref(out), C.byref(unseen)) != 0
    assert L.apd_fusion_last_error().startswith(b"apd_points_rendered_visibility: ")
    assert out.value == 1234 and unseen.value == -7
    with pytest.raises(pkg.ApdError):
        pts.render(cam)
    with pytest.raises(pkg.ApdError):
        pts.with_rendered_visibility([cam])
    pts.close()
