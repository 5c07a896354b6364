"""The colouring of a mesh's vertices from the views that see them without a device: the sequential checker
(tests/helpers/mesh_colour_ref.cpp, contract C26) against facts that can be derived -- an affine image is its own bilinear
interpolation, a sheet behind another is hidden from the camera in front of both, a footprint that leaves the image takes nothing, a
cosine on either side of min_cos -- and the refusals and the empty meshes through the library.  The meshes, cameras and images of
test_gpu_mesh_colour.py are made here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mesh_checker as MC
import mesh_colour_checker as CC
from test_mesh import colours_of, joined, sheet
from test_mesh_render import flat, oblique_sheet, reversed_winding
from test_points_render import look_at, pinhole, ring_cameras, unit_camera

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAN = float("nan")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return CC.build(tmp_path_factory.mktemp("mesh_colour_checker"))


@pytest.fixture(scope="module")
def mesh_lib(tmp_path_factory):
    return MC.build(tmp_path_factory.mktemp("mesh_checker"))


# --------------------------------------------------------------------------------------------------------------------
# meshes, cameras and images
# --------------------------------------------------------------------------------------------------------------------

RAMP = ((0.5, 2.0, 1.25), (200.0, -1.5, -0.75), (30.0, 0.25, 3.0))   # per channel a, b, c of a + b * column + c * row: 0 .. 255 on 65 x 63


def ramp(cam, channels=3):
    """An image that is an affine function of the pixel position in every channel, every value a binary32 number."""
    r, c = np.mgrid[0:int(cam.height), 0:int(cam.width)].astype(np.float64)
    img = np.stack([a + b * c + k * r for a, b, k in RAMP], -1)
    assert img.min() >= 0 and img.max() <= 255 and np.array_equal(img, img.astype(F))
    return np.ascontiguousarray(img if channels == 3 else img[..., 0], F)


def ramp_at(u, w):
    return np.stack([a + b * u + k * w for a, b, k in RAMP], -1)


def noise(cam, channels=3, seed=5):
    """A random image with values beyond 0 .. 255 at a few places, so that the clamp is reached."""
    shape = (int(cam.height), int(cam.width)) + ((3,) if channels == 3 else ())
    return np.random.default_rng(seed + int(cam.width)).uniform(-20.0, 275.0, shape).astype(F)


def grid(nx, ny, x0, y0, depth, step=1.0):
    """A front-facing sheet whose vertex (i, j) lands on pixel coordinates (x0 + i * step, y0 + j * step) of unit_camera exactly."""
    m = sheet(nx, ny, spacing=step)
    return reversed_winding(flat(m.vertices[:, :2].astype(np.float64) + [x0, y0], m.faces, depth))


def fronto_sheet():
    """A sheet parallel to the image of pinhole(pkg, 65, 63, 50.0), 5 in front of it, facing it, no vertex on a pixel centre."""
    m = sheet(12, 10, spacing=0.25)
    return reversed_winding(MC.Mesh(m.vertices + F([-2.03, -1.51, 5.0]), m.faces, colours_of(len(m.vertices))))


def two_sheets(colour=True):
    """(mesh, far vertices [11, 15] by (row, column)): a far sheet at depth 4 whose vertex (i, j) is at pixel (i + 0.5, j + 0.5) of
    unit_camera(16, 12), and after it a near sheet at depth 2 over [5, 8] x [3, 6]: it covers the pixel centres 5 .. 7 x 3 .. 5.  With
    a focal length of one pixel the cosines at the frame's far corner fall below 0.1: these cases run with min_cos = 0."""
    far, near = grid(15, 11, 0.5, 0.5, 4.0), grid(4, 4, 5.0, 3.0, 2.0)
    return joined(far, near, colour=colour), np.arange(15 * 11).reshape(11, 15)


def side_camera(pkg):
    """unit_camera(16, 12) moved to (20, 12, 0): the near sheet of two_sheets() is left of and above its frame, and the far vertices
    that the near sheet hides from the origin land on (0.5 .. 2.5, 0.5 .. 2.5)."""
    return pinhole(pkg, 16, 12, 1.0, t=[-20.0, -12.0, 0.0], cx=0.0, cy=0.0)


PROBES = ((7.0, 2.0, 0), (6.5, 2.0, 1), (7.5, 2.0, 0), (-0.5, 2.0, 0), (0.0, 2.0, 1), (2.0, 5.0, 0), (2.0, 4.5, 1), (2.0, 5.5, 0), (2.0, -0.25, 0),
          (2.0, 0.0, 1), (6.0, 4.0, 1), (3.0e9, 2.0, 0), (2.0, -3.0e9, 0), (NAN, 2.0, 0))   # u, w in unit_camera(8, 6), and the samples


def probes():
    """(mesh, probe vertices): a face over the whole frame of unit_camera(8, 6) at depth 4 and, at depth 2 in front of it, one small
    front-facing face per entry of PROBES whose first corner is at the entry's (u, w)."""
    back = reversed_winding(flat([(-1000, -1000), (3000, -1000), (-1000, 3000)], [[0, 1, 2]], 4.0))
    small = [reversed_winding(flat([(u, w), (u + 0.25, w), (u, w + 0.25)], [[0, 1, 2]], 2.0)) for u, w, _ in PROBES]
    return joined(back, *small), 3 + 3 * np.arange(len(PROBES))


def with_loose_vertex(mesh):
    """One more vertex that no face names, in front of the middle of the mesh."""
    V = np.concatenate([mesh.vertices, mesh.vertices.mean(0, keepdims=True) + F([0, 0, 0.01])])
    return MC.Mesh(V, mesh.faces, None if mesh.colours is None else np.concatenate([mesh.colours, [[1, 2, 3]]]).astype(np.uint8))


GRAZING_TOLERANCE = 0.5   # at 70 degrees and 40 pixels a unit the sheet's depth changes by 7 % from one pixel to the next: rule 4 at 0.01 takes nearly no vertex


def grazing_camera(pkg):
    """Sees oblique_sheet() (normal +z) at about 70 degrees from its normal."""
    return look_at(pkg, [3.5, 0.3, 1.3], 65, 63, 40.0)


def colour_cases(pkg):
    """(name, mesh, cameras, images, rel_tolerance, min_cos): every mesh of the CPU tests, for the device tests to repeat."""
    cam = pinhole(pkg, 65, 63, 50.0)
    yield "ramp", fronto_sheet(), [cam], [ramp(cam)], 0.01, 0.1
    yield "ramp, one channel", fronto_sheet(), [cam], [ramp(cam, 1)], 0.01, 0.1
    front, side = unit_camera(pkg, 16, 12), side_camera(pkg)
    for colour in (True, False):
        yield "two sheets, colour %d" % colour, two_sheets(colour)[0], [front], [noise(front)], 0.01, 0.0
        yield "two sheets and the side camera, colour %d" % colour, two_sheets(colour)[0], [front, side], [noise(front), noise(side, seed=6)], 0.01, 0.0
    small = unit_camera(pkg, 8, 6)
    yield "probes", probes()[0], [small], [noise(small)], 0.01, 0.1
    graze = grazing_camera(pkg)
    yield "grazing", with_loose_vertex(oblique_sheet(12)), [graze], [noise(graze)], GRAZING_TOLERANCE, 0.3
    behind = look_at(pkg, [1.0, 0.5, -4.0], 65, 63, 40.0)
    yield "from behind", with_loose_vertex(oblique_sheet(12)), [behind, graze], [noise(behind, 1), noise(graze, 1)], GRAZING_TOLERANCE, 0.0


# --------------------------------------------------------------------------------------------------------------------
# the rule
# --------------------------------------------------------------------------------------------------------------------

def test_an_affine_image_colours_every_vertex_with_the_function_at_its_projection(pkg, checker, mesh_lib):
    mesh, cam = fronto_sheet(), pinhole(pkg, 65, 63, 50.0)
    got, views, uncoloured = CC.colour_from_views(checker, mesh, [cam], [ramp(cam)])
    u, w, d, c = CC.geometry(checker, MC.with_normals(mesh_lib, mesh), cam)
    assert (d > 0).all() and (c > 0.85).all()
    inner = np.zeros((10, 12), bool)
    inner[1:-1, 1:-1] = True
    assert (views[inner.ravel()] == 1).all() and uncoloured == int((views == 0).sum()) <= 2 * (10 + 12)
    want = ramp_at(u, w)
    coloured = views > 0
    error = np.abs(got.colours[coloured].astype(np.float64) - want[coloured])
    print("largest |colour - function| = %.4f levels over %d vertices" % (error.max(), coloured.sum()))
    assert error.max() <= 1.0   # half a level of rounding to a byte, and the binary32 steps may land on either side of a .5
    assert np.array_equal(got.colours[~coloured], mesh.colours[~coloured])
    assert np.array_equal(got.vertices.view(np.uint32), mesh.vertices.view(np.uint32)) and np.array_equal(got.faces, mesh.faces) and got.normals is None
    # one channel is its three copies
    one = ramp(cam, 1)
    a = CC.colour_from_views(checker, mesh, [cam], [one])
    b = CC.colour_from_views(checker, mesh, [cam], [np.stack([one] * 3, -1)])
    assert np.array_equal(a[0].colours, b[0].colours) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert np.array_equal(a[0].colours[coloured, 0], got.colours[coloured, 0]) and (a[0].colours[coloured, 0] == a[0].colours[coloured, 2]).all()


def test_a_sheet_behind_another_is_coloured_only_by_the_camera_that_sees_past_it(pkg, checker):
    front, side = unit_camera(pkg, 16, 12), side_camera(pkg)
    j, i = np.mgrid[0:11, 0:15]   # far vertex (i, j) has c0 = i, r0 = j: its footprint is the pixels i | i + 1, j | j + 1
    touches = (i + 1 >= 5) & (i <= 7) & (j + 1 >= 3) & (j <= 5)      # a tap under the near sheet: 5 .. 7 x 3 .. 5
    wholly = (i >= 5) & (i + 1 <= 7) & (j >= 3) & (j + 1 <= 5)
    border = (i == 0) | (j == 0) | (i == 14) | (j == 10)   # the far sheet spans 0.5 .. 14.5 x 0.5 .. 10.5: the pixel centres of columns 0 and 15 and of rows 0 and 11 lie outside it
    assert wholly.sum() == 4 and (touches & ~wholly).sum() == 12
    for colour in (True, False):
        mesh, far = two_sheets(colour)
        got, views, uncoloured = CC.colour_from_views(checker, mesh, [front], [noise(front)], min_cos=0.0)
        fv = views[far]
        assert (fv[touches] == 0).all() and (fv[~touches & ~border] == 1).all() and (fv[border] == 0).all()
        hidden = far[touches]
        assert np.array_equal(got.colours[hidden], mesh.colours[hidden] if colour else np.zeros((len(hidden), 3), np.uint8))
        assert uncoloured == int((views == 0).sum())
        both, views2, _ = CC.colour_from_views(checker, mesh, [front, side], [noise(front), noise(side, seed=6)], min_cos=0.0)
        reach = touches & (i >= 5) & (j >= 3)   # far vertex (i, j) is at (i - 4.5, j - 2.5) in the side camera: the others are outside its frame
        assert reach.sum() == 9 and (views2[far][reach] == 1).all() and (views2[far][touches & ~reach] == 0).all() and (views2 >= views).all()
        seen_twice = views2 == 2
        assert seen_twice.any() and (views2[views == 1] >= 1).all()
        only_side = CC.colour_from_views(checker, mesh, [side], [noise(side, seed=6)], min_cos=0.0)
        assert np.array_equal(both.colours[far[reach]], only_side[0].colours[far[reach]])   # the front view gave them nothing


def test_a_footprint_that_leaves_the_image_takes_no_sample(pkg, checker):
    mesh, at = probes()
    cam = unit_camera(pkg, 8, 6)
    got, views, _ = CC.colour_from_views(checker, mesh, [cam], [noise(cam)])
    u, w, d, _ = CC.geometry(checker, MC.Mesh(mesh.vertices, mesh.faces, None, np.zeros_like(mesh.vertices)), cam)
    for k, (pu, pw, samples) in enumerate(PROBES):
        if np.isfinite(pu):
            assert u[at[k]] == F(pu) and w[at[k]] == F(pw) and d[at[k]] == 2.0, k   # exactly: cols - 1 is cols - 1
        assert views[at[k]] == samples, (k, pu, pw)
    assert (got.colours[at[views[at] == 0]] == 0).all()


def test_the_cosine_decides_on_either_side_of_min_cos(pkg, checker, mesh_lib):
    mesh = with_loose_vertex(oblique_sheet(12))
    loose = len(mesh.vertices) - 1
    normals = MC.with_normals(mesh_lib, mesh)
    assert (normals.normals[loose] == 0).all() and (normals.normals[:loose, 2] > 0.99).all()
    cam = grazing_camera(pkg)
    c = CC.geometry(checker, normals, cam)[3]
    _, views, _ = CC.colour_from_views(checker, mesh, [cam], [noise(cam)], GRAZING_TOLERANCE, 0.0)
    assert views[loose] == 0 and views.sum() > 60
    pick = int(np.flatnonzero(views)[len(np.flatnonzero(views)) // 2])
    assert 0.2 < c[pick] < 0.5, c[pick]
    below = np.nextafter(F(c[pick]), F(0)) if float(F(c[pick])) >= c[pick] else F(c[pick])       # the largest binary32 number < c
    above = np.nextafter(below, F(1))                                                             # the smallest >= c
    assert float(below) < c[pick] <= float(above)
    for min_cos, taken in ((below, 1), (above, 0)):
        got = CC.colour_from_views(checker, mesh, [cam], [noise(cam)], GRAZING_TOLERANCE, min_cos)[1]
        assert got[pick] == taken and (c[got > 0] > float(min_cos)).all() and np.array_equal(got > 0, (views > 0) & (c > float(min_cos))), min_cos
    # the same bits whether the normals are the mesh's own or made by the call
    own = CC.colour_from_views(checker, normals, [cam], [noise(cam)], GRAZING_TOLERANCE, 0.3)
    made = CC.colour_from_views(checker, mesh, [cam], [noise(cam)], GRAZING_TOLERANCE, 0.3)
    assert np.array_equal(own[0].colours, made[0].colours) and np.array_equal(own[1], made[1]) and own[0].normals is not None and made[0].normals is None
    # from behind no cosine is positive
    behind = look_at(pkg, [1.0, 0.5, -4.0], 65, 63, 40.0)
    got, views, uncoloured = CC.colour_from_views(checker, mesh, [behind], [noise(behind)], GRAZING_TOLERANCE, 0.0)
    assert (views == 0).all() and uncoloured == len(mesh.vertices) and np.array_equal(got.colours, mesh.colours)
    assert (CC.geometry(checker, normals, behind)[3][:loose] < 0).all()


# --------------------------------------------------------------------------------------------------------------------
# the C ABI without a device
# --------------------------------------------------------------------------------------------------------------------

def empty_mesh(pkg):
    return pkg.Mesh.from_arrays(np.zeros((0, 3), F), np.zeros((0, 3), np.int32))


def test_header_and_library_have_the_entry_point(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "apd_mi355x.h")).read(), flags=re.S)
    assert re.search(r"int\s+apd_mesh_colour_from_views\s*\(\s*apd_mesh_t\s+\w+\s*,\s*int\s+\w+\s*,\s*const\s+apd_camera\s*\*\s*\w+\s*,"
                     r"\s*const\s+float\s*\*\s*const\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*float\s+\w+\s*,\s*float\s+\w+\s*,"
                     r"\s*apd_mesh_t\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*,\s*long\s+long\s*\*\s*\w+\s*\)", text)
    L = pkg.lib()
    assert hasattr(L, "apd_mesh_colour_from_views") and len(L.apd_mesh_colour_from_views.argtypes) == 11


def test_refusals_that_need_no_device(pkg):
    L = pkg.lib()
    m = empty_mesh(pkg)
    good = unit_camera(pkg, 5, 4)
    image = np.zeros((4, 5, 3), F)
    cams = (pkg.Camera * 2)(good, good)
    table = (C.c_void_p * 2)(image.ctypes.data, image.ctypes.data)
    views, none, out = np.full(1, 7, np.uint32), C.c_longlong(-7), C.c_void_p(1234)

    def sized(W, H):
        cam = pkg.Camera.from_buffer_copy(good)
        cam.width, cam.height = W, H
        return cam

    def refused(message, mesh=m._m, cameras=cams, images=table, V=2, channels=3, tol=0.01, min_cos=0.1, result=out):
        rc = L.apd_mesh_colour_from_views(mesh, V, None if cameras is None else C.byref(cameras), images, channels, 0, tol, min_cos,
                                          None if result is None else C.byref(result), C.c_void_p(views.ctypes.data), C.byref(none))
        assert rc == -1 and L.apd_fusion_last_error().decode() == "apd_mesh_colour_from_views: " + message
        assert views[0] == 7 and none.value == -7 and out.value == 1234

    refused("null argument", mesh=None)
    refused("null argument", cameras=None)
    refused("null argument", images=None)
    refused("null argument", result=None)
    refused("view 1 has no image", images=(C.c_void_p * 2)(image.ctypes.data, None))
    refused("0 views", V=0)
    refused("-3 views", V=-3)
    refused("images of 2 channels, not 1 or 3", channels=2)
    refused("images of 0 channels, not 1 or 3", channels=0)
    refused("a relative tolerance of -0.5, not a non-negative finite number", tol=-0.5)
    refused("a relative tolerance of inf, not a non-negative finite number", tol=float("inf"))
    refused("a relative tolerance of nan, not a non-negative finite number", tol=NAN)
    refused("a min_cos of -0.25, not in [0, 1)", min_cos=-0.25)
    refused("a min_cos of 1, not in [0, 1)", min_cos=1.0)
    refused("a min_cos of nan, not in [0, 1)", min_cos=NAN)
    refused("a min_cos of inf, not in [0, 1)", min_cos=float("inf"))
    refused("camera 1 has 0 x 4 pixels", cameras=(pkg.Camera * 2)(good, sized(0, 4)))
    refused("camera 0 has 5 x -1 pixels", cameras=(pkg.Camera * 2)(sized(5, -1), good))
    refused("camera 1 has 65536 x 32768 pixels, 2^31 or more", cameras=(pkg.Camera * 2)(good, sized(65536, 32768)))
    with pytest.raises(pkg.ApdError, match="apd_mesh_colour_from_views: a min_cos of 1, not in"):
        m.colour_from_views([good], [image], min_cos=1.0)
    with pytest.raises(pkg.ApdError, match="apd_mesh_colour_from_views: 0 views"):
        m.colour_from_views([], [])
    with pytest.raises(ValueError, match="2 cameras, 1 images"):
        m.colour_from_views([good, good], [image])
    with pytest.raises(ValueError, match="view 0 has an image of"):
        m.colour_from_views([good], [np.zeros((5, 4, 3), F)])
    assert m.uncoloured is None
    m.close()


def test_a_mesh_without_vertices_gives_an_empty_coloured_mesh_without_a_device(pkg):
    m = empty_mesh(pkg)
    assert m.colours is None
    cams = ring_cameras(pkg, 3)
    for channels in (1, 3):
        out = m.colour_from_views(cams, [noise(c, channels) for c in cams])
        assert out.colours is not None and out.colours.shape == (0, 3) and out.colours.dtype == np.uint8 and out.normals is None
        assert len(out.vertices) == 0 and len(out.faces) == 0 and out.uncoloured == 0 and m.uncoloured == 0
        assert out.coloured_views.shape == (0,) and out.coloured_views.dtype == np.uint32
        ms = (C.c_double * 3)()
        pkg.lib().apd_fusion_last_timing(C.byref(ms, 0), C.byref(ms, 8), C.byref(ms, 16))
        assert list(ms) == [0.0, 0.0, 0.0]
        out.close()
    m.close()


def test_pipeline_mesh_checks_recolour_before_anything_runs(pkg):
    import inspect

    from apd_mvs_amd import pipeline
    sig = inspect.signature(pipeline.mesh)
    assert sig.parameters["recolour"].default is None and list(sig.parameters)[-1] == "recolour"
    for bad in ((0.01,), (0.01, 0.1, 3), False, 0.01):
        with pytest.raises(ValueError, match="recolour"):
            pipeline.mesh(None, None, None, 0.1, recolour=bad)
