"""apd_mesh_render, apd_mesh_face_visibility and apd_mesh_remove_unseen on the device (csrc/apd_mesh_render.hip, contract C25), bitwise
against the sequential checker (tests/helpers/mesh_render_ref.cpp): every map, count and trimmed mesh, each run twice for the same
bytes, with the input read back unchanged; every split between the lane-per-face and the wave-per-face kernel for the same bytes; and
the chain through pipeline.mesh and the drop-in binary.  The meshes and the checker's own tests: test_mesh_render.py."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import fusion_cases
import mesh_checker as MC
import mesh_render_checker as RC
from test_gpu_dropin_binary import APD_BIN, _write_dense_folder
from test_gpu_fusion_options import _read_dmb, _scene
from test_mesh import F, colours_of, strip
from test_mesh_render import NO, assert_maps, mixed, oblique_camera, oblique_sheet, render_cases, visibility_cases
from test_points_render import pinhole, ring_cameras, unit_camera

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return RC.build(tmp_path_factory.mktemp("mesh_render_checker"))


def device_mesh(pkg, mesh):
    return pkg.Mesh.from_arrays(mesh.vertices, mesh.faces, mesh.colours)


def unchanged(m, mesh, what):
    m.refresh()
    MC.assert_mesh_equal(MC.of(m), MC.Mesh(mesh.vertices, mesh.faces, mesh.colours), (what, "input"))


def check_render(pkg, checker, mesh, cam, what, culls=("none", "back")):
    m = device_mesh(pkg, mesh)
    drawn = 0
    for cull in culls:
        want = RC.render(checker, mesh, cam, cull)
        for again in (0, 1):
            got = m.render(cam, cull)
            assert got[0].dtype == F and got[1].dtype == np.uint32
            assert_maps(got, want, (what, cull, again))
        drawn += int((want[1] != NO).sum())
    unchanged(m, mesh, what)
    m.close()
    return drawn


def check_visibility(pkg, checker, mesh, cams, what, settings=(("back", 1, 0.01),), min_views=(1,)):
    m = device_mesh(pkg, mesh)
    for cull, min_pixels, tol in settings:
        want = RC.face_visibility(checker, mesh, cams, cull, min_pixels, tol)
        for again in (0, 1):
            views, pixels = m.face_visibility(cams, cull, min_pixels, tol)
            assert views.dtype == np.uint32 and pixels.dtype == np.uint64
            assert np.array_equal(views, want[0]), (what, cull, min_pixels, tol, again, np.argwhere(views != want[0])[:5])
            assert np.array_equal(pixels, want[1]) and m.unseen == want[2], (what, cull, min_pixels, tol, again)
        for k in min_views:
            trimmed, removed = RC.remove_unseen(checker, mesh, cams, k, cull, min_pixels, tol)
            for again in (0, 1):
                got = m.remove_unseen(cams, k, cull, min_pixels, tol)
                MC.assert_mesh_equal(MC.of(got), trimmed, (what, "trimmed", k, again))
                assert got.removed_faces == removed and m.removed_faces == removed
                got.close()
    unchanged(m, mesh, what)
    m.close()
    return want


def sort_tile(pkg):
    t, s = C.c_int(0), C.c_int(0)
    pkg.lib().apd_sort_tile_sizes(C.byref(t), C.byref(s))
    return t.value


def test_every_cpu_case_on_the_device(gpu_pkg, checker):
    drawn = sum(check_render(gpu_pkg, checker, mesh, cam, name) for name, mesh, cam in render_cases(gpu_pkg))
    assert drawn > 20000


def test_counts_at_the_wave_block_and_sort_tile_edges(gpu_pkg, checker):
    """Strips of n faces (n + 2 vertices) and of n vertices, seen obliquely: the scan of the large flags and every one-lane-per-face or
    per-vertex kernel at its block edges."""
    cam = pinhole(gpu_pkg, 65, 63, 50.0)
    tile = sort_tile(gpu_pkg)
    for n in (63, 64, 65, 255, 256, 257, tile + 1):
        for faces in (n, n - 2):
            base = strip(faces)
            # 60 pixels wide and 30 high at depth 50, whatever the count: faces from 30 pixels down to slivers between the pixel columns
            mesh = MC.Mesh(base.vertices * F([120.0 / (faces + 2), 30.0, 1.0]) + F([-30, -15, 50]), base.faces, colours_of(len(base.vertices)))
            gpu_pkg.lib().apd_mesh_render_split(8)   # both kernels draw
            try:
                assert check_render(gpu_pkg, checker, mesh, cam, ("strip", faces)) > 0
            finally:
                gpu_pkg.lib().apd_mesh_render_split(0)
    check_visibility(gpu_pkg, checker, MC.Mesh(mesh.vertices, mesh.faces, mesh.colours), [cam, unit_camera(gpu_pkg, 7, 5)], "strip", (("none", 1, 0.01),))


def test_every_split_gives_the_same_bytes(gpu_pkg, checker):
    mesh, cam = mixed(gpu_pkg)
    want = [RC.render(checker, mesh, cam, cull) for cull in ("none", "back")]
    assert len(np.unique(want[0][1])) > 200 and (want[0][1] != NO).all()
    seen = RC.face_visibility(checker, mesh, [cam, oblique_camera(gpu_pkg)], "none", 2, 0.01)
    m = device_mesh(gpu_pkg, mesh)
    try:
        for split in (1, 2 ** 30, 0, 40):
            gpu_pkg.lib().apd_mesh_render_split(split)
            for k, cull in enumerate(("none", "back")):
                assert_maps(m.render(cam, cull), want[k], ("split", split, cull))
            views, pixels = m.face_visibility([cam, oblique_camera(gpu_pkg)], "none", 2, 0.01)
            assert np.array_equal(views, seen[0]) and np.array_equal(pixels, seen[1]) and m.unseen == seen[2], split
    finally:
        gpu_pkg.lib().apd_mesh_render_split(0)
    m.close()


def test_a_face_that_fills_a_larger_frame_is_sliced_over_many_waves(gpu_pkg, checker):
    """1280 x 960: the face's box has 19200 tiles, so the large kernel runs with the most slices; in front of it a sheet of faces of
    every size between the two kernels."""
    cam = pinhole(gpu_pkg, 1280, 960, 700.0)
    sheet_ = oblique_sheet(40, 0.01)
    front = MC.Mesh(sheet_.vertices * F([0.6, 0.9, 1]) + F([0.1, -0.2, 3.0]), sheet_.faces)
    back = np.array([[-30, -30, 10], [90, -30, 10], [-30, 90, 10]], F)
    mesh = MC.Mesh(np.concatenate([back, front.vertices]), np.concatenate([[[0, 1, 2]], front.faces + 3]).astype(np.int32))
    assert check_render(gpu_pkg, checker, mesh, cam, "sliced", ("none",)) == 1280 * 960


def last_timing(pkg):
    ms = (C.c_double * 3)()
    pkg.lib().apd_fusion_last_timing(C.byref(ms, 0), C.byref(ms, 8), C.byref(ms, 16))
    return list(ms)


def test_last_timing_reports_the_three_calls(gpu_pkg):
    """Set-up and work are reported, the file time is 0, as after the other mesh calls; a call that touches no device reports zeros."""
    mesh, cam = mixed(gpu_pkg)
    m = device_mesh(gpu_pkg, mesh)
    calls = (lambda: m.render(cam), lambda: m.face_visibility([cam, cam]), lambda: m.remove_unseen([cam], 1).close())
    for call in calls:
        gpu_pkg.Mesh.from_arrays(np.zeros((0, 3), F), np.zeros((0, 3), np.int32)).render(cam)
        assert last_timing(gpu_pkg) == [0.0, 0.0, 0.0]
        call()
        setup, work, file_ = last_timing(gpu_pkg)
        assert setup > 0.0 and work > 0.0 and file_ == 0.0, (setup, work, file_)
    m.close()


def test_visibility_and_removal_over_1_2_and_33_cameras(gpu_pkg, checker):
    mesh = oblique_sheet(17, 0.05)
    for V in (1, 2, 33):
        cams = ring_cameras(gpu_pkg, V)
        want = check_visibility(gpu_pkg, checker, mesh, cams, ("ring", V), (("back", 1, 0.01), ("none", 4, 0.0)), (1, max(1, V // 3), V + 1))
        assert want[0].max() <= V
    assert want[0].max() > 8
    for name, mesh, cams in visibility_cases(gpu_pkg):
        check_visibility(gpu_pkg, checker, mesh, cams, name, (("back", 1, 0.01), ("none", 3, 0.0)), (1, 2))
    # colours and normals are carried: the trimmed mesh of a mesh with normals has the kept vertices' normals, bit for bit
    mesh, cam = mixed(gpu_pkg)
    m = device_mesh(gpu_pkg, mesh).with_vertex_normals()
    with_normals = MC.of(m)
    assert with_normals.normals is not None and with_normals.colours is not None
    got = m.remove_unseen([cam], 1, "none")
    want, removed = RC.remove_unseen(checker, with_normals, [cam], 1, "none")
    MC.assert_mesh_equal(MC.of(got), want, "with normals")
    assert got.removed_faces == removed > 0 and got.normals is not None
    empty = m.remove_unseen([cam], 2, "none")
    assert len(empty.faces) == 0 and len(empty.vertices) == 0 and empty.removed_faces == len(mesh.faces)
    for x in (got, empty, m):
        x.close()


def test_through_the_pipeline(gpu_pkg, checker, tmp_path):
    from apd_mvs_amd import pipeline
    case = fusion_cases.case("mixed_sizes")
    scene, results = _scene(gpu_pkg, pipeline, case)
    voxel = 0.05
    options = gpu_pkg.default_fusion_options(factor_strong=0.0, factor_weak=0.0)
    _, points = pipeline.fuse(scene, results, None, options=options, return_points=True)
    nv, nf, plain, rendered = pipeline.mesh(scene, results, tmp_path / "plain.ply", voxel, bounds=points, options=options, return_mesh=True, depth_maps=True)
    assert (tmp_path / "plain.ply").read_bytes() == MC.ply_bytes(MC.of(plain)) and nf == len(plain.faces) > 20
    maps = pipeline.filter_maps(scene, results, options=options)
    cams, _ = pipeline.mesh_views(scene, results, None)
    assert len(rendered) == scene.num_views
    for v in range(scene.num_views):
        want = RC.render(checker, MC.of(plain), cams[v])[0]
        assert np.array_equal(rendered[v].view(np.uint32), want.view(np.uint32)), v
        filtered = np.asarray(maps[v].depth, F)
        both = (rendered[v] > 0) & (filtered > 0)
        assert both.sum() > 1000, (v, both.sum())   # every view of the scene looks at the surface the volume was built from
        median = float(np.median(np.abs(rendered[v][both] - filtered[both])))
        print("view %d: median |rendered - filtered| = %.4g over %d pixels, voxel %.3g" % (v, median, both.sum(), voxel))
        assert median < voxel, (v, median)
    # trim = 1 removes faces, and none that owns a pixel in any view
    views, pixels, unseen = RC.face_visibility(checker, MC.of(plain), cams, "back", 1, 0.01)
    want, removed = RC.remove_unseen(checker, MC.of(plain), cams, 1)
    assert removed == unseen >= 1 and (pixels[views == 0] == 0).all()
    nv, nf, got = pipeline.mesh(scene, results, tmp_path / "trim.ply", voxel, bounds=points, options=options, return_mesh=True, trim=1)
    MC.assert_mesh_equal(MC.of(got), want, "trim = 1")
    assert (nv, nf) == (len(want.vertices), len(want.faces)) and (tmp_path / "trim.ply").read_bytes() == MC.ply_bytes(want)
    want3, _ = RC.remove_unseen(checker, MC.of(plain), cams, 2, "back", 3, 0.02)
    _, _, got3 = pipeline.mesh(scene, results, None, voxel, bounds=points, options=options, return_mesh=True, trim=(2, 3, 0.02))
    MC.assert_mesh_equal(MC.of(got3), want3, "trim = (2, 3, 0.02)")
    for m in (plain, got, got3):
        m.close()
    points.close()


def test_binary_trims_and_writes_the_rendered_depth_maps(gpu_pkg, synth, checker, tmp_path):
    """--mesh-trim 1 --mesh-depth-maps: APD.ply.mesh holds the bytes of pipeline.mesh(trim=1) on the run's own maps and every view has a
    depths_mesh.dmb, the checker's rendering of that mesh; with neither flag the mesh file is the untrimmed one and no map is written."""
    from apd_mvs_amd import pipeline
    folder = tmp_path / "dense"
    folder.mkdir()
    _write_dense_folder(folder, synth, 96, 72, 4)
    base = [APD_BIN, str(folder), "0", "--seed", "21", "--iters", "1", "--keep-maps", "--mesh", "0.05"]
    r = subprocess.run(base, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "All done" in r.stdout, r.stdout[-2000:]
    scene = pipeline.load_dense_folder(str(folder), gpu_pkg.Camera)
    results = {}
    for v in range(scene.num_views):
        d = folder / "APD" / ("%08d" % scene.ids[v])
        assert not (d / "depths_mesh.dmb").exists()
        results[v] = pipeline.ViewState(_read_dmb(d / "depths.dmb"), _read_dmb(d / "normals.dmb"), _read_dmb(d / "weak.bin"), _read_dmb(d / "selected_views.bin"))
    colour = pipeline.load_colour_images(str(folder), scene.ids[:scene.num_views])
    _, _, plain = pipeline.mesh(scene, results, None, 0.05, colour_images=colour, return_mesh=True)
    assert (folder / "APD" / "APD.ply.mesh").read_bytes() == MC.ply_bytes(MC.of(plain))
    nv, nf, trimmed = pipeline.mesh(scene, results, tmp_path / "trim.ply", 0.05, colour_images=colour, return_mesh=True, trim=1)
    assert nf < len(plain.faces)
    r = subprocess.run(base + ["--mesh-trim", "1", "--mesh-depth-maps"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "All done" in r.stdout, r.stdout[-2000:]
    assert (folder / "APD" / "APD.ply.mesh").read_bytes() == (tmp_path / "trim.ply").read_bytes()
    line = "Mesh without the faces that fewer than 1 of %d views see: %d vertices and %d faces -> %d vertices and %d faces" % (
        scene.num_views, len(plain.vertices), len(plain.faces), nv, nf)
    assert line in r.stdout, r.stdout[-1500:]
    cams, _ = pipeline.mesh_views(scene, results, colour)
    for v in range(scene.num_views):
        got = _read_dmb(folder / "APD" / ("%08d" % scene.ids[v]) / "depths_mesh.dmb")
        want = RC.render(checker, MC.of(trimmed), cams[v])[0]
        assert got.dtype == F and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), v
        assert (got > 0).any()
    bad = subprocess.run(base + ["--mesh-trim", "0"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert bad.returncode != 0 and "bad value '0' of --mesh-trim" in bad.stdout and "USAGE" in bad.stdout
    alone = subprocess.run([APD_BIN, str(folder), "0", "--mesh-depth-maps"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert alone.returncode != 0 and "--mesh-depth-maps renders the mesh of --mesh VOXEL[,TRUNC]: not without it" in alone.stdout and "USAGE" in alone.stdout
    plain.close()
    trimmed.close()
