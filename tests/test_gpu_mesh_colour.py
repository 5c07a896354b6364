"""apd_mesh_colour_from_views on the device (csrc/apd_mesh_colour.hip, contract C26), bitwise against the sequential checker
(tests/helpers/mesh_colour_ref.cpp): the colours, the per-vertex view counts and the number of uncoloured vertices, each call run twice
for the same bytes, with the input read back unchanged; images on the host and on the device, of one and of three channels, cameras of
different sizes in one call, inputs with and without colour and normals; and the chain through pipeline.mesh and the drop-in binary.
The meshes and the checker's own tests: test_mesh_colour.py."""
import subprocess

import numpy as np
import pytest

import fusion_cases
import mesh_checker as MC
import mesh_colour_checker as CC
from test_gpu_dropin_binary import APD_BIN, _write_dense_folder
from test_gpu_fusion_options import _read_dmb, _scene
from test_gpu_mesh_render import last_timing, sort_tile
from test_mesh import F, joined, strip
from test_mesh_colour import colour_cases, noise
from test_mesh_render import mixed, oblique_camera, oblique_sheet, reversed_winding
from test_points_render import pinhole, ring_cameras

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return CC.build(tmp_path_factory.mktemp("mesh_colour_checker"))


def on_device(images):
    import torch
    return [torch.from_numpy(a).to("cuda:0") for a in images]


def check_colour(pkg, checker, mesh, cams, images, what, tol=0.01, min_cos=0.1, places=("host", "device"), normals=False):
    """The device call against the checker on colours, views and uncoloured, twice per place of the images; returns the checker's."""
    m = pkg.Mesh.from_arrays(mesh.vertices, mesh.faces, mesh.colours)
    held = MC.Mesh(mesh.vertices, mesh.faces, mesh.colours)
    if normals:
        plain, m = m, m.with_vertex_normals()
        plain.close()
        held = MC.of(m)
    want, views, uncoloured = CC.colour_from_views(checker, held, cams, images, tol, min_cos)
    for place in places:
        given = on_device(images) if place == "device" else images
        for again in (0, 1):
            got = m.colour_from_views(cams, given, tol, min_cos)
            assert got.colours is not None and got.colours.dtype == np.uint8 and got.coloured_views.dtype == np.uint32
            MC.assert_mesh_equal(MC.of(got), want, (what, place, again))
            assert np.array_equal(got.coloured_views, views), (what, place, again, np.argwhere(got.coloured_views != views)[:5])
            assert got.uncoloured == uncoloured and m.uncoloured == uncoloured, (what, place, again)
            got.close()
    m.refresh()
    MC.assert_mesh_equal(MC.of(m), held, (what, "input"))
    m.close()
    return want, views, uncoloured


def test_every_cpu_case_on_the_device(gpu_pkg, checker):
    coloured = 0
    for name, mesh, cams, images, tol, min_cos in colour_cases(gpu_pkg):
        want, views, uncoloured = check_colour(gpu_pkg, checker, mesh, cams, images, name, tol, min_cos)
        coloured += len(views) - uncoloured
    assert coloured > 400


def test_counts_at_the_wave_block_and_sort_tile_edges(gpu_pkg, checker):
    """Strips of n vertices seen obliquely, as in test_gpu_mesh_render.py: every one-lane-per-vertex kernel at its block edges, with
    both raster kernels feeding the depth map."""
    cam = pinhole(gpu_pkg, 65, 63, 50.0)
    image = noise(cam)
    for n in (63, 64, 65, 255, 256, 257, sort_tile(gpu_pkg) + 1):
        base = strip(n - 5)   # n - 3 vertices, every one on the strip's border: behind it a face that fills the frame, so that every tap has a depth
        back = MC.Mesh(np.array([[-300, -300, 60], [-300, 600, 60], [600, -300, 60]], F), np.array([[0, 1, 2]], np.int32))
        mesh = joined(MC.Mesh(base.vertices * F([120.0 / n, 30.0, 1.0]) + F([-30, -15, 50]), base.faces), back, colour=True)
        assert len(mesh.vertices) == n
        gpu_pkg.lib().apd_mesh_render_split(8)   # both kernels draw
        try:
            _, views, uncoloured = check_colour(gpu_pkg, checker, mesh, [cam], [image], ("strip", n), 0.05, 0.0)
        finally:
            gpu_pkg.lib().apd_mesh_render_split(0)
        assert n - uncoloured >= n - 8, (n, uncoloured)   # the strip faces the camera: all but the vertices at its two ends and the face behind


def test_1_2_and_33_views_sizes_channels_places_colour_and_normals(gpu_pkg, checker):
    sheet_ = oblique_sheet(17, 0.05)
    most = 0
    for V in (1, 2, 33):
        cams = ring_cameras(gpu_pkg, V)
        for s, cam in enumerate(cams):   # cameras of different sizes in one call: the buffers are sized for the largest
            if s % 3 == 1:
                grown = ring_cameras(gpu_pkg, V, 56, 42)[s]
                cams[s] = grown
        for channels in (1, 3):
            images = [noise(c, channels, seed=s) for s, c in enumerate(cams)]
            for mesh in (sheet_, MC.Mesh(sheet_.vertices, sheet_.faces)):   # with and without colour
                _, views, _ = check_colour(gpu_pkg, checker, mesh, cams, images, ("ring", V, channels, mesh.colours is not None), 0.05)
                assert views.max() <= V
                most = max(most, int(views.max()))
    assert most > 4
    mesh, cam = mixed(gpu_pkg)
    mesh = reversed_winding(mesh)   # towards the camera
    cams = [cam, oblique_camera(gpu_pkg), pinhole(gpu_pkg, 64, 48, 40.0)]
    images = [noise(c, 3, seed=s) for s, c in enumerate(cams)]
    plain = check_colour(gpu_pkg, checker, mesh, cams, images, "mixed", 0.02)
    carried = check_colour(gpu_pkg, checker, mesh, cams, images, "mixed with normals", 0.02, normals=True)
    assert carried[0].normals is not None and plain[0].normals is None
    assert np.array_equal(plain[0].colours, carried[0].colours) and np.array_equal(plain[1], carried[1]) and plain[2] == carried[2]
    assert 0 < plain[2] < len(mesh.vertices)
    # a mesh with vertices and no faces: nothing is drawn, every vertex keeps its colour
    loose = MC.Mesh(mesh.vertices[:70], np.zeros((0, 3), np.int32), mesh.colours[:70])
    want, views, uncoloured = check_colour(gpu_pkg, checker, loose, cams, images, "no faces")
    assert uncoloured == 70 and np.array_equal(want.colours, loose.colours)


def test_last_timing_reports_the_call(gpu_pkg):
    mesh, cam = mixed(gpu_pkg)
    m = gpu_pkg.Mesh.from_arrays(mesh.vertices, mesh.faces, mesh.colours)
    empty = gpu_pkg.Mesh.from_arrays(np.zeros((0, 3), F), np.zeros((0, 3), np.int32))
    for images in ([noise(cam)], on_device([noise(cam)])):
        empty.colour_from_views([cam], images).close()
        assert last_timing(gpu_pkg) == [0.0, 0.0, 0.0]
        m.colour_from_views([cam], images).close()
        setup, work, file_ = last_timing(gpu_pkg)
        assert setup > 0.0 and work > 0.0 and file_ == 0.0, (setup, work, file_)
    m.close()
    empty.close()


def test_through_the_pipeline(gpu_pkg, checker, tmp_path):
    from apd_mvs_amd import pipeline
    case = fusion_cases.case("mixed_sizes")
    scene, results = _scene(gpu_pkg, pipeline, case)
    voxel = 0.05
    options = gpu_pkg.default_fusion_options(factor_strong=0.0, factor_weak=0.0)
    _, points = pipeline.fuse(scene, results, None, options=options, return_points=True)
    _, _, plain = pipeline.mesh(scene, results, None, voxel, bounds=points, options=options, return_mesh=True, normals=True)
    nv, nf, got = pipeline.mesh(scene, results, tmp_path / "recoloured.ply", voxel, bounds=points, options=options, return_mesh=True, normals=True, recolour=True)
    assert plain.colours is not None and got.colours is not None and (nv, nf) == (len(plain.vertices), len(plain.faces))
    geometry = lambda m: MC.Mesh(m.vertices, m.faces, None, m.normals)
    MC.assert_mesh_equal(geometry(got), geometry(plain), "the colourless volume gives the same surface")
    cams, imgs = pipeline.mesh_views(scene, results, None)
    want, views, uncoloured = CC.colour_from_views(checker, geometry(plain), cams, imgs)
    MC.assert_mesh_equal(MC.of(got), want, "recolour=True")
    assert (tmp_path / "recoloured.ply").read_bytes() == MC.ply_bytes(want)
    coloured = views > 0
    difference = np.abs(want.colours[coloured].astype(np.int32) - plain.colours[coloured].astype(np.int32))
    nx, ny, nz = [int(np.ceil((hi - lo + 8 * voxel) / voxel)) + 1 for lo, hi in zip(*pipeline.mesh_bounds(points))]
    print("recolour: %d of %d vertices uncoloured (%.1f %%); median |recoloured - volume colour| = %.1f levels over %d vertices; a volume of "
          "%d x %d x %d samples is %d bytes without colour and %d with" % (uncoloured, len(views), 100.0 * uncoloured / len(views), float(np.median(difference)),
                                                                            coloured.sum(), nx, ny, nz, 8 * nx * ny * nz, 24 * nx * ny * nz))
    assert coloured.any()
    _, _, tuned = pipeline.mesh(scene, results, None, voxel, bounds=points, options=options, return_mesh=True, recolour=(0.05, 0.3))
    want2 = CC.colour_from_views(checker, MC.Mesh(tuned.vertices, tuned.faces), cams, imgs, 0.05, 0.3)[0]
    MC.assert_mesh_equal(MC.of(tuned), want2, "recolour=(0.05, 0.3)")
    for m in (plain, got, tuned):
        m.close()
    points.close()


def test_binary_recolours(gpu_pkg, synth, tmp_path):
    """--mesh 0.05 --mesh-recolour: APD.ply.mesh holds the bytes of pipeline.mesh(recolour=True) on the run's own maps; without the flag
    the bytes of pipeline.mesh(); the flag without --mesh and a malformed value end with the usage line."""
    from apd_mvs_amd import pipeline
    folder = tmp_path / "dense"
    folder.mkdir()
    _write_dense_folder(folder, synth, 96, 72, 4)
    base = [APD_BIN, str(folder), "0", "--seed", "21", "--iters", "1", "--keep-maps", "--mesh", "0.05"]
    r = subprocess.run(base, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "All done" in r.stdout and "recoloured" not in r.stdout, r.stdout[-2000:]
    scene = pipeline.load_dense_folder(str(folder), gpu_pkg.Camera)
    results = {}
    for v in range(scene.num_views):
        d = folder / "APD" / ("%08d" % scene.ids[v])
        results[v] = pipeline.ViewState(_read_dmb(d / "depths.dmb"), _read_dmb(d / "normals.dmb"), _read_dmb(d / "weak.bin"), _read_dmb(d / "selected_views.bin"))
    colour = pipeline.load_colour_images(str(folder), scene.ids[:scene.num_views])
    _, _, plain = pipeline.mesh(scene, results, None, 0.05, colour_images=colour, return_mesh=True)
    assert (folder / "APD" / "APD.ply.mesh").read_bytes() == MC.ply_bytes(MC.of(plain))
    nv, nf, want = pipeline.mesh(scene, results, tmp_path / "recoloured.ply", 0.05, colour_images=colour, return_mesh=True, recolour=True)
    r = subprocess.run(base + ["--mesh-recolour"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "All done" in r.stdout, r.stdout[-2000:]
    assert (folder / "APD" / "APD.ply.mesh").read_bytes() == (tmp_path / "recoloured.ply").read_bytes()
    assert "%d vertices, %d left uncoloured" % (nv, want.uncoloured) in r.stdout and nv > want.uncoloured, r.stdout[-1500:]
    nv2, _, want2 = pipeline.mesh(scene, results, tmp_path / "tuned.ply", 0.05, colour_images=colour, return_mesh=True, recolour=(0.05, 0.3))
    r = subprocess.run(base + ["--mesh-recolour", "0.05,0.3"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and (folder / "APD" / "APD.ply.mesh").read_bytes() == (tmp_path / "tuned.ply").read_bytes(), r.stdout[-1500:]
    bad = subprocess.run(base + ["--mesh-recolour", "x"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert bad.returncode != 0 and "bad value 'x' of --mesh-recolour" in bad.stdout and "USAGE" in bad.stdout
    bad = subprocess.run(base + ["--mesh-recolour", "0.01,1"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert bad.returncode != 0 and "bad value '0.01,1' of --mesh-recolour" in bad.stdout and "USAGE" in bad.stdout
    alone = subprocess.run([APD_BIN, str(folder), "0", "--mesh-recolour"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert alone.returncode != 0 and "--mesh-recolour changes the mesh of --mesh VOXEL[,TRUNC]: not without it" in alone.stdout and "USAGE" in alone.stdout
    for m in (plain, want, want2):
        m.close()
