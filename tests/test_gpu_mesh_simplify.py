"""apd_mesh_simplify on the device (csrc/apd_mesh_simplify.hip, contract C23), bitwise against the sequential checker
(tests/helpers/mesh_simplify_ref.cpp) for both placements, each run twice for the same bytes.  The meshes and the checker's own
tests: test_mesh_simplify.py.  The face sort always takes its two passes (the rotated triple is 96 bits), so every case here covers
them; no case needs 2^21 clusters."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import fusion_cases
import mesh_checker as MC
import mesh_simplify_checker as SC
from test_gpu_dropin_binary import APD_BIN, _write_dense_folder
from test_gpu_fusion_options import _read_dmb, _scene
from test_mesh import F, colours_of, fan, islands, joined, moved, octahedron, sheet, soup, strip, with_count
from test_mesh_simplify import PLACEMENTS, np_rotated, sphere_rms, structure
from test_volume import sphere_field

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return SC.build(tmp_path_factory.mktemp("mesh_simplify_checker"))


@pytest.fixture(scope="module")
def cleaner(tmp_path_factory):
    return MC.build(tmp_path_factory.mktemp("mesh_checker"))


def device_mesh(pkg, mesh):
    return pkg.Mesh.from_arrays(mesh.vertices, mesh.faces, mesh.colours)


def check(pkg, checker, mesh, cell, origin=None, what="", placements=PLACEMENTS):
    """Both placements against the checker, twice each; the counts of the C call; the input stays as it was.  Returns the checker's
    results."""
    m = device_mesh(pkg, mesh)
    L = pkg.lib()
    wants = {}
    for placement in placements:
        want = SC.simplify(checker, mesh, cell, origin, placement)
        for again in (0, 1):
            got = m.simplify(cell, origin=origin, placement=placement)
            MC.assert_mesh_equal(MC.of(got), want, (what, placement, again))
            got.close()
        out, nv, nf = C.c_void_p(), C.c_longlong(-1), C.c_longlong(-1)
        org = None if origin is None else (C.c_float * 3)(*[float(x) for x in origin])
        assert L.apd_mesh_simplify(m._m, float(cell), org, SC.PLACEMENTS[placement], C.byref(out), C.byref(nv), C.byref(nf)) == 0
        assert (nv.value, nf.value) == (len(mesh.vertices) - len(want.vertices), len(mesh.faces) - len(want.faces)), (what, placement)
        L.apd_mesh_destroy(out)
        structure(mesh, want, cell, origin)
        wants[placement] = want
    m.refresh()
    MC.assert_mesh_equal(MC.of(m), MC.Mesh(mesh.vertices, mesh.faces, mesh.colours), (what, "input"))
    m.close()
    return wants


def sort_tile(pkg):
    t, s = C.c_int(0), C.c_int(0)
    pkg.lib().apd_sort_tile_sizes(C.byref(t), C.byref(s))
    return t.value


def test_counts_at_the_wave_block_and_sort_tile_edges(gpu_pkg, checker):
    tile = sort_tile(gpu_pkg)
    for n in (63, 64, 65, 255, 256, 257, tile - 1, tile, tile + 1):
        for what in (0, 1):   # n vertices, n faces
            mesh = with_count(n, what)
            assert (len(mesh.vertices), len(mesh.faces))[what] == n
            check(gpu_pkg, checker, mesh, 0.8, (0.1, 0.2, 0.3), (n, what))
    # and as many corners as the tile, one below and one above it where 3 divides them
    for corners in (tile - 2, tile + 1):
        check(gpu_pkg, checker, with_count(corners // 3, 1), 1.3, None, ("corners", corners))


def test_a_fan_whose_hub_run_of_corners_crosses_a_sort_tile(gpu_pkg, checker):
    """The hub and its neighbours on the cone's top in one cell: more than a tile of corners in one run."""
    mesh = fan(3 * sort_tile(gpu_pkg) // 2)
    want = check(gpu_pkg, checker, mesh, 0.7, (-0.35, -0.35, 0.1), "fan")["quadric"]
    assert 0 < len(want.faces) < len(mesh.faces)


def test_a_cluster_of_many_members_and_clusters_of_one(gpu_pkg, checker):
    many = sheet(20, 20, 0.3, spacing=0.05)   # 400 vertices in about one cell of 1.5, with neighbours: the member sum's order
    mesh = joined(moved(many, [0.2, 0.2, 0.75]), moved(sheet(6, 6, 0.2), [3.0, 0, 0.75]), colour=True)
    inside = ((mesh.vertices >= 0) & (mesh.vertices < 1.5)).all(1)
    assert inside.sum() > 256
    check(gpu_pkg, checker, mesh, 1.5, None, "many members")
    ones = sheet(18, 17, 0.2)   # 306 clusters of one member each: nothing goes
    want = check(gpu_pkg, checker, ones, 0.5, (0.25, 0.25, 0.25), "one member each")
    assert len(want["mean"].vertices) == 306 and np.array_equal(want["mean"].faces, ones.faces)
    MC.assert_mesh_equal(want["mean"], ones, "mean of one")


def test_the_shuffled_strip_and_islands(gpu_pkg, checker):
    for shuffled in (False, True):
        check(gpu_pkg, checker, strip(5000, shuffled), 1.7, None, ("strip", shuffled))
    check(gpu_pkg, checker, islands(300, 2000), 2.0, None, "islands")


def test_duplicates_outside_vertices_colour_normals_and_negative_cells(gpu_pkg, checker, cleaner):
    a = moved(sheet(9, 9, 0.05), [0.3, 0.3, 0.5])
    one = check(gpu_pkg, checker, a, 2.0, None, "one sheet")["mean"]
    two = check(gpu_pkg, checker, joined(a, moved(a, [0, 0, 0.1])), 2.0, None, "two sheets of one orientation")["mean"]
    assert np.array_equal(two.faces, one.faces)
    flipped = MC.Mesh(a.vertices + F([0, 0, 0.1]), a.faces[:, ::-1].copy())
    both = check(gpu_pkg, checker, joined(a, flipped, colour=True), 2.0, None, "two sheets of opposite orientation")["quadric"]
    assert len(both.faces) == 2 * len(one.faces)
    base = sheet(12, 11, 0.1)
    bad = MC.Mesh(np.concatenate([base.vertices, [[100, 100, 100]]]).astype(F), base.faces, colours_of(len(base.vertices) + 1))   # one unreferenced
    bad.vertices[27, 2] = np.nan
    bad.vertices[3, 0] = -5e6
    bad.vertices[60, 1] = np.inf
    want = check(gpu_pkg, checker, bad, 2.0, None, "nan, outside, unreferenced, colour")["quadric"]
    assert np.isfinite(want.vertices).all() and len(want.faces) > 0
    check(gpu_pkg, checker, moved(base, [-50, -60, -70]), 2.0, (0.5, 0.25, 0.125), "negative cells")
    for placement in PLACEMENTS:   # all in one cell, and all outside the grid
        got = device_mesh(gpu_pkg, moved(sheet(5, 5, 0.0, spacing=0.1), [0.05, 0.05, 0.05])).simplify(1.0, placement=placement)
        assert got.vertices.shape == (0, 3) and got.faces.shape == (0, 3) and got.normals is None
        got = device_mesh(gpu_pkg, MC.Mesh(np.full((3, 3), np.nan, F), np.array([[0, 1, 2]], np.int32))).simplify(1.0, placement=placement)
        assert got.vertices.shape == (0, 3) and got.faces.shape == (0, 3)
        got = device_mesh(gpu_pkg, MC.Mesh(base.vertices, np.zeros((0, 3), np.int32))).simplify(1.0, placement=placement)
        assert got.vertices.shape == (0, 3) and got.faces.shape == (0, 3)
        # normals in, none out
        shaded = device_mesh(gpu_pkg, base).with_vertex_normals()
        got = shaded.simplify(2.0, placement=placement)
        assert shaded.normals is not None and got.normals is None
        MC.assert_mesh_equal(MC.of(got), SC.simplify(checker, base, 2.0, None, placement), "normals in")


def test_a_mesh_of_seventy_thousand_faces_at_two_cell_sizes(gpu_pkg, checker):
    mesh = sheet(190, 186, 0.2)
    assert len(mesh.faces) == 69930
    for cell in (1.5, 4.0):
        want = check(gpu_pkg, checker, mesh, cell, None, cell)["quadric"]
        assert 100 < len(want.faces) < len(mesh.faces)


def test_device_arrays_in(gpu_pkg, checker):
    import torch
    L = gpu_pkg.lib()
    mesh = sheet(30, 28, 0.2)
    xyz, idx = torch.from_numpy(mesh.vertices).cuda(), torch.from_numpy(mesh.faces).cuda()
    torch.cuda.synchronize()
    out = C.c_void_p()
    assert L.apd_mesh_create(0, len(mesh.vertices), C.c_void_p(xyz.data_ptr()), None, len(mesh.faces), C.c_void_p(idx.data_ptr()), 1, C.byref(out)) == 0
    m = gpu_pkg.Mesh(out)
    for placement in PLACEMENTS:
        MC.assert_mesh_equal(MC.of(m.simplify(2.5, placement=placement)), SC.simplify(checker, mesh, 2.5, None, placement), placement)


def test_chains_with_the_cleaning_calls(gpu_pkg, checker, cleaner):
    mesh = joined(soup(islands(40, 500), colour=False), moved(soup(octahedron()), [30, 0, 0]), colour=True)
    for placement in PLACEMENTS:
        got = device_mesh(gpu_pkg, mesh).weld(1e-3).simplify(2.0, placement=placement).with_vertex_normals()
        want = MC.with_normals(cleaner, SC.simplify(checker, MC.weld(cleaner, mesh, 1e-3), 2.0, None, placement))
        MC.assert_mesh_equal(MC.of(got), want, ("weld, simplify, normals", placement))
        assert want.normals is not None and 0 < len(want.faces) < len(mesh.faces)
        got = device_mesh(gpu_pkg, mesh).simplify(0.9, placement=placement).remove_small_components(5)
        want = MC.remove_small(cleaner, SC.simplify(checker, mesh, 0.9, None, placement), 5)
        MC.assert_mesh_equal(MC.of(got), want, ("simplify, remove", placement))


def test_the_sphere_of_a_device_volume(gpu_pkg, checker):
    grid, tsdf, weight = sphere_field((24, 22, 20), 7.0)[:3]
    volume = gpu_pkg.Volume(grid.dims, grid.origin, grid.voxel, grid.trunc, grid.max_weight)
    volume.set_state(tsdf, weight)
    raw = volume.extract_mesh()
    volume.close()
    centre = (np.array((24, 22, 20)) - 1) * 0.25 + np.array([0.11, -0.07, 0.05])
    rms = {}
    for placement in PLACEMENTS:
        got = raw.simplify(4 * float(grid.voxel), placement=placement)
        MC.assert_mesh_equal(MC.of(got), SC.simplify(checker, MC.of(raw), 4 * float(grid.voxel), None, placement), placement)
        assert 0 < len(got.faces) < len(raw.faces)
        rms[placement] = sphere_rms(got.vertices, centre, 3.5)
    assert rms["quadric"] < rms["mean"]


def test_through_the_pipeline(gpu_pkg, checker, cleaner, tmp_path):
    from apd_mvs_amd import pipeline
    case = fusion_cases.case("mixed_sizes")
    scene, results = _scene(gpu_pkg, pipeline, case)
    voxel = 0.05
    options = gpu_pkg.default_fusion_options(factor_strong=0.0, factor_weak=0.0)
    _, points = pipeline.fuse(scene, results, None, options=options, return_points=True)
    _, _, plain = pipeline.mesh(scene, results, None, voxel, bounds=points, options=options, return_mesh=True)
    cleaned = MC.remove_small(cleaner, MC.weld(cleaner, MC.of(plain), voxel * 1e-4), 20)
    for simplify, placement in ((3 * voxel, "quadric"), ((3 * voxel, "mean"), "mean")):
        want = MC.with_normals(cleaner, SC.simplify(checker, cleaned, 3 * voxel, None, placement))
        nv, nf, got = pipeline.mesh(scene, results, tmp_path / "small.ply", voxel, bounds=points, options=options, return_mesh=True, weld=voxel * 1e-4,
                                    min_component=20, simplify=simplify, normals=True)
        MC.assert_mesh_equal(MC.of(got), want, placement)
        assert (nv, nf) == (len(want.vertices), len(want.faces)) and 20 < nf < len(cleaned.faces)
        assert (tmp_path / "small.ply").read_bytes() == MC.ply_bytes(want)


def test_binary_writes_the_simplified_mesh_of_the_checkers_chain(gpu_pkg, synth, checker, cleaner, tmp_path):
    """--mesh-simplify in its place of the chain: APD.ply.mesh holds the bytes of weld, simplify, normals by the checkers on the mesh
    pipeline.mesh extracts from the run's own maps; one line tells the counts."""
    from apd_mvs_amd import pipeline
    folder = tmp_path / "dense"
    folder.mkdir()
    _write_dense_folder(folder, synth, 96, 72, 4)
    voxel = F(0.05)
    flags = ["--mesh-normals", "--mesh-simplify", "0.15,mean", "--mesh", "0.05", "--mesh-weld", "%.9g" % F(float(voxel) * 1e-4)]
    r = subprocess.run([APD_BIN, str(folder), "0", "--seed", "21", "--iters", "1", "--keep-maps"] + flags, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert r.returncode == 0 and "All done" in r.stdout, r.stdout[-2000:]
    scene = pipeline.load_dense_folder(str(folder), gpu_pkg.Camera)
    results = {}
    for v in range(scene.num_views):
        d = folder / "APD" / ("%08d" % scene.ids[v])
        results[v] = pipeline.ViewState(_read_dmb(d / "depths.dmb"), _read_dmb(d / "normals.dmb"), _read_dmb(d / "weak.bin"), _read_dmb(d / "selected_views.bin"))
    colour = pipeline.load_colour_images(str(folder), scene.ids[:scene.num_views])
    _, _, plain = pipeline.mesh(scene, results, None, float(voxel), colour_images=colour, return_mesh=True)
    welded = MC.weld(cleaner, MC.of(plain), F(float(voxel) * 1e-4))
    small = SC.simplify(checker, welded, F(0.15), None, "mean")
    want = MC.with_normals(cleaner, small)
    assert (folder / "APD" / "APD.ply.mesh").read_bytes() == MC.ply_bytes(want)
    assert 0 < len(small.faces) < len(welded.faces)
    line = "Mesh simplified in cells of 0.150000 (mean): %d vertices and %d faces -> %d vertices and %d faces" % (
        len(welded.vertices), len(welded.faces), len(small.vertices), len(small.faces))
    assert line in r.stdout, r.stdout[-1500:]
