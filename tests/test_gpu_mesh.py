"""Cleaning a mesh on the device (apd_mesh_create, apd_mesh_weld, apd_mesh_components, apd_mesh_remove_small_components,
apd_mesh_with_vertex_normals; csrc/apd_mesh.hip), bitwise against the sequential checker (tests/helpers/mesh_ref.cpp): positions and
normals as uint32, colours, faces, labels and sizes.  The meshes are made in test_mesh.py, where the checker is held against a numpy
restatement."""
import shutil
import subprocess

import numpy as np
import pytest

import fusion_cases
import mesh_checker as MC
from test_gpu_dropin_binary import APD_BIN, _write_dense_folder
from test_gpu_fusion_options import _read_dmb, _run, _scene
from test_mesh import (EDGE_COUNTS, F, colours_of, fan, islands, joined, moved, octahedron, sheet, soup, strip, weldable, with_count)
from test_volume import sphere_field

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return MC.build(tmp_path_factory.mktemp("mesh_checker"))


def device_mesh(pkg, mesh):
    got = pkg.Mesh.from_arrays(mesh.vertices, mesh.faces, mesh.colours)
    MC.assert_mesh_equal(MC.of(got), MC.Mesh(mesh.vertices, mesh.faces, mesh.colours), "from_arrays")
    return got


def check_all(pkg, checker, mesh, tolerance, min_faces, what):
    """Every operation on one mesh against the checker; the input stays as it was."""
    m = device_mesh(pkg, mesh)
    MC.assert_mesh_equal(MC.of(m.weld(tolerance)), MC.weld(checker, mesh, tolerance), (what, "weld"))
    label, size, count = m.components()
    want = MC.components(checker, mesh)
    assert np.array_equal(label, want[0]) and np.array_equal(size, want[1]) and count == want[2], (what, "components")
    MC.assert_mesh_equal(MC.of(m.remove_small_components(min_faces)), MC.remove_small(checker, mesh, min_faces), (what, "remove"))
    MC.assert_mesh_equal(MC.of(m.with_vertex_normals()), MC.with_normals(checker, mesh), (what, "normals"))
    m.refresh()   # the arrays of the object are copies made when it was built: read the device again
    MC.assert_mesh_equal(MC.of(m), MC.Mesh(mesh.vertices, mesh.faces, mesh.colours), (what, "input"))


def test_counts_at_the_wave_and_tile_edges(gpu_pkg, checker):
    """0, 1, 63, 64, 65, 2047, 2048, 2049 vertices, and as many faces: a strip, as it is and as unshared triangles, and a mesh of
    exactly that many vertices that welding merges all along, so that the weld's scans and gathers have work at every count."""
    for n in EDGE_COUNTS:
        for what in (0, 1):
            mesh = with_count(n, what)
            check_all(gpu_pkg, checker, mesh, 0.3, 2, (n, what))
            if n and what:
                check_all(gpu_pkg, checker, soup(mesh, colour=True), 1e-3, 2, (n, what, "soup"))
        if n >= 3:
            mesh = weldable(n)
            assert len(mesh.vertices) == n and len(MC.weld(checker, mesh, 1e-3).vertices) == n // 3 + 2
            check_all(gpu_pkg, checker, mesh, 1e-3, 2, (n, "weldable"))


def test_a_mesh_of_seventy_thousand_faces(gpu_pkg, checker):
    """Several sort and scan blocks and a second level of the scan: a jittered sheet, as it is (one component) and as unshared
    triangles in pieces (welded back)."""
    mesh = sheet(190, 186, 0.2)
    assert len(mesh.faces) == 69930
    m = device_mesh(gpu_pkg, mesh)
    MC.assert_mesh_equal(MC.of(m.with_vertex_normals()), MC.with_normals(checker, mesh), "normals")
    label, size, count = m.components()
    assert count == 1 and (label == 0).all() and (size == 69930).all()
    pieces = joined(soup(sheet(60, 50, 0.2)), moved(sheet(150, 141, 0.2), [0, 0, 5]), colour=True)
    assert len(pieces.faces) > 47000
    p = device_mesh(gpu_pkg, pieces)
    welded, want = p.weld(1e-3), MC.weld(checker, pieces, 1e-3)
    MC.assert_mesh_equal(MC.of(welded), want, "weld")
    assert len(want.vertices) == 60 * 50 + 150 * 141
    label, size, count = p.components()
    ref = MC.components(checker, pieces)
    assert np.array_equal(label, ref[0]) and np.array_equal(size, ref[1]) and count == ref[2] == 2 * 59 * 49 + 1
    MC.assert_mesh_equal(MC.of(p.remove_small_components(2)), MC.remove_small(checker, pieces, 2), "remove")


def test_a_fan_whose_run_of_corners_crosses_a_sort_tile(gpu_pkg, checker):
    mesh = fan(2100)
    got = device_mesh(gpu_pkg, mesh).with_vertex_normals()
    MC.assert_mesh_equal(MC.of(got), MC.with_normals(checker, mesh))
    assert got.normals[0, 2] > 0.5 and np.allclose(np.linalg.norm(got.normals, axis=1), 1, atol=1e-6)


def test_a_strip_in_index_order_and_shuffled(gpu_pkg, checker):
    """Deep union-find paths in index order; shuffled, label and size still come out as functions of the input alone."""
    for shuffled in (False, True):
        mesh = strip(5000, shuffled)
        check_all(gpu_pkg, checker, mesh, 0.3, 10, shuffled)
        label, size, count = device_mesh(gpu_pkg, mesh).components()
        assert count == 1 and (label == 0).all() and (size == 5000).all()
    two = joined(strip(2500, True), moved(strip(2500, True, seed=2), [0, 50, 0]))
    label, size, count = device_mesh(gpu_pkg, two).components()
    assert count == 2 and set(label.tolist()) == {0, 2500} and (size == 2500).all()


def test_three_hundred_triangles_and_one_large_piece(gpu_pkg, checker):
    mesh = islands(300, 2000)
    m = device_mesh(gpu_pkg, mesh)
    for min_faces in (0, 1, 2, 2000, 10 ** 6):
        got, want = m.remove_small_components(min_faces), MC.remove_small(checker, mesh, min_faces)
        MC.assert_mesh_equal(MC.of(got), want, min_faces)
    assert len(m.remove_small_components(1).faces) == len(mesh.faces) and len(m.remove_small_components(2).faces) == len(mesh.faces) - 300
    assert m.components()[2] == 301


def test_a_nan_coordinate_an_unreferenced_vertex_and_colour(gpu_pkg, checker):
    base = soup(sheet(9, 8, 0.1))
    base.vertices[10, 1] = np.nan
    base.vertices[40, 2] = np.inf
    V = np.concatenate([base.vertices, [[3, 3, 3]]]).astype(F)   # the last vertex: no face names it
    for colours in (None, colours_of(len(V))):
        mesh = MC.Mesh(V, base.faces, colours)
        check_all(gpu_pkg, checker, mesh, 1e-3, 2, colours is not None)
        m = device_mesh(gpu_pkg, mesh)
        welded = m.weld(1e-3)
        assert np.isnan(welded.vertices).sum() == 1 and np.isinf(welded.vertices).sum() == 1   # joined to nothing, kept by their faces
        normals = m.with_vertex_normals().normals
        assert not normals[mesh.faces[10 // 3]].any() and not normals[-1].any() and not np.isnan(normals).any()


def test_weld_then_remove_then_normals_chained(gpu_pkg, checker):
    mesh = joined(soup(islands(40, 500), colour=False), moved(soup(octahedron()), [30, 0, 0]), colour=True)
    got = device_mesh(gpu_pkg, mesh).with_vertex_normals().weld(1e-3).remove_small_components(5)
    want = MC.remove_small(checker, MC.weld(checker, MC.with_normals(checker, mesh), 1e-3), 5)
    MC.assert_mesh_equal(MC.of(got), want, "normals carried")
    assert want.normals is not None and len(want.faces) == len(mesh.faces) - 40
    got = device_mesh(gpu_pkg, mesh).weld(1e-3).remove_small_components(5).with_vertex_normals()
    want = MC.with_normals(checker, MC.remove_small(checker, MC.weld(checker, mesh, 1e-3), 5))
    MC.assert_mesh_equal(MC.of(got), want, "chain")
    assert np.allclose(np.linalg.norm(want.normals, axis=1), 1, atol=1e-6)


def test_the_file_of_a_mesh_with_normals(gpu_pkg, checker, tmp_path):
    mesh = MC.Mesh(octahedron().vertices, octahedron().faces, colours_of(6))
    for m in (mesh, MC.Mesh(mesh.vertices, mesh.faces)):
        got = device_mesh(gpu_pkg, m).with_vertex_normals()
        got.write_ply(tmp_path / "n.ply")
        want = MC.with_normals(checker, m)
        assert (tmp_path / "n.ply").read_bytes() == MC.ply_bytes(want)
        pts = gpu_pkg.Points.read_ply(tmp_path / "n.ply")
        assert np.array_equal(MC.bits(np.asarray(pts.xyz)), MC.bits(want.vertices)) and np.array_equal(MC.bits(np.asarray(pts.normal)), MC.bits(want.normals))
        device_mesh(gpu_pkg, m).write_ply(tmp_path / "p.ply")
        assert (tmp_path / "p.ply").read_bytes() == MC.ply_bytes(m)


def test_device_arrays_and_their_range_check(gpu_pkg):
    import ctypes as C
    import torch
    L = gpu_pkg.lib()
    mesh = octahedron()
    xyz, idx = torch.from_numpy(mesh.vertices).cuda(), torch.from_numpy(mesh.faces).cuda()
    torch.cuda.synchronize()
    out = C.c_void_p()
    assert L.apd_mesh_create(0, 6, C.c_void_p(xyz.data_ptr()), None, 8, C.c_void_p(idx.data_ptr()), 1, C.byref(out)) == 0
    MC.assert_mesh_equal(MC.of(gpu_pkg.Mesh(out)), mesh)
    for bad in (6, -1):
        wrong = mesh.faces.copy()
        wrong[5, 1] = bad
        idx = torch.from_numpy(wrong).cuda()
        torch.cuda.synchronize()
        out = C.c_void_p(1234)
        assert L.apd_mesh_create(0, 6, C.c_void_p(xyz.data_ptr()), None, 8, C.c_void_p(idx.data_ptr()), 1, C.byref(out)) == -1
        assert L.apd_fusion_last_error().decode() == "apd_mesh_create: a face index outside 0 .. 6" and out.value == 1234


def test_the_mesh_of_a_sphere_with_samples_at_zero(gpu_pkg, checker):
    """Samples set to exactly 0.0f put several vertices at one position; after weld(voxel * 1e-4) no two vertices share their bits and
    no face repeats an index."""
    grid, tsdf, weight = sphere_field((24, 22, 20), 7.0)[:3]
    tsdf = tsdf.copy()
    near = np.argsort(np.abs(tsdf))[:60]
    tsdf[near] = 0.0
    volume = gpu_pkg.Volume(grid.dims, grid.origin, grid.voxel, grid.trunc, grid.max_weight)
    volume.set_state(tsdf, weight)
    raw = volume.extract_mesh()
    volume.close()
    mesh = MC.of(raw)
    assert len(np.unique(MC.bits(mesh.vertices), axis=0)) < len(mesh.vertices)   # coincident vertices really occur
    tol = float(grid.voxel) * 1e-4
    got, want = raw.weld(tol), MC.weld(checker, mesh, tol)
    MC.assert_mesh_equal(MC.of(got), want)
    zero_as_one = np.where(got.vertices == 0, F(0), got.vertices)   # -0.0 and +0.0 are one position
    assert len(np.unique(MC.bits(zero_as_one), axis=0)) == len(got.vertices) < len(mesh.vertices)
    f = got.faces
    assert len(f) < len(mesh.faces) and not ((f[:, 0] == f[:, 1]) | (f[:, 0] == f[:, 2]) | (f[:, 1] == f[:, 2])).any()
    MC.assert_mesh_equal(MC.of(got.with_vertex_normals()), MC.with_normals(checker, want), "normals")


# --------------------------------------------------------------------------------------------------------------------
# end to end
# --------------------------------------------------------------------------------------------------------------------

def test_through_the_pipeline(gpu_pkg, checker, tmp_path):
    """pipeline.mesh with the three arguments against the checker applied, in the same order, to what it gives without them."""
    from apd_mvs_amd import pipeline
    case = fusion_cases.case("mixed_sizes")
    scene, results = _scene(gpu_pkg, pipeline, case)
    voxel = 0.05
    options = gpu_pkg.default_fusion_options(factor_strong=0.0, factor_weak=0.0)
    _, points = pipeline.fuse(scene, results, None, options=options, return_points=True)
    nv0, nf0, plain = pipeline.mesh(scene, results, tmp_path / "plain.ply", voxel, bounds=points, options=options, return_mesh=True)
    assert plain.normals is None and (nv0, nf0) == (len(plain.vertices), len(plain.faces))
    want = MC.with_normals(checker, MC.remove_small(checker, MC.weld(checker, MC.of(plain), voxel * 1e-4), 20))
    nv, nf, got = pipeline.mesh(scene, results, tmp_path / "clean.ply", voxel, bounds=points, options=options, return_mesh=True, weld=voxel * 1e-4,
                                min_component=20, normals=True)
    MC.assert_mesh_equal(MC.of(got), want)
    assert (nv, nf) == (len(want.vertices), len(want.faces)) and nf > 100
    assert (tmp_path / "clean.ply").read_bytes() == MC.ply_bytes(want)
    assert (tmp_path / "plain.ply").read_bytes() == MC.ply_bytes(MC.of(plain))
    only = pipeline.mesh(scene, results, None, voxel, bounds=points, options=options, min_component=20)
    assert only == (lambda m: (len(m.vertices), len(m.faces)))(MC.remove_small(checker, MC.of(plain), 20))


@pytest.fixture(scope="module")
def folders(gpu_pkg, synth, tmp_path_factory):
    """One small synthetic dense folder (the size of the drop-in tests) run with --mesh alone and with the three options."""
    root = tmp_path_factory.mktemp("dense")
    a = root / "a"
    a.mkdir()
    _write_dense_folder(a, synth, 96, 72, 4)
    shutil.copytree(a, root / "clean")
    voxel = "0.05"
    _run(a, "--mesh", voxel)
    flags = ("--mesh-normals", "--mesh", voxel, "--mesh-min-component", "8", "--mesh-weld", "%.9g" % F(float(voxel) * 1e-4))
    r = subprocess.run([APD_BIN, str(root / "clean"), "0", "--seed", "21", "--iters", "1", "--keep-maps"] + list(flags), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "All done" in r.stdout, r.stdout[-2000:]
    return {"plain": a, "clean": root / "clean", "voxel": float(F(voxel)), "log": r.stdout}


def test_binary_writes_the_cleaned_mesh_of_the_pipeline(gpu_pkg, folders, checker, tmp_path):
    """With the three options APD.ply.mesh holds the bytes pipeline.mesh writes with the same three; without them the bytes of
    pipeline.mesh with its defaults, as before; every other output is the same in both runs; one line per step tells the counts."""
    from apd_mvs_amd import pipeline
    outputs = {}
    for which in ("plain", "clean"):
        root = folders[which] / "APD"
        outputs[which] = {str(p.relative_to(root)): p.read_bytes() for p in sorted(root.rglob("*")) if p.is_file()}
    assert set(outputs["plain"]) == set(outputs["clean"])
    assert all(outputs["plain"][n] == outputs["clean"][n] for n in outputs["plain"] if n != "APD.ply.mesh")
    folder = folders["clean"]
    scene = pipeline.load_dense_folder(str(folder), gpu_pkg.Camera)
    results = {}
    for v in range(scene.num_views):
        d = folder / "APD" / ("%08d" % scene.ids[v])
        results[v] = pipeline.ViewState(_read_dmb(d / "depths.dmb"), _read_dmb(d / "normals.dmb"), _read_dmb(d / "weak.bin"), _read_dmb(d / "selected_views.bin"))
    colour = pipeline.load_colour_images(str(folder), scene.ids[:scene.num_views])
    voxel = folders["voxel"]
    nv0, nf0, plain = pipeline.mesh(scene, results, tmp_path / "plain.ply", voxel, colour_images=colour, return_mesh=True)
    assert outputs["plain"]["APD.ply.mesh"] == (tmp_path / "plain.ply").read_bytes() and nf0 > 0
    nv, nf = pipeline.mesh(scene, results, tmp_path / "clean.ply", voxel, colour_images=colour, weld=F(voxel * 1e-4), min_component=8, normals=True)
    assert outputs["clean"]["APD.ply.mesh"] == (tmp_path / "clean.ply").read_bytes()
    want = MC.with_normals(checker, MC.remove_small(checker, MC.weld(checker, MC.of(plain), F(voxel * 1e-4)), 8))
    assert outputs["clean"]["APD.ply.mesh"] == MC.ply_bytes(want) and (nv, nf) == (len(want.vertices), len(want.faces))
    log = folders["log"]
    assert "Mesh welded within" in log and "Mesh without the components of fewer than 8 faces" in log and "Mesh with vertex normals: " in log
    assert "%d vertices and %d faces -> " % (nv0, nf0) in log and " -> %d vertices and %d faces" % (nv, nf) in log
    assert gpu_pkg.Points.read_ply(folder / "APD" / "APD.ply.mesh").count == nv
