"""apd_mesh_adjacency and apd_mesh_smooth on the device (csrc/apd_mesh_smooth.hip, contract C24), bitwise against the sequential checker
(tests/helpers/mesh_smooth_ref.cpp): valence, boundary flags and the three counts, and every smoothed mesh, each run twice for the
same bytes, with the input read back unchanged.  The meshes and the checker's own tests: test_mesh_smooth.py."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import fusion_cases
import mesh_checker as MC
import mesh_simplify_checker as SC
import mesh_smooth_checker as KC
from test_gpu_dropin_binary import APD_BIN, _write_dense_folder
from test_gpu_fusion_options import _read_dmb, _scene
from test_mesh import F, colours_of, fan, islands, joined, moved, octahedron, sheet, soup, strip, with_count
from test_mesh_smooth import MODES, noisy_sphere, quality
from test_volume import sphere_field

pytestmark = pytest.mark.gpu

TAUBIN = (0.5, -0.53)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return KC.build(tmp_path_factory.mktemp("mesh_smooth_checker"))


@pytest.fixture(scope="module")
def cleaner(tmp_path_factory):
    return MC.build(tmp_path_factory.mktemp("mesh_checker"))


@pytest.fixture(scope="module")
def simplifier(tmp_path_factory):
    return SC.build(tmp_path_factory.mktemp("mesh_simplify_checker"))


def device_mesh(pkg, mesh):
    return pkg.Mesh.from_arrays(mesh.vertices, mesh.faces, mesh.colours)


def check_adjacency(m, checker, mesh, what):
    want, got = KC.adjacency(checker, mesh), m.adjacency()
    assert got[0].dtype == np.uint32 and got[1].dtype == bool
    assert np.array_equal(got[0], want[0]), (what, "valence", np.argwhere(got[0] != want[0])[:5])
    assert np.array_equal(got[1], want[1]), (what, "boundary", np.argwhere(got[1] != want[1])[:5])
    assert got[2:] == want[2:], (what, got[2:], want[2:])
    return want


def check(pkg, checker, mesh, steps=((2,) + TAUBIN + ("along",),), what=""):
    """The adjacency and every (iterations, lam, mu, mode) of `steps` against the checker, each smoothing twice; the input stays as it
    was.  Returns the checker's last result."""
    m = device_mesh(pkg, mesh)
    check_adjacency(m, checker, mesh, what)
    want = None
    for iterations, lam, mu, mode in steps:
        want, first = KC.smooth(checker, mesh, iterations, lam, mu, mode)
        for again in (0, 1):
            got = m.smooth(iterations, lam, mu, mode)
            MC.assert_mesh_equal(MC.of(got), want, (what, iterations, lam, mu, mode, again))
            assert m.moved == first and got.moved == first, (what, mode, m.moved, first)
            got.close()
    m.refresh()
    MC.assert_mesh_equal(MC.of(m), MC.Mesh(mesh.vertices, mesh.faces, mesh.colours), (what, "input"))
    m.close()
    return want


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
            check(gpu_pkg, checker, mesh, what=(n, what))
    # 6 F one below and one above the tile, as near as a multiple of 6 comes
    below, above = (tile - 1) // 6, tile // 6 + 1
    assert 6 * below < tile < 6 * above
    for faces in (below, above):
        check(gpu_pkg, checker, with_count(faces, 1), what=("pairs", 6 * faces))


def test_a_fan_whose_hub_row_is_longer_than_a_sort_tile(gpu_pkg, checker):
    tile = sort_tile(gpu_pkg)
    mesh = fan(tile // 2 + 40)   # the hub's pairs: two per face, more than a tile, at the start of the sorted keys
    want = KC.adjacency(checker, mesh)
    assert 2 * len(mesh.faces) > tile and want[0][0] == len(mesh.faces) + 1 and want[1][0]
    check(gpu_pkg, checker, mesh, [(2,) + TAUBIN + (mode,) for mode in MODES], "fan")
    # and one run longer than a tile: the same face more often than a tile has entries
    many = MC.Mesh(octahedron().vertices, np.concatenate([octahedron().faces, np.tile([[0, 2, 4]], (tile + 3, 1))]).astype(np.int32))
    assert KC.adjacency(checker, many)[2:] == (12, 0, 3)
    check(gpu_pkg, checker, many, [(1,) + TAUBIN + (mode,) for mode in MODES], "a long run")


def test_the_shuffled_strip_and_islands(gpu_pkg, checker):
    check(gpu_pkg, checker, strip(5000, shuffled=True), [(3,) + TAUBIN + (mode,) for mode in MODES], "shuffled strip")
    check(gpu_pkg, checker, islands(300, 2000), [(3,) + TAUBIN + (mode,) for mode in MODES], "islands")


def test_edge_and_vertex_kinds(gpu_pkg, checker):
    every = [(2,) + TAUBIN + (mode,) for mode in MODES]
    base = sheet(2, 2)
    third = MC.Mesh(np.concatenate([base.vertices, [[0.5, 0.5, 1.0]]]).astype(F), np.concatenate([base.faces, [[0, 3, 4]]]).astype(np.int32))
    check(gpu_pkg, checker, third, every, "a non-manifold edge")
    a = sheet(9, 8, 0.2)
    two = MC.Mesh(a.vertices, np.concatenate([a.faces, a.faces[::3, ::-1]]))   # a second sheet on the same vertices, a third of the faces, reflected
    assert KC.adjacency(checker, two)[4] > 0 and KC.adjacency(checker, two)[3] < KC.adjacency(checker, a)[3]
    check(gpu_pkg, checker, two, every, "two sheets on the same vertices")
    # a duplicate gives multiplicity 2 where a single face leaves a border: that is the rule
    one = MC.Mesh(a.vertices[[0, 1, 9]], np.array([[0, 1, 2]], np.int32))
    twice = MC.Mesh(one.vertices, np.array([[0, 1, 2], [0, 1, 2]], np.int32))
    m = device_mesh(gpu_pkg, one)
    assert check_adjacency(m, checker, one, "one face")[2:] == (3, 3, 0)
    m = device_mesh(gpu_pkg, twice)
    assert check_adjacency(m, checker, twice, "the face twice")[2:] == (3, 0, 0) and not m.adjacency()[1].any()
    check(gpu_pkg, checker, twice, every, "the face twice")
    check(gpu_pkg, checker, MC.Mesh(np.concatenate([a.vertices, a.vertices[:3] + 9]), np.concatenate([a.faces, [[72, 72, 73], [74, 74, 74]]]).astype(np.int32)),
          every, "repeated indices")
    bad = MC.Mesh(np.concatenate([a.vertices, [[100, 100, 100]]]).astype(F), a.faces, colours_of(len(a.vertices) + 1))   # one unreferenced
    bad.vertices[27, 2] = np.nan
    bad.vertices[3, 0] = -5e6
    bad.vertices[40, 1] = np.inf
    want = check(gpu_pkg, checker, bad, every, "nan, inf, far, unreferenced, colour")
    assert np.array_equal(MC.bits(want.vertices[[27, 40, 72]]), MC.bits(bad.vertices[[27, 40, 72]])) and np.array_equal(want.colours, bad.colours)
    assert np.isfinite(np.delete(want.vertices, [27, 40], 0)).all()
    shaded = device_mesh(gpu_pkg, a).with_vertex_normals()
    got = shaded.smooth(2)
    assert shaded.normals is not None and got.normals is None
    MC.assert_mesh_equal(MC.of(got), KC.smooth(checker, a, 2)[0], "normals in")


def test_empty_meshes(gpu_pkg, checker):
    none = MC.Mesh(sheet(5, 4, 0.1).vertices, np.zeros((0, 3), np.int32), colours_of(20))
    want = check(gpu_pkg, checker, none, what="no faces")
    assert np.array_equal(MC.bits(want.vertices), MC.bits(none.vertices))
    m = device_mesh(gpu_pkg, none)
    assert m.smooth(1).moved == 0 and m.adjacency()[2:] == (0, 0, 0) and not m.adjacency()[0].any()
    check(gpu_pkg, checker, MC.Mesh(np.zeros((0, 3), F), np.zeros((0, 3), np.int32)), what="no vertices")


def test_steps_iterations_and_lambda(gpu_pkg, checker):
    mesh = joined(sheet(23, 19, 0.3), moved(octahedron(), [40, 0, 0]), colour=True)
    steps = [(n, 0.5, mu, mode) for n in (1, 2, 7) for mu in (0.0, -0.53) for mode in ("along", "fixed")]
    steps += [(2, 1.0, 0.0, "free"), (3, 1.0, -2.0, "along"), (1, 0.33, -0.34, "free")]
    check(gpu_pkg, checker, mesh, steps, "steps")


def test_both_layouts_of_the_positions_give_the_same_bits(gpu_pkg, checker):
    L = gpu_pkg.lib()
    mesh = sheet(40, 37, 0.3)
    before = L.apd_mesh_smooth_layout(0)
    try:
        for wide in (0, 1):
            L.apd_mesh_smooth_layout(wide)
            check(gpu_pkg, checker, mesh, [(n,) + TAUBIN + ("along",) for n in (1, 2)] + [(1, 0.5, 0.0, "free"), (3, 0.5, 0.0, "fixed")], ("layout", wide))
    finally:
        L.apd_mesh_smooth_layout(before)


def test_a_mesh_of_seventy_thousand_faces(gpu_pkg, checker):
    mesh = sheet(190, 186, 0.2)
    assert len(mesh.faces) == 69930
    check(gpu_pkg, checker, mesh, [(5,) + TAUBIN + ("along",)], "size")


def test_device_arrays_in(gpu_pkg, checker):
    import torch
    L = gpu_pkg.lib()
    mesh = sheet(30, 28, 0.2)
    xyz, idx = torch.from_numpy(mesh.vertices).cuda(), torch.from_numpy(mesh.faces).cuda()
    torch.cuda.synchronize()
    out = C.c_void_p()
    assert L.apd_mesh_create(0, len(mesh.vertices), C.c_void_p(xyz.data_ptr()), None, len(mesh.faces), C.c_void_p(idx.data_ptr()), 1, C.byref(out)) == 0
    m = gpu_pkg.Mesh(out)
    check_adjacency(m, checker, mesh, "device arrays")
    MC.assert_mesh_equal(MC.of(m.smooth(3)), KC.smooth(checker, mesh, 3)[0], "device arrays")


def test_chains_with_the_cleaning_calls_and_the_simplification(gpu_pkg, checker, cleaner, simplifier):
    mesh = joined(soup(islands(40, 500), colour=False), moved(soup(octahedron()), [30, 0, 0]), colour=True)
    got = device_mesh(gpu_pkg, mesh).weld(1e-3).smooth(3).simplify(2.0).with_vertex_normals()
    welded = MC.weld(cleaner, mesh, 1e-3)
    want = MC.with_normals(cleaner, SC.simplify(simplifier, KC.smooth(checker, welded, 3)[0], 2.0, None, "quadric"))
    MC.assert_mesh_equal(MC.of(got), want, "weld, smooth, simplify, normals")
    assert want.normals is not None and 0 < len(want.faces) < len(mesh.faces)
    assert not np.array_equal(KC.smooth(checker, welded, 3)[0].vertices, welded.vertices)


def test_the_sphere_of_a_device_volume(gpu_pkg, checker):
    grid, tsdf, weight = sphere_field((24, 22, 20), 7.0)[:3]
    volume = gpu_pkg.Volume(grid.dims, grid.origin, grid.voxel, grid.trunc, grid.max_weight)
    volume.set_state(tsdf, weight)
    raw = volume.extract_mesh()
    volume.close()
    centre = (np.array((24, 22, 20)) - 1) * 0.25 + np.array([0.11, -0.07, 0.05])
    assert check_adjacency(raw, checker, MC.of(raw), "sphere")[3:] == (0, 0)
    MC.assert_mesh_equal(MC.of(raw.smooth(10)), KC.smooth(checker, MC.of(raw), 10)[0], "sphere")

    def on_device(mesh, iterations, lam, mu):
        return device_mesh(gpu_pkg, mesh).smooth(iterations, lam, mu).vertices

    quality(on_device, MC.Mesh(raw.vertices, raw.faces), centre, 3.5, "the sphere of a device volume")
    quality(on_device, noisy_sphere(MC.Mesh(raw.vertices, raw.faces), centre, 3.5), centre, 3.5, "the same with radial noise")


def test_through_the_pipeline(gpu_pkg, checker, cleaner, simplifier, tmp_path):
    from apd_mvs_amd import pipeline
    case = fusion_cases.case("mixed_sizes")
    scene, results = _scene(gpu_pkg, pipeline, case)
    voxel = 0.05
    options = gpu_pkg.default_fusion_options(factor_strong=0.0, factor_weak=0.0)
    _, points = pipeline.fuse(scene, results, None, options=options, return_points=True)
    _, _, plain = pipeline.mesh(scene, results, None, voxel, bounds=points, options=options, return_mesh=True)
    cleaned = MC.remove_small(cleaner, MC.weld(cleaner, MC.of(plain), voxel * 1e-4), 20)
    smoothed, first = KC.smooth(checker, cleaned, 3, 0.5, -0.53, "along")
    assert 0 < first <= len(cleaned.vertices) and not np.array_equal(smoothed.vertices, cleaned.vertices)
    for smooth, simplify in (((3, 0.5, -0.53, "along"), None), (3, 3 * voxel), ((3, 0.5, -0.53), None)):
        want = MC.with_normals(cleaner, smoothed if simplify is None else SC.simplify(simplifier, smoothed, simplify, None, "quadric"))
        nv, nf, got = pipeline.mesh(scene, results, tmp_path / "smooth.ply", voxel, bounds=points, options=options, return_mesh=True, weld=voxel * 1e-4,
                                    min_component=20, smooth=smooth, simplify=simplify, normals=True)
        MC.assert_mesh_equal(MC.of(got), want, (smooth, simplify))
        assert (nv, nf) == (len(want.vertices), len(want.faces)) and nf > 20
        assert (tmp_path / "smooth.ply").read_bytes() == MC.ply_bytes(want)
    with pytest.raises(ValueError, match="smooth"):
        pipeline.mesh(scene, results, None, voxel, bounds=points, options=options, smooth=(3, 0.5))


def test_binary_writes_the_smoothed_mesh_of_the_checkers_chain(gpu_pkg, synth, checker, cleaner, tmp_path):
    """--mesh-smooth in its place of the chain: APD.ply.mesh holds the bytes of weld, smooth, normals by the checkers on the mesh
    pipeline.mesh extracts from the run's own maps; one line tells how many vertices moved."""
    from apd_mvs_amd import pipeline
    folder = tmp_path / "dense"
    folder.mkdir()
    _write_dense_folder(folder, synth, 96, 72, 4)
    voxel = F(0.05)
    flags = ["--mesh-normals", "--mesh-smooth", "3", "--mesh", "0.05", "--mesh-weld", "%.9g" % F(float(voxel) * 1e-4)]
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
    smoothed, first = KC.smooth(checker, welded, 3, 0.5, -0.53, "along")
    want = MC.with_normals(cleaner, smoothed)
    assert (folder / "APD" / "APD.ply.mesh").read_bytes() == MC.ply_bytes(want)
    assert first > 0
    line = "Mesh smoothed in 3 iterations (lambda 0.500000, mu -0.530000, along boundary): %d of %d vertices moved" % (first, len(welded.vertices))
    assert line in r.stdout, r.stdout[-1500:]
    bad = subprocess.run([APD_BIN, str(folder), "0", "--mesh", "0.05", "--mesh-smooth", "3,0.5,0.2"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                         timeout=60)
    assert bad.returncode != 0 and "bad value '3,0.5,0.2' of --mesh-smooth" in bad.stdout and "USAGE" in bad.stdout
