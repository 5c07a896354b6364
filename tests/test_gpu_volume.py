"""The signed distance volume and its mesh on the device (apd_volume_*, apd_mesh_*; csrc/apd_volume.hip), bitwise against the
sequential checker (tests/helpers/volume_ref.cpp): distances, weights and colours as uint32 (so that -0 or a NaN would show),
vertices, colours and faces.  The grids, views and fields are made in test_volume.py, where the checker is held against a numpy
restatement on them."""
import shutil
import subprocess

import numpy as np
import pytest

import fusion_cases
import volume_checker as VC
from test_gpu_dropin_binary import _write_dense_folder
from test_gpu_fusion_options import APD_BIN, _read_dmb, _run, _scene
from test_points_render import ring_cameras, unit_camera
from test_volume import (F, INTEGRATE_DIMS, box_grid, extract_cases, field_with_count, integrate_cases, mixed_weights, one_cell, planted_plane, random_field,
                         sphere_depth, view_images)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return VC.build(tmp_path_factory.mktemp("volume_checker"))


def volume_of(pkg, grid, colour=False):
    return pkg.Volume(grid.dims, grid.origin, grid.voxel, grid.trunc, grid.max_weight, colour=colour)


def state_of(volume):
    s = VC.State.__new__(VC.State)
    s.tsdf, s.weight, s.colour = volume.state()
    return s


def device_integrate(pkg, volume, cams, depths, images, weights, on_device):
    if on_device:
        import torch
        up = lambda arrs: None if arrs is None else [torch.from_numpy(np.ascontiguousarray(a, F)).cuda() for a in arrs]
        depths, images = up(depths), up(images)
    volume.integrate(cams, depths, images, weights, maps_on_device=on_device)


def mesh_arrays(mesh):
    return VC.MeshArrays(mesh.vertices, mesh.colours, mesh.faces)


def device_extract(pkg, grid, tsdf, weight, colour=None):
    volume = volume_of(pkg, grid, colour is not None)
    volume.set_state(tsdf, weight, colour)
    mesh = volume.extract_mesh()
    volume.close()
    return mesh


# --------------------------------------------------------------------------------------------------------------------
# integrate
# --------------------------------------------------------------------------------------------------------------------

def test_every_integration_case_with_maps_on_host_and_on_device(gpu_pkg, checker):
    """Rows of samples around a wave and a workgroup and off every multiple; 1, 3 and chunk + 1 ring cameras with skew, roll and
    fx != fy; a sphere and a plane; with and without colour, 1 and 3 channels, mixed weights; the planted plane after 1, 2 and
    max_weight + 3 views (saturation); samples on the image border, behind the camera and on depths 0, negative, inf and NaN;
    16384 x 2 and 2 x 16384 maps read at their corners."""
    chunk = gpu_pkg.lib().apd_volume_view_chunk()
    names = []
    for name, grid, cams, depths, images, weights in integrate_cases(gpu_pkg, chunk):
        want = VC.integrate(checker, grid, VC.State(grid, colour=images is not None), cams, depths, images, weights)
        for on_device in (False, True):
            volume = volume_of(gpu_pkg, grid, images is not None)
            device_integrate(gpu_pkg, volume, cams, depths, images, weights, on_device)
            VC.assert_state_equal(state_of(volume), want, (name, on_device))
            volume.close()
        names.append(name)
    assert any("%d views" % (chunk + 1) in n for n in names) and all(any(repr(d) in n for n in names) for d in INTEGRATE_DIMS)


def test_two_calls_equal_one_and_a_colour_volume_without_images(gpu_pkg, checker):
    grid = box_grid((17, 9, 6), max_weight=3.0)
    cams = ring_cameras(gpu_pkg, 6)
    depths, images, weights = [sphere_depth(c) for c in cams], view_images(cams, 3), mixed_weights(6)
    want = VC.integrate(checker, grid, VC.State(grid, colour=True), cams, depths, images, weights)
    assert (want.weight == 3.0).any() and (want.colour[:, 3] > 0).any()
    once, twice = volume_of(gpu_pkg, grid, True), volume_of(gpu_pkg, grid, True)
    once.integrate(cams, depths, images, weights)
    twice.integrate(cams[:3], depths[:3], images[:3], weights[:3])
    twice.integrate(cams[3:], depths[3:], images[3:], weights[3:])
    VC.assert_state_equal(state_of(once), want, "one call")
    VC.assert_state_equal(state_of(twice), want, "two calls")
    bare = volume_of(gpu_pkg, grid, True)
    bare.integrate(cams, depths, None, weights)
    got = state_of(bare)
    assert np.array_equal(got.tsdf.view(np.uint32), want.tsdf.view(np.uint32)) and (got.colour == 0).all()


def test_a_new_volume_and_set_state(gpu_pkg):
    grid = box_grid((9, 5, 3))
    volume = volume_of(gpu_pkg, grid, True)
    tsdf, weight, colour = volume.state()
    assert (tsdf.view(np.uint32) == F(1).view(np.uint32)).all() and (weight.view(np.uint32) == 0).all() and (colour.view(np.uint32) == 0).all()
    _, t, w, c = random_field((9, 5, 3), 5, colour=True)
    volume.set_state(t, None, c)
    got = volume.state()
    assert np.array_equal(got[0], t) and (got[1] == 0).all() and np.array_equal(got[2], c)
    volume.set_state(None, w)
    assert np.array_equal(volume.state()[1], w)


# --------------------------------------------------------------------------------------------------------------------
# extract
# --------------------------------------------------------------------------------------------------------------------

def test_every_field(gpu_pkg, checker, tmp_path):
    """Random fields with unknown samples, with and without colour (CW == 0 at one and at both ends of an edge), zeros and negative
    zeros at samples (triangles without area), nothing known, nothing inside, the sphere whole and in a shell."""
    for name, grid, tsdf, weight, colour in extract_cases():
        want = VC.extract(checker, grid, tsdf, weight, colour)
        mesh = device_extract(gpu_pkg, grid, tsdf, weight, colour)
        VC.assert_mesh_equal(mesh_arrays(mesh), want, name)
        mesh.write_ply(tmp_path / "m.ply")
        assert (tmp_path / "m.ply").read_bytes() == VC.ply_bytes(want), name
        if "nothing" in name:
            assert len(mesh.vertices) == 0 and len(mesh.faces) == 0
        if "zeros" in name:
            V = want.vertices[want.faces]
            assert (np.linalg.norm(np.cross(V[:, 1] - V[:, 0], V[:, 2] - V[:, 0]), axis=1) == 0).any()
        if colour is not None:
            assert (colour[:, 3] == 0).any() and want.colours.any()


def test_every_pattern_of_one_cell(gpu_pkg, checker):
    volume = volume_of(gpu_pkg, one_cell(0)[0])
    for signs in range(256):
        for grid, tsdf, weight in (one_cell(signs), one_cell(0b10010110, known=signs)):
            volume.set_state(tsdf, weight)
            VC.assert_mesh_equal(mesh_arrays(volume.extract_mesh()), VC.extract(checker, grid, tsdf, weight), signs)


def test_counts_around_the_scan_tile(gpu_pkg, checker):
    import ctypes as C
    sort_tile, scan_tile = C.c_int(0), C.c_int(0)
    gpu_pkg.lib().apd_sort_tile_sizes(C.byref(sort_tile), C.byref(scan_tile))
    for target in (scan_tile.value - 1, scan_tile.value, scan_tile.value + 1):
        for what in (0, 1):
            (grid, tsdf, weight), want = field_with_count(checker, target, what)
            assert (len(want.vertices), len(want.faces))[what] == target
            VC.assert_mesh_equal(mesh_arrays(device_extract(gpu_pkg, grid, tsdf, weight)), want, (target, what))


def test_the_mesh_of_an_integrated_volume(gpu_pkg, checker, tmp_path):
    """The planted plane, integrated and extracted on the device, read back as points."""
    grid, size, z0 = planted_plane()
    cam = unit_camera(gpu_pkg, *size)
    volume = volume_of(gpu_pkg, grid, True)
    volume.integrate([cam] * 2, [np.full(size[::-1], z0, F)] * 2, [np.full(size[::-1], 77.0, F)] * 2)
    state = state_of(volume)
    want = VC.extract(checker, grid, state.tsdf, state.weight, state.colour)
    mesh = volume.extract_mesh()
    VC.assert_mesh_equal(mesh_arrays(mesh), want)
    assert len(want.faces) > 50 and (want.vertices[:, 2] == z0).all() and (want.colours == 77).all()
    mesh.write_ply(tmp_path / "plane.ply")
    pts = gpu_pkg.Points.read_ply(tmp_path / "plane.ply")
    assert np.array_equal(np.asarray(pts.xyz).view(np.uint32), want.vertices.view(np.uint32)) and np.array_equal(np.asarray(pts.bgr), want.colours)


# --------------------------------------------------------------------------------------------------------------------
# end to end
# --------------------------------------------------------------------------------------------------------------------

def test_through_the_pipeline(gpu_pkg, ob, checker, tmp_path):
    """pipeline.mesh on a synthetic ring with views of two sizes: the filtered maps stay on the device, and the mesh and its file are
    the checker's of those maps, downloaded, in the box of the fused points.  The filter runs without the consistency factors: with
    them it keeps a tenth of this case's pixels at most, and a tetrahedron needs four observed corners."""
    from apd_mvs_amd import pipeline
    case = fusion_cases.case("mixed_sizes")
    scene, results = _scene(gpu_pkg, pipeline, case)
    voxel = 0.05
    options = gpu_pkg.default_fusion_options(factor_strong=0.0, factor_weak=0.0)
    nv, nf, mesh = pipeline.mesh(scene, results, tmp_path / "mesh.ply", voxel, options=options, return_mesh=True)
    _, points = pipeline.fuse(scene, results, None, options=options, return_points=True)
    lo, hi = pipeline.mesh_bounds(points)
    shape = gpu_pkg.Volume.around(lo, hi, voxel, 4 * voxel, colour=True)
    assert max(shape.dims) < 64 and shape.trunc == F(4 * voxel)
    grid = VC.Grid(shape.dims, shape.origin, shape.voxel, shape.trunc, shape.max_weight)
    maps = pipeline.filter_maps(scene, results, options=options, on_device=True)
    cams, images = pipeline.mesh_views(scene, results, None)
    assert {(c.width, c.height) for c in cams} == {(240, 180), (120, 90)}
    state = VC.integrate(checker, grid, VC.State(grid, colour=True), cams, [m.depth.cpu().numpy() for m in maps], images)
    want = VC.extract(checker, grid, state.tsdf, state.weight, state.colour)
    # The scene is one surface across the box, seen whole by five views in which at least six pixels of ten carry a depth: it crosses
    # every column of cells, and a crossed cell whose corners are known gives six triangles or more (all six tetrahedra share the
    # diagonal the surface cuts).  One triangle for every second column is a bound far below that.
    assert len(want.faces) >= (shape.dims[0] - 1) * (shape.dims[1] - 1) // 2
    VC.assert_mesh_equal(mesh_arrays(mesh), want)
    assert (nv, nf) == (len(want.vertices), len(want.faces))
    assert (tmp_path / "mesh.ply").read_bytes() == VC.ply_bytes(want)
    pts = gpu_pkg.Points.read_ply(tmp_path / "mesh.ply")
    assert np.array_equal(np.asarray(pts.xyz).view(np.uint32), want.vertices.view(np.uint32))
    assert pipeline.mesh(scene, results, None, voxel, bounds=points, options=options) == (nv, nf)
    assert pipeline.mesh(scene, results, None, voxel, bounds=(lo, hi), options=options) == (nv, nf)
    # the surface lies where the ring's scene is: about 2.2 in front of view 0
    assert 1.5 < np.median(want.vertices[:, 2]) < 3.0
    # a map that is not on the volume's device is refused before the library sees its address
    with pytest.raises(ValueError, match="torch tensor on cuda:0"):
        shape.integrate(cams[:1], [maps[0].depth.cpu()], maps_on_device=True)
    with pytest.raises(ValueError, match="torch tensor on cuda:0"):
        shape.integrate(cams[:1], [maps[0].depth.cpu().numpy()], maps_on_device=True)


# --------------------------------------------------------------------------------------------------------------------
# the binary
# --------------------------------------------------------------------------------------------------------------------

def _outputs(folder):
    """{relative path: bytes} of everything under <folder>/APD."""
    root = folder / "APD"
    return {str(p.relative_to(root)): p.read_bytes() for p in sorted(root.rglob("*")) if p.is_file()}


@pytest.fixture(scope="module")
def folders(gpu_pkg, synth, tmp_path_factory):
    """One small synthetic dense folder (the size of the drop-in tests), run without the flag and then with it, at a voxel of a 40th
    of the longest side of the box of the cloud the first run wrote."""
    root = tmp_path_factory.mktemp("dense")
    a = root / "a"
    a.mkdir()
    _write_dense_folder(a, synth, 96, 72, 4)
    shutil.copytree(a, root / "plain")
    out = {"plain": (root / "plain", _run(root / "plain"))}
    cloud = gpu_pkg.Points.read_ply(root / "plain" / "APD" / "APD.ply")
    xyz = np.asarray(cloud.xyz)
    voxel = "%.9g" % F((xyz.max(0) - xyz.min(0)).max() / 40)
    shutil.copytree(a, root / "mesh")
    out["mesh"] = (root / "mesh", _run(root / "mesh", "--mesh", voxel))
    out["voxel"] = float(F(voxel))
    return out


def test_binary_writes_the_mesh_of_the_pipeline(gpu_pkg, folders, tmp_path):
    """APD.ply.mesh beside the cloud holds the bytes pipeline.mesh writes of the maps the binary kept, with the views' colour images;
    every other output has the bytes it has without the flag."""
    from apd_mvs_amd import pipeline
    folder, ply = folders["mesh"]
    plain, with_mesh = _outputs(folders["plain"][0]), _outputs(folder)
    assert ply == folders["plain"][1] and "APD.ply.mesh" not in plain
    assert set(with_mesh) == set(plain) | {"APD.ply.mesh"}
    assert all(with_mesh[name] == plain[name] for name in plain)
    scene = pipeline.load_dense_folder(str(folder), gpu_pkg.Camera)
    results = {}
    for v in range(scene.num_views):
        d = folder / "APD" / ("%08d" % scene.ids[v])
        results[v] = pipeline.ViewState(_read_dmb(d / "depths.dmb"), _read_dmb(d / "normals.dmb"), _read_dmb(d / "weak.bin"), _read_dmb(d / "selected_views.bin"))
    colour = pipeline.load_colour_images(str(folder), scene.ids[:scene.num_views])
    nv, nf = pipeline.mesh(scene, results, tmp_path / "pipe.ply", folders["voxel"], colour_images=colour)
    assert with_mesh["APD.ply.mesh"] == (tmp_path / "pipe.ply").read_bytes()
    assert with_mesh["APD.ply.mesh"].startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % nv) and b"element face %d\n" % nf in with_mesh["APD.ply.mesh"][:400]
    assert gpu_pkg.Points.read_ply(folder / "APD" / "APD.ply.mesh").count == nv


def test_binary_refuses_a_bad_mesh_value_before_anything_is_read(tmp_path):
    for bad in ("", "0", "-1", "x", "0.1,", ",0.4", "0.1,0", "0.1,nan", "inf", "0.1,0.4,1"):
        r = subprocess.run([APD_BIN, str(tmp_path / "no_such_folder"), "0", "--mesh", bad], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
        assert r.returncode != 0 and "bad value '%s' of --mesh" % bad in r.stdout and "USAGE" in r.stdout, (bad, r.stdout[-500:])
    r = subprocess.run([APD_BIN, str(tmp_path / "no_such_folder"), "0", "--mesh", "0.1", "--no-fusion"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=60)
    assert r.returncode != 0 and "not with --no-fusion" in r.stdout and "USAGE" in r.stdout
    for good in ("0.1", "0.1,0.4", "1e-3,0.5"):
        r = subprocess.run([APD_BIN, str(tmp_path / "no_such_folder"), "0", "--mesh", good], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
        assert r.returncode != 0 and "bad value" not in r.stdout and "USAGE" not in r.stdout, (good, r.stdout[-500:])
