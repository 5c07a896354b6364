"""The rendered maps and the rendered visibility on the device (apd_points_render, apd_points_rendered_visibility;
csrc/apd_points_render.hip), bitwise against the sequential checker (tests/helpers/points_render_ref.cpp): depth as uint32 (so that
-0 or a NaN would show), index, `unseen`, the lists, support, the merged flag and every copied array, for host- and for
device-resident points, the input unchanged afterwards.  The clouds and cameras are made in test_points_render.py, where the checker
is held against a numpy restatement on them."""
import shutil
import subprocess

import numpy as np
import pytest

import fusion_cases
import points_render_checker as PRC
import points_voxel_checker as PV
import vis_checker as VC
from test_gpu_dropin_binary import _write_dense_folder
from test_gpu_fusion_options import APD_BIN, _fuse_saved_maps, _run, _scene
from test_gpu_points_average import fused
from test_points_radius import dressed
from test_points_render import (F, H0, SIZES, SMALL_IMAGES, SPLATS, W0, assert_maps, contention_cases, long_axis_case, not_drawn_case, pinhole, pixel_points,
                                ring_cameras, size_case, sphere_points, two_planes, unit_camera)
from test_points_voxel import arrays_of, from_cloud, ply_bytes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return PRC.build(tmp_path_factory.mktemp("points_render_checker"))


@pytest.fixture(scope="module")
def voxel_checker(tmp_path_factory):
    return PV.build(tmp_path_factory.mktemp("points_voxel_checker"))


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def maps_of(pts, cam, splat):
    depth, index = pts.render(cam, splat)
    depth, index = host(depth), host(index)
    assert depth.dtype == np.float32 and depth.shape == index.shape == (cam.height, cam.width)
    return depth, index.view(np.uint32)


def check_render(pkg, checker, c, views, cams, splats, what=""):
    """render() of the cloud `c` (a PV.Cloud over views = (rows, cols, pairs)) into every camera at every splat, as host- and as
    device-resident points, against the checker; the input is unchanged afterwards.  Returns the checker's maps of the last call."""
    want = {(s, splat): PRC.render(checker, c, cam, splat) for s, cam in enumerate(cams) for splat in splats}
    for dev in (False, True):
        pts = from_cloud(pkg, c, *views, on_device=dev)
        for (s, splat), maps in want.items():
            assert_maps(maps_of(pts, cams[s], splat), maps, (what, dev, s, splat))
        PV.assert_equal(arrays_of(pts), c, (what, dev, "the input"))
        pts.close()
    return list(want.values())[-1]


def check_lists(pts, c, want, cams, splat, tol, what=""):
    """with_rendered_visibility of `pts`, which holds the cloud `c`, against the checker's lists `want`.  Returns the new object."""
    new, unseen = pts.with_rendered_visibility(cams, splat, tol)
    assert new.on_device == pts.on_device and new.merged and new.count == c.count and unseen == want.unseen, (what, unseen, want.unseen)
    PV.assert_equal(arrays_of(new), PRC.with_lists(c, want), what)   # the lists and support are the checker's, the six other arrays are copied
    return new


def check_visibility(pkg, checker, c, views, cams, settings, what=""):
    """Every (splat, rel_tolerance) of `settings`, as host- and as device-resident points; the input is unchanged afterwards.
    Returns the checker's lists per setting."""
    want = {st: PRC.visibility(checker, c, cams, *st) for st in settings}
    for dev in (False, True):
        pts = from_cloud(pkg, c, *views, on_device=dev)
        before = arrays_of(pts)
        for st, lists in want.items():
            check_lists(pts, c, lists, cams, *st, what=(what, dev, st)).close()
        PV.assert_equal(arrays_of(pts), before, (what, dev, "the input"))
        pts.close()
    return want


# --------------------------------------------------------------------------------------------------------------------
# the maps
# --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_waves_and_blocks(gpu_pkg, checker, n):
    c, views = size_case(n)
    _, index = check_render(gpu_pkg, checker, c, views, [pinhole(gpu_pkg, W0, H0)], (0, 1), what=n)
    assert n < 63 or (index != PRC.NO_INDEX).any()   # the one point of n = 1 may lie outside the image


@pytest.mark.parametrize("W,H", SMALL_IMAGES)
def test_small_images_with_clipped_footprints(gpu_pkg, checker, W, H):
    """Points on every pixel, so on every corner and edge; a footprint of 17 x 17 pixels is larger than every one of these images."""
    c, views = dressed(np.random.default_rng(1), pixel_points(np.random.default_rng(2), W, H))
    _, index = check_render(gpu_pkg, checker, c, views, [unit_camera(gpu_pkg, W, H)], SPLATS, what=(W, H))
    assert (index != PRC.NO_INDEX).all()


@pytest.mark.parametrize("W,H", [(16384, 2), (2, 16384)])
def test_long_axes(gpu_pkg, checker, W, H):
    c, views = dressed(np.random.default_rng(3), long_axis_case(np.random.default_rng(4), W, H))
    _, index = check_render(gpu_pkg, checker, c, views, [unit_camera(gpu_pkg, W, H)], (0, 2), what=(W, H))
    assert index[0, 0] != PRC.NO_INDEX and index[H - 1, W - 1] != PRC.NO_INDEX


def test_contention_on_one_pixel(gpu_pkg, checker):
    """4096 points on one pixel: distinct depths in random order, one depth (index 0 wins), two adjacent binary32 depths."""
    cam = unit_camera(gpu_pkg, 5, 4)
    for name, xyz in contention_cases(np.random.default_rng(71)).items():
        c, views = dressed(np.random.default_rng(5), xyz)
        _, index = check_render(gpu_pkg, checker, c, views, [cam], (0, 2), what=name)
        assert (index != PRC.NO_INDEX).all() and len(set(index.ravel().tolist())) == 1   # a footprint of 5 x 5 covers the image: one winner
        assert name != "same" or index[1, 2] == 0
        check_visibility(gpu_pkg, checker, c, views, [cam], [(0, 0.0), (2, 0.0)], what=name)


def test_the_same_call_five_times_gives_identical_bytes(gpu_pkg, checker):
    cam = unit_camera(gpu_pkg, 5, 4)
    c, views = dressed(np.random.default_rng(5), contention_cases(np.random.default_rng(71))["distinct"])
    pts = from_cloud(gpu_pkg, c, *views, on_device=True)
    runs = []
    for _ in range(5):
        depth, index = maps_of(pts, cam, 2)
        new, unseen = pts.with_rendered_visibility([cam, cam], 1, 0.0)
        lists = arrays_of(new)
        runs.append((depth.tobytes(), index.tobytes(), lists.offsets.tobytes(), lists.views.tobytes(), lists.support.tobytes(), unseen))
        new.close()
    assert all(r == runs[0] for r in runs[1:]) and runs[0][5] == c.count - 1


def test_points_that_are_not_drawn(gpu_pkg, checker):
    xyz, drawn = not_drawn_case()
    c, views = dressed(np.random.default_rng(6), xyz)
    cam = unit_camera(gpu_pkg, 5, 4)
    _, index = check_render(gpu_pkg, checker, c, views, [cam], (0, 1))
    assert set(index[index != PRC.NO_INDEX].tolist()) <= set(np.flatnonzero(drawn).tolist())
    want = check_visibility(gpu_pkg, checker, c, views, [cam], [(0, 1e30)])
    assert np.array_equal(np.diff(want[(0, 1e30)].offsets) == 1, drawn)


def test_rotated_translated_skewed_cameras_and_one_behind_the_cloud(gpu_pkg, checker):
    rng = np.random.default_rng(7)
    c, views = dressed(rng, sphere_points(rng))
    cams = ring_cameras(gpu_pkg, 5)
    assert any(cam.K[1] != 0 for cam in cams) and any(cam.K[0] != cam.K[4] for cam in cams)
    check_render(gpu_pkg, checker, c, views, cams, (0, 1))
    behind = pinhole(gpu_pkg, W0, H0, R=np.diag([-1.0, 1.0, -1.0]).reshape(9))
    far, _ = dressed(rng, sphere_points(rng) + F([0, 0, 5]))
    depth, index = check_render(gpu_pkg, checker, far, views, [behind], (1,))
    assert (index == PRC.NO_INDEX).all() and (depth.view(np.uint32) == 0).all()
    assert check_visibility(gpu_pkg, checker, far, views, [behind], [(1, 0.01)])[(1, 0.01)].unseen == far.count


# --------------------------------------------------------------------------------------------------------------------
# the lists
# --------------------------------------------------------------------------------------------------------------------

def test_two_planes_from_three_cameras(gpu_pkg, checker):
    xyz, cams, front, behind = two_planes(gpu_pkg, 2)
    c, views = dressed(np.random.default_rng(8), xyz)
    want = check_visibility(gpu_pkg, checker, c, views, cams, [(1, 0.01), (0, 0.01), (1, 0.0)])
    seen_by_first = lambda lists: np.array([0 in lists.views[a:b] for a, b in zip(lists.offsets[:-1], lists.offsets[1:])])
    assert seen_by_first(want[(1, 0.01)])[front].all() and not seen_by_first(want[(1, 0.01)])[behind].any()
    assert seen_by_first(want[(0, 0.01)])[behind].any()


@pytest.mark.parametrize("V", [1, 32, 33, 40])
def test_ring_of_cameras_around_a_sphere(gpu_pkg, checker, voxel_checker, V, tmp_path):
    """The bitset's word boundary; tolerances of 0, 0.01 and one that sees every drawn point; the result written, and merged again."""
    rng = np.random.default_rng(9)
    c, views = dressed(rng, sphere_points(rng))
    cams = ring_cameras(gpu_pkg, V)
    want = check_visibility(gpu_pkg, checker, c, views, cams, [(1, 0.0), (1, 0.01), (0, 1e30)], what=V)
    assert len(want[(1, 0.0)].views) < len(want[(1, 0.01)].views) < len(want[(0, 1e30)].views)
    assert int(want[(0, 1e30)].views.max()) == V - 1
    lists = want[(1, 0.01)]
    for dev in (False, True):
        new, _ = from_cloud(gpu_pkg, c, *views, on_device=dev).with_rendered_visibility(cams, 1, 0.01)
        new.write_vis(tmp_path / "v.vis")
        assert (tmp_path / "v.vis").read_bytes() == VC.vis_bytes(lists.offsets, lists.views)
        new.write_ply(tmp_path / "v.ply", normals=True)
        assert (tmp_path / "v.ply").read_bytes() == ply_bytes(c, True)
        again, _ = new.merge_voxels(0.25)
        PV.assert_equal(arrays_of(again), PV.merge(voxel_checker, PRC.with_lists(c, lists), 0.25), (V, dev))
        kept, _ = new.remove_sparse(0.2, 3)
        assert kept.merged and 0 < kept.count <= c.count
        with pytest.raises(gpu_pkg.ApdError, match="merged points name no sources"):
            new.average(cams, [np.zeros((4, 5), F)] * V, [np.zeros((4, 5, 3), F)] * V)


def test_a_merged_object_as_input(gpu_pkg, checker, voxel_checker):
    rng = np.random.default_rng(10)
    c, views = dressed(rng, sphere_points(rng))
    first = PV.merge(voxel_checker, c, 0.1)
    cams = ring_cameras(gpu_pkg, 7)
    want = PRC.visibility(checker, first, cams, 1, 0.01)
    for dev in (False, True):
        merged, _ = from_cloud(gpu_pkg, c, *views, on_device=dev).merge_voxels(0.1)
        check_lists(merged, first, want, cams, 1, 0.01, what=dev)
        PV.assert_equal(arrays_of(merged), first, "the input")


def test_a_real_cloud_into_each_of_its_views(gpu_pkg, ob, checker):
    case = fusion_cases.case("mixed_sizes")
    cams = list(case.cameras(gpu_pkg.make_camera))
    for dev in (False, True):
        pts = fused(gpu_pkg, ob, case, "eth", dev)
        before = arrays_of(pts)
        for s, cam in enumerate(cams):
            for splat in (0, 1):
                maps = PRC.render(checker, before, cam, splat)
                assert (maps[1] != PRC.NO_INDEX).any()
                assert_maps(maps_of(pts, cam, splat), maps, (dev, s, splat))
        want = PRC.visibility(checker, before, cams, 1, 0.01)
        assert 0 < len(want.views)
        check_lists(pts, before, want, cams, 1, 0.01, what=dev)
        PV.assert_equal(arrays_of(pts), before, "the input")


# --------------------------------------------------------------------------------------------------------------------
# the pipeline and the binary
# --------------------------------------------------------------------------------------------------------------------

def test_through_the_pipeline(gpu_pkg, ob, checker, tmp_path):
    """fuse(render_visibility=...) returns and writes the points with the rendered lists, after every other step; the PLY file keeps
    its bytes."""
    from apd_mvs_amd import pipeline
    case = fusion_cases.case("mixed_sizes")
    scene, results = _scene(gpu_pkg, pipeline, case)
    cams = [scene.cameras[v] for v in range(scene.num_views)]
    for kw in (dict(), dict(average=True, voxel=0.05)):
        _, whole = pipeline.fuse(scene, results, tmp_path / "before.ply", return_points=True, **kw)
        w = arrays_of(whole)
        want = PRC.visibility(checker, w, cams, 1, 0.01)
        n, new = pipeline.fuse(scene, results, tmp_path / "m.ply", return_points=True, vis_path=tmp_path / "m.vis", render_visibility=(1, 0.01), **kw)
        assert n == w.count and new.merged
        PV.assert_equal(arrays_of(new), PRC.with_lists(w, want), kw)
        assert (tmp_path / "m.ply").read_bytes() == (tmp_path / "before.ply").read_bytes()
        assert (tmp_path / "m.vis").read_bytes() == VC.vis_bytes(want.offsets, want.views)
        assert pipeline.fuse(scene, results, None, vis_path=tmp_path / "only.vis", render_visibility=(1, 0.01), **kw) == n
        assert (tmp_path / "only.vis").read_bytes() == (tmp_path / "m.vis").read_bytes()


@pytest.fixture(scope="module")
def folders(gpu_pkg, synth, tmp_path_factory):
    """One small synthetic dense folder (the size of the drop-in tests), run without the flag and with it."""
    root = tmp_path_factory.mktemp("dense")
    a = root / "a"
    a.mkdir()
    _write_dense_folder(a, synth, 96, 72, 4)
    out = {}
    for name, extra in (("plain", []), ("rendered", ["--ply-render-vis", "1,0.01"])):
        shutil.copytree(a, root / name)
        out[name] = (root / name, _run(root / name, *extra))
    return out


def test_binary_writes_the_rendered_lists(gpu_pkg, checker, folders):
    """APD.ply keeps the bytes it has without the flag; APD.ply.vis, which the flag implies, holds the checker's lists of the points the
    pipeline makes from the binary's maps, drawn into the folder's cameras."""
    from apd_mvs_amd import pipeline
    folder, ply = folders["rendered"]
    assert ply == folders["plain"][1]
    assert not (folders["plain"][0] / "APD" / "APD.ply.vis").exists()
    _, whole = _fuse_saved_maps(gpu_pkg, folder, None, return_points=True)
    scene = pipeline.load_dense_folder(str(folder), gpu_pkg.Camera)
    want = PRC.visibility(checker, arrays_of(whole), [scene.cameras[v] for v in range(scene.num_views)], 1, 0.01)
    assert 0 < len(want.views)
    assert (folder / "APD" / "APD.ply.vis").read_bytes() == VC.vis_bytes(want.offsets, want.views)


def test_binary_refuses_a_bad_value_before_anything_is_read(tmp_path):
    for bad in ("9,0.01", "-1,0.01", "1", "1,", ",0.01", "1,-0.5", "1,nan", "1,inf", "1,x", "1x,0.01", "1.5,0.01", "01,0.01", ""):
        r = subprocess.run([APD_BIN, str(tmp_path / "no_such_folder"), "0", "--ply-render-vis", bad], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=60)
        assert r.returncode != 0 and "bad value '%s' of --ply-render-vis" % bad in r.stdout and "USAGE" in r.stdout, (bad, r.stdout[-500:])
    for good in ("0,0", "8,0.01", "1,1e30"):
        r = subprocess.run([APD_BIN, str(tmp_path / "no_such_folder"), "0", "--ply-render-vis", good], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=60)
        assert r.returncode != 0 and "bad value" not in r.stdout and "USAGE" not in r.stdout, (good, r.stdout[-500:])
