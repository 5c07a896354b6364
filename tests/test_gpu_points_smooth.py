"""The smoothed positions on the device (apd_points_smoothed_positions, apd_points_with_smoothed_positions;
csrc/apd_points_smooth.hip, compact_points of csrc/apd_points.hip), bitwise against the grid mode of the sequential checker
(tests/helpers/points_smooth_ref.cpp): positions and offsets as uint32 (so that inf, NaN payloads and -0 count), `moved`, all seven
arrays and the lists of the new object, for host- and for device-resident points, the input unchanged afterwards; the sizes and the
cells a walk can go wrong on; the longest binary64 sums; planted, noisy, degenerate and order clouds; iterations that change
cells; a real cloud; a merged object; a chain; the pipeline and the drop-in binary.  The clouds are made in test_points_radius.py,
test_points_normals.py and test_points_smooth.py, where the checker's brute-force mode is held against the grid mode on them."""
import shutil
import subprocess

import numpy as np
import pytest

import fusion_cases
import points_normals_checker as PN
import points_radius_checker as PR
import points_smooth_checker as PS
import points_voxel_checker as PV
import vis_checker as VC
from test_gpu_dropin_binary import _write_dense_folder
from test_gpu_fusion_options import APD_BIN, _fuse_saved_maps, _run, _scene
from test_gpu_points_average import fused
from test_points_normals import REAL_CLOUD, REAL_MIN, SIZE_MINS, bits32, cube_case, degenerate_cases, order_cases, plane_case, sign_cases, sphere_case
from test_points_radius import (DENSE_ORIGIN, DENSE_RADIUS, MERGED_RADIUS, border_case, dense_case, determinism_case, dressed, grid_edge_case, large_case,
                                merged_many_views_case, outside_case, real_cloud_radius, size_case, size_list)
from test_points_smooth import ITERATIONS, LIFT_RADIUS, lifted_lattice_case, noisy_plane_case, noisy_slab_case
from test_points_voxel import arrays_of, from_cloud, ply_bytes, views_of

pytestmark = pytest.mark.gpu
PLAIN_VIEWS = views_of(1)     # of the clouds test_points_normals.py and test_points_smooth.py make: one view without sources


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return PS.build(tmp_path_factory.mktemp("points_smooth_checker"))


@pytest.fixture(scope="module")
def normals_checker(tmp_path_factory):
    return PN.build(tmp_path_factory.mktemp("points_normals_checker"))


@pytest.fixture(scope="module")
def radius_checker(tmp_path_factory):
    return PR.build(tmp_path_factory.mktemp("points_radius_checker"))


@pytest.fixture(scope="module")
def voxel_checker(tmp_path_factory):
    return PV.build(tmp_path_factory.mktemp("points_voxel_checker"))


def host_bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    assert a.dtype == np.float32
    return bits32(a)


def check_points(pts, c, want, radius, k, origin=None, merged=False, what=""):
    """smoothed_positions (against want[1]) and with_smoothed_positions for every iteration count of `want` ({iterations: the
    checker's result}) of `pts`, which holds the cloud `c`; the input is unchanged afterwards.  Returns the last new object."""
    xyz, offset = pts.smoothed_positions(radius, k, origin)
    assert xyz.shape == (c.count, 3) and offset.shape == (c.count,), what
    differ = np.flatnonzero((host_bits(xyz) != bits32(want[1].xyz)).any(axis=1) | (host_bits(offset) != bits32(want[1].offset)))
    assert differ.size == 0, (what, differ[:5], want[1].xyz[differ[:5]], want[1].offset[differ[:5]], want[1].sweeps[differ[:5]])
    new = None
    for it, res in want.items():
        new, moved = pts.with_smoothed_positions(radius, k, it, origin)
        assert new.on_device == pts.on_device and new.merged == merged and new.count == c.count and moved == res.moved, (what, it, moved, res.moved)
        PV.assert_equal(arrays_of(new), PS.with_positions(c, res), (what, it))
    PV.assert_equal(arrays_of(pts), c, (what, "the input"))
    return new


def check(pkg, checker, c, views, radius, ks, origin=None, iterations=ITERATIONS, what=""):
    """Every min_neighbours of `ks` and every iteration count on `c` (a PV.Cloud over views = (rows, cols, pairs)), as host- and
    as device-resident points, against the checker's grid mode.  Returns {min_neighbours: {iterations: the checker's result}}."""
    want = {k: {it: PS.run(checker, c, radius, k, it, origin) for it in (1,) + tuple(i for i in iterations if i != 1)} for k in ks}
    for dev in (False, True):
        pts = from_cloud(pkg, c, *views, on_device=dev)
        for k, by in want.items():
            check_points(pts, c, {it: by[it] for it in iterations}, radius, k, origin, what=(what, dev, k))
        pts.close()
    return want


# --------------------------------------------------------------------------------------------------------------------
# sizes, cells, long sums
# --------------------------------------------------------------------------------------------------------------------

def test_sizes_around_waves_blocks_and_tiles(gpu_pkg, checker):
    """n = 0, 1, 2, around a wave and a block, 3 T + 17 and 5 T + 17, about three points per cell at radius 1, min_neighbours 2 and 7."""
    for n in size_list(gpu_pkg):
        c, views = size_case(gpu_pkg, n)
        got = check(gpu_pkg, checker, c, views, 1.0, SIZE_MINS, what=n)
        assert n < 63 or (0 < got[7][1].moved < got[2][1].moved < n)


def test_cell_borders(gpu_pkg, checker):
    """Pairs at exactly the radius and at the next binary32 after it, in positive and negative cells, across a border and two cells
    apart, coincident points: a point has an estimate where the hand-computed count reaches 2."""
    xyz, counts = border_case()
    c, views = dressed(np.random.default_rng(1), xyz)
    got = check(gpu_pkg, checker, c, views, 1.0, (2, 7))
    assert np.array_equal(got[2][1].estimated, np.array(counts) >= 2)


def test_edges_of_the_grid(gpu_pkg, checker):
    xyz, counts = grid_edge_case()
    c, views = dressed(np.random.default_rng(2), xyz)
    got = check(gpu_pkg, checker, c, views, 1.0, (2, 7))
    assert np.array_equal(got[2][1].estimated, np.array(counts) >= 2) and got[2][1].moved > 0


def test_points_outside_the_grid(gpu_pkg, checker):
    """NaN, infinities and points 3 * 2^20 cells out among ordinary points keep their position, bit for bit, and get +inf; and a
    cloud with every point outside: nothing moves."""
    xyz, bad = outside_case(np.random.default_rng(4))
    c, views = dressed(np.random.default_rng(3), xyz)
    got = check(gpu_pkg, checker, c, views, 1.0, (2, 7))
    for it in ITERATIONS:
        assert not got[2][it].ever[bad].any() and np.isinf(got[2][it].offset[bad]).all() and got[2][it].moved > 0
        assert np.array_equal(bits32(got[2][it].xyz[bad]), bits32(c.xyz[bad]))
    none = dressed(np.random.default_rng(5), np.full((300, 3), np.nan, np.float32))
    assert check(gpu_pkg, checker, *none, 1.0, (2, 7))[2][3].moved == 0


def test_one_cell_of_twenty_thousand_members(gpu_pkg, checker):
    """20 001 points in one cell: the longest binary64 sums, and every lane of a wave has its own.  One iteration."""
    c, views = dressed(np.random.default_rng(7), dense_case(np.random.default_rng(8)))
    got = check(gpu_pkg, checker, c, views, DENSE_RADIUS, SIZE_MINS, origin=DENSE_ORIGIN, iterations=(1,))
    assert got[2][1].estimated.all() and got[7][1].estimated.all()


def test_two_hundred_thousand_points(gpu_pkg, checker):
    """One iteration."""
    c, views = dressed(np.random.default_rng(9), large_case(np.random.default_rng(10)))
    got = check(gpu_pkg, checker, c, views, 1.0, SIZE_MINS, iterations=(1,))
    assert 0 < got[7][1].moved < got[2][1].moved < c.count


# --------------------------------------------------------------------------------------------------------------------
# planted, noisy, degenerate and order clouds; iterations that change cells
# --------------------------------------------------------------------------------------------------------------------

def test_planted_clouds(gpu_pkg, checker):
    plane, _ = plane_case(np.random.default_rng(31))
    assert check(gpu_pkg, checker, plane, PLAIN_VIEWS, 1.0, SIZE_MINS, what="plane")[7][1].moved > 0.95 * plane.count
    noisy, _ = noisy_plane_case(np.random.default_rng(41))
    assert check(gpu_pkg, checker, noisy, PLAIN_VIEWS, 1.0, SIZE_MINS, what="noisy plane")[7][1].moved > 0.95 * noisy.count
    sphere = sphere_case(np.random.default_rng(32))
    assert check(gpu_pkg, checker, sphere, PLAIN_VIEWS, 1.0, SIZE_MINS, what="sphere")[7][1].moved > 0.8 * sphere.count
    cube, _ = cube_case(np.random.default_rng(33))
    assert check(gpu_pkg, checker, cube, PLAIN_VIEWS, 1.0, SIZE_MINS, what="cube")[7][1].estimated.all()
    lattice, _ = lifted_lattice_case()
    got = check(gpu_pkg, checker, lattice, PLAIN_VIEWS, LIFT_RADIUS, SIZE_MINS + (24,), what="lifted lattice")
    assert got[7][1].estimated.all() and 0 < got[24][1].moved < lattice.count     # neighbours at exactly the radius count


def test_iterations_that_change_cells(gpu_pkg, checker):
    """The noisy slab around a cell border, where one iteration takes hundreds of points into another cell
    (test_points_smooth.py): the device rebuilds the grid and the order for every iteration, or the bits differ."""
    c, outside = noisy_slab_case(np.random.default_rng(42))
    got = check(gpu_pkg, checker, c, PLAIN_VIEWS, 1.0, SIZE_MINS, iterations=(1, 2, 3), what="noisy slab")[7]
    assert not np.array_equal(bits32(got[2].xyz), bits32(got[1].xyz)) and not np.array_equal(bits32(got[3].xyz), bits32(got[2].xyz))
    assert not got[3].ever[outside].any()


def test_degenerate_sign_and_order_clouds(gpu_pkg, checker):
    """Zero, NaN and exactly orthogonal stored normals; coincident and collinear points; one cell's points in three input orders,
    where the order of the sums shows in the results."""
    for name, c in sign_cases(np.random.default_rng(34)).items():
        assert check(gpu_pkg, checker, c, PLAIN_VIEWS, 1.0, SIZE_MINS, what=name)[2][1].moved >= c.count - 1
    for name, c in degenerate_cases().items():
        got = check(gpu_pkg, checker, c, PLAIN_VIEWS, 1.0, SIZE_MINS if c.count > 7 else (2,), what=name)[2]
        assert got[3].estimated.all() and np.isfinite(got[3].xyz).all()
    for j, (c, _) in enumerate(order_cases(np.random.default_rng(35))):
        assert check(gpu_pkg, checker, c, PLAIN_VIEWS, 1.0, SIZE_MINS, what=("order", j))[7][1].estimated.all()


# --------------------------------------------------------------------------------------------------------------------
# a real cloud, merged objects, two runs, a chain
# --------------------------------------------------------------------------------------------------------------------

def test_a_real_cloud(gpu_pkg, ob, radius_checker, checker):
    """Fused on the device and smoothed where it is, at the radius of the radius filter's tests: some points move and some do
    not.  The lists of the result, built from its sources, are the input's."""
    name, variant, _ = REAL_CLOUD
    case = fusion_cases.case(name)
    radius = None
    for dev in (False, True):
        pts = fused(gpu_pkg, ob, case, variant, dev)
        before = arrays_of(pts)
        radius = radius or real_cloud_radius(radius_checker, before)
        want = {it: PS.run(checker, before, radius, REAL_MIN, it) for it in ITERATIONS}
        assert 0 < want[1].moved < before.count
        check_points(pts, before, want, radius, REAL_MIN, what=(name, variant, dev))


def test_a_merged_object_of_many_views(gpu_pkg, checker, voxel_checker):
    """Lists of up to 200 views that no mask holds: the lists and the merged flag are handed on."""
    c, views, first = merged_many_views_case(voxel_checker)
    want = {k: {it: PS.run(checker, first, MERGED_RADIUS, k, it) for it in ITERATIONS} for k in SIZE_MINS}
    assert 0 < want[2][1].moved and np.diff(first.offsets).max() > 32
    for dev in (False, True):
        merged, _ = from_cloud(gpu_pkg, c, *views, on_device=dev).merge_voxels(1.0)
        for k in SIZE_MINS:
            new = check_points(merged, first, want[k], MERGED_RADIUS, k, merged=True, what=(dev, k))
            assert np.array_equal(arrays_of(new).support, first.support)


def test_two_runs_give_the_same_bits(gpu_pkg, checker):
    c, views = determinism_case()
    origin = [0.25, -0.5, 0.125]
    pts = from_cloud(gpu_pkg, c, *views, on_device=True)
    runs = []
    for run in range(2):
        new, moved = pts.with_smoothed_positions(1.0, 4, 3, origin)
        xyz, offset = pts.smoothed_positions(1.0, 4, origin)
        runs.append((host_bits(new.xyz).tobytes(), host_bits(xyz).tobytes(), host_bits(offset).tobytes(), moved))
    assert runs[0] == runs[1]
    want = PS.run(checker, c, 1.0, 4, 3, origin)
    assert 0 < want.moved < c.count and runs[0][0] == bits32(want.xyz).tobytes() and runs[0][3] == want.moved


def plain(c):
    return PV.Cloud(*[getattr(c, f) for f in PV.FIELDS], c.offsets, c.views)


def test_remove_sparse_then_smooth_then_estimate_normals(gpu_pkg, ob, radius_checker, normals_checker, checker, tmp_path):
    """The chain a user runs, against the checkers chained the same way: the files have the checkers' bytes."""
    case = fusion_cases.case("mixed_sizes")
    for dev in (False, True):
        pts = fused(gpu_pkg, ob, case, "eth", dev)
        before = arrays_of(pts)
        radius = real_cloud_radius(radius_checker, before)
        kept_want = plain(PR.remove(radius_checker, before, radius, 2))
        kept, _ = pts.remove_sparse(radius, 2)
        smooth_want = PS.run(checker, kept_want, radius, REAL_MIN, 2)
        assert 0 < smooth_want.moved
        smoothed, moved = kept.with_smoothed_positions(radius, REAL_MIN, 2)
        assert moved == smooth_want.moved
        smoothed_want = PS.with_positions(kept_want, smooth_want)
        normal_want = PN.run(normals_checker, smoothed_want, radius, REAL_MIN)
        final, estimated = smoothed.with_estimated_normals(radius, REAL_MIN)
        assert estimated == normal_want.count > 0
        final_want = PN.with_normals(smoothed_want, normal_want)
        PV.assert_equal(arrays_of(final), final_want, dev)
        final.write_ply(tmp_path / "n.ply", normals=True)
        final.write_vis(tmp_path / "n.vis")
        assert (tmp_path / "n.ply").read_bytes() == ply_bytes(final_want, True)
        assert (tmp_path / "n.vis").read_bytes() == VC.vis_bytes(final_want.offsets, final_want.views)


# --------------------------------------------------------------------------------------------------------------------
# the pipeline and the binary
# --------------------------------------------------------------------------------------------------------------------

SMOOTH_ITERATIONS = 2


def chosen(radius_checker, checker, whole):
    """(radius, the cloud, the checker's result) for a Points object: the radius of the real clouds, REAL_MIN neighbours."""
    w = arrays_of(whole)
    radius = real_cloud_radius(radius_checker, w)
    want = PS.run(checker, w, radius, REAL_MIN, SMOOTH_ITERATIONS)
    assert want.moved > 0
    return radius, w, want


def test_through_the_pipeline(gpu_pkg, ob, radius_checker, normals_checker, checker, tmp_path):
    """fuse(smooth=...) returns and writes the points with the new positions, after the filters and before the normals: the bytes
    of file-only against the returned points against the manual chain, which are the checkers'."""
    from apd_mvs_amd import pipeline
    case = fusion_cases.case("mixed_sizes")
    scene, results = _scene(gpu_pkg, pipeline, case)
    options = gpu_pkg.default_fusion_options(ply_normals=1)
    for kw in (dict(), dict(average=True, voxel=0.05, component_filter=(0.2, 2))):
        _, whole = pipeline.fuse(scene, results, None, return_points=True, **kw)
        radius, w, want = chosen(radius_checker, checker, whole)
        expect = PS.with_positions(w, want)
        manual, _ = whole.with_smoothed_positions(radius, REAL_MIN, SMOOTH_ITERATIONS)
        manual.write_ply(tmp_path / "manual.ply", normals=True)
        manual.write_vis(tmp_path / "manual.vis")
        smooth = (radius, REAL_MIN, SMOOTH_ITERATIONS)
        n, new = pipeline.fuse(scene, results, tmp_path / "m.ply", return_points=True, vis_path=tmp_path / "m.vis", smooth=smooth, options=options, **kw)
        assert n == w.count == new.count and new.merged == ("voxel" in kw)
        PV.assert_equal(arrays_of(new), expect, kw)
        assert (tmp_path / "m.ply").read_bytes() == (tmp_path / "manual.ply").read_bytes() == ply_bytes(expect, True)
        assert (tmp_path / "m.vis").read_bytes() == (tmp_path / "manual.vis").read_bytes() == VC.vis_bytes(w.offsets, w.views)
        assert pipeline.fuse(scene, results, tmp_path / "file_only.ply", smooth=smooth, options=options, **kw) == n
        assert (tmp_path / "file_only.ply").read_bytes() == (tmp_path / "m.ply").read_bytes()
        # the normals are estimated on the smoothed cloud
        normal_want = PN.run(normals_checker, expect, radius, REAL_MIN)
        n, both = pipeline.fuse(scene, results, tmp_path / "both.ply", return_points=True, smooth=smooth, estimate_normals=(radius, REAL_MIN),
                                options=options, **kw)
        PV.assert_equal(arrays_of(both), PN.with_normals(expect, normal_want), kw)
        assert (tmp_path / "both.ply").read_bytes() == ply_bytes(PN.with_normals(expect, normal_want), True)


VOXEL = "0.25"
# the flags of a run before --ply-smooth and what the pipeline needs to make the points the step starts from
RUNS = {"smooth": ([], dict()),
        "smooth_all": (["--ply-mean", "--ply-voxel", VOXEL, "--ply-vis", "--ply-normals", "--ply-stat-filter", "2,1,3", "--ply-radius-filter", "2,1",
                        "--ply-component-filter", "2,2"],
                       dict(average=True, voxel=float(VOXEL), stat_filter=(2.0, 1, 3.0), radius_filter=(2.0, 1), component_filter=(2.0, 2)))}


@pytest.fixture(scope="module")
def folders(gpu_pkg, synth, radius_checker, checker, tmp_path_factory):
    """One small synthetic dense folder (the size of the drop-in tests) run without the flag; then, at the radius the checker
    chooses on the points the pipeline makes from that run's maps, with the flag alone and with every other --ply-* flag before it."""
    root = tmp_path_factory.mktemp("dense")
    a = root / "a"
    a.mkdir()
    _write_dense_folder(a, synth, 96, 72, 4)
    shutil.copytree(a, root / "plain")
    _run(root / "plain")
    out = {}
    for name, (flags, kw) in RUNS.items():
        options = gpu_pkg.default_fusion_options(ply_normals=1) if "--ply-normals" in flags else None
        _, whole = _fuse_saved_maps(gpu_pkg, root / "plain", None, return_points=True, options=options, **kw)
        radius, _, _ = chosen(radius_checker, checker, whole)
        shutil.copytree(a, root / name)
        _run(root / name, *flags, "--ply-smooth", "%.9g,%d,%d" % (radius, REAL_MIN, SMOOTH_ITERATIONS))
        out[name] = (root / name, radius)
    return out


def test_binary_writes_the_smoothed_positions(gpu_pkg, radius_checker, checker, folders):
    """APD.ply and APD.ply.vis of the binary against the checker's positions on the points the pipeline makes from the binary's maps."""
    for name, (flags, kw) in RUNS.items():
        folder, radius = folders[name]
        normals = "--ply-normals" in flags
        options = gpu_pkg.default_fusion_options(ply_normals=1) if normals else None
        _, whole = _fuse_saved_maps(gpu_pkg, folder, None, return_points=True, options=options, **kw)
        w = arrays_of(whole)
        want = PS.run(checker, w, radius, REAL_MIN, SMOOTH_ITERATIONS)
        assert want.moved > 0, name
        assert (folder / "APD" / "APD.ply").read_bytes() == ply_bytes(PS.with_positions(w, want), normals), name
        assert (folder / "APD" / "APD.ply").read_bytes() != ply_bytes(w, normals), name
        vis = folder / "APD" / "APD.ply.vis"
        assert vis.exists() == ("--ply-vis" in flags)
        if vis.exists():
            assert vis.read_bytes() == VC.vis_bytes(w.offsets, w.views), name


def test_binary_refuses_a_bad_value_before_anything_is_read(tmp_path):
    """The bad values of --ply-estimate-normals' test, and iterations outside 1 .. 16."""
    for bad in ("0,2", "-1,2", "nan,2", "inf,2", "1e30,2", "1e-30,2", "1", "1,", ",2", "1,-1", "1,x", "1x,2", "", "1,0", "1,1", "1,2147483648",
                "1,99999999999999999999", "1,2,", "1,2,0", "1,2,17", "1,2,x", "1,2,3,4", "1,2,-1", "1,2,100"):
        r = subprocess.run([APD_BIN, str(tmp_path / "no_such_folder"), "0", "--ply-smooth", bad], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=60)
        assert r.returncode != 0 and "bad value '%s' of --ply-smooth" % bad in r.stdout and "USAGE" in r.stdout, (bad, r.stdout[-500:])
    for good in ("1,2", "0.5,2147483647", "1e-3,10,1", "1,2,16"):
        r = subprocess.run([APD_BIN, str(tmp_path / "no_such_folder"), "0", "--ply-smooth", good], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=60)
        assert r.returncode != 0 and "bad value" not in r.stdout and "USAGE" not in r.stdout, (good, r.stdout[-500:])
