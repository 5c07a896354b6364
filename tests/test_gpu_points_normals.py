"""The estimated normals on the device (apd_points_estimate_normals, apd_points_with_estimated_normals;
csrc/apd_points_normals.hip, compact_points of csrc/apd_points.hip), bitwise against the grid mode of the sequential checker
(tests/helpers/points_normals_ref.cpp): normals and variation as uint32 (so that inf, NaN payloads and -0 count), `estimated`, all
seven arrays and the lists of the new object, for host- and for device-resident points, the input unchanged afterwards; the sizes
and the cells a walk can go wrong on; the longest binary64 sums; planted, sign-rule and degenerate clouds; a real cloud; a merged
object; the files; a chain; the pipeline and the drop-in binary.  The comparison is also the check that the device's binary64
division and sqrt round like the host's.  The clouds are made in test_points_radius.py and test_points_normals.py, where the
checker's brute-force mode is held against the grid mode on them."""
import hashlib
import shutil
import subprocess

import numpy as np
import pytest

import fusion_cases
import points_knn_checker as PK
import points_normals_checker as PN
import points_radius_checker as PR
import points_voxel_checker as PV
import vis_checker as VC
from test_gpu_dropin_binary import _write_dense_folder
from test_gpu_fusion_options import APD_BIN, _fuse_saved_maps, _run, _scene
from test_gpu_points_average import averaged, fused
from test_points_knn import real_cloud_choice
from test_points_normals import (REAL_CLOUD, REAL_MIN, SIZE_MINS, bits32, cube_case, degenerate_cases, order_cases, plane_case, sign_cases, sphere_case)
from test_points_radius import (DENSE_ORIGIN, DENSE_RADIUS, MERGED_RADIUS, border_case, dense_case, determinism_case, dressed, grid_edge_case, large_case,
                                merged_many_views_case, outside_case, real_cloud_radius, size_case, size_list)
from test_points_voxel import arrays_of, from_cloud, ply_bytes, views_of

pytestmark = pytest.mark.gpu
PLAIN_VIEWS = views_of(1)     # of the clouds test_points_normals.py makes: one view without sources


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return PN.build(tmp_path_factory.mktemp("points_normals_checker"))


@pytest.fixture(scope="module")
def radius_checker(tmp_path_factory):
    return PR.build(tmp_path_factory.mktemp("points_radius_checker"))


@pytest.fixture(scope="module")
def knn_checker(tmp_path_factory):
    return PK.build(tmp_path_factory.mktemp("points_knn_checker"))


@pytest.fixture(scope="module")
def voxel_checker(tmp_path_factory):
    return PV.build(tmp_path_factory.mktemp("points_voxel_checker"))


def host_bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    assert a.dtype == np.float32
    return bits32(a)


def check_points(pts, c, want, radius, k, origin=None, merged=False, what=""):
    """estimate_normals and with_estimated_normals of `pts`, which holds the cloud `c`, against the checker's result `want`; the
    input is unchanged afterwards.  Returns the new object."""
    normals, variation = pts.estimate_normals(radius, k, origin)
    assert normals.shape == (c.count, 3) and variation.shape == (c.count,), what
    differ = np.flatnonzero((host_bits(normals) != bits32(want.normal)).any(axis=1) | (host_bits(variation) != bits32(want.variation)))
    assert differ.size == 0, (what, differ[:5], want.normal[differ[:5]], want.variation[differ[:5]], want.sweeps[differ[:5]])
    new, estimated = pts.with_estimated_normals(radius, k, origin)
    assert new.on_device == pts.on_device and new.merged == merged and new.count == c.count and estimated == want.count, (what, estimated, want.count)
    PV.assert_equal(arrays_of(new), PN.with_normals(c, want), what)
    PV.assert_equal(arrays_of(pts), c, (what, "the input"))
    return new


def check(pkg, checker, c, views, radius, ks, origin=None, what=""):
    """Every min_neighbours of `ks` on `c` (a PV.Cloud over views = (rows, cols, pairs)), as host- and as device-resident points,
    against the checker's grid mode, which the cap stops nowhere.  Returns the checker's results per min_neighbours."""
    want = {k: PN.run(checker, c, radius, k, origin) for k in ks}
    for dev in (False, True):
        pts = from_cloud(pkg, c, *views, on_device=dev)
        for k, res in want.items():
            assert not res.capped.any(), (what, k)
            check_points(pts, c, res, radius, k, origin, what=(what, dev, k)).close()
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
        assert n < 63 or (0 < got[7].count < got[2].count < n)


def test_cell_borders(gpu_pkg, checker):
    """Pairs at exactly the radius and at the next binary32 after it, in positive and negative cells, across a border and two cells
    apart, coincident points: a point has an estimate where the hand-computed count reaches 2."""
    xyz, counts = border_case()
    c, views = dressed(np.random.default_rng(1), xyz)
    got = check(gpu_pkg, checker, c, views, 1.0, (2,))
    assert np.array_equal(got[2].estimated, np.array(counts) >= 2)


def test_edges_of_the_grid(gpu_pkg, checker):
    xyz, counts = grid_edge_case()
    c, views = dressed(np.random.default_rng(2), xyz)
    got = check(gpu_pkg, checker, c, views, 1.0, (2,))
    assert np.array_equal(got[2].estimated, np.array(counts) >= 2) and got[2].count > 0


def test_points_outside_the_grid(gpu_pkg, checker):
    """NaN, infinities and points 3 * 2^20 cells out among ordinary points keep their stored normal and get +inf; and a cloud with
    every point outside: nothing is estimated."""
    xyz, bad = outside_case(np.random.default_rng(4))
    c, views = dressed(np.random.default_rng(3), xyz)
    got = check(gpu_pkg, checker, c, views, 1.0, (2, 3))
    assert not got[2].estimated[bad].any() and np.isinf(got[2].variation[bad]).all() and got[2].count > 0
    assert np.array_equal(bits32(got[2].normal[bad]), bits32(c.normal[bad]))
    none = dressed(np.random.default_rng(5), np.full((300, 3), np.nan, np.float32))
    assert check(gpu_pkg, checker, *none, 1.0, (2,))[2].count == 0


def test_one_cell_of_twenty_thousand_members(gpu_pkg, checker):
    """20 001 points in one cell: the longest binary64 sums, and every lane of a wave has its own."""
    c, views = dressed(np.random.default_rng(7), dense_case(np.random.default_rng(8)))
    got = check(gpu_pkg, checker, c, views, DENSE_RADIUS, (2,), origin=DENSE_ORIGIN)
    assert got[2].estimated.all()


def test_two_hundred_thousand_points(gpu_pkg, checker):
    c, views = dressed(np.random.default_rng(9), large_case(np.random.default_rng(10)))
    got = check(gpu_pkg, checker, c, views, 1.0, (4,))
    assert 0 < got[4].count < c.count


# --------------------------------------------------------------------------------------------------------------------
# planted, sign-rule and degenerate clouds
# --------------------------------------------------------------------------------------------------------------------

def test_planted_plane_and_sphere(gpu_pkg, checker):
    plane, _ = plane_case(np.random.default_rng(31))
    assert check(gpu_pkg, checker, plane, PLAIN_VIEWS, 1.0, (5,), what="plane")[5].count > 0.95 * plane.count
    sphere = sphere_case(np.random.default_rng(32))
    assert check(gpu_pkg, checker, sphere, PLAIN_VIEWS, 1.0, (5,), what="sphere")[5].count > 0.9 * sphere.count
    cube, _ = cube_case(np.random.default_rng(33))
    assert check(gpu_pkg, checker, cube, PLAIN_VIEWS, 1.0, (5,), what="cube")[5].estimated.all()


def test_sign_rule_and_degenerate_clouds(gpu_pkg, checker):
    """Zero, NaN and exactly orthogonal stored normals; coincident and collinear points; one cell's points in three input orders,
    where the order of the sums shows in the results."""
    for name, c in sign_cases(np.random.default_rng(34)).items():
        assert check(gpu_pkg, checker, c, PLAIN_VIEWS, 1.0, (3,), what=name)[3].count >= c.count - 1
    for name, c in degenerate_cases().items():
        got = check(gpu_pkg, checker, c, PLAIN_VIEWS, 1.0, (2,), what=name)[2]
        assert got.estimated.all() and not np.isnan(got.normal).any() and (got.variation < 1e-10).all()
    for j, (c, _) in enumerate(order_cases(np.random.default_rng(35))):
        assert check(gpu_pkg, checker, c, PLAIN_VIEWS, 1.0, (2,), what=("order", j))[2].estimated.all()


# --------------------------------------------------------------------------------------------------------------------
# a real cloud, merged objects, files, a chain
# --------------------------------------------------------------------------------------------------------------------

def test_a_real_cloud(gpu_pkg, ob, radius_checker, checker):
    """Fused on the device and estimated where it is, at the radius of the radius filter's tests: some points get an estimate and
    some do not.  The lists of the result, built from its sources, are the input's."""
    name, variant, _ = REAL_CLOUD
    case = fusion_cases.case(name)
    radius = None
    for dev in (False, True):
        pts = fused(gpu_pkg, ob, case, variant, dev)
        before = arrays_of(pts)
        radius = radius or real_cloud_radius(radius_checker, before)
        want = PN.run(checker, before, radius, REAL_MIN)
        assert 0 < want.count < before.count and not want.capped.any()
        check_points(pts, before, want, radius, REAL_MIN, what=(name, variant, dev))


def test_a_merged_object_of_many_views(gpu_pkg, checker, voxel_checker):
    """Lists of up to 200 views that no mask holds: the lists and the merged flag are handed on."""
    c, views, first = merged_many_views_case(voxel_checker)
    want = PN.run(checker, first, MERGED_RADIUS, 3)
    assert 0 < want.count and np.diff(first.offsets).max() > 32
    for dev in (False, True):
        merged, _ = from_cloud(gpu_pkg, c, *views, on_device=dev).merge_voxels(1.0)
        new = check_points(merged, first, want, MERGED_RADIUS, 3, merged=True, what=dev)
        assert np.array_equal(arrays_of(new).support, first.support)


def test_two_runs_give_the_same_bytes(gpu_pkg, checker, tmp_path):
    c, views = determinism_case()
    origin = [0.25, -0.5, 0.125]
    pts = from_cloud(gpu_pkg, c, *views, on_device=True)
    files = []
    for run in range(2):
        new, estimated = pts.with_estimated_normals(1.0, 4, origin)
        new.write_ply(tmp_path / ("%d.ply" % run), normals=True)
        new.write_vis(tmp_path / ("%d.vis" % run))
        normals, variation = pts.estimate_normals(1.0, 4, origin)
        files.append(((tmp_path / ("%d.ply" % run)).read_bytes(), (tmp_path / ("%d.vis" % run)).read_bytes(), host_bits(normals).tobytes(),
                      host_bits(variation).tobytes(), estimated))
    assert files[0] == files[1]
    want = PN.run(checker, c, 1.0, 4, origin)
    assert 0 < want.count < c.count
    assert files[0][0] == ply_bytes(PN.with_normals(c, want), True) and files[0][1] == VC.vis_bytes(c.offsets, c.views)


def plain(c):
    return PV.Cloud(*[getattr(c, f) for f in PV.FIELDS], c.offsets, c.views)


def test_average_then_merge_then_remove_statistical_then_estimate(gpu_pkg, ob, radius_checker, knn_checker, checker, voxel_checker, tmp_path):
    """The chain a user runs, against the checkers chained the same way: the result stays a merged object with the checkers' lists."""
    case = fusion_cases.case("mixed_sizes")
    for dev in (False, True):
        pts = fused(gpu_pkg, ob, case, "eth", dev)
        mean = averaged(gpu_pkg, case, pts, dev)
        merged, _ = mean.merge_voxels(0.02)
        m = arrays_of(merged)
        PV.assert_equal(m, PV.merge(voxel_checker, arrays_of(mean), 0.02))
        radius, k, ratio = real_cloud_choice(radius_checker, knn_checker, m)
        kept_want = plain(PK.remove(knn_checker, m, radius, k, ratio))
        kept, _, _ = merged.remove_statistical(radius, k, ratio)
        want = PN.run(checker, kept_want, radius, REAL_MIN)
        assert want.count > 0 and not want.capped.any()
        new = check_points(kept, kept_want, want, radius, REAL_MIN, merged=True, what=dev)
        new.write_vis(tmp_path / "n.vis")
        assert (tmp_path / "n.vis").read_bytes() == VC.vis_bytes(kept_want.offsets, kept_want.views)


# --------------------------------------------------------------------------------------------------------------------
# the pipeline and the binary
# --------------------------------------------------------------------------------------------------------------------

def chosen(radius_checker, checker, whole):
    """(radius, the checker's result) for a Points object: the radius of the real clouds, REAL_MIN neighbours."""
    w = arrays_of(whole)
    radius = real_cloud_radius(radius_checker, w)
    want = PN.run(checker, w, radius, REAL_MIN)
    assert want.count > 0 and not want.capped.any()
    return radius, w, want


def test_through_the_pipeline(gpu_pkg, ob, radius_checker, checker, tmp_path):
    """fuse(estimate_normals=...) returns and writes the points with the new normals, after every other step: the bytes of file-only
    against the returned points against the manual chain, which are the checker's.  Without ply_normals the file keeps its bytes."""
    from apd_mvs_amd import pipeline
    case = fusion_cases.case("mixed_sizes")
    scene, results = _scene(gpu_pkg, pipeline, case)
    options = gpu_pkg.default_fusion_options(ply_normals=1)
    for kw in (dict(), dict(average=True, voxel=0.05, component_filter=(0.2, 2))):
        _, whole = pipeline.fuse(scene, results, tmp_path / "before.ply", return_points=True, **kw)
        radius, w, want = chosen(radius_checker, checker, whole)
        expect = PN.with_normals(w, want)
        manual, _ = whole.with_estimated_normals(radius, REAL_MIN)
        manual.write_ply(tmp_path / "manual.ply", normals=True)
        manual.write_vis(tmp_path / "manual.vis")
        n, new = pipeline.fuse(scene, results, tmp_path / "m.ply", return_points=True, vis_path=tmp_path / "m.vis", estimate_normals=(radius, REAL_MIN),
                               options=options, **kw)
        assert n == w.count == new.count and new.merged == ("voxel" in kw)
        PV.assert_equal(arrays_of(new), expect, kw)
        assert (tmp_path / "m.ply").read_bytes() == (tmp_path / "manual.ply").read_bytes() == ply_bytes(expect, True)
        assert (tmp_path / "m.vis").read_bytes() == (tmp_path / "manual.vis").read_bytes() == VC.vis_bytes(w.offsets, w.views)
        assert pipeline.fuse(scene, results, tmp_path / "file_only.ply", estimate_normals=(radius, REAL_MIN), options=options, **kw) == n
        assert (tmp_path / "file_only.ply").read_bytes() == (tmp_path / "m.ply").read_bytes()
        # without normals in the file the step changes no byte of it, and still acts on the returned points
        n, quiet = pipeline.fuse(scene, results, tmp_path / "quiet.ply", return_points=True, estimate_normals=(radius, REAL_MIN), **kw)
        assert (tmp_path / "quiet.ply").read_bytes() == (tmp_path / "before.ply").read_bytes()
        PV.assert_equal(arrays_of(quiet), expect, kw)


VOXEL = "0.25"
# the flags of a run before --ply-estimate-normals and what the pipeline needs to make the points the step starts from
RUNS = {"normals": ([], dict()),
        "normals_shown": (["--ply-normals", "--ply-vis"], dict()),
        "normals_all": (["--ply-mean", "--ply-voxel", VOXEL, "--ply-vis", "--ply-normals", "--ply-stat-filter", "2,1,3", "--ply-radius-filter", "2,1",
                         "--ply-component-filter", "2,2"],
                        dict(average=True, voxel=float(VOXEL), stat_filter=(2.0, 1, 3.0), radius_filter=(2.0, 1), component_filter=(2.0, 2)))}


@pytest.fixture(scope="module")
def folders(gpu_pkg, synth, radius_checker, checker, tmp_path_factory):
    """One small synthetic dense folder (the size of the drop-in tests) run without the flag; then, at the radius the checker
    chooses on the points the pipeline makes from that run's maps, with the flag alone, with --ply-normals, and with every
    other --ply-* flag."""
    root = tmp_path_factory.mktemp("dense")
    a = root / "a"
    a.mkdir()
    _write_dense_folder(a, synth, 96, 72, 4)
    shutil.copytree(a, root / "plain")
    _run(root / "plain")
    out = {"plain": (root / "plain", None)}
    for name, (flags, kw) in RUNS.items():
        options = gpu_pkg.default_fusion_options(ply_normals=1) if "--ply-normals" in flags else None
        _, whole = _fuse_saved_maps(gpu_pkg, root / "plain", None, return_points=True, options=options, **kw)
        radius, _, _ = chosen(radius_checker, checker, whole)
        shutil.copytree(a, root / name)
        _run(root / name, *flags, "--ply-estimate-normals", "%.9g,%d" % (radius, REAL_MIN))
        out[name] = (root / name, radius)
    return out


def test_binary_writes_the_estimated_normals(gpu_pkg, radius_checker, checker, folders):
    """APD.ply and APD.ply.vis of the binary against the checker's normals on the points the pipeline makes from the binary's maps."""
    for name, (flags, kw) in RUNS.items():
        folder, radius = folders[name]
        normals = "--ply-normals" in flags
        options = gpu_pkg.default_fusion_options(ply_normals=1) if normals else None
        _, whole = _fuse_saved_maps(gpu_pkg, folder, None, return_points=True, options=options, **kw)
        w = arrays_of(whole)
        want = PN.run(checker, w, radius, REAL_MIN)
        assert want.count > 0 and not want.capped.any(), name
        assert (folder / "APD" / "APD.ply").read_bytes() == ply_bytes(PN.with_normals(w, want), normals), name
        vis = folder / "APD" / "APD.ply.vis"
        assert vis.exists() == ("--ply-vis" in flags)
        if vis.exists():
            assert vis.read_bytes() == VC.vis_bytes(w.offsets, w.views), name


def test_binary_without_the_flag_keeps_its_bytes(gpu_pkg, folders, tmp_path):
    """A run without the flag is the pipeline's plain file; the flag alone, without --ply-normals, changes no byte of it."""
    plain_ply = (folders["plain"][0] / "APD" / "APD.ply").read_bytes()
    assert _fuse_saved_maps(gpu_pkg, folders["plain"][0], tmp_path / "pipe.ply") > 0
    assert hashlib.md5(plain_ply).hexdigest() == hashlib.md5((tmp_path / "pipe.ply").read_bytes()).hexdigest()
    assert (folders["normals"][0] / "APD" / "APD.ply").read_bytes() == plain_ply
    assert (folders["normals_shown"][0] / "APD" / "APD.ply").read_bytes() != plain_ply


def test_binary_refuses_a_bad_value_before_anything_is_read(tmp_path):
    """The bad values of --ply-radius-filter's test, which are bad here too, and the counts below 2 and past 2^31 - 1."""
    for bad in ("0,2", "-1,2", "nan,2", "inf,2", "1e30,2", "1e-30,2", "1", "1,", ",2", "1,-1", "1,x", "1x,2", "1,2,3", "", "1,0", "1,1", "1,2147483648",
                "1,99999999999999999999"):
        r = subprocess.run([APD_BIN, str(tmp_path / "no_such_folder"), "0", "--ply-estimate-normals", bad], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=60)
        assert r.returncode != 0 and "bad value '%s' of --ply-estimate-normals" % bad in r.stdout and "USAGE" in r.stdout, (bad, r.stdout[-500:])
    for good in ("1,2", "0.5,2147483647", "1e-3,10"):
        r = subprocess.run([APD_BIN, str(tmp_path / "no_such_folder"), "0", "--ply-estimate-normals", good], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=60)
        assert r.returncode != 0 and "bad value" not in r.stdout and "USAGE" not in r.stdout, (good, r.stdout[-500:])
