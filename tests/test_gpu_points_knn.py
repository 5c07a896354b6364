"""The k-nearest mean distances and the statistical removal on the device (apd_points_knn_mean_distances,
apd_points_remove_statistical; csrc/apd_points_knn.hip, compact_points of csrc/apd_points.hip), bitwise against the grid mode of the
sequential checker (tests/helpers/points_knn_ref.cpp): the scores as uint32 (so that inf and -0 count), the threshold as bits,
`removed`, all seven arrays of the kept points and their lists, for host- and for device-resident points; the sizes, the cells and
the arrival orders a selection can go wrong on; real clouds; merged objects; the files; the pipeline and the drop-in binary.  The
clouds are made in test_points_radius.py and test_points_knn.py, where the checker's brute-force mode is held against the grid
mode on them."""
import hashlib
import shutil
import subprocess

import numpy as np
import pytest

import fusion_cases
import points_knn_checker as PK
import points_radius_checker as PR
import points_voxel_checker as PV
import vis_checker as VC
from test_gpu_dropin_binary import _write_dense_folder
from test_gpu_fusion_options import APD_BIN, _fuse_saved_maps, _run, _scene
from test_gpu_points_average import averaged, fused
from test_points_knn import (ARRIVAL_KS, LATTICE_KS, SIZE_KS, arrival_case, assert_not_vacuous, bits32, bits64, lattice_case, real_cloud_choice)
from test_points_radius import (DENSE_ORIGIN, DENSE_RADIUS, MERGED_RADIUS, border_case, dense_case, determinism_case, dressed, grid_edge_case, large_case,
                                merged_many_views_case, outside_case, real_cloud_min_neighbours, real_cloud_radius, size_case, size_list)
from test_points_voxel import REAL_CLOUDS, arrays_of, from_cloud, ply_bytes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return PK.build(tmp_path_factory.mktemp("points_knn_checker"))


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


def plain(c):
    """The arrays and lists of a checker result as a PV.Cloud without its extras."""
    return PV.Cloud(*[getattr(c, f) for f in PV.FIELDS], c.offsets, c.views)


def check_removal(pts, want, radius, k, ratio, origin=None, merged=False, what=""):
    kept, removed, threshold = pts.remove_statistical(radius, k, ratio, origin)
    assert kept.on_device == pts.on_device and kept.merged == merged and kept.count == want.count and removed == want.removed, what
    assert bits64(threshold) == bits64(want.threshold), (what, threshold, want.threshold)
    PV.assert_equal(arrays_of(kept), plain(want), what)
    return kept


def check(pkg, checker, c, views, radius, ks, ratios=(1.0,), origin=None, what=""):
    """Scores at every k and removal at every (k, ratio) of `c` (a PV.Cloud over views = (rows, cols, pairs)), as host- and as
    device-resident points, against the checker's grid mode.  Returns the checker's scores per k."""
    want = {(k, ratio): PK.run(checker, c, radius, k, ratio, origin) for k in ks for ratio in ratios}
    for dev in (False, True):
        pts = from_cloud(pkg, c, *views, on_device=dev)
        for (k, ratio), (scores, kept) in want.items():
            got = host_bits(pts.knn_mean_distances(radius, k, origin))
            assert got.shape == scores.shape and np.array_equal(got, bits32(scores)), (what, dev, k)
            check_removal(pts, kept, radius, k, ratio, origin, what=(what, dev, k, ratio)).close()
        pts.close()
    return {k: want[(k, ratios[0])][0] for k in ks}


# --------------------------------------------------------------------------------------------------------------------
# sizes, cells, arrival orders
# --------------------------------------------------------------------------------------------------------------------

def test_sizes_around_waves_blocks_and_tiles(gpu_pkg, checker):
    """n = 0, 1, 2, around a wave and a block, 3 T + 17 and 5 T + 17, about three points per cell at radius 1, k = 1, 2, 7, 33, 64:
    the small k find full points, the large ones mostly none."""
    for n in size_list(gpu_pkg):
        c, views = size_case(gpu_pkg, n)
        got = check(gpu_pkg, checker, c, views, 1.0, SIZE_KS, what=n)
        assert n < 63 or (np.isfinite(got[1]).any() and np.isinf(got[1]).any() and np.isfinite(got[7]).any())


def test_cell_borders(gpu_pkg, checker):
    """Pairs at exactly the radius and at the next binary32 after it, in positive and negative cells, across a border and two
    cells apart, coincident points: a score is finite where the hand-computed count reaches k."""
    xyz, counts = border_case()
    c, views = dressed(np.random.default_rng(1), xyz)
    got = check(gpu_pkg, checker, c, views, 1.0, (1, 2), ratios=(0.0,))
    assert np.array_equal(np.isfinite(got[1]), np.array(counts) >= 1) and np.array_equal(np.isfinite(got[2]), np.array(counts) >= 2)
    assert got[1][3] == 1.0 and got[1][5] == np.inf


def test_edges_of_the_grid(gpu_pkg, checker):
    xyz, counts = grid_edge_case()
    c, views = dressed(np.random.default_rng(2), xyz)
    got = check(gpu_pkg, checker, c, views, 1.0, (1, 2), ratios=(0.0,))
    assert np.array_equal(np.isfinite(got[1]), np.array(counts) >= 1) and np.array_equal(np.isfinite(got[2]), np.array(counts) >= 2)


def test_points_outside_the_grid(gpu_pkg, checker):
    """NaN, infinities and points 3 * 2^20 cells out among ordinary points: +inf, nobody's neighbour, never kept; and a cloud with
    every point outside: all +inf, T = 0, an object without points."""
    xyz, bad = outside_case(np.random.default_rng(4))
    c, views = dressed(np.random.default_rng(3), xyz)
    got = check(gpu_pkg, checker, c, views, 1.0, (1, 3), ratios=(0.5, 100.0))
    assert np.isinf(got[1][bad]).all() and np.isfinite(got[1]).any()
    assert not np.isin(bad, PK.remove(checker, c, 1.0, 1, 100.0).index).any()
    none = dressed(np.random.default_rng(5), np.full((300, 3), np.nan, np.float32))
    check(gpu_pkg, checker, *none, 1.0, (1,))
    for dev in (False, True):
        kept, removed, threshold = from_cloud(gpu_pkg, none[0], *none[1], on_device=dev).remove_statistical(1.0, 1, 1.0)
        assert kept.count == 0 and removed == 300 and threshold == 0.0 and kept.visibility()[0].tolist() == [0]


def test_arrival_orders(gpu_pkg, checker):
    """One cell's points around its centre, nearest first in one copy, nearest last in another, shuffled in a third: no replacement
    after the first k, a replacement at every candidate, and everything in between; k = 1 (one slot), 7, 33, 64."""
    c, views = dressed(np.random.default_rng(21), arrival_case(np.random.default_rng(22)))
    got = check(gpu_pkg, checker, c, views, 1.0, ARRIVAL_KS, ratios=(0.0, -0.5))
    assert all(np.isfinite(got[k]).all() for k in ARRIVAL_KS)


def test_tie_lattice(gpu_pkg, checker):
    """Multiples of 1/4: many candidates tie at the k-th distance, and a candidate equal to the held maximum is not accepted."""
    c, views = dressed(np.random.default_rng(23), lattice_case())
    got = check(gpu_pkg, checker, c, views, 1.0, LATTICE_KS, ratios=(0.0, 1.0))
    assert np.isfinite(got[64]).sum() > 100 and np.isinf(got[64]).any()


def test_one_cell_of_twenty_thousand_members(gpu_pkg, checker):
    """20 001 points in one cell at k = 64: every candidate is a possible replacement, and every lane of a wave has its own."""
    c, views = dressed(np.random.default_rng(7), dense_case(np.random.default_rng(8)))
    got = check(gpu_pkg, checker, c, views, DENSE_RADIUS, (64,), origin=DENSE_ORIGIN)
    assert np.isfinite(got[64]).all()


def test_a_table_scan_of_several_blocks(gpu_pkg, checker):
    """2 * 10^5 points over n / 4 cells at k = 8: several hundred chunks of the threshold's sums."""
    c, views = dressed(np.random.default_rng(9), large_case(np.random.default_rng(10)))
    got = check(gpu_pkg, checker, c, views, 1.0, (8,))
    assert np.isfinite(got[8]).any() and np.isinf(got[8]).any()


# --------------------------------------------------------------------------------------------------------------------
# real clouds, merged objects, chains
# --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,variant", [(n, v) for n, v, _ in REAL_CLOUDS])
def test_real_clouds(gpu_pkg, ob, radius_checker, checker, name, variant):
    """Fused on the device and filtered where they are, with the choices of test_points_knn.py.  The lists of the result, built
    from its sources, are the input's at the kept indices."""
    case = fusion_cases.case(name)
    choice = None
    for dev in (False, True):
        pts = fused(gpu_pkg, ob, case, variant, dev)
        before = arrays_of(pts)
        choice = choice or real_cloud_choice(radius_checker, checker, before)
        radius, k, ratio = choice
        want = assert_not_vacuous(checker, before, radius, k, ratio, what=(name, variant))
        assert np.array_equal(host_bits(pts.knn_mean_distances(radius, k)), bits32(PK.scores(checker, before, radius, k)))
        got = arrays_of(check_removal(pts, want, radius, k, ratio, what=(name, variant, dev)))
        assert np.array_equal(np.diff(got.offsets), np.diff(before.offsets)[want.index])
        assert np.array_equal(got.views, np.concatenate([before.views[before.offsets[i]:before.offsets[i + 1]] for i in want.index]))
        PV.assert_equal(arrays_of(pts), before, "the input")


def test_average_then_merge_then_remove_statistical_then_remove_sparse(gpu_pkg, ob, radius_checker, checker, voxel_checker, tmp_path):
    """The chain a user runs, against the checkers chained the same way: the result stays a merged object with the checkers' lists."""
    case = fusion_cases.case("mixed_sizes")
    for dev in (False, True):
        pts = fused(gpu_pkg, ob, case, "eth", dev)
        mean = averaged(gpu_pkg, case, pts, dev)
        merged, _ = mean.merge_voxels(0.02)
        m = arrays_of(merged)
        PV.assert_equal(m, PV.merge(voxel_checker, arrays_of(mean), 0.02))
        radius, k, ratio = real_cloud_choice(radius_checker, checker, m)
        want = assert_not_vacuous(checker, m, radius, k, ratio, what="merged means")
        kept = check_removal(merged, want, radius, k, ratio, merged=True, what=dev)
        kept.write_vis(tmp_path / "k.vis")
        assert (tmp_path / "k.vis").read_bytes() == VC.vis_bytes(want.offsets, want.views)
        least = real_cloud_min_neighbours(PR.counts(radius_checker, plain(want), radius))
        last = PR.remove(radius_checker, plain(want), radius, least)
        assert 0 < last.removed < want.count
        sparse, removed = kept.remove_sparse(radius, least)
        assert sparse.merged and removed == last.removed
        PV.assert_equal(arrays_of(sparse), PV.Cloud(*[getattr(last, f) for f in PV.FIELDS], last.offsets, last.views), dev)
        PV.assert_equal(arrays_of(merged), m, "the input")


def test_a_merged_object_of_many_views(gpu_pkg, checker, voxel_checker):
    """Lists of up to 200 views that no mask holds: the kept points' lists, the merged flag and support are the checker's."""
    c, views, first = merged_many_views_case(voxel_checker)
    want = PK.remove(checker, first, MERGED_RADIUS, 3, 0.5)
    assert 0 < want.removed < first.count and np.diff(want.offsets).max() > 32
    for dev in (False, True):
        merged, _ = from_cloud(gpu_pkg, c, *views, on_device=dev).merge_voxels(1.0)
        assert np.array_equal(host_bits(merged.knn_mean_distances(MERGED_RADIUS, 3)), bits32(PK.scores(checker, first, MERGED_RADIUS, 3)))
        kept = check_removal(merged, want, MERGED_RADIUS, 3, 0.5, merged=True, what=dev)
        assert np.array_equal(arrays_of(kept).support, first.support[want.index])


def test_two_runs_give_the_same_bytes(gpu_pkg, checker, tmp_path):
    c, views = determinism_case()
    origin = [0.25, -0.5, 0.125]
    pts = from_cloud(gpu_pkg, c, *views, on_device=True)
    files = []
    for run in range(2):
        kept, _, threshold = pts.remove_statistical(1.0, 4, 1.0, origin)
        kept.write_ply(tmp_path / ("%d.ply" % run), normals=True)
        kept.write_vis(tmp_path / ("%d.vis" % run))
        files.append(((tmp_path / ("%d.ply" % run)).read_bytes(), (tmp_path / ("%d.vis" % run)).read_bytes(),
                      host_bits(pts.knn_mean_distances(1.0, 4, origin)).tobytes(), bits64(threshold)))
    assert files[0] == files[1]
    want = PK.remove(checker, c, 1.0, 4, 1.0, origin)
    assert 0 < want.removed < c.count
    assert files[0][0] == ply_bytes(want, True) and files[0][1] == VC.vis_bytes(want.offsets, want.views)


# --------------------------------------------------------------------------------------------------------------------
# the pipeline and the binary
# --------------------------------------------------------------------------------------------------------------------

def chosen(radius_checker, checker, whole):
    """(radius, k, ratio, the checker's kept points) for a Points object: the choice of the real clouds."""
    w = arrays_of(whole)
    radius, k, ratio = real_cloud_choice(radius_checker, checker, w)
    return radius, k, ratio, assert_not_vacuous(checker, w, radius, k, ratio, what="pipeline points")


def test_through_the_pipeline(gpu_pkg, ob, radius_checker, checker, tmp_path):
    """fuse(stat_filter=...) returns and writes the filtered points, after the averaging and the merge and before the radius filter
    when those are asked for: the bytes of file-only against the returned points against the manual chain, which are the
    checkers'."""
    from apd_mvs_amd import pipeline
    case = fusion_cases.case("mixed_sizes")
    scene, results = _scene(gpu_pkg, pipeline, case)
    options = gpu_pkg.default_fusion_options(ply_normals=1)
    for kw, then_radius in ((dict(), False), (dict(average=True, voxel=0.05), True)):
        _, whole = pipeline.fuse(scene, results, None, return_points=True, **kw)
        radius, k, ratio, want = chosen(radius_checker, checker, whole)
        manual, _, _ = whole.remove_statistical(radius, k, ratio)
        more = dict(kw)
        if then_radius:
            least = real_cloud_min_neighbours(PR.counts(radius_checker, plain(want), radius))
            last = PR.remove(radius_checker, plain(want), radius, least)
            assert 0 < last.removed < want.count
            want = PV.Cloud(*[getattr(last, f) for f in PV.FIELDS], last.offsets, last.views)
            manual, _ = manual.remove_sparse(radius, least)
            more["radius_filter"] = (radius, least)
        manual.write_ply(tmp_path / "manual.ply", normals=True)
        manual.write_vis(tmp_path / "manual.vis")
        n, kept = pipeline.fuse(scene, results, tmp_path / "m.ply", return_points=True, vis_path=tmp_path / "m.vis", stat_filter=(radius, k, ratio),
                                options=options, **more)
        assert n == want.count == kept.count and kept.merged == ("voxel" in kw)
        PV.assert_equal(arrays_of(kept), plain(want), kw)
        assert (tmp_path / "m.ply").read_bytes() == (tmp_path / "manual.ply").read_bytes() == ply_bytes(want, True)
        assert (tmp_path / "m.vis").read_bytes() == (tmp_path / "manual.vis").read_bytes() == VC.vis_bytes(want.offsets, want.views)
        assert pipeline.fuse(scene, results, tmp_path / "file_only.ply", stat_filter=(radius, k, ratio), options=options, **more) == n
        assert (tmp_path / "file_only.ply").read_bytes() == (tmp_path / "m.ply").read_bytes()


VOXEL = "0.25"
# the flags of a run before --ply-stat-filter, what the pipeline needs to make the points the filter starts from, normals, and
# whether --ply-radius-filter follows
RUNS = {"stat": ([], dict(), False, False),
        "stat_all": (["--ply-mean", "--ply-voxel", VOXEL, "--ply-vis", "--ply-normals"], dict(average=True, voxel=float(VOXEL)), True, True),
        "stat_tat": (["--fusion", "tat-advanced", "--ply-vis"], dict(variant="tat_advanced"), False, False)}


@pytest.fixture(scope="module")
def folders(gpu_pkg, synth, radius_checker, checker, tmp_path_factory):
    """One small synthetic dense folder (the size of the drop-in tests) run without the flag; then, with the choices the checkers
    make on the points the pipeline makes from that run's maps, with the flag alone, with every other --ply-* flag, and with a
    Tanks and Temples loop."""
    root = tmp_path_factory.mktemp("dense")
    a = root / "a"
    a.mkdir()
    _write_dense_folder(a, synth, 96, 72, 4)
    shutil.copytree(a, root / "plain")
    _run(root / "plain")
    out = {"plain": (root / "plain", None)}
    for name, (flags, kw, normals, then_radius) in RUNS.items():
        options = gpu_pkg.default_fusion_options(ply_normals=1) if normals else None
        _, whole = _fuse_saved_maps(gpu_pkg, root / "plain", None, return_points=True, options=options, **kw)
        radius, k, ratio, want = chosen(radius_checker, checker, whole)
        extra, least = [], None
        if then_radius:
            least = real_cloud_min_neighbours(PR.counts(radius_checker, plain(want), radius))
            extra = ["--ply-radius-filter", "%.9g,%d" % (radius, least)]
        shutil.copytree(a, root / name)
        _run(root / name, *flags, "--ply-stat-filter", "%.9g,%d,%.9g" % (radius, k, ratio), *extra)
        out[name] = (root / name, (radius, k, ratio, least))
    return out


def test_binary_writes_the_filtered_points(gpu_pkg, radius_checker, checker, folders):
    """APD.ply and APD.ply.vis of the binary against the checkers' removal from the points the pipeline makes from the binary's maps."""
    for name, (flags, kw, normals, then_radius) in RUNS.items():
        folder, (radius, k, ratio, least) = folders[name]
        options = gpu_pkg.default_fusion_options(ply_normals=1) if normals else None
        _, whole = _fuse_saved_maps(gpu_pkg, folder, None, return_points=True, options=options, **kw)
        want = PK.remove(checker, arrays_of(whole), radius, k, ratio)
        assert 0 < want.removed < whole.count, name
        if then_radius:
            want = PR.remove(radius_checker, plain(want), radius, least)
            assert want.removed > 0, name
        assert (folder / "APD" / "APD.ply").read_bytes() == ply_bytes(want, normals), name
        vis = folder / "APD" / "APD.ply.vis"
        assert vis.exists() == ("--ply-vis" in flags)
        if vis.exists():
            assert vis.read_bytes() == VC.vis_bytes(want.offsets, want.views), name


def test_binary_without_the_flag_keeps_its_bytes(gpu_pkg, folders, tmp_path):
    plain_ply = (folders["plain"][0] / "APD" / "APD.ply").read_bytes()
    assert _fuse_saved_maps(gpu_pkg, folders["plain"][0], tmp_path / "pipe.ply") > 0
    assert hashlib.md5(plain_ply).hexdigest() == hashlib.md5((tmp_path / "pipe.ply").read_bytes()).hexdigest()
    assert len((folders["stat"][0] / "APD" / "APD.ply").read_bytes()) < len(plain_ply)


def test_binary_refuses_a_bad_value_before_anything_is_read(tmp_path):
    """The bad values of --ply-radius-filter's test, which are bad here too, but for "1,2,3": with three fields that is RADIUS 1, K 2,
    RATIO 3, a good value, so its place is taken by "1,2,3,4" and it is held to be accepted below; then k = 0, k = 65, a ratio
    that is no number and a missing ratio."""
    for bad in ("0,1", "-1,2", "nan,1", "inf,1", "1e30,1", "1e-30,1", "1", "1,", ",1", "1,-1", "1,x", "1x,1", "1,2,3,4", "",
                "1,0,1", "1,65,1", "1,2,nan", "1,2", "0,2,1", "-1,2,1", "nan,2,1", "inf,2,1", "1e30,2,1", "1e-30,2,1", "1,2,", "1,,1", ",2,1", "1,-2,1",
                "1,2,x", "1,2,1x", "1,2,inf"):
        r = subprocess.run([APD_BIN, str(tmp_path / "no_such_folder"), "0", "--ply-stat-filter", bad], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=60)
        assert r.returncode != 0 and "bad value '%s' of --ply-stat-filter" % bad in r.stdout and "USAGE" in r.stdout, (bad, r.stdout[-500:])
    for good in ("1,2,3", "0.5,64,-1.5", "1,1,0"):
        r = subprocess.run([APD_BIN, str(tmp_path / "no_such_folder"), "0", "--ply-stat-filter", good], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=60)
        assert r.returncode != 0 and "bad value" not in r.stdout and "USAGE" not in r.stdout, (good, r.stdout[-500:])
