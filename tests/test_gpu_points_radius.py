"""Neighbours within a radius and the removal of sparse points on the device (apd_points_neighbour_counts, apd_points_remove_sparse;
csrc/apd_points_radius.hip, compact_points of csrc/apd_points.hip), bitwise against the grid mode of the sequential checker
(tests/helpers/points_radius_ref.cpp): the counts, all seven arrays of the kept points, their lists and `removed`, for host- and
for device-resident points; the sizes and the cells a search can go wrong on; real clouds; merged objects; the files; the Python
layer, the pipeline and the drop-in binary.  The clouds are made in test_points_radius.py, where the checker's brute-force mode
is held against the grid mode on them."""
import hashlib
import shutil
import subprocess

import numpy as np
import pytest

import fusion_cases
import points_radius_checker as PR
import points_voxel_checker as PV
import vis_checker as VC
from test_gpu_dropin_binary import _write_dense_folder
from test_gpu_fusion_options import APD_BIN, _fuse_saved_maps, _run, _scene
from test_gpu_points_average import averaged, fused
from test_points_radius import (DENSE_ORIGIN, DENSE_RADIUS, MERGED_MIN, MERGED_RADIUS, border_case, dense_case, determinism_case, dressed, grid_edge_case,
                                large_case, merged_many_views_case, modes_agree, outside_case, real_cloud_min_neighbours, real_cloud_radius, size_case,
                                size_list, three_per_cell)
from test_points_voxel import REAL_CLOUDS, arrays_of, from_cloud, ply_bytes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return PR.build(tmp_path_factory.mktemp("points_radius_checker"))


@pytest.fixture(scope="module")
def voxel_checker(tmp_path_factory):
    return PV.build(tmp_path_factory.mktemp("points_voxel_checker"))


def host_counts(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32)


def plain(c):
    """The arrays and lists of a checker result as a PV.Cloud without its extras."""
    return PV.Cloud(*[getattr(c, f) for f in PV.FIELDS], c.offsets, c.views)


def check(pkg, checker, c, views, radius, origin=None, caps=(0, 2), mins=(1, 3), must_remove=True, what=""):
    """Counts at every cap and removal at every minimum of `c` (a PV.Cloud over views = (rows, cols, pairs)), as host- and as
    device-resident points, against the checker's grid mode.  Returns the checker's uncapped counts."""
    want_counts = {cap: PR.counts(checker, c, radius, cap, origin) for cap in caps}
    want_kept = {k: PR.remove(checker, c, radius, k, origin) for k in mins}
    for k, want in want_kept.items():
        assert not must_remove or 0 < want.removed < c.count, (what, k, want.removed)
    for dev in (False, True):
        pts = from_cloud(pkg, c, *views, on_device=dev)
        for cap, want in want_counts.items():
            got = host_counts(pts.neighbour_counts(radius, cap, origin))
            assert got.shape == want.shape and np.array_equal(got, want), (what, dev, cap)
        for k, want in want_kept.items():
            kept, removed = pts.remove_sparse(radius, k, origin)
            assert kept.on_device == dev and not kept.merged and kept.count == want.count and removed == want.removed, (what, dev, k)
            PV.assert_equal(arrays_of(kept), plain(want), (what, dev, k))
            kept.close()
        pts.close()
    return want_counts.get(0)


# --------------------------------------------------------------------------------------------------------------------
# sizes and cells
# --------------------------------------------------------------------------------------------------------------------

def test_sizes_around_waves_blocks_and_tiles(gpu_pkg, checker):
    """n = 0, 1, 2, around a wave and a block, 3 T + 17 and 5 T + 17, about three points per cell at radius 1: counts without a cap
    and with cap 2, removal at 1 and at 3 neighbours."""
    for n in size_list(gpu_pkg):
        c, views = size_case(gpu_pkg, n)
        check(gpu_pkg, checker, c, views, 1.0, must_remove=n >= 63, what=n)


def test_cell_borders(gpu_pkg, checker):
    """Points on cell borders, pairs at exactly the radius and at the next binary32 after it, in positive and negative cells,
    across a border and two cells apart, coincident points: the hand-computed counts of test_points_radius.py."""
    xyz, want = border_case()
    c, views = dressed(np.random.default_rng(1), xyz)
    got = check(gpu_pkg, checker, c, views, 1.0, must_remove=False)
    assert got.tolist() == want


def test_edges_of_the_grid(gpu_pkg, checker):
    """x cells 2^20 - 1 and -2^20 of adjacent y rows have consecutive keys and are not neighbours; the outermost y and z cells."""
    xyz, want = grid_edge_case()
    c, views = dressed(np.random.default_rng(2), xyz)
    got = check(gpu_pkg, checker, c, views, 1.0, mins=(1, 2), must_remove=False)
    assert got.tolist() == want


def test_points_outside_the_grid(gpu_pkg, checker):
    """NaN, infinities and points 3 * 2^20 cells out among ordinary points: they count 0, nobody counts them, they go at 1
    neighbour and stay at 0; with 0 the result is the input in all seven arrays and the lists."""
    xyz, bad = outside_case(np.random.default_rng(4))
    c, views = dressed(np.random.default_rng(3), xyz)
    got = check(gpu_pkg, checker, c, views, 1.0)
    inside = np.setdiff1d(np.arange(c.count), bad)
    assert (got[bad] == 0).all() and np.array_equal(got[inside], PR.counts(checker, plain_subset(c, inside), 1.0))
    assert not np.isin(bad, PR.remove(checker, c, 1.0, 1).index).any()
    for dev in (False, True):
        pts = from_cloud(gpu_pkg, c, *views, on_device=dev)
        kept, removed = pts.remove_sparse(1.0, 0)
        assert removed == 0 and kept.count == c.count
        PV.assert_equal(arrays_of(kept), c, dev)
    # and every point outside: no counts, an object without points
    none = dressed(np.random.default_rng(5), np.full((300, 3), np.nan, np.float32))
    check(gpu_pkg, checker, *none, 1.0, mins=(0,), must_remove=False)
    for dev in (False, True):
        kept, removed = from_cloud(gpu_pkg, none[0], *none[1], on_device=dev).remove_sparse(1.0, 1)
        assert kept.count == 0 and removed == 300 and kept.visibility()[0].tolist() == [0]


def plain_subset(c, index):
    return PV.Cloud(*[getattr(c, f)[index] for f in PV.FIELDS], *PV.source_lists(np.zeros(len(index), np.int32), np.zeros(len(index), np.uint32), [[]]))


def test_cap(gpu_pkg, checker):
    """counts(cap = c) == minimum(counts(cap = 0), c) on one cloud with an origin off the lattice."""
    c, views = dressed(np.random.default_rng(5), three_per_cell(np.random.default_rng(6), 3000))
    origin = [0.25, -0.5, 0.125]
    full = check(gpu_pkg, checker, c, views, 1.0, origin, caps=(0, 1, 3, 1000), mins=(2,))
    assert full.max() > 3
    for dev in (False, True):
        pts = from_cloud(gpu_pkg, c, *views, on_device=dev)
        for cap in (1, 3, 1000):
            assert np.array_equal(host_counts(pts.neighbour_counts(1.0, cap, origin)), np.minimum(full, cap)), (dev, cap)


def test_one_cell_of_twenty_thousand_members(gpu_pkg, checker):
    """20 001 points in one cell, no cap: every lane walks the whole cell, 4 * 10^8 distance tests."""
    c, views = dressed(np.random.default_rng(7), dense_case(np.random.default_rng(8)))
    got = check(gpu_pkg, checker, c, views, DENSE_RADIUS, DENSE_ORIGIN, caps=(0,), mins=(), must_remove=False)
    assert 0 < got.min() < got.max() <= c.count - 1


def test_a_table_scan_of_several_blocks(gpu_pkg, checker):
    """2 * 10^5 points over n / 4 cells: the sort's [digit][block] table takes several blocks of its scan."""
    c, views = dressed(np.random.default_rng(9), large_case(np.random.default_rng(10)))
    check(gpu_pkg, checker, c, views, 1.0, caps=(0,), mins=(2,))


# --------------------------------------------------------------------------------------------------------------------
# real clouds, merged objects
# --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,variant", [(n, v) for n, v, _ in REAL_CLOUDS])
def test_real_clouds(gpu_pkg, ob, checker, name, variant):
    """Fused on the device and filtered where they are, at three times the median nearest-point spacing and a minimum that the
    checker says removes about a tenth.  The lists of the result, built from its sources, are the input's at the kept indices."""
    case = fusion_cases.case(name)
    radius = k = None
    for dev in (False, True):
        pts = fused(gpu_pkg, ob, case, variant, dev)
        before = arrays_of(pts)
        if radius is None:
            radius = real_cloud_radius(checker, before)
            k = real_cloud_min_neighbours(PR.counts(checker, before, radius))
        want = PR.remove(checker, before, radius, k)
        assert 0 < want.removed < before.count
        if before.count <= 20001 and not dev:   # the device's own fusion, held against the loop over all pairs too
            modes_agree(checker, before, radius, (k,), what=(name, variant))
        assert np.array_equal(host_counts(pts.neighbour_counts(radius)), PR.counts(checker, before, radius))
        kept, removed = pts.remove_sparse(radius, k)
        assert kept.on_device == dev and removed == want.removed
        got = arrays_of(kept)
        PV.assert_equal(got, plain(want), (name, variant, dev))
        lengths = np.diff(before.offsets)[want.index]
        assert np.array_equal(np.diff(got.offsets), lengths)
        assert np.array_equal(got.views, np.concatenate([before.views[before.offsets[i]:before.offsets[i + 1]] for i in want.index]))
        PV.assert_equal(arrays_of(pts), before, "the input")


def test_average_then_merge_then_remove(gpu_pkg, ob, checker, voxel_checker, tmp_path):
    """The chain a user runs: the lists and the .vis bytes of the filtered merged points are the checker's, the result is a merged
    object, average() refuses it, and it can be filtered again."""
    case = fusion_cases.case("mixed_sizes")
    for dev in (False, True):
        pts = fused(gpu_pkg, ob, case, "eth", dev)
        mean = averaged(gpu_pkg, case, pts, dev)
        merged, _ = mean.merge_voxels(0.02)
        m = arrays_of(merged)
        PV.assert_equal(m, PV.merge(voxel_checker, arrays_of(mean), 0.02))
        radius = real_cloud_radius(checker, m)
        k = real_cloud_min_neighbours(PR.counts(checker, m, radius))
        want = PR.remove(checker, m, radius, k)
        assert 0 < want.removed < m.count
        if m.count <= 20001 and not dev:
            modes_agree(checker, m, radius, (k,), what="merged means")
        kept, removed = merged.remove_sparse(radius, k)
        assert kept.merged and kept.on_device == dev and removed == want.removed
        PV.assert_equal(arrays_of(kept), plain(want), dev)
        kept.write_vis(tmp_path / "k.vis")
        assert (tmp_path / "k.vis").read_bytes() == VC.vis_bytes(want.offsets, want.views)
        with pytest.raises(gpu_pkg.ApdError, match="apd_points_average: merged points name no sources"):
            averaged(gpu_pkg, case, kept, dev)
        again = PR.remove(checker, plain(want), radius, k)
        twice, removed = kept.remove_sparse(radius, k)
        assert twice.merged and removed == again.removed
        PV.assert_equal(arrays_of(twice), plain(again), dev)
        PV.assert_equal(arrays_of(merged), m, "the input")


def test_a_merged_object_of_many_views(gpu_pkg, checker, voxel_checker):
    """Lists of up to 200 views that no mask holds: the kept points' lists, the merged flag and support are the checker's."""
    c, views, first = merged_many_views_case(voxel_checker)
    want = PR.remove(checker, first, MERGED_RADIUS, MERGED_MIN)
    assert 0 < want.removed < first.count and np.diff(want.offsets).max() > 32
    for dev in (False, True):
        merged, _ = from_cloud(gpu_pkg, c, *views, on_device=dev).merge_voxels(1.0)
        assert np.array_equal(host_counts(merged.neighbour_counts(MERGED_RADIUS, 5)), PR.counts(checker, first, MERGED_RADIUS, 5))
        kept, removed = merged.remove_sparse(MERGED_RADIUS, MERGED_MIN)
        assert kept.merged and removed == want.removed
        PV.assert_equal(arrays_of(kept), plain(want), dev)
        assert np.array_equal(arrays_of(kept).support, first.support[want.index])


def test_two_runs_give_the_same_bytes(gpu_pkg, checker, tmp_path):
    c, views = determinism_case()
    pts = from_cloud(gpu_pkg, c, *views, on_device=True)
    files = []
    for run in range(2):
        kept, _ = pts.remove_sparse(1.0, 3)
        kept.write_ply(tmp_path / ("%d.ply" % run), normals=True)
        kept.write_vis(tmp_path / ("%d.vis" % run))
        files.append(((tmp_path / ("%d.ply" % run)).read_bytes(), (tmp_path / ("%d.vis" % run)).read_bytes(),
                      host_counts(pts.neighbour_counts(1.0)).tobytes()))
    assert files[0] == files[1]
    want = PR.remove(checker, c, 1.0, 3)
    assert files[0][0] == ply_bytes(want, True) and files[0][1] == VC.vis_bytes(want.offsets, want.views)


# --------------------------------------------------------------------------------------------------------------------
# the pipeline and the binary
# --------------------------------------------------------------------------------------------------------------------

def chosen(checker, whole):
    """(radius, min_neighbours, the checker's kept points) for a Points object: the choice of the real clouds."""
    w = arrays_of(whole)
    radius = real_cloud_radius(checker, w)
    k = real_cloud_min_neighbours(PR.counts(checker, w, radius))
    want = PR.remove(checker, w, radius, k)
    assert 0 < want.removed < w.count
    if w.count <= 20001:
        modes_agree(checker, w, radius, (k,), what="pipeline points")
    return radius, k, want


def test_through_the_pipeline(gpu_pkg, ob, checker, tmp_path):
    """fuse(radius_filter=...) returns and writes the filtered points, after the averaging and the merge when those are asked for:
    the bytes of Points.write_ply / write_vis of the manual chain, which are the checker's."""
    from apd_mvs_amd import pipeline
    case = fusion_cases.case("mixed_sizes")
    scene, results = _scene(gpu_pkg, pipeline, case)
    options = gpu_pkg.default_fusion_options(ply_normals=1)
    for kw in (dict(), dict(average=True, voxel=0.05)):
        _, whole = pipeline.fuse(scene, results, None, return_points=True, **kw)
        radius, k, want = chosen(checker, whole)
        manual, _ = whole.remove_sparse(radius, k)
        manual.write_ply(tmp_path / "manual.ply", normals=True)
        manual.write_vis(tmp_path / "manual.vis")
        n, kept = pipeline.fuse(scene, results, tmp_path / "m.ply", return_points=True, vis_path=tmp_path / "m.vis", radius_filter=(radius, k),
                                options=options, **kw)
        assert n == want.count == kept.count and kept.merged == ("voxel" in kw)
        PV.assert_equal(arrays_of(kept), plain(want), kw)
        assert (tmp_path / "m.ply").read_bytes() == (tmp_path / "manual.ply").read_bytes() == ply_bytes(want, True)
        assert (tmp_path / "m.vis").read_bytes() == (tmp_path / "manual.vis").read_bytes() == VC.vis_bytes(want.offsets, want.views)
        assert pipeline.fuse(scene, results, tmp_path / "file_only.ply", radius_filter=(radius, k), options=options, **kw) == n
        assert (tmp_path / "file_only.ply").read_bytes() == (tmp_path / "m.ply").read_bytes()


VOXEL = "0.25"
# the flags of a run before --ply-radius-filter, and what the pipeline needs to make the points the filter starts from
RUNS = {"filter": ([], dict(), False),
        "filter_all": (["--ply-mean", "--ply-voxel", VOXEL, "--ply-vis", "--ply-normals"], dict(average=True, voxel=float(VOXEL)), True),
        "filter_tat": (["--fusion", "tat-advanced", "--ply-vis"], dict(variant="tat_advanced"), False)}


@pytest.fixture(scope="module")
def folders(gpu_pkg, synth, checker, tmp_path_factory):
    """One small synthetic dense folder (the size of the drop-in tests) run without the flag; then, with the radius and the minimum
    the checker chooses on the points the pipeline makes from that run's maps, with the flag alone, with the mean, the merge, the
    lists and the normals, and with a Tanks and Temples loop."""
    root = tmp_path_factory.mktemp("dense")
    a = root / "a"
    a.mkdir()
    _write_dense_folder(a, synth, 96, 72, 4)
    shutil.copytree(a, root / "plain")
    _run(root / "plain")
    out = {"plain": (root / "plain", None, None)}
    for name, (flags, kw, _) in RUNS.items():
        options = gpu_pkg.default_fusion_options(ply_normals=1) if "--ply-normals" in flags else None
        _, whole = _fuse_saved_maps(gpu_pkg, root / "plain", None, return_points=True, options=options, **kw)
        radius, k, _ = chosen(checker, whole)
        shutil.copytree(a, root / name)
        _run(root / name, *flags, "--ply-radius-filter", "%.9g,%d" % (radius, k))
        out[name] = (root / name, radius, k)
    return out


def test_binary_writes_the_filtered_points(gpu_pkg, checker, folders):
    """APD.ply and APD.ply.vis of the binary against the checker's removal from the points the pipeline makes from the binary's maps."""
    for name, (flags, kw, normals) in RUNS.items():
        folder, radius, k = folders[name]
        options = gpu_pkg.default_fusion_options(ply_normals=1) if normals else None
        _, whole = _fuse_saved_maps(gpu_pkg, folder, None, return_points=True, options=options, **kw)
        want = PR.remove(checker, arrays_of(whole), radius, k)
        assert 0 < want.removed < whole.count, name
        assert (folder / "APD" / "APD.ply").read_bytes() == ply_bytes(want, normals), name
        manual, _ = whole.remove_sparse(radius, k)
        assert arrays_of(manual).count == want.count
        vis = folder / "APD" / "APD.ply.vis"
        assert vis.exists() == ("--ply-vis" in flags)
        if vis.exists():
            assert vis.read_bytes() == VC.vis_bytes(want.offsets, want.views), name


def test_binary_without_the_flag_keeps_its_bytes(gpu_pkg, folders, tmp_path):
    plain_ply = (folders["plain"][0] / "APD" / "APD.ply").read_bytes()
    assert _fuse_saved_maps(gpu_pkg, folders["plain"][0], tmp_path / "pipe.ply") > 0
    assert hashlib.md5(plain_ply).hexdigest() == hashlib.md5((tmp_path / "pipe.ply").read_bytes()).hexdigest()
    assert len((folders["filter"][0] / "APD" / "APD.ply").read_bytes()) < len(plain_ply)


def test_binary_refuses_a_bad_value_before_anything_is_read(tmp_path):
    for bad in ("0,1", "-1,2", "nan,1", "inf,1", "1e30,1", "1e-30,1", "1", "1,", ",1", "1,-1", "1,x", "1x,1", "1,2,3", ""):
        r = subprocess.run([APD_BIN, str(tmp_path / "no_such_folder"), "0", "--ply-radius-filter", bad], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=60)
        assert r.returncode != 0 and "bad value '%s' of --ply-radius-filter" % bad in r.stdout and "USAGE" in r.stdout, (bad, r.stdout[-500:])
