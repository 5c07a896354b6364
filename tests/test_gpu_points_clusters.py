"""Connected components within a radius and the removal of small ones on the device (apd_points_components,
apd_points_remove_small_components; csrc/apd_points_clusters.hip, compact_points of csrc/apd_points.hip), bitwise against the grid
mode of the sequential checker (tests/helpers/points_cluster_ref.cpp): the labels, the sizes, the number of components, all seven
arrays of the kept points, their lists and `removed`, for host- and for device-resident points; the shapes a concurrent union-find
can go wrong on; real clouds; merged objects; the files; the Python layer, the pipeline and the drop-in binary.  The clouds are
made in test_points_clusters.py, where the checker's brute-force mode is held against the grid mode on them."""
import hashlib
import shutil
import subprocess

import numpy as np
import pytest

import fusion_cases
import points_cluster_checker as PC
import points_knn_checker as PK
import points_radius_checker as PR
import points_voxel_checker as PV
import vis_checker as VC
from test_gpu_dropin_binary import _write_dense_folder
from test_gpu_fusion_options import APD_BIN, _fuse_saved_maps, _run, _scene
from test_gpu_points_average import averaged, fused
from test_points_clusters import (CHAIN, TEETH, TOOTH, WIDE_MINS, chain_case, comb_case, consistent, modes_agree, real_cloud_min_size, two_chains_case,
                                  wide_case)
from test_points_knn import real_cloud_choice
from test_points_radius import (DENSE_ORIGIN, DENSE_RADIUS, border_case, dense_case, determinism_case, dressed, grid_edge_case, large_case, outside_case,
                                real_cloud_min_neighbours, real_cloud_radius, size_case, size_list)
from test_points_voxel import REAL_CLOUDS, arrays_of, from_cloud, ply_bytes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return PC.build(tmp_path_factory.mktemp("points_cluster_checker"))


@pytest.fixture(scope="module")
def radius_checker(tmp_path_factory):
    return PR.build(tmp_path_factory.mktemp("points_radius_checker"))


@pytest.fixture(scope="module")
def knn_checker(tmp_path_factory):
    return PK.build(tmp_path_factory.mktemp("points_knn_checker"))


@pytest.fixture(scope="module")
def voxel_checker(tmp_path_factory):
    return PV.build(tmp_path_factory.mktemp("points_voxel_checker"))


def host_u32(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32)


def plain(c):
    """The arrays and lists of a checker result as a PV.Cloud without its extras."""
    return PV.Cloud(*[getattr(c, f) for f in PV.FIELDS], c.offsets, c.views)


def check(pkg, checker, c, views, radius, origin=None, mins=(2, 4), must_remove=True, what=""):
    """Labels, sizes and the number of components of `c` (a PV.Cloud over views = (rows, cols, pairs)) and its removal at every
    minimum, as host- and as device-resident points, against the checker's grid mode.  Returns the checker's (label, size,
    components)."""
    want = PC.components(checker, c, radius, origin)
    want_kept = {k: PC.remove(checker, c, radius, k, origin) for k in mins}
    for k, w in want_kept.items():
        assert not must_remove or 0 < w.removed < c.count, (what, k, w.removed)
    for dev in (False, True):
        pts = from_cloud(pkg, c, *views, on_device=dev)
        label, size, components = pts.components(radius, origin)
        assert hasattr(label, "cpu") == dev and hasattr(size, "cpu") == dev, (what, dev)
        label, size = host_u32(label), host_u32(size)
        assert label.shape == want[0].shape and np.array_equal(label, want[0]), (what, dev, "label")
        assert size.shape == want[1].shape and np.array_equal(size, want[1]), (what, dev, "size")
        assert components == want[2], (what, dev, components, want[2])
        for k, w in want_kept.items():
            kept, removed, components = pts.remove_small_components(radius, k, origin)
            assert kept.on_device == dev and not kept.merged and kept.count == w.count and removed == w.removed, (what, dev, k)
            assert components == want[2], (what, dev, k)
            PV.assert_equal(arrays_of(kept), plain(w), (what, dev, k))
            kept.close()
        pts.close()
    return want


def choose(checker, radius_checker, c):
    """(radius, min_size) for a cloud whose shape nobody knows beforehand, from the checkers alone: the radius of the real clouds,
    halved until the components are not all of one size, and the smallest minimum that then removes some points and not all."""
    radius = real_cloud_radius(radius_checker, c)
    for _ in range(8):
        k = real_cloud_min_size(PC.components(checker, c, radius)[1])
        if k is not None:
            return radius, k
        radius = float(np.float32(0.5 * radius))
    raise AssertionError("one size of components at every radius tried")


def run_binary(folder, *extra):
    """_run of test_gpu_fusion_options.py, returning what the binary printed."""
    r = subprocess.run([APD_BIN, str(folder), "0", "--seed", "21", "--iters", "1", "--keep-maps"] + list(extra), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "All done" in r.stdout, r.stdout[-2000:]
    return r.stdout


# --------------------------------------------------------------------------------------------------------------------
# sizes and shapes
# --------------------------------------------------------------------------------------------------------------------

def test_sizes_around_waves_blocks_and_tiles(gpu_pkg, checker):
    """n = 0, 1, 2, around a wave and a block, 3 T + 17 and 5 T + 17, about three points per cell at radius 1: labels, sizes, and
    removal at 2 and at 4 points."""
    for n in size_list(gpu_pkg):
        c, views = size_case(gpu_pkg, n)
        label, size, components = check(gpu_pkg, checker, c, views, 1.0, must_remove=n >= 63, what=n)
        consistent(label, size, components)


def test_one_chain_in_shuffled_order(gpu_pkg, checker):
    """5 000 points on a line 0.75 apart: one component that carries the label of input point 0 everywhere -- deep trees, hooks
    across waves and blocks."""
    c, views = dressed(np.random.default_rng(21), chain_case(np.random.default_rng(22))[0])
    label, size, components = check(gpu_pkg, checker, c, views, 1.0, mins=(2,), must_remove=False)
    assert components == 1 and (label == 0).all() and (size == CHAIN).all()


def test_a_chain_with_one_gap_of_the_next_binary32_after_the_radius(gpu_pkg, checker):
    c, views = dressed(np.random.default_rng(23), chain_case(np.random.default_rng(24), True)[0])
    label, size, components = check(gpu_pkg, checker, c, views, 1.0, mins=(CHAIN // 2 + 1,))
    assert components == 2 and sorted(np.unique(size).tolist()) == [CHAIN - CHAIN // 2 - 1, CHAIN // 2 + 1]


def test_two_chains_in_adjacent_cells_that_never_touch(gpu_pkg, checker):
    """1.5 apart, interleaved in input order: every walk meets the other chain's points and unites none of them."""
    c, views = dressed(np.random.default_rng(25), two_chains_case())
    label, size, components = check(gpu_pkg, checker, c, views, 1.0, mins=(2,), must_remove=False)
    assert components == 2 and label.tolist() == [0, 1] * (c.count // 2) and (size == c.count // 2).all()


@pytest.mark.parametrize("along", [0, 1])
def test_a_comb_joins_late(gpu_pkg, checker, along):
    """64 teeth of 200 points: 64 components without the spine at their far end, one with it -- components that span many
    workgroups and merge through single edges."""
    c, views = dressed(np.random.default_rng(26), comb_case(np.random.default_rng(27 + along), along, False)[0])
    label, size, components = check(gpu_pkg, checker, c, views, 1.0, mins=(TOOTH, TOOTH + 1), must_remove=False)
    assert components == TEETH and (size == TOOTH).all()
    c, views = dressed(np.random.default_rng(26), comb_case(np.random.default_rng(27 + along), along, True)[0])
    label, size, components = check(gpu_pkg, checker, c, views, 1.0, mins=(TOOTH, TOOTH + 1), must_remove=False)
    assert components == 1 and (label == 0).all() and (size == TEETH * TOOTH + TEETH - 1).all()


def test_cell_borders_and_coincident_points(gpu_pkg, checker):
    """Points on cell borders, pairs at exactly the radius and at the next binary32 after it, coincident points: the hand-computed
    components of test_points_clusters.py."""
    c, views = dressed(np.random.default_rng(1), border_case()[0])
    label, size, components = check(gpu_pkg, checker, c, views, 1.0, mins=(2, 3))
    assert components == 14 and size.tolist() == [3, 3, 3, 2, 2, 1, 1, 2, 2, 1, 1, 2, 2, 2, 2, 1, 1, 2, 2, 3, 3, 3, 3, 3, 3]
    assert label[19:].tolist() == [19, 19, 19, 22, 22, 22]


def test_edges_of_the_grid(gpu_pkg, checker):
    """x cells 2^20 - 1 and -2^20 of adjacent y rows have consecutive keys and stay in different components."""
    c, views = dressed(np.random.default_rng(2), grid_edge_case()[0])
    label, size, components = check(gpu_pkg, checker, c, views, 1.0, mins=(2, 3), must_remove=False)   # 2 removes nothing: no point stands alone
    assert label.tolist() == [0, 1, 0, 1, 1, 5, 5, 7, 7, 9, 9, 11, 11, 13, 13, 15, 15] and components == 8
    assert PC.remove(checker, c, 1.0, 3).index.tolist() == [1, 3, 4]


def test_an_origin_off_the_lattice(gpu_pkg, checker):
    c, views = dressed(np.random.default_rng(5), wide_case()[:3000] * 0.5)
    check(gpu_pkg, checker, c, views, 1.0, [0.25, -0.5, 0.125], mins=(3,))


def test_points_outside_the_grid(gpu_pkg, checker):
    """NaN, infinities and points 3 * 2^20 cells out among ordinary points: each is a component of its own, goes at a minimum of 2
    and stays at 0 and 1, where the result is the input in all seven arrays and the lists."""
    xyz, bad = outside_case(np.random.default_rng(4))
    c, views = dressed(np.random.default_rng(3), xyz)
    label, size, _ = check(gpu_pkg, checker, c, views, 1.0, mins=(2,))
    assert label[bad].tolist() == bad and (size[bad] == 1).all()
    assert not np.isin(bad, PC.remove(checker, c, 1.0, 2).index).any()
    for dev in (False, True):
        pts = from_cloud(gpu_pkg, c, *views, on_device=dev)
        for k in (0, 1):
            kept, removed, components = pts.remove_small_components(1.0, k)
            assert removed == 0 and kept.count == c.count and components == PC.components(checker, c, 1.0)[2]
            PV.assert_equal(arrays_of(kept), c, (dev, k))
    # and every point outside: n components, an object without points
    none = dressed(np.random.default_rng(5), np.full((300, 3), np.nan, np.float32))
    label, size, components = check(gpu_pkg, checker, *none, 1.0, mins=(0, 1), must_remove=False)
    assert components == 300 and label.tolist() == list(range(300)) and (size == 1).all()
    for dev in (False, True):
        kept, removed, components = from_cloud(gpu_pkg, none[0], *none[1], on_device=dev).remove_small_components(1.0, 2)
        assert kept.count == 0 and removed == 300 and components == 300 and kept.visibility()[0].tolist() == [0]


def test_one_cell_of_twenty_thousand_members(gpu_pkg, checker):
    """20 001 points in one cell: after the first few every edge joins two points of one tree, and every wave reduces into one
    root.  One component."""
    c, views = dressed(np.random.default_rng(7), dense_case(np.random.default_rng(8)))
    label, size, components = check(gpu_pkg, checker, c, views, DENSE_RADIUS, DENSE_ORIGIN, mins=(2,), must_remove=False)
    assert components == 1 and (label == 0).all() and (size == c.count).all()


def test_a_wide_distribution_of_sizes(gpu_pkg, checker):
    """20 000 uniform points at 0.6 to a cell: thousands of components from singletons to hundreds of points; removal at 2, 8, 64."""
    c, views = dressed(np.random.default_rng(12), wide_case())
    label, size, components = check(gpu_pkg, checker, c, views, 1.0, mins=WIDE_MINS)
    consistent(label, size, components)
    assert components >= 1000 and size.max() >= 64


def test_a_table_scan_of_several_blocks(gpu_pkg, checker):
    """2 * 10^5 points over n / 4 cells: the sort's [digit][block] table and the scan of the component flags take several blocks."""
    c, views = dressed(np.random.default_rng(9), large_case(np.random.default_rng(10)))
    label, size, components = check(gpu_pkg, checker, c, views, 1.0, mins=(4,))
    consistent(label, size, components)


# --------------------------------------------------------------------------------------------------------------------
# real clouds, merged objects
# --------------------------------------------------------------------------------------------------------------------

SINGLE = []   # the real clouds that are one component at their radius


@pytest.mark.parametrize("name,variant", [(n, v) for n, v, _ in REAL_CLOUDS])
def test_real_clouds(gpu_pkg, ob, checker, radius_checker, name, variant):
    """Fused on the device and filtered where they are, at three times the median nearest-point spacing and the smallest minimum
    for which the checker removes something and not everything.  The lists of the result, built from its sources, are the
    input's at the kept indices."""
    case = fusion_cases.case(name)
    radius = k = None
    for dev in (False, True):
        pts = fused(gpu_pkg, ob, case, variant, dev)
        before = arrays_of(pts)
        if radius is None:
            radius = real_cloud_radius(radius_checker, before)
        want = PC.components(checker, before, radius)
        label, size, components = pts.components(radius)
        assert np.array_equal(host_u32(label), want[0]) and np.array_equal(host_u32(size), want[1]) and components == want[2]
        k = real_cloud_min_size(want[1])
        if k is None:   # the labels of both residences are checked; the removal has nothing to show
            continue
        w = PC.remove(checker, before, radius, k)
        assert 0 < w.removed < before.count
        if before.count <= 20001 and not dev:   # the device's own fusion, held against the loop over all pairs too
            modes_agree(checker, before, radius, (k,), what=(name, variant))
        kept, removed, components = pts.remove_small_components(radius, k)
        assert kept.on_device == dev and removed == w.removed and components == want[2]
        got = arrays_of(kept)
        PV.assert_equal(got, plain(w), (name, variant, dev))
        assert np.array_equal(np.diff(got.offsets), np.diff(before.offsets)[w.index])
        assert np.array_equal(got.views, np.concatenate([before.views[before.offsets[i]:before.offsets[i + 1]] for i in w.index]))
        PV.assert_equal(arrays_of(pts), before, "the input")
    if k is None:
        SINGLE.append((name, variant))
        assert len(set(SINGLE)) <= 1, SINGLE
        pytest.skip("%s %s has components of one size only at radius %g: no minimum removes some points and not all" % (name, variant, radius))


def test_the_chain_a_user_runs(gpu_pkg, ob, checker, radius_checker, knn_checker, voxel_checker, tmp_path):
    """average, merge_voxels, remove_statistical, remove_sparse, remove_small_components: the lists and the .vis bytes of the
    result are the checkers', the result is a merged object, average() refuses it, and it can be filtered again."""
    case = fusion_cases.case("mixed_sizes")
    for dev in (False, True):
        pts = fused(gpu_pkg, ob, case, "eth", dev)
        mean = averaged(gpu_pkg, case, pts, dev)
        merged, _ = mean.merge_voxels(0.02)
        m = arrays_of(merged)
        PV.assert_equal(m, PV.merge(voxel_checker, arrays_of(mean), 0.02))
        radius, neighbours, ratio = real_cloud_choice(radius_checker, knn_checker, m)
        stat, _, _ = merged.remove_statistical(radius, neighbours, ratio)
        s = arrays_of(stat)
        PV.assert_equal(s, plain(PK.remove(knn_checker, m, radius, neighbours, ratio)), (dev, "statistical"))
        least = real_cloud_min_neighbours(PR.counts(radius_checker, s, radius))
        sparse, _ = stat.remove_sparse(radius, least)
        before = arrays_of(sparse)
        PV.assert_equal(before, plain(PR.remove(radius_checker, s, radius, least)), (dev, "sparse"))
        radius, k = choose(checker, radius_checker, before)
        want = PC.remove(checker, before, radius, k)
        assert 0 < want.removed < before.count
        if before.count <= 20001 and not dev:
            modes_agree(checker, before, radius, (k,), what="the chain")
        kept, removed, _ = sparse.remove_small_components(radius, k)
        assert kept.merged and kept.on_device == dev and removed == want.removed
        PV.assert_equal(arrays_of(kept), plain(want), dev)
        kept.write_vis(tmp_path / "k.vis")
        assert (tmp_path / "k.vis").read_bytes() == VC.vis_bytes(want.offsets, want.views)
        with pytest.raises(gpu_pkg.ApdError, match="apd_points_average: merged points name no sources"):
            averaged(gpu_pkg, case, kept, dev)
        bigger = real_cloud_min_size(PC.components(checker, plain(want), radius)[1]) or k + 1
        again = PC.remove(checker, plain(want), radius, bigger)
        twice, removed, _ = kept.remove_small_components(radius, bigger)
        assert twice.merged and removed == again.removed
        PV.assert_equal(arrays_of(twice), plain(again), dev)
        PV.assert_equal(arrays_of(sparse), before, "the input")


def test_two_runs_give_the_same_bytes(gpu_pkg, checker, tmp_path):
    c, views = determinism_case()
    pts = from_cloud(gpu_pkg, c, *views, on_device=True)
    files = []
    for run in range(2):
        kept, _, _ = pts.remove_small_components(1.0, 3)
        kept.write_ply(tmp_path / ("%d.ply" % run), normals=True)
        kept.write_vis(tmp_path / ("%d.vis" % run))
        label, size, _ = pts.components(1.0)
        files.append(((tmp_path / ("%d.ply" % run)).read_bytes(), (tmp_path / ("%d.vis" % run)).read_bytes(), host_u32(label).tobytes(),
                      host_u32(size).tobytes()))
    assert files[0] == files[1]
    want = PC.remove(checker, c, 1.0, 3)
    assert 0 < want.removed < c.count
    assert files[0][0] == ply_bytes(want, True) and files[0][1] == VC.vis_bytes(want.offsets, want.views)
    assert files[0][2] == PC.components(checker, c, 1.0)[0].tobytes()


# --------------------------------------------------------------------------------------------------------------------
# the pipeline and the binary
# --------------------------------------------------------------------------------------------------------------------

def chosen(checker, radius_checker, whole):
    """(radius, min_size, the checker's kept points) for a Points object."""
    w = arrays_of(whole)
    radius, k = choose(checker, radius_checker, w)
    want = PC.remove(checker, w, radius, k)
    assert 0 < want.removed < w.count
    if w.count <= 20001:
        modes_agree(checker, w, radius, (k,), what="pipeline points")
    return radius, k, want


def test_through_the_pipeline(gpu_pkg, ob, checker, radius_checker, tmp_path):
    """fuse(component_filter=...) returns and writes the filtered points, alone and after the averaging, the merge and the radius
    filter: the bytes of Points.write_ply / write_vis of the manual chain, which are the checker's."""
    from apd_mvs_amd import pipeline
    case = fusion_cases.case("mixed_sizes")
    scene, results = _scene(gpu_pkg, pipeline, case)
    options = gpu_pkg.default_fusion_options(ply_normals=1)
    _, merged = pipeline.fuse(scene, results, None, return_points=True, average=True, voxel=0.05)
    m = arrays_of(merged)
    sparse_radius = real_cloud_radius(radius_checker, m)
    sparse = (sparse_radius, real_cloud_min_neighbours(PR.counts(radius_checker, m, sparse_radius)))
    for kw in (dict(), dict(average=True, voxel=0.05, radius_filter=sparse)):
        _, whole = pipeline.fuse(scene, results, None, return_points=True, **kw)
        radius, k, want = chosen(checker, radius_checker, whole)
        manual, _, _ = whole.remove_small_components(radius, k)
        manual.write_ply(tmp_path / "manual.ply", normals=True)
        manual.write_vis(tmp_path / "manual.vis")
        n, kept = pipeline.fuse(scene, results, tmp_path / "m.ply", return_points=True, vis_path=tmp_path / "m.vis", component_filter=(radius, k),
                                options=options, **kw)
        assert n == want.count == kept.count and kept.merged == ("voxel" in kw)
        PV.assert_equal(arrays_of(kept), plain(want), kw)
        assert (tmp_path / "m.ply").read_bytes() == (tmp_path / "manual.ply").read_bytes() == ply_bytes(want, True)
        assert (tmp_path / "m.vis").read_bytes() == (tmp_path / "manual.vis").read_bytes() == VC.vis_bytes(want.offsets, want.views)
        assert pipeline.fuse(scene, results, tmp_path / "file_only.ply", component_filter=(radius, k), options=options, **kw) == n
        assert (tmp_path / "file_only.ply").read_bytes() == (tmp_path / "m.ply").read_bytes()


VOXEL = "0.25"
# the flags of a run before --ply-component-filter, what the pipeline needs to make the points the filter starts from, and whether
# the radius filter runs before it (with the radius and the minimum the radius checker chooses)
RUNS = {"filter": ([], dict(), False, False),
        "filter_all": (["--ply-mean", "--ply-voxel", VOXEL, "--ply-vis", "--ply-normals"], dict(average=True, voxel=float(VOXEL)), True, True)}


@pytest.fixture(scope="module")
def folders(gpu_pkg, synth, checker, radius_checker, tmp_path_factory):
    """One small synthetic dense folder (the size of the drop-in tests) run without the flag; then, with the radius and the minimum
    the checkers choose on the points the pipeline makes from that run's maps, with the flag alone, and with the mean, the merge,
    the lists, the normals and the radius filter."""
    root = tmp_path_factory.mktemp("dense")
    a = root / "a"
    a.mkdir()
    _write_dense_folder(a, synth, 96, 72, 4)
    shutil.copytree(a, root / "plain")
    _run(root / "plain")
    out = {"plain": (root / "plain", None, None, None)}
    for name, (flags, kw, normals, with_radius) in RUNS.items():
        options = gpu_pkg.default_fusion_options(ply_normals=1) if normals else None
        sparse = None
        if with_radius:
            _, first = _fuse_saved_maps(gpu_pkg, root / "plain", None, return_points=True, options=options, **kw)
            f = arrays_of(first)
            r = real_cloud_radius(radius_checker, f)
            sparse = (r, real_cloud_min_neighbours(PR.counts(radius_checker, f, r)))
            kw = dict(kw, radius_filter=sparse)
            flags = flags + ["--ply-radius-filter", "%.9g,%d" % sparse]
        _, whole = _fuse_saved_maps(gpu_pkg, root / "plain", None, return_points=True, options=options, **kw)
        radius, k, _ = chosen(checker, radius_checker, whole)
        shutil.copytree(a, root / name)
        out[name] = (root / name, radius, k, sparse, run_binary(root / name, *flags, "--ply-component-filter", "%.9g,%d" % (radius, k)))
    return out


def test_binary_writes_the_filtered_points(gpu_pkg, checker, folders):
    """APD.ply and APD.ply.vis of the binary against the checker's removal from the points the pipeline makes from the binary's
    maps; the binary prints the components and the removed points."""
    for name, (flags, kw, normals, _) in RUNS.items():
        folder, radius, k, sparse, output = folders[name]
        options = gpu_pkg.default_fusion_options(ply_normals=1) if normals else None
        kw = dict(kw, radius_filter=sparse) if sparse else kw
        _, whole = _fuse_saved_maps(gpu_pkg, folder, None, return_points=True, options=options, **kw)
        w = arrays_of(whole)
        want = PC.remove(checker, w, radius, k)
        assert 0 < want.removed < whole.count, name
        assert (folder / "APD" / "APD.ply").read_bytes() == ply_bytes(want, normals), name
        manual, removed, components = whole.remove_small_components(radius, k)
        assert arrays_of(manual).count == want.count and components == PC.components(checker, w, radius)[2]
        assert ("Removed %d of %d points in connected components of fewer than %d points, of %d components" % (removed, w.count, k, components)) in output, name
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
        r = subprocess.run([APD_BIN, str(tmp_path / "no_such_folder"), "0", "--ply-component-filter", bad], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=60)
        assert r.returncode != 0 and "bad value '%s' of --ply-component-filter" % bad in r.stdout and "USAGE" in r.stdout, (bad, r.stdout[-500:])
