"""The voxel-grid merge on the device (apd_points_merge_voxels over the radix sort of csrc/apd_sort.hip), bitwise against the
sequential checker (tests/helpers/points_voxel_ref.cpp): all seven arrays, the lists and `dropped`; host- and device-resident
points made with Points.from_arrays at the sizes and with the keys a sort can go wrong on; many views; real clouds; a merged
object merged again; the files; the Python layer, the pipeline and the drop-in binary."""
import ctypes as C
import hashlib
import shutil
import subprocess

import numpy as np
import pytest

import fusion_cases
import points_voxel_checker as PV
import vis_checker as VC
from test_gpu_dropin_binary import _write_dense_folder
from test_gpu_fusion_options import APD_BIN, _fuse_saved_maps, _run, _scene
from test_gpu_points_average import averaged, fused
from test_points_voxel import REAL_CLOUDS, arrays_of, cloud, from_cloud, ply_bytes, views_of

pytestmark = pytest.mark.gpu

BIG = 1e9   # one cell of this size at origin -BIG / 2 holds every coordinate of magnitude up to 5e8


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return PV.build(tmp_path_factory.mktemp("points_voxel_checker"))


@pytest.fixture(scope="module")
def tiles(gpu_pkg):
    """(T, S): elements per workgroup of a sort pass, entries per workgroup of the scan under it -- the implementation's constants."""
    t, s = C.c_int(), C.c_int()
    gpu_pkg.lib().apd_sort_tile_sizes(C.byref(t), C.byref(s))
    assert t.value >= 256 and s.value >= 256
    return t.value, s.value


def check(pkg, checker, c, views, size, origin=None, on_device=(False, True), what=""):
    """Merges `c` (a PV.Cloud over views = (rows, cols, pairs)) as host- and as device-resident points and holds every array, the
    lists and `dropped` to the checker's.  Returns the checker's result."""
    want = PV.merge(checker, c, size, origin)
    for dev in on_device:
        pts = from_cloud(pkg, c, *views, on_device=dev)
        merged, dropped = pts.merge_voxels(size, origin)
        assert merged.on_device == dev and merged.merged and not pts.merged and merged.count == want.count, (what, dev)
        PV.assert_equal(arrays_of(merged), want, (what, dev))
        assert dropped == want.dropped, (what, dev)
        merged.close()
        pts.close()
    return want


def random_cloud(rng, xyz, num_views=3, nsrc=2):
    n = len(xyz)
    rows, cols, pairs = views_of(num_views, nsrc)
    view = rng.integers(0, num_views, n).astype(np.int32)
    sources = rng.integers(0, 1 << nsrc, n).astype(np.uint32)
    c = cloud(xyz, normal=rng.normal(size=(n, 3)).astype(np.float32), bgr=rng.integers(0, 256, (n, 3)).astype(np.uint8), view=view, sources=sources,
              pairs=pairs)
    return c, (rows, cols, pairs)


def cells_from_a_pool(rng, n, lo, hi, pool):
    """n points in cells drawn from a pool of `pool` random cells of [lo, hi)^3 (voxel size 1), at random places inside them."""
    cells = rng.integers(lo, hi, (max(pool, 1), 3))
    return (cells[rng.integers(0, max(pool, 1), n)] + rng.random((n, 3)) * 0.5 + 0.25).astype(np.float32)


# --------------------------------------------------------------------------------------------------------------------
# sizes and keys
# --------------------------------------------------------------------------------------------------------------------

def test_sizes_around_waves_blocks_and_tiles(gpu_pkg, checker, tiles):
    """n = 0, 1, around a wave and a block, 3 T + 17 and 5 T + 17: full-range cells (every one of the eight digits varies), a third
    as many cells as points, so cells have several members standing apart in the input."""
    T, _ = tiles
    rng = np.random.default_rng(5)
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 3 * T + 17, 5 * T + 17):
        c, views = random_cloud(rng, cells_from_a_pool(rng, n, -2 ** 20, 2 ** 20, n // 3))
        want = check(gpu_pkg, checker, c, views, 1.0, what=n)
        assert want.dropped == 0 and (n < 3 or want.count < n)


def test_a_table_scan_of_several_blocks(gpu_pkg, checker, tiles):
    """2 * 10^5 points: the [digit][block] table of a pass has 256 * ceil(n / T) entries, more than one block S of its scan."""
    T, S = tiles
    n = 200000
    assert 256 * ((n + T - 1) // T) > 2 * S
    rng = np.random.default_rng(6)
    c, views = random_cloud(rng, cells_from_a_pool(rng, n, -2 ** 20, 2 ** 20, n // 4))
    want = check(gpu_pkg, checker, c, views, 1.0)
    assert 1 < want.count <= n // 4


def ring_lists(view, sources, num_views, nsrc):
    """PV.source_lists for the ring source lists of views_of(num_views, nsrc), without a Python loop over the points."""
    view = np.asarray(view, np.int64)[:, None]
    candidates = np.concatenate([view, (view + 1 + np.arange(nsrc)) % num_views], axis=1)
    listed = np.concatenate([np.ones_like(view), (np.asarray(sources, np.int64)[:, None] >> np.arange(nsrc)) & 1], axis=1).astype(bool)
    return np.concatenate([[0], np.cumsum(listed.sum(1))]).astype(np.int64), candidates[listed].astype(np.int32)


def test_scans_with_two_block_sums_in_a_lane_of_the_top_scan(gpu_pkg, checker, tiles):
    """S * 1024 + S + 17 kept points, device-resident: the scan of the keep flags and the scans of `head` and `length` over the kept
    points have more blocks than the 1024 lanes of the workgroup that scans the block sums, so every lane owns two sums and the
    upper lanes none.  (The sort and the scan on their own at this boundary and past it: tools/sort_check.hip, test_gpu_sort_scan.py.)"""
    T, S = tiles
    n = S * 1024 + S + 17
    assert n > S * 1024
    rng = np.random.default_rng(16)
    num_views, nsrc = 3, 2
    rows, cols, pairs = views_of(num_views, nsrc)
    view = rng.integers(0, num_views, n).astype(np.int32)
    sources = rng.integers(0, 1 << nsrc, n).astype(np.uint32)
    lists = ring_lists(view, sources, num_views, nsrc)
    few = PV.source_lists(view[:1000], sources[:1000], pairs)
    assert np.array_equal(lists[0][:1001], few[0]) and np.array_equal(lists[1][:few[0][-1]], few[1])
    c = cloud(cells_from_a_pool(rng, n, -2 ** 20, 2 ** 20, n // 4), normal=rng.normal(size=(n, 3)).astype(np.float32),
              bgr=rng.integers(0, 256, (n, 3)).astype(np.uint8), view=view, sources=sources, pairs=pairs, lists=lists)
    want = check(gpu_pkg, checker, c, (rows, cols, pairs), 1.0, on_device=(True,))
    assert want.dropped == 0 and 1 < want.count <= n // 4


def test_one_varying_digit(gpu_pkg, checker, tiles):
    """x cells 0 .. 255, y and z fixed: only the lowest digit differs between keys and seven passes are skipped.  And 0 .. 255 in
    z alone: the digits in between are skipped, a high one is not."""
    T, _ = tiles
    rng = np.random.default_rng(7)
    n = 3 * T + 17
    for axis in (0, 2):
        xyz = np.full((n, 3), 3.5, np.float32)
        xyz[:, axis] = rng.integers(0, 256, n) + rng.random(n).astype(np.float32) * 0.5
        c, views = random_cloud(rng, xyz)
        want = check(gpu_pkg, checker, c, views, 1.0, what=axis)
        assert want.count == 256


def test_one_cell_of_seventy_thousand_members(gpu_pkg, checker):
    """Every key equal (no pass runs): one lane adds 70001 members up in input order.  Coordinates of every magnitude up to 5e8, so
    that another order gives other bits."""
    rng = np.random.default_rng(8)
    n = 70001
    xyz = (rng.normal(size=(n, 3)) * 10.0 ** rng.integers(-2, 9, (n, 3))).astype(np.float32)
    xyz = np.clip(xyz, -4e8, 4e8)
    c, views = random_cloud(rng, xyz)
    want = check(gpu_pkg, checker, c, views, BIG, origin=[-BIG / 2] * 3)
    assert want.count == 1 and want.dropped == 0
    shuffled = rng.permutation(n)   # the sum does depend on the order: the test can tell
    other = PV.merge(checker, cloud(xyz[shuffled]), BIG, origin=[-BIG / 2] * 3)
    assert not np.array_equal(other.xyz.view(np.uint32), want.xyz.view(np.uint32))


def test_all_keys_distinct(gpu_pkg, checker, tiles):
    T, _ = tiles
    n = 3 * T + 17
    rng = np.random.default_rng(9)
    k = rng.permutation(n)
    xyz = np.stack([k % 97 - 48, k // 97 - 30, (k * 7919) % 1000003 - 500000], axis=1).astype(np.float32) + np.float32(0.5)
    c, views = random_cloud(rng, xyz)
    want = check(gpu_pkg, checker, c, views, 1.0)
    assert want.count == n


def test_equal_keys_interleaved_with_order_sensitive_values(gpu_pkg, checker, tiles):
    """Five huge cells along z; the members of each stand interleaved with the others' and carry y values of 1e8, 1, -1e8, ...:
    1e8 + 1 - 1e8 is not 1e8 - 1e8 + 1 in binary32, so two members of a cell in the wrong order change the mean's bits."""
    T, _ = tiles
    n = 4 * T + 17
    rng = np.random.default_rng(10)
    xyz = np.zeros((n, 3), np.float32)
    xyz[:, 0] = rng.normal(size=n) * 1e3
    xyz[:, 1] = rng.choice(np.float32([1e8, 1.0, -1e8, 3e7, 0.25, -7.0]), n)
    xyz[:, 2] = rng.integers(0, 5, n) * BIG
    c, views = random_cloud(rng, xyz)
    want = check(gpu_pkg, checker, c, views, BIG, origin=[-BIG / 2] * 3)
    assert want.count == 5
    assert not np.array_equal(PV.merge(checker, cloud(xyz[::-1]), BIG, origin=[-BIG / 2] * 3).xyz[:, 1].view(np.uint32), want.xyz[:, 1].view(np.uint32))


def test_dropped_points_at_the_edges(gpu_pkg, checker, tiles):
    """NaN, infinities and coordinates out of range at the first and last index and on both sides of a block of 256 and of a tile."""
    T, _ = tiles
    n = 3 * T + 17
    rng = np.random.default_rng(11)
    xyz = cells_from_a_pool(rng, n, -1000, 1000, n // 3)
    bad = [0, 1, 255, 256, 257, T - 1, T, T + 1, 2 * T, n - 2, n - 1]
    values = [np.nan, np.inf, -np.inf, 2.0 ** 20, -2.0 ** 20 - 1, 3e38]
    for j, k in enumerate(bad):
        xyz[k, j % 3] = values[j % len(values)]
    c, views = random_cloud(rng, xyz)
    want = check(gpu_pkg, checker, c, views, 1.0)
    assert want.dropped == len(bad)
    # and every point dropped: an object without points
    none = check(gpu_pkg, checker, cloud(np.full((300, 3), np.nan, np.float32)), views_of(1), 1.0)
    assert none.count == 0 and none.dropped == 300


# --------------------------------------------------------------------------------------------------------------------
# visibility
# --------------------------------------------------------------------------------------------------------------------

def many_views_cloud(rng, n, pool):
    rows, cols, _ = views_of(200)
    pairs = [[int(s) for s in rng.permutation([u for u in range(200) if u != v])[:rng.integers(0, 33)]] for v in range(200)]
    pairs[0], pairs[1] = pairs[0][:0], (pairs[1] + [u for u in range(2, 40)])[:32]
    pairs[1] = list(dict.fromkeys(pairs[1]))
    view = rng.integers(0, 200, n).astype(np.int32)
    sources = np.array([rng.integers(0, 1 << len(pairs[v])) if pairs[v] else 0 for v in view.tolist()], np.uint64).astype(np.uint32)
    c = cloud(cells_from_a_pool(rng, n, -50, 50, pool), bgr=rng.integers(0, 256, (n, 3)).astype(np.uint8), view=view, sources=sources, pairs=pairs)
    return c, (rows, cols, pairs)


def test_two_hundred_views_and_unions_past_32_and_64(gpu_pkg, checker, tmp_path):
    """3000 points of 200 views with up to 32 sources each in 40 cells: lists of more than 64 views, which no mask holds; and in
    300 cells: some between 33 and 64.  support saturates at 255 nowhere here; the .vis file holds the checker's lists."""
    rng = np.random.default_rng(12)
    for pool, low, high in ((40, 65, 201), (300, 33, 65)):
        c, views = many_views_cloud(rng, 3000, pool)
        want = check(gpu_pkg, checker, c, views, 1.0, what=pool)
        lengths = np.diff(want.offsets)
        assert ((lengths >= low) & (lengths < high)).any() and np.array_equal(want.support, np.minimum(lengths - 1, 255))
        for dev in (False, True):
            pts = from_cloud(gpu_pkg, c, *views, on_device=dev)
            merged, _ = pts.merge_voxels(1.0)
            merged.write_vis(tmp_path / "m.vis")
            assert (tmp_path / "m.vis").read_bytes() == VC.vis_bytes(want.offsets, want.views)


def test_lists_that_overlap_completely_and_not_at_all(gpu_pkg, checker):
    """Cell 0: six points of view 0 with the same two sources -- the list is those three views.  Cell 1: points of views 0, 3, 6 with
    sources {1, 2}, {4, 5}, {7, 8} -- nine views, each once."""
    rows, cols, _ = views_of(9)
    pairs = [[1, 2], [], [], [4, 5], [], [], [7, 8], [], []]
    xyz = [[0.5, 0, 0]] * 6 + [[1.5, 0, 0]] * 3
    c = cloud(xyz, view=[0] * 6 + [6, 0, 3], sources=[3] * 9, pairs=pairs)
    want = check(gpu_pkg, checker, c, (rows, cols, pairs), 1.0)
    assert want.offsets.tolist() == [0, 3, 12] and want.views.tolist() == [0, 1, 2] + list(range(9)) and want.support.tolist() == [2, 8]


def test_a_merged_object_merged_again(gpu_pkg, checker, tmp_path):
    """The second merge, on a grid twice as coarse, takes the union of the first's lists (its sources name a representative's only),
    weighs every first-level cell as one point, and equals the checker run on the checker's first result."""
    rng = np.random.default_rng(13)
    c, views = many_views_cloud(rng, 5000, 600)
    first = PV.merge(checker, c, 1.0)
    second = PV.merge(checker, first, 2.0)
    assert 1 < second.count < first.count < c.count and len(second.views) > second.count
    for dev in (False, True):
        pts = from_cloud(gpu_pkg, c, *views, on_device=dev)
        one, _ = pts.merge_voxels(1.0)
        two, dropped = one.merge_voxels(2.0)
        assert two.merged and two.on_device == dev and dropped == 0
        PV.assert_equal(arrays_of(two), second, dev)
        PV.assert_equal(arrays_of(one), first, dev)   # the first stays as it was
        two.write_vis(tmp_path / "two.vis")
        assert (tmp_path / "two.vis").read_bytes() == VC.vis_bytes(second.offsets, second.views)


# --------------------------------------------------------------------------------------------------------------------
# real clouds
# --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,variant,sizes", REAL_CLOUDS)
def test_real_clouds(gpu_pkg, ob, checker, name, variant, sizes):
    """Fused on the device, merged where they are at the two sizes chosen in test_points_voxel.py; the lists the merge starts from
    are the fusion's own (apd_points_visibility)."""
    case = fusion_cases.case(name)
    for dev in (False, True):
        pts = fused(gpu_pkg, ob, case, variant, dev)
        before = arrays_of(pts)
        for size in sizes:
            want = PV.merge(checker, before, size)
            assert 1 < want.count < before.count
            merged, dropped = pts.merge_voxels(size)
            assert merged.on_device == dev and dropped == want.dropped
            PV.assert_equal(arrays_of(merged), want, (name, variant, dev, size))
        PV.assert_equal(arrays_of(pts), before, "the input")


# --------------------------------------------------------------------------------------------------------------------
# the object, the Python layer, the pipeline and the binary
# --------------------------------------------------------------------------------------------------------------------

def test_average_refuses_a_merged_object_and_write_ply_packs_its_arrays(gpu_pkg, ob, tmp_path):
    case = fusion_cases.case("mixed_sizes")
    for dev in (False, True):
        pts = fused(gpu_pkg, ob, case, "eth", dev)
        merged, _ = pts.merge_voxels(0.05)
        with pytest.raises(gpu_pkg.ApdError, match="apd_points_average: merged points name no sources"):
            averaged(gpu_pkg, case, merged, dev)
        got = arrays_of(merged)
        for normals in (False, True):
            merged.write_ply(tmp_path / "m.ply", normals=normals)
            assert (tmp_path / "m.ply").read_bytes() == ply_bytes(got, normals)
        averaged(gpu_pkg, case, pts, dev).close()   # the points it came from are averaged as before


def test_two_merges_give_the_same_bytes(gpu_pkg, checker):
    rng = np.random.default_rng(14)
    c, views = many_views_cloud(rng, 20000, 2000)
    pts = from_cloud(gpu_pkg, c, *views, on_device=True)
    a, b = arrays_of(pts.merge_voxels(1.0)[0]), arrays_of(pts.merge_voxels(1.0)[0])
    PV.assert_equal(a, b)
    PV.assert_equal(a, PV.merge(checker, c, 1.0))


def test_merge_reports_its_timing(gpu_pkg):
    L = gpu_pkg.lib()
    rng = np.random.default_rng(15)
    c, views = random_cloud(rng, cells_from_a_pool(rng, 5000, -10, 10, 500))
    from_cloud(gpu_pkg, c, *views).merge_voxels(1.0)
    ms = [C.c_double(-1) for _ in range(3)]
    assert L.apd_fusion_last_timing(*[C.byref(m) for m in ms]) == 0
    assert ms[0].value > 0 and ms[1].value > 0 and ms[2].value == 0


def test_through_the_pipeline(gpu_pkg, ob, checker, tmp_path):
    """fuse(voxel=...) returns and writes the merged points; with average=True the merge comes after the averaging."""
    from apd_mvs_amd import pipeline
    case = fusion_cases.case("mixed_sizes")
    scene, results = _scene(gpu_pkg, pipeline, case)
    options = gpu_pkg.default_fusion_options(ply_normals=1)
    for average in (False, True):
        _, whole = pipeline.fuse(scene, results, None, return_points=True, average=average)
        want = PV.merge(checker, arrays_of(whole), 0.05)
        n, merged = pipeline.fuse(scene, results, tmp_path / "m.ply", return_points=True, vis_path=tmp_path / "m.vis", average=average, voxel=0.05,
                                  options=options)
        assert n == want.count == merged.count and merged.merged and 1 < n < whole.count
        PV.assert_equal(arrays_of(merged), want, average)
        assert (tmp_path / "m.ply").read_bytes() == ply_bytes(want, True)
        assert (tmp_path / "m.vis").read_bytes() == VC.vis_bytes(want.offsets, want.views)
        assert pipeline.fuse(scene, results, tmp_path / "file_only.ply", average=average, voxel=0.05, options=options) == n
        assert (tmp_path / "file_only.ply").read_bytes() == (tmp_path / "m.ply").read_bytes()
        shifted = PV.merge(checker, arrays_of(whole), 0.05, origin=[0.01, 0.02, 0.03])
        assert pipeline.fuse(scene, results, tmp_path / "o.ply", average=average, voxel=0.05, voxel_origin=[0.01, 0.02, 0.03]) == shifted.count
        assert (tmp_path / "o.ply").read_bytes() == ply_bytes(shifted, False)


VOXEL = "0.25"
RUNS = {"voxel": ["--ply-voxel", VOXEL], "voxel_all": ["--ply-voxel", VOXEL, "--ply-mean", "--ply-vis", "--ply-normals"],
        "voxel_tat": ["--ply-voxel", VOXEL, "--fusion", "tat-advanced", "--ply-vis"], "plain": []}


@pytest.fixture(scope="module")
def folders(gpu_pkg, synth, tmp_path_factory):
    """One small synthetic dense folder (the size of the drop-in tests) run with the flag alone, with the mean, the lists and the
    normals, with a Tanks and Temples loop, and without the flag."""
    root = tmp_path_factory.mktemp("dense")
    a = root / "a"
    a.mkdir()
    _write_dense_folder(a, synth, 96, 72, 4)
    out = {}
    for name, extra in RUNS.items():
        shutil.copytree(a, root / name)
        _run(root / name, *extra)
        out[name] = root / name
    return out


def test_binary_writes_the_merged_points(gpu_pkg, checker, folders, tmp_path):
    """APD.ply and APD.ply.vis of the binary against the checker's merge of the points the pipeline fuses from the binary's maps."""
    for name, kw, normals in (("voxel", {}, False), ("voxel_all", dict(average=True, options=gpu_pkg.default_fusion_options(ply_normals=1)), True),
                              ("voxel_tat", dict(variant="tat_advanced"), False)):
        _, whole = _fuse_saved_maps(gpu_pkg, folders[name], None, return_points=True, **kw)
        want = PV.merge(checker, arrays_of(whole), float(VOXEL))
        assert 1 < want.count < whole.count, name
        assert (folders[name] / "APD" / "APD.ply").read_bytes() == ply_bytes(want, normals), name
        vis = folders[name] / "APD" / "APD.ply.vis"
        assert vis.exists() == ("--ply-vis" in RUNS[name])
        if vis.exists():
            assert vis.read_bytes() == VC.vis_bytes(want.offsets, want.views), name


def test_binary_without_the_flag_keeps_its_bytes(gpu_pkg, folders, tmp_path):
    plain = (folders["plain"] / "APD" / "APD.ply").read_bytes()
    assert _fuse_saved_maps(gpu_pkg, folders["plain"], tmp_path / "pipe.ply") > 0
    assert hashlib.md5(plain).hexdigest() == hashlib.md5((tmp_path / "pipe.ply").read_bytes()).hexdigest()
    assert len((folders["voxel"] / "APD" / "APD.ply").read_bytes()) < len(plain)


def test_binary_refuses_a_bad_size_before_anything_is_read(tmp_path):
    for bad in ("0", "-1", "nan", "inf", "1x", ""):
        r = subprocess.run([APD_BIN, str(tmp_path / "no_such_folder"), "0", "--ply-voxel", bad], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           timeout=60)
        assert r.returncode != 0 and "bad value '%s' of --ply-voxel" % bad in r.stdout and "USAGE" in r.stdout, (bad, r.stdout[-500:])
