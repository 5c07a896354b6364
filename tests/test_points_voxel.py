"""The voxel-grid merge without a device: hand-computed answers for the sequential checker (tests/helpers/points_voxel_ref.cpp) on
every clause of contract C10; apd_points_create -- its refusals, and a host object that lists and writes itself with no GPU; the
refusals of apd_points_merge_voxels that need no device; the loud failure of a merge without a GPU; and the choice of the voxel
sizes of the device tests' real clouds, made with the checkers alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fusion_cases
import points_voxel_checker as PV
import vis_checker as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("apd_points_create", "apd_points_merge_voxels", "apd_points_merged")

# The real clouds of the device tests and the two voxel sizes each is merged at.  test_real_cloud_sizes_merge holds the choice to
# its purpose: at both sizes the checker finds fewer cells than points, and not one cell.
# The tiny scene is a plane 8 x 6 units wide at depth 10 with 63 points, the ring scene of mixed_sizes is about 2 units across.
REAL_CLOUDS = [("tiny_9x7", "eth", (1.0, 4.0)), ("mixed_sizes", "eth", (0.02, 0.1)), ("mixed_sizes", "tat_advanced", (0.02, 0.1))]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return PV.build(tmp_path_factory.mktemp("points_voxel_checker"))


@pytest.fixture(scope="module")
def vis(tmp_path_factory):
    return VC.build(tmp_path_factory.mktemp("vis_checker"))


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def views_of(num_views, nsrc=0, rows=4, cols=5):
    """rows, cols and ring source lists of `num_views` views of rows x cols pixels with nsrc sources each."""
    pairs = [[(v + 1 + j) % num_views for j in range(nsrc)] for v in range(num_views)]
    return [rows] * num_views, [cols] * num_views, pairs


def cloud(xyz, normal=None, bgr=None, view=None, sources=None, pairs=None, lists=None):
    """A PV.Cloud of points at `xyz`: normals +z, black, of view 0 without sources, unless given.  lists: (offsets, views) in place
    of the lists that view / sources / pairs imply."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    normal = np.tile(np.float32([0, 0, 1]), (n, 1)) if normal is None else normal
    bgr = np.zeros((n, 3), np.uint8) if bgr is None else bgr
    view = np.zeros(n, np.int32) if view is None else np.asarray(view, np.int32)
    sources = np.zeros(n, np.uint32) if sources is None else np.asarray(sources, np.uint32)
    pairs = [[]] * (int(view.max()) + 1 if n else 1) if pairs is None else pairs
    support = np.unpackbits(sources.view(np.uint8).reshape(-1, 4), axis=1).sum(1).astype(np.uint8)
    offsets, views = PV.source_lists(view, sources, pairs) if lists is None else lists
    return PV.Cloud(xyz, normal, bgr, support, view, np.arange(n, dtype=np.int32) % 20, sources, offsets, views)


def ply_bytes(c, normals):
    """ExportPointCloud's file of a cloud, packed with numpy alone."""
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n%s"
            "property uchar diffuse_blue\nproperty uchar diffuse_green\nproperty uchar diffuse_red\nend_header\n"
            % (c.count, "property float nx\nproperty float ny\nproperty float nz\n" if normals else ""))
    fields = [("xyz", "<f4", (3,))] + ([("normal", "<f4", (3,))] if normals else []) + [("bgr", "u1", (3,))]
    rec = np.zeros(c.count, np.dtype(fields))
    for name, _, _ in fields:
        rec[name] = getattr(c, name)
    return head.encode() + rec.tobytes()


def arrays_of(pts):
    """A PV.Cloud of a Points object, whichever memory it is in."""
    host = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    offsets, views = pts.visibility()
    return PV.Cloud(*[host(getattr(pts, f)) for f in PV.FIELDS], host(offsets), host(views))


def from_cloud(pkg, c, rows, cols, pairs, on_device=False):
    return pkg.Points.from_arrays(c.xyz, c.normal, c.bgr, c.support, c.view, c.pixel, c.sources, rows, cols, pairs, on_device=on_device)


# --------------------------------------------------------------------------------------------------------------------
# the checker: hand-computed answers
# --------------------------------------------------------------------------------------------------------------------

def key_of(ix, iy, iz):
    return ((iz + 2 ** 20) << 42) | ((iy + 2 ** 20) << 21) | (ix + 2 ** 20)


def test_checker_cells_of_negative_zero_and_boundary_coordinates(checker):
    """Voxel size 1, origin 0.  x = -0.5 lies in cell -1 (floor, not truncation), x = -0.0 and x = 0.25 in cell 0, x = 1.0 -- exactly
    on a boundary -- in cell 1 with x = 1.5.  The cells come out in key order -1, 0, 1; every mean is exact."""
    c = cloud([[1.5, 0, 0], [-0.5, 0, 0], [-0.0, 0, 0], [1.0, 0, 0], [0.25, 0, 0]])
    got = PV.merge(checker, c, 1.0)
    assert got.count == 3 and got.dropped == 0
    assert np.array_equal(got.xyz, np.float32([[-0.5, 0, 0], [0.125, 0, 0], [1.25, 0, 0]]))
    assert got.pixel.tolist() == [1, 2, 0]   # the representatives: the first member in input order
    # with an origin the subtraction comes first: 0.25 - 0.5 = -0.25 -> cell -1; 1.0 - 0.5 -> cell 0
    got = PV.merge(checker, cloud([[0.25, 0, 0], [1.0, 0, 0]]), 1.0, origin=[0.5, 0, 0])
    assert got.count == 2 and got.xyz[:, 0].tolist() == [0.25, 1.0]


def test_checker_key_order_is_z_major(checker):
    """One point in each of the cells (1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, -1, -1): ascending keys are z, then y, then x."""
    pts = np.float32([[1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.5, 0.5, 1.5], [-0.5, -0.5, -0.5]])
    got = PV.merge(checker, cloud(pts), 1.0)
    order = sorted(range(4), key=lambda k: key_of(*np.floor(pts[k]).astype(int).tolist()))
    assert order == [3, 0, 1, 2] and np.array_equal(got.xyz, pts[order])


def test_checker_range_edges_and_non_finite_points_are_dropped(checker):
    """f = -1048576 is kept and f = 1048576 dropped; NaN, +inf and -inf in any component are dropped; `dropped` counts them and
    the others merge as if the dropped were not there."""
    inf, nan = np.inf, np.nan
    c = cloud([[-1048576.0, 0, 0], [1048576.0, 0, 0], [1048575.5, 0, 0], [nan, 0, 0], [0, inf, 0], [0, 0, -inf], [0, -1048577.0, 0],
               [0.5, 0.5, 0.5]])
    got = PV.merge(checker, c, 1.0)
    assert got.dropped == 5 and got.count == 3
    assert got.pixel.tolist() == [0, 7, 2]
    assert np.array_equal(got.xyz[:, 0], np.float32([-1048576.0, 0.5, 1048575.5]))
    # at size 0.5 the first is at f = -2097152: dropped as well
    assert PV.merge(checker, c, 0.5).dropped == 7


def test_checker_sums_in_member_order(checker):
    """1e8 + 1 - 1e8 is 0 in binary32 and 1e8 - 1e8 + 1 is 1: the mean of a cell pins the order of its members.  The y coordinates
    carry the values (one huge cell along y), z tells the two cells apart, and a point of another cell stands between members."""
    big = 1e9
    a = [[0, 1e8, 0], [0, 0, big / 2 + 7], [0, 1.0, 0], [0, -1e8, 0]]
    b = [[0, 1e8, 0], [0, -1e8, 0], [0, 0, big / 2 + 7], [0, 1.0, 0]]
    ga, gb = PV.merge(checker, cloud(a), big, origin=[-big / 2] * 3), PV.merge(checker, cloud(b), big, origin=[-big / 2] * 3)
    assert ga.count == gb.count == 2
    assert ga.xyz[0, 1] == np.float32(0.0) / np.float32(3) and gb.xyz[0, 1] == np.float32(1.0) / np.float32(3)
    assert bits(ga.xyz[0, 1]) != bits(gb.xyz[0, 1])


def test_checker_normals_are_renormalised_and_zero_when_they_cancel(checker):
    n = np.float32([[0, 0, 2], [0, 2, 0], [1, 0, 0], [-1, 0, 0], [np.nan, 0, 0]])
    c = cloud([[0.5, 0, 0], [0.5, 0, 0], [1.5, 0, 0], [1.5, 0, 0], [2.5, 0, 0]], normal=n)
    got = PV.merge(checker, c, 1.0)
    r = np.float32(1) / np.sqrt(np.float32(2))   # (0, 1, 1): sum / 2, length sqrt(2)
    assert np.array_equal(bits(got.normal[0]), bits([0, r, r]))
    assert np.array_equal(got.normal[1:], np.zeros((2, 3), np.float32))   # length 0, and NaN


def test_checker_colour_rounds_half_up(checker):
    """(sum + m / 2) / m: 1 + 2 over 2 -> (3 + 1) / 2 = 2 (the tie goes up); 1 + 1 + 2 over 3 -> (4 + 1) / 3 = 1; 255 alone -> 255."""
    bgr = np.uint8([[1, 0, 255], [2, 1, 255], [1, 1, 255], [1, 1, 255], [2, 2, 255]])
    got = PV.merge(checker, cloud([[0.5, 0, 0], [0.5, 0, 0], [1.5, 0, 0], [1.5, 0, 0], [1.5, 0, 0]], bgr=bgr), 1.0)
    assert got.bgr.tolist() == [[2, 1, 255], [1, 1, 255]]


def test_checker_lists_are_the_sorted_union_and_support_their_length(checker):
    """Three members with lists {2, 0, 1}, {1, 3} and {2}: the cell lists 0 1 2 3 and has support 3.  view, pixel and sources are
    the first member's.  A lone point keeps its list, sorted."""
    rows, cols, pairs = views_of(4, nsrc=3)   # view 2 lists 3, 0, 1; view 1 lists 2, 3, 0
    c = cloud([[0.5, 0, 0], [0.5, 0, 0], [0.5, 0, 0], [1.5, 0, 0]], view=[2, 1, 2, 1], sources=[0b110, 0b010, 0, 0b101], pairs=pairs)
    assert c.views.tolist() == [2, 0, 1, 1, 3, 2, 1, 2, 0]
    got = PV.merge(checker, c, 1.0)
    assert got.offsets.tolist() == [0, 4, 7] and got.views.tolist() == [0, 1, 2, 3, 0, 1, 2]
    assert got.support.tolist() == [3, 2] and got.view.tolist() == [2, 1] and got.sources.tolist() == [0b110, 0b101]
    # merged again on a grid twice as coarse, from the lists (the sources bits would give {2, 0, 1} and {1, 2, 0} only)
    again = PV.merge(checker, got, 2.0)
    assert again.count == 1 and again.views.tolist() == [0, 1, 2, 3] and again.support.tolist() == [3]


# --------------------------------------------------------------------------------------------------------------------
# the C ABI without a device
# --------------------------------------------------------------------------------------------------------------------

def test_header_declares_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "apd_mi355x.h")).read(), flags=re.S)
    assert re.search(r"int\s+apd_points_create\s*\(\s*int\s+device\s*,\s*int\s+on_device\s*,\s*long\s+long\s+count\s*,", text)
    assert re.search(r"int\s+apd_points_merge_voxels\s*\(\s*apd_points_t\s+\w+\s*,\s*float\s+\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,"
                     r"\s*apd_points_t\s*\*\s*\w+\s*,\s*long\s+long\s*\*\s*\w+\s*\)", text)
    assert re.search(r"int\s+apd_points_merged\s*\(\s*apd_points_t\s+\w+\s*\)", text)


def test_library_exports_the_entry_points(pkg):
    L = pkg.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    assert L.apd_points_merged(None) == 0


class CreateArgs:
    """The arguments of a valid apd_points_create of four points over three views of 4 x 5 pixels with two sources each."""

    def __init__(self):
        self.count = 4
        self.xyz = np.arange(12, dtype=np.float32)
        self.normal = np.ones(12, np.float32)
        self.bgr = np.arange(12, dtype=np.uint8)
        self.sources = np.uint32([0b11, 0b01, 0, 0b10])
        self.support = np.uint8([2, 1, 0, 1])
        self.view = np.int32([0, 1, 2, 2])
        self.pixel = np.int32([0, 19, 7, 3])
        self.num_views = 3
        self.rows, self.cols = np.int32([4, 4, 4]), np.int32([5, 5, 5])
        self.pair_offsets, self.pair_indices = np.int32([0, 2, 4, 6]), np.int32([1, 2, 2, 0, 0, 1])

    def call(self, L, out, on_device=0, null=()):
        p = lambda name: None if name in null else C.c_void_p(getattr(self, name).ctypes.data)
        ip = lambda name: None if name in null else getattr(self, name).ctypes.data_as(C.POINTER(C.c_int))
        return L.apd_points_create(0, on_device, self.count, p("xyz"), p("normal"), p("bgr"), p("support"), p("view"), p("pixel"), p("sources"),
                                   self.num_views, ip("rows"), ip("cols"), ip("pair_offsets"), ip("pair_indices"), None if "out" in null else C.byref(out))


def _set(name, value, index=None):
    def change(a):
        if index is None:
            setattr(a, name, value)
        else:
            getattr(a, name)[index] = value
    return change


REFUSALS = [
    ("negative count", _set("count", -1), "a count of -1 points"),
    ("no views", _set("num_views", 0), "0 views"),
    ("zero rows", _set("rows", 0, 1), "view 1 has 5 x 0 pixels"),
    ("negative cols", _set("cols", -5, 2), "view 2 has -5 x 4 pixels"),
    ("offsets not from 0", _set("pair_offsets", 1, 0), "pair_offsets starts at 1, not at 0"),
    ("offsets descend", _set("pair_offsets", 1, 2), "pair_offsets descends at view 1"),
    ("index too large", _set("pair_indices", 3, 4), "source 0 of view 2 is view 3 of 3"),
    ("index negative", _set("pair_indices", -1, 0), "source 0 of view 0 is view -1 of 3"),
    ("own source", _set("pair_indices", 1, 2), "view 1 is its own source"),
    ("view outside", _set("view", 3, 1), "point 1 is of view 3 of 3"),
    ("view negative", _set("view", -1, 0), "point 0 is of view -1 of 3"),
    ("pixel outside", _set("pixel", 20, 2), "point 2 is pixel 20 of view 2, which has 20"),
    ("pixel negative", _set("pixel", -1, 3), "point 3 is pixel -1 of view 2, which has 20"),
    ("bit above the list", _set("sources", 0b100, 2), "point 2 names sources 0x4, its view 2 has 2"),
    ("support", _set("support", 2, 1), "point 1 names 1 sources and has a support of 2"),
]


@pytest.mark.parametrize("what,change,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_create_refuses(pkg, what, change, message):
    L = pkg.lib()
    a, out = CreateArgs(), C.c_void_p(1234)
    change(a)
    assert a.call(L, out) == -1, what
    assert L.apd_fusion_last_error().decode() == "apd_points_create: " + message
    assert out.value == 1234


def test_create_refuses_null_arguments_and_long_source_lists(pkg):
    L = pkg.lib()
    for name in ("xyz", "normal", "bgr", "support", "view", "pixel", "sources", "rows", "cols", "pair_offsets", "pair_indices", "out"):
        out = C.c_void_p(1234)
        assert CreateArgs().call(L, out, null=(name,)) == -1, name
        assert L.apd_fusion_last_error() == b"apd_points_create: null argument" and out.value == 1234
    # 33 sources: 34 views, view 0 lists all the others
    a, out = CreateArgs(), C.c_void_p(1234)
    a.num_views = 34
    a.rows, a.cols = np.full(34, 4, np.int32), np.full(34, 5, np.int32)
    a.pair_offsets, a.pair_indices = np.int32([0] + [33] * 34), np.arange(1, 34, dtype=np.int32)
    a.sources[:], a.support[:] = 0, 0
    assert a.call(L, out) == -1 and out.value == 1234
    assert L.apd_fusion_last_error() == b"apd_points_create: view 0 has 33 sources, more than 32"
    a.pair_offsets, a.pair_indices = np.int32([0] + [32] * 34), np.arange(1, 33, dtype=np.int32)   # 32 are allowed
    assert a.call(L, out) == 0 and L.apd_points_count(out) == 4
    L.apd_points_destroy(out)


def test_create_without_points_may_pass_null_arrays(pkg):
    L = pkg.lib()
    a, out = CreateArgs(), C.c_void_p()
    a.count = 0
    assert a.call(L, out, null=("xyz", "normal", "bgr", "support", "view", "pixel", "sources")) == 0
    assert L.apd_points_count(out) == 0 and L.apd_points_merged(out) == 0
    merged, dropped = C.c_void_p(), C.c_longlong(-1)
    assert L.apd_points_merge_voxels(out, 1.0, None, C.byref(merged), C.byref(dropped)) == 0   # no points: no device touched
    assert L.apd_points_count(merged) == 0 and dropped.value == 0 and L.apd_points_merged(merged) == 1
    L.apd_points_destroy(merged)
    L.apd_points_destroy(out)


def test_created_host_object_returns_lists_and_writes_itself(pkg, ob, vis, tmp_path):
    """The sequential fusion's points of a case, handed to Points.from_arrays as host memory: the accessors return the arrays, the
    lists are the fusion checker's, and the PLY (both record forms) and the .vis file have the bytes numpy packs.  No device."""
    case = fusion_cases.case("mixed_sizes")
    want = VC.fuse_case(vis, ob, "eth", case)
    assert want.count > 1000
    rows, cols = [d.shape[0] for d in case.depths], [d.shape[1] for d in case.depths]
    pts = pkg.Points.from_arrays(want.xyz, want.normal, want.bgr, want.support, want.view, want.pixel, want.sources, rows, cols, case.pairs)
    assert not pts.on_device and not pts.merged and pts.count == want.count
    got = arrays_of(pts)
    PV.assert_equal(got, PV.Cloud(*[getattr(want, f) for f in PV.FIELDS], want.offsets, want.views))
    for normals in (False, True):
        path = tmp_path / ("n%d.ply" % normals)
        pts.write_ply(path, normals=normals)
        assert path.read_bytes() == ply_bytes(got, normals)
    pts.write_vis(tmp_path / "a.vis")
    assert (tmp_path / "a.vis").read_bytes() == VC.vis_bytes(want.offsets, want.views)
    pts.close()


@pytest.mark.parametrize("count", [0, 1, 257])
def test_created_host_object_of_a_few_points_keeps_every_byte(pkg, tmp_path, count):
    """apd_points_create of host-resident points over 3 views of 4 x 5 pixels with 2 sources each, with no point, one point and
    one more than a block of 256: every accessor returns the bytes given, apd_points_write_ply (both record forms) writes the
    bytes packed here, apd_points_visibility and apd_points_write_vis give the lists that view / sources / pairs imply, and
    apd_points_destroy returns APD_OK.  No device."""
    rng = np.random.RandomState(7 + count)
    rows, cols, pairs = views_of(3, nsrc=2)
    sources = rng.randint(0, 4, count).astype(np.uint32)
    want = cloud(rng.standard_normal((count, 3)).astype(np.float32), normal=rng.standard_normal((count, 3)).astype(np.float32),
                 bgr=rng.randint(0, 256, (count, 3)).astype(np.uint8), view=rng.randint(0, 3, count), sources=sources, pairs=pairs)
    assert want.count == count and len(want.offsets) == count + 1 and want.offsets[-1] == count + int(want.support.sum())
    pts = from_cloud(pkg, want, rows, cols, pairs)
    assert not pts.on_device and not pts.merged and pts.count == count == len(pts)
    for f in PV.FIELDS:
        got = np.asarray(getattr(pts, f))
        assert got.dtype == getattr(want, f).dtype and got.tobytes() == getattr(want, f).tobytes(), f
    offsets, views = pts.visibility()
    assert offsets.dtype == np.int64 and offsets.tobytes() == np.asarray(want.offsets, np.int64).tobytes()
    assert views.dtype == np.int32 and views.tobytes() == np.asarray(want.views, np.int32).tobytes()
    for normals in (False, True):
        path = tmp_path / ("n%d.ply" % normals)
        pts.write_ply(path, normals=normals)
        assert path.read_bytes() == ply_bytes(want, normals)
    pts.write_vis(tmp_path / "a.vis")
    assert (tmp_path / "a.vis").read_bytes() == VC.vis_bytes(want.offsets, want.views)
    handle, pts._p = pts._p, None
    del offsets, views, got
    assert pkg.lib().apd_points_destroy(handle) == 0


def test_merge_refusals_that_need_no_device(pkg):
    L = pkg.lib()
    c = cloud([[0.5, 0, 0], [0.6, 0, 0]])
    pts = from_cloud(pkg, c, [4], [5], [[]])
    out, dropped = C.c_void_p(1234), C.c_longlong(-7)

    def refused(p, size, origin, outp, code, message):
        org = None if origin is None else (C.c_float * 3)(*origin)
        assert L.apd_points_merge_voxels(p, size, org, outp, C.byref(dropped)) == code
        assert L.apd_fusion_last_error().decode() == "apd_points_merge_voxels: " + message
        assert out.value == 1234 and dropped.value == -7

    refused(None, 1.0, None, C.byref(out), -1, "null argument")
    refused(pts._p, 1.0, None, None, -1, "null argument")
    refused(pts._p, 0.0, None, C.byref(out), -1, "a voxel size of 0, not a positive finite number")
    refused(pts._p, -1.0, None, C.byref(out), -1, "a voxel size of -1, not a positive finite number")
    refused(pts._p, float("inf"), None, C.byref(out), -1, "a voxel size of inf, not a positive finite number")
    refused(pts._p, float("nan"), None, C.byref(out), -1, "a voxel size of nan, not a positive finite number")
    refused(pts._p, 1.0, [0.0, float("nan"), 0.0], C.byref(out), -1, "origin component 1 is nan")
    refused(pts._p, 1.0, [0.0, 0.0, float("-inf")], C.byref(out), -1, "origin component 2 is -inf")
    with pytest.raises(pkg.ApdError, match="apd_points_merge_voxels: a voxel size of 0"):
        pts.merge_voxels(0.0)
    pts.close()


def test_no_gpu_means_the_merge_fails_loudly(pkg):
    """There is no host implementation of the merge: without a device a non-empty host object is refused with a message, and *out
    and *dropped stay as they were."""
    if pkg.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = pkg.lib()
    pts = from_cloud(pkg, cloud([[0.5, 0, 0], [0.6, 0, 0]]), [4], [5], [[]])
    out, dropped = C.c_void_p(1234), C.c_longlong(-7)
    assert L.apd_points_merge_voxels(pts._p, 1.0, None, C.byref(out), C.byref(dropped)) != 0
    assert L.apd_fusion_last_error().startswith(b"apd_points_merge_voxels: ")
    assert out.value == 1234 and dropped.value == -7
    with pytest.raises(pkg.ApdError):
        pts.merge_voxels(1.0)
    pts.close()


# --------------------------------------------------------------------------------------------------------------------
# the real clouds of the device tests
# --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,variant,sizes", REAL_CLOUDS)
def test_real_cloud_sizes_merge(ob, vis, checker, name, variant, sizes):
    """At its two sizes the checker alone, on the sequential fusion's points, finds fewer cells than points and more than one."""
    want = VC.fuse_case(vis, ob, variant, fusion_cases.case(name))
    c = PV.Cloud(*[getattr(want, f) for f in PV.FIELDS], want.offsets, want.views)
    cells = [PV.merge(checker, c, size).count for size in sizes]
    print(name, variant, c.count, cells)
    assert all(1 < n < c.count for n in cells) and cells[1] < cells[0]
