"""Connected components within a radius and the removal of small ones without a device: the two modes of the sequential checker
(tests/helpers/points_cluster_ref.cpp) against each other and against hand-computed answers on every clause of contract C13; the
clouds the device tests run, made here; the refusals of apd_points_components and apd_points_remove_small_components, which need
no device; objects without points; the loud failure without a GPU; the choice for the device tests' real clouds, made with the
checkers alone; and the scratch size of the kernels."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fusion_cases
from common import walk_kernel_resources
import points_cluster_checker as PC
import points_radius_checker as PR
import points_voxel_checker as PV
import vis_checker as VC
from test_points_radius import (BAD, DENSE_ORIGIN, DENSE_RADIUS, UP, border_case, dense_case, determinism_case, dressed, grid_edge_case, outside_case,
                                real_cloud_radius, size_case, size_list)
from test_points_voxel import REAL_CLOUDS, cloud, from_cloud, views_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("apd_points_components", "apd_points_remove_small_components")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return PC.build(tmp_path_factory.mktemp("points_cluster_checker"))


@pytest.fixture(scope="module")
def radius_checker(tmp_path_factory):
    return PR.build(tmp_path_factory.mktemp("points_radius_checker"))


@pytest.fixture(scope="module")
def vis(tmp_path_factory):
    return VC.build(tmp_path_factory.mktemp("vis_checker"))


# --------------------------------------------------------------------------------------------------------------------
# the clouds of the device tests (test_gpu_points_clusters.py), all at radius 1 and origin 0 unless they say otherwise
# --------------------------------------------------------------------------------------------------------------------

CHAIN = 5000
STEP = 0.75


def chain_case(rng, gap=False):
    """CHAIN points on a line along x, STEP apart, in shuffled input order: one component at radius 1, a deep tree for a
    union-find whose hooks cross waves and blocks.  gap: the chain is centred on 0 and the one step from 0 upwards is the binary32
    after 1.0 -- there it is exact -- so the chain falls into the points up to 0 and the points above.  (xyz, order): order[j] is
    the position along the chain of input point j."""
    k = np.arange(CHAIN)
    if gap:
        half = CHAIN // 2
        x = np.where(k <= half, STEP * (k - half), UP + STEP * (k - half - 1))
    else:
        x = STEP * k
    order = rng.permutation(CHAIN)
    xyz = np.zeros((CHAIN, 3))
    xyz[:, 0] = x[order]
    xyz[:, 1:] = 0.5
    return xyz.astype(np.float32), order


def two_chains_case(n=2500):
    """Two chains along x, 1.5 apart in y -- in adjacent rows of cells throughout, never within the radius --, interleaved in input
    order: even indices are the first chain, odd ones the second."""
    xyz = np.zeros((2 * n, 3), np.float32)
    xyz[0::2, 0] = xyz[1::2, 0] = STEP * np.arange(n)
    xyz[0::2, 1], xyz[1::2, 1] = 0.25, 1.75
    xyz[:, 2] = 0.5
    return xyz


TEETH, TOOTH = 64, 200


def comb_case(rng, along, spine=True):
    """TEETH teeth of TOOTH points each, STEP apart along axis `along` (0 or 1), the teeth 1.5 apart on the other axis: separate
    along their length.  spine: TEETH - 1 more points between the far ends of the teeth, which join them all -- each tooth to the
    next through one point and two edges.  Along y a row of cells holds a point of every tooth, so in cell order every tooth is
    spread over all workgroups and the teeth meet in the last row; along x a tooth is a run of cell order.  Shuffled input order."""
    across = 1 - along
    pts = np.zeros((TEETH, TOOTH, 3))
    pts[:, :, along] = STEP * np.arange(TOOTH)[None, :]
    pts[:, :, across] = 1.5 * np.arange(TEETH)[:, None]
    pts = pts.reshape(-1, 3)
    if spine:
        s = np.zeros((TEETH - 1, 3))
        s[:, along] = STEP * (TOOTH - 1)
        s[:, across] = 1.5 * np.arange(TEETH - 1) + 0.75
        pts = np.concatenate([pts, s])
    pts[:, 2] = 0.5
    order = rng.permutation(len(pts))
    return pts[order].astype(np.float32), order


WIDE, WIDE_DENSITY, WIDE_MINS = 20000, 0.6, (2, 8, 64)


def wide_case():
    """WIDE uniform points at WIDE_DENSITY points per unit cell: at radius 1 that is below the percolation threshold, so the
    components run from singletons to a few hundred points."""
    side = (WIDE / WIDE_DENSITY) ** (1.0 / 3.0)
    return (np.random.default_rng(11).random((WIDE, 3)) * side).astype(np.float32)


def small_cases(pkg):
    """name -> (cloud, views, radius, origin, minima) of every synthetic device case with at most 20 001 points, with the minima
    its device test runs."""
    out = {}
    for n in size_list(pkg):
        out["n=%d" % n] = (*size_case(pkg, n), 1.0, None, (2, 4))
    out["chain"] = (*dressed(np.random.default_rng(21), chain_case(np.random.default_rng(22))[0]), 1.0, None, (2,))
    out["chain with a gap"] = (*dressed(np.random.default_rng(23), chain_case(np.random.default_rng(24), True)[0]), 1.0, None, (CHAIN // 2 + 1,))
    out["two chains"] = (*dressed(np.random.default_rng(25), two_chains_case()), 1.0, None, (2,))
    for along in (0, 1):
        for spine in (False, True):
            out["comb %d %d" % (along, spine)] = (*dressed(np.random.default_rng(26), comb_case(np.random.default_rng(27 + along), along, spine)[0]),
                                                 1.0, None, (TOOTH, TOOTH + 1))
    out["borders"] = (*dressed(np.random.default_rng(1), border_case()[0]), 1.0, None, (2, 3))
    out["grid edges"] = (*dressed(np.random.default_rng(2), grid_edge_case()[0]), 1.0, None, (2, 3))
    out["outside"] = (*dressed(np.random.default_rng(3), outside_case(np.random.default_rng(4))[0]), 1.0, None, (0, 1, 2))
    out["origin"] = (*dressed(np.random.default_rng(5), wide_case()[:3000] * 0.5), 1.0, [0.25, -0.5, 0.125], (3,))
    out["dense"] = (*dressed(np.random.default_rng(7), dense_case(np.random.default_rng(8))), DENSE_RADIUS, DENSE_ORIGIN, (2,))
    out["wide"] = (*dressed(np.random.default_rng(12), wide_case()), 1.0, None, WIDE_MINS)
    out["determinism"] = (*determinism_case(), 1.0, None, (3,))
    return out


def modes_agree(checker, c, radius, mins, origin=None, what=""):
    """The union-find over all pairs and the breadth-first search over the 27 cells on one cloud: the same labels, sizes and
    number of components, the same points kept at every minimum, with the same arrays and lists.  Returns the grid mode's
    (label, size, components)."""
    assert c.count <= 20001, what
    brute, grid = PC.components(checker, c, radius, origin, PC.BRUTE), PC.components(checker, c, radius, origin, PC.GRID)
    assert np.array_equal(brute[0], grid[0]) and np.array_equal(brute[1], grid[1]) and brute[2] == grid[2], what
    for k in mins:
        a, b = PC.remove(checker, c, radius, k, origin, PC.BRUTE), PC.remove(checker, c, radius, k, origin, PC.GRID)
        assert np.array_equal(a.index, b.index) and a.removed == b.removed, (what, k)
        PV.assert_equal(a, b, (what, k))
    return grid


def consistent(label, size, components):
    """What holds for the labels and sizes of any cloud: a label names a point that has itself as its label and is not above the
    point, the size is the number of points with that label, the components are the labels that name themselves."""
    n = len(label)
    assert (label <= np.arange(n)).all() and np.array_equal(label[label], label)
    assert np.array_equal(size, np.bincount(label, minlength=n)[label])
    assert components == int((label == np.arange(n)).sum())


def real_cloud_min_size(size):
    """The smallest min_size that removes something and not everything: one more than the size of the smallest component.  None
    when every component has the same size -- a cloud that is one component among them."""
    sizes = np.unique(size)
    return None if len(sizes) < 2 else int(sizes[0]) + 1


# --------------------------------------------------------------------------------------------------------------------
# the checker
# --------------------------------------------------------------------------------------------------------------------

def test_checker_components_on_cell_borders(checker):
    """border_case: the groups stand 10 cells apart.  Hand-computed: (0,0,0)-(1,0,0)-(0,1,0) hang together through the first;
    a pair at exactly the radius is one component, at the next binary32 two; three coincident points are one."""
    xyz, _ = border_case()
    want_size = [3, 3, 3, 2, 2, 1, 1, 2, 2, 1, 1, 2, 2, 2, 2, 1, 1, 2, 2, 3, 3, 3, 3, 3, 3]
    want_label = [0, 0, 0, 3, 3, 5, 6, 7, 7, 9, 10, 11, 11, 13, 13, 15, 16, 17, 17, 19, 19, 19, 22, 22, 22]
    for mode in (PC.BRUTE, PC.GRID):
        label, size, components = PC.components(checker, cloud(xyz), 1.0, mode=mode)
        assert label.tolist() == want_label and size.tolist() == want_size and components == 14, mode
    pair = cloud([[0.1, 0.2, 0.3], [0.4, 0.2, 0.3]])   # a radius that is no power of two, an origin
    assert PC.components(checker, pair, 0.31, origin=[0.05, 0, 0])[0].tolist() == [0, 0]
    assert PC.components(checker, pair, 0.29, origin=[0.05, 0, 0])[0].tolist() == [0, 1]


def test_checker_components_at_the_edges_of_the_grid(checker):
    """x cells 2^20 - 1 and -2^20 of adjacent rows have consecutive keys and stay in different components."""
    xyz, _ = grid_edge_case()
    for mode in (PC.BRUTE, PC.GRID):
        label, size, components = PC.components(checker, cloud(xyz), 1.0, mode=mode)
        assert label.tolist() == [0, 1, 0, 1, 1, 5, 5, 7, 7, 9, 9, 11, 11, 13, 13, 15, 15], mode
        assert size.tolist() == [2, 3, 2, 3, 3] + [2] * 12 and components == 8, mode


def test_checker_points_outside_the_grid_are_components_of_their_own(checker):
    xyz, bad = outside_case(np.random.default_rng(4))
    c = cloud(xyz)
    inside = np.setdiff1d(np.arange(c.count), bad)
    label, size, components = PC.components(checker, c, 1.0)
    consistent(label, size, components)
    assert label[bad].tolist() == bad and (size[bad] == 1).all()
    alone = PC.components(checker, cloud(xyz[inside]), 1.0)   # as if they were not there
    assert np.array_equal(size[inside], alone[1]) and np.array_equal(label[inside], inside[alone[0]]) and components == alone[2] + len(bad)
    at2, at1, at0 = (PC.remove(checker, c, 1.0, k) for k in (2, 1, 0))
    assert not np.isin(bad, at2.index).any() and 0 < at2.removed < c.count
    for kept in (at1, at0):
        assert kept.removed == 0 and np.array_equal(kept.index, np.arange(c.count))
        PV.assert_equal(PV.Cloud(*[getattr(kept, f) for f in PV.FIELDS], kept.offsets, kept.views), c)
    none = cloud(np.full((7, 3), np.nan, np.float32))
    label, size, components = PC.components(checker, none, 1.0)
    assert label.tolist() == list(range(7)) and size.tolist() == [1] * 7 and components == 7
    assert PC.remove(checker, none, 1.0, 2).count == 0 and PC.remove(checker, none, 1.0, 1).count == 7


def test_checker_labels_sizes_and_removal(checker):
    """Six points on a line at radius 1: 0.0 0.9 1.8 | 3.0 3.5 | 5.0, given in the order 5.0 1.8 3.5 0.0 3.0 0.9."""
    c = cloud([[5.0, 0, 0], [1.8, 0, 0], [3.5, 0, 0], [0.0, 0, 0], [3.0, 0, 0], [0.9, 0, 0]], view=[0, 1, 2, 1, 0, 2], sources=[1, 2, 3, 0, 1, 2],
              pairs=views_of(3, 2)[2])
    for mode in (PC.BRUTE, PC.GRID):
        label, size, components = PC.components(checker, c, 1.0, mode=mode)
        assert label.tolist() == [0, 1, 2, 1, 2, 1] and size.tolist() == [1, 3, 2, 3, 2, 3] and components == 3
        kept = PC.remove(checker, c, 1.0, 2, mode=mode)
        assert kept.index.tolist() == [1, 2, 3, 4, 5] and kept.removed == 1
        kept = PC.remove(checker, c, 1.0, 3, mode=mode)
        assert kept.index.tolist() == [1, 3, 5] and kept.removed == 3
        assert np.array_equal(kept.xyz, c.xyz[[1, 3, 5]]) and kept.sources.tolist() == [2, 0, 2] and kept.view.tolist() == [1, 1, 2]
        assert kept.offsets.tolist() == [0, 2, 3, 5]
        assert kept.views.tolist() == np.concatenate([c.views[c.offsets[i]:c.offsets[i + 1]] for i in (1, 3, 5)]).tolist()
        assert PC.remove(checker, c, 1.0, 4, mode=mode).count == 0


def test_checker_chains_and_combs(checker):
    """The hand-computed answers of the shapes the device tests run: one chain, the chain with a gap of the next binary32 after
    the radius, two chains that never touch, combs with and without their spine."""
    xyz, order = chain_case(np.random.default_rng(22))
    label, size, components = PC.components(checker, cloud(xyz), 1.0)
    assert components == 1 and (label == 0).all() and (size == CHAIN).all()
    xyz, order = chain_case(np.random.default_rng(24), True)
    label, size, components = PC.components(checker, cloud(xyz), 1.0)
    low = order <= CHAIN // 2
    assert components == 2 and (size[low] == CHAIN // 2 + 1).all() and (size[~low] == CHAIN - CHAIN // 2 - 1).all()
    assert (label[low] == np.flatnonzero(low)[0]).all() and (label[~low] == np.flatnonzero(~low)[0]).all()
    label, size, components = PC.components(checker, cloud(two_chains_case()), 1.0)
    assert components == 2 and label.tolist() == [0, 1] * 2500 and (size == 2500).all()
    for along in (0, 1):
        xyz, order = comb_case(np.random.default_rng(27 + along), along, False)
        label, size, components = PC.components(checker, cloud(xyz), 1.0)
        assert components == TEETH and (size == TOOTH).all()
        tooth = order // TOOTH
        assert label.tolist() == [int(np.flatnonzero(tooth == t)[0]) for t in tooth]
        xyz, order = comb_case(np.random.default_rng(27 + along), along, True)
        label, size, components = PC.components(checker, cloud(xyz), 1.0)
        assert components == 1 and (label == 0).all() and (size == TEETH * TOOTH + TEETH - 1).all()


def test_brute_force_and_grid_agree_on_every_small_device_case(pkg, checker):
    """The union-find over all pairs and the breadth-first search over the 27 cells give the same integers and keep the same
    points: the cell condition is part of the relation.  Every synthetic cloud of the device tests with at most 20 001 points."""
    for name, (c, _, radius, origin, mins) in small_cases(pkg).items():
        label, size, components = modes_agree(checker, c, radius, mins, origin, what=name)
        consistent(label, size, components)
        if name == "dense":
            assert components == 1 and (size == c.count).all() and (label == 0).all()
        if name == "wide":   # what the device test relies on
            print("wide: %d components, %d singletons, the largest of %d, %d of at least 64, %d points in components below 8"
                  % (components, int((size == 1).sum()), int(size.max()), int(((size >= 64) & (label == np.arange(c.count))).sum()), int((size < 8).sum())))
            assert components >= 1000
            for k in mins:
                assert 0 < PC.remove(checker, c, radius, k, origin).removed < c.count, k


# --------------------------------------------------------------------------------------------------------------------
# the C ABI without a device
# --------------------------------------------------------------------------------------------------------------------

def test_header_declares_the_entry_points_as_ctypes_calls_them(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "apd_mi355x.h")).read(), flags=re.S)
    assert re.search(r"int\s+apd_points_components\s*\(\s*apd_points_t\s+\w+\s*,\s*float\s+\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,"
                     r"\s*uint32_t\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*,\s*long\s+long\s*\*\s*\w+\s*\)", text)
    assert re.search(r"int\s+apd_points_remove_small_components\s*\(\s*apd_points_t\s+\w+\s*,\s*float\s+\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,"
                     r"\s*unsigned\s+\w+\s*,\s*apd_points_t\s*\*\s*\w+\s*,\s*long\s+long\s*\*\s*\w+\s*,\s*long\s+long\s*\*\s*\w+\s*\)", text)
    L = pkg.lib()
    fp, vpp, llp = C.POINTER(C.c_float), C.POINTER(C.c_void_p), C.POINTER(C.c_longlong)
    assert L.apd_points_components.argtypes == [C.c_void_p, C.c_float, fp, C.c_void_p, C.c_void_p, llp]
    assert L.apd_points_remove_small_components.argtypes == [C.c_void_p, C.c_float, fp, C.c_uint, vpp, llp, llp]


def test_library_exports_the_entry_points(pkg):
    for name in NEW_SYMBOLS:
        assert hasattr(pkg.lib(), name), name


def test_refusals_that_need_no_device(pkg):
    """Every bad argument answers APD_ERR_INVALID with its message and leaves the outputs as they were: no device is touched,
    so this passes on a machine without one."""
    L = pkg.lib()
    pts = from_cloud(pkg, cloud([[0.5, 0, 0], [0.6, 0, 0]]), [4], [5], [[]])
    label, size = np.full(2, 77, np.uint32), np.full(2, 78, np.uint32)
    out, removed, components = C.c_void_p(1234), C.c_longlong(-7), C.c_longlong(-8)

    def both(p, radius, origin, null_output, message):
        org = None if origin is None else (C.c_float * 3)(*origin)
        assert L.apd_points_components(p, radius, org, None if null_output else C.c_void_p(label.ctypes.data), C.c_void_p(size.ctypes.data),
                                       C.byref(components)) == -1
        assert L.apd_fusion_last_error().decode() == "apd_points_components: " + message
        assert L.apd_points_remove_small_components(p, radius, org, 2, None if null_output else C.byref(out), C.byref(removed), C.byref(components)) == -1
        assert L.apd_fusion_last_error().decode() == "apd_points_remove_small_components: " + message
        assert out.value == 1234 and removed.value == -7 and components.value == -8 and label.tolist() == [77, 77] and size.tolist() == [78, 78]

    both(None, 1.0, None, False, "null argument")
    both(pts._p, 1.0, None, True, "null argument")
    for (radius, origin), message in BAD:
        both(pts._p, radius, origin, False, message)
    with pytest.raises(pkg.ApdError, match="apd_points_components: a radius of 0"):
        pts.components(0.0)
    with pytest.raises(pkg.ApdError, match="apd_points_remove_small_components: origin component 0 is inf"):
        pts.remove_small_components(1.0, 2, origin=[float("inf"), 0, 0])
    with pytest.raises(ValueError, match="a minimum of -2 points"):   # the Python layer: a negative count does not wrap into an unsigned one
        pts.remove_small_components(1.0, -2)
    pts.close()
    with pytest.raises(pkg.ApdError, match="Points.components: the points are closed"):
        pts.components(1.0)
    with pytest.raises(pkg.ApdError, match="Points.remove_small_components: the points are closed"):
        pts.remove_small_components(1.0, 2)


def test_objects_without_points_give_empty_results_without_a_device(pkg):
    empty = cloud(np.zeros((0, 3), np.float32))
    pts = from_cloud(pkg, empty, [4], [5], [[]])
    label, size, components = pts.components(1.0)
    assert label.dtype == size.dtype == np.uint32 and label.shape == size.shape == (0,) and components == 0
    kept, removed, components = pts.remove_small_components(1.0, 2, origin=[1, 2, 3])
    assert kept.count == 0 and removed == 0 and components == 0 and not kept.merged and not kept.on_device
    assert kept.visibility()[0].tolist() == [0]
    again, removed, _ = kept.remove_small_components(0.5, 0)
    assert again.count == 0 and removed == 0
    merged, _ = pts.merge_voxels(1.0)           # a merged object without points stays merged
    kept_merged, _, _ = merged.remove_small_components(1.0, 1)
    assert kept_merged.merged and kept_merged.count == 0
    # `size`, `removed` and `components` may be NULL
    L, out, spot = pkg.lib(), C.c_void_p(), (C.c_uint32 * 1)()
    assert L.apd_points_components(pts._p, 1.0, None, C.c_void_p(C.addressof(spot)), None, None) == 0
    assert L.apd_points_remove_small_components(pts._p, 1.0, None, 1, C.byref(out), None, None) == 0
    L.apd_points_destroy(out)


def test_no_gpu_means_the_components_fail_loudly(pkg):
    """There is no host implementation: without a device a non-empty host object is refused with a message, and the outputs
    stay as they were."""
    if pkg.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = pkg.lib()
    pts = from_cloud(pkg, cloud([[0.5, 0, 0], [0.6, 0, 0]]), [4], [5], [[]])
    out, removed, components = C.c_void_p(1234), C.c_longlong(-7), C.c_longlong(-8)
    for min_size in (0, 2):
        assert L.apd_points_remove_small_components(pts._p, 1.0, None, min_size, C.byref(out), C.byref(removed), C.byref(components)) != 0
        assert L.apd_fusion_last_error().startswith(b"apd_points_remove_small_components: hipSetDevice(")
        assert out.value == 1234 and removed.value == -7 and components.value == -8
    with pytest.raises(pkg.ApdError, match=r"apd_points_components: hipSetDevice\("):
        pts.components(1.0)
    pts.close()


# --------------------------------------------------------------------------------------------------------------------
# the real clouds of the device tests
# --------------------------------------------------------------------------------------------------------------------

def test_real_cloud_choice_removes_some_points_and_not_all(ob, vis, radius_checker, checker):
    """At the radius of the radius filter's tests -- three times the median nearest-point spacing, no power of two -- the checker
    alone, on the sequential fusion's points: one more than the smallest component's size removes some points and keeps some, on
    all but at most one of the clouds (a cloud that is one component at that radius has no such size); and on the clouds with at
    most 20 001 points the brute-force mode gives what the grid mode gives."""
    single = []
    for name, variant, _ in REAL_CLOUDS:
        want = VC.fuse_case(vis, ob, variant, fusion_cases.case(name))
        c = PV.Cloud(*[getattr(want, f) for f in PV.FIELDS], want.offsets, want.views)
        radius = real_cloud_radius(radius_checker, c)
        label, size, components = PC.components(checker, c, radius)
        consistent(label, size, components)
        k = real_cloud_min_size(size)
        print(name, variant, c.count, radius, components, k)
        if k is None:
            single.append((name, variant))
            continue
        assert 0 < PC.remove(checker, c, radius, k).removed < c.count
        if c.count <= 20001:
            modes_agree(checker, c, radius, (k,), what=(name, variant))
    assert len(single) <= 1, single


# --------------------------------------------------------------------------------------------------------------------
# the kernels
# --------------------------------------------------------------------------------------------------------------------

def test_the_kernels_use_no_scratch_memory_and_no_lds(tmp_path):
    """apd_points_clusters.hip compiled for gfx950 with the library's flags: the compiler reports 0 bytes of scratch per lane, no
    spilled register and no LDS for every kernel of the file, the union-find and the per-wave combining among them."""
    found = walk_kernel_resources("k_cluster_link", tmp_path)
    for kernel in ("k_cluster_link", "k_cluster_flatten", "k_cluster_reduce", "k_cluster_emit"):
        assert len([k for k in found if kernel in k]) == 1, (kernel, sorted(found))
    for name, v in found.items():
        assert v["ScratchSize [bytes/lane]"] == "0" and v["VGPRs Spill"] == "0" and v["SGPRs Spill"] == "0" and v["LDS Size [bytes/block]"] == "0", (name, v)
