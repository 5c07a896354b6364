"""The mean geometry of fused points without a device: the C ABI declares, exports and guards apd_points_average and
apd_points_write_ply; the sequential checker (tests/helpers/points_average_ref.cpp) agrees with a float64 restatement of its sums
to the rounding of binary32 and has the properties a mean has; the product's own arithmetic (apd_fusion::mean_point of
apd_fusion_math.h, compiled by the host compiler) gives the checker's bits on the cases the device tests use; and the case of the
device tests' skip path is chosen here, with the checkers alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import filter_checker as F
import fusion_cases
import points_average_checker as PA
import vis_checker as VC
from test_fusion_cases import VARIANTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("apd_points_average", "apd_points_write_ply")

# The skip path of the device tests: ETH points of this case averaged over the depth maps of the geometric filter with this rule
# in place of the fused ones.  A filtered map is 0 where the filter rejects the pixel, so a source whose pixel was rejected is
# skipped.  test_skip_case_skips_some_sources_and_not_all holds the choice to what its name says.
SKIP_CASE, SKIP_RULE = "mixed_sizes", dict(min_consistent=2)


@pytest.fixture(scope="module")
def vis(tmp_path_factory):
    return VC.build(tmp_path_factory.mktemp("vis_checker"))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return PA.build(tmp_path_factory.mktemp("points_average_checker"))


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    return PA.build_header(tmp_path_factory.mktemp("points_average_header"))


@pytest.fixture(scope="module")
def filter_lib(tmp_path_factory):
    return F.build(tmp_path_factory.mktemp("filter_checker"))


def popcount(a):
    return np.unpackbits(np.ascontiguousarray(a, "<u4").view(np.uint8).reshape(-1, 4), axis=1).sum(1).astype(np.int64)


def filtered_depths(filter_lib, ob, case, **rule):
    """depth_out of the geometric filter's checker for every view of the case."""
    return [depth for depth, _, _ in F.filter_case(filter_lib, ob, case, **rule)]


# --------------------------------------------------------------------------------------------------------------------
# the C ABI
# --------------------------------------------------------------------------------------------------------------------

def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "apd_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int\s+apd_points_average\s*\(\s*apd_points_t\s+\w+\s*,\s*int\s+\w+\s*,\s*const\s+apd_camera\s*\*\s*\w+\s*,"
                     r"\s*const\s+float\s*\*\s*const\s*\*\s*\w+\s*,\s*const\s+float\s*\*\s*const\s*\*\s*\w+\s*,\s*const\s+int\s*\*\s*\w+\s*,"
                     r"\s*const\s+int\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*apd_points_t\s*\*\s*\w+\s*\)", text)
    assert re.search(r"int\s+apd_points_write_ply\s*\(\s*apd_points_t\s+\w+\s*,\s*const\s+char\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)", text)


def test_library_exports_and_guards_the_entry_points(pkg, tmp_path):
    """Every refusal that can be asked for without a points object, i.e. without a fusion: NULL arguments.  They answer
    APD_ERR_INVALID with their message, *out stays as it was and no file appears.  (The refusals that need an object -- another
    view count, another size, a source without a map, a path that cannot be written -- are in test_gpu_points_average.py.)"""
    L = pkg.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    out = C.c_void_p(1234)
    one = (C.c_int * 1)(4)
    maps = (C.c_void_p * 1)()
    cams = (pkg.Camera * 1)()
    assert L.apd_points_average(None, 1, C.byref(cams), maps, maps, one, one, 0, C.byref(out)) == -1
    assert L.apd_fusion_last_error() == b"apd_points_average: null argument" and out.value == 1234
    path = tmp_path / "x.ply"
    for with_normals in (0, 1):
        assert L.apd_points_write_ply(None, str(path).encode(), with_normals) == -1 and not path.exists()
        assert L.apd_fusion_last_error() == b"apd_points_write_ply: null argument"


# --------------------------------------------------------------------------------------------------------------------
# the checker against float64
# --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", ["mixed_sizes", "source_lists", "blocks_641x409"])
def test_checker_against_a_float64_restatement(ob, vis, checker, name, variant):
    """Ring scenes, the fusion checker's points, the fused maps themselves.  The checker reports the lifted point of every
    source that contributed; numpy adds them to the stored point in float64 and divides.  The two means differ by the binary32
    rounding of the sums alone: at most (used + 1) * 2^-23 * max |coordinate| over the point's contributions -- (used + 1) *
    2^-24 * max for `used` rounded additions and one rounded division of terms no larger than max, doubled for the terms of
    second order -- a bound computed per point from the data, not chosen.  The normals' sums are restated the same way (their
    terms are at most 1).  Largest deviation seen over the nine runs: 0.3332 of the bound for positions (3.3e-7 absolute), 0.066
    of theirs for the unit normals.  Every mean lies in the box of its contributions, used == popcount(kept), and with the
    fused maps nothing is skipped."""
    case = fusion_cases.case(name)
    points = VC.fuse_case(vis, ob, variant, case)
    assert points.count > 0
    got = PA.average_case(checker, ob, case, points, contributions=True)
    used = got.support.astype(np.int64)
    assert np.array_equal(used, popcount(got.sources))
    if variant == "eth":   # a T&T point may carry a source of an earlier pixel, which its own projection need not reach
        assert np.array_equal(got.sources, points.sources) and np.array_equal(got.support, points.support)
    assert (got.sources & ~points.sources).max() == 0
    for f in ("bgr", "view", "pixel"):
        assert np.array_equal(getattr(got, f), getattr(points, f)), f
    took = ((got.sources[:, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool)       # [N, 32]
    terms = np.concatenate([points.xyz[:, None, :], got.contributions], axis=1).astype(np.float64)   # [N, 33, 3]
    took = np.concatenate([np.ones((len(took), 1), bool), took], axis=1)
    assert (got.contributions[~took[:, 1:]] == 0).all()
    mean = (terms * took[..., None]).sum(1) / (used + 1)[:, None]
    lo = np.where(took[..., None], terms, np.inf).min(1)
    hi = np.where(took[..., None], terms, -np.inf).max(1)
    assert (got.xyz >= lo).all() and (got.xyz <= hi).all()
    largest = np.abs(np.where(took[..., None], terms, 0.0)).max((1, 2))
    bound = (used + 1) * 2.0 ** -23 * largest
    deviation = np.abs(got.xyz.astype(np.float64) - mean).max(1)
    print(name, variant, "points", points.count, "deviation / bound", (deviation / bound).max(), "absolute", deviation.max())
    assert (deviation <= bound).all()
    # the normals: the unit vector of the float64 mean of the same sources' normals.  Per component the float32 mean is off by at
    # most (used + 1) * 2^-23 as above (terms of at most 1); the squares, their sum, the root and the division add fewer than
    # 8 roundings of 2^-24 relative to a unit vector; a vector off by e in every component turns by at most sqrt(3) e / length.
    nterms = np.concatenate([points.normal[:, None, :], got.normal_contributions], axis=1).astype(np.float64)
    nmean = (nterms * took[..., None]).sum(1) / (used + 1)[:, None]
    length = np.linalg.norm(nmean, axis=1)
    assert (length > 0.9).all()   # the scenes' normals agree to a few degrees
    nbound = 2 * np.sqrt(3.0) * (used + 1) * 2.0 ** -23 / length + 8 * 2.0 ** -24
    ndev = np.abs(got.normal.astype(np.float64) - nmean / length[:, None]).max(1)
    print(name, variant, "normal deviation / bound", (ndev / nbound).max())
    assert (ndev <= nbound).all()


# --------------------------------------------------------------------------------------------------------------------
# the product's arithmetic on the host compiler
# --------------------------------------------------------------------------------------------------------------------

HEADER_CASES = ["tiny_1x1", "tiny_9x7", "tiny_16x16", "mixed_sizes", "sources_31", "sources_32", "source_lists", "non_finite", "all_blocked"]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", HEADER_CASES)
def test_header_function_gives_the_checkers_bits(ob, vis, checker, header, name, variant):
    """apd_fusion::mean_point, as g++ compiles it under -ffp-contract=off, against the checker's own loop, bit for bit.  One
    exception, read off the data: a Tanks and Temples point of the non-finite case may name a source through an entry of an
    earlier pixel, and the pixel its own projection reaches there may hold a NaN or infinite depth, which the rule does not skip.
    Its mean position is then NaN, and IEEE 754 leaves the sign and payload of a NaN that two NaN operands produce to the
    implementation (x86 returns its first operand, so the bits depend on how the compiler orders a commutative add; a device
    generates its own default NaN).  Those components are compared as NaN == NaN; an ETH point never has one, because a vote
    needs a finite source depth."""
    case = fusion_cases.case(name)
    points = VC.fuse_case(vis, ob, variant, case)
    assert (points.count == 0) == (name == "all_blocked")
    want = PA.average_case(checker, ob, case, points)
    got = PA.average_case(header, ob, case, points, header=True)
    nan = np.isnan(want.xyz)
    assert not nan.any() or (name == "non_finite" and variant != "eth")
    assert not np.isnan(want.normal).any()   # a NaN length gives (0, 0, 0)
    assert np.array_equal(np.isnan(got.xyz), nan)
    got.xyz[nan] = want.xyz[nan]
    for f in PA.FIELDS:
        assert getattr(got, f).tobytes() == getattr(want, f).tobytes(), f


def test_high_mask_bits_contribute(ob, vis, checker):
    """sources_32: view 0 lists 32 sources and its points are accepted with those at positions 5 and 31; both contribute."""
    case = fusion_cases.case("sources_32")
    assert len(case.pairs[0]) == 32
    points = VC.fuse_case(vis, ob, "eth", case)
    got = PA.average_case(checker, ob, case, points)
    own = got.sources[got.view == 0]
    assert len(own) > 0 and (own == np.uint32(1 << 31 | 1 << 5)).all() and (got.support[got.view == 0] == 2).all()


def test_skip_case_skips_some_sources_and_not_all(ob, vis, checker, header, filter_lib):
    """The reference computation alone: ETH points of SKIP_CASE over the filter checker's depth maps lose some of their sources and
    keep others, some points lose all of theirs and stay where they were, bit for bit, and the header function agrees."""
    case = fusion_cases.case(SKIP_CASE)
    points = VC.fuse_case(vis, ob, "eth", case)
    depths = filtered_depths(filter_lib, ob, case, **SKIP_RULE)
    got = PA.average_case(checker, ob, case, points, depths=depths)
    before, after = int(popcount(points.sources).sum()), int(popcount(got.sources).sum())
    print("sources before", before, "after", after, "points", points.count, "without any", int((got.support == 0).sum()))
    assert 0 < after < before and (got.sources & ~points.sources).max() == 0
    assert np.array_equal(got.support.astype(np.int64), popcount(got.sources))
    alone = got.support == 0
    assert alone.any() and not alone.all()
    assert got.xyz[alone].tobytes() == points.xyz[alone].tobytes()   # P / 1.0f
    same = PA.average_case(header, ob, case, points, depths=depths, header=True)
    for f in PA.FIELDS:
        assert getattr(same, f).tobytes() == getattr(got, f).tobytes(), f
