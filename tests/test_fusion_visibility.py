"""The visibility of fused points without a device: the sequential checker that keeps the agreeing sources
(tests/helpers/fusion_vis_ref.cpp) is tied to the two existing checkers through the PLY bytes on every committed case, its masks
and lists agree with each other, the scan-edge cases have the point counts their names give, the .vis file round-trips, and the
C ABI declares, exports and guards the new entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import eth_fusion_checker as E
import fusion_cases
import tat_checker
import vis_checker as VC
from test_fusion_cases import VARIANTS, reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("apd_points_sources", "apd_points_visibility", "apd_points_write_vis")


@pytest.fixture(scope="module")
def vis(tmp_path_factory):
    return VC.build(tmp_path_factory.mktemp("vis_checker"))


@pytest.fixture(scope="module")
def eth(tmp_path_factory):
    return E.build(tmp_path_factory.mktemp("eth_checker"))


@pytest.fixture(scope="module")
def tat(ob, tmp_path_factory):
    return tat_checker.build(ob, tmp_path_factory.mktemp("tat_checker"))


def check_lists(res, pairs):
    """What holds for every result, of the checker or of the device: popcount(sources) == support, support + 1 entries per point,
    the own view first, then the sources behind the set bits in ascending bit order."""
    sources = np.ascontiguousarray(res.sources, "<u4")
    bits = np.unpackbits(sources.view(np.uint8).reshape(-1, 4), axis=1).sum(1).astype(np.int64)
    assert np.array_equal(bits, res.support.astype(np.int64))
    assert res.offsets[0] == 0 and np.array_equal(np.diff(res.offsets), bits + 1) and res.offsets[-1] == len(res.views)
    table = np.full((len(pairs), 32), -1, np.int32)   # table[v][j]: the j-th source of view v
    for v, p in enumerate(pairs):
        table[v, :len(p)] = p
    for k0 in range(0, len(sources), 1 << 18):
        k1 = min(len(sources), k0 + (1 << 18))
        view = np.asarray(res.view[k0:k1], np.int32)
        row = np.concatenate([view[:, None], table[view]], axis=1)   # the own view, then every source in list order
        take = np.concatenate([np.ones((k1 - k0, 1), bool), ((sources[k0:k1, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool)], axis=1)
        assert np.array_equal(res.views[res.offsets[k0]:res.offsets[k1]], row[take])


@pytest.mark.parametrize("name", fusion_cases.names())
def test_checker_writes_the_ply_of_the_existing_checkers(ob, vis, eth, tat, tmp_path, name):
    case = fusion_cases.case(name)
    for variant in VARIANTS:
        got = VC.fuse_case(vis, ob, variant, case, tmp_path / "vis.ply")
        if variant == "eth":
            want = E.fuse_case(eth, ob, case, tmp_path / "ref.ply", points=True)
            n = want.count
            for field in ("support", "view", "pixel", "normal"):
                assert getattr(got, field).tobytes() == getattr(want, field).tobytes(), field
        else:
            n = reference(ob, tat, case, variant, tmp_path / "ref.ply")
        assert got.count == n, variant
        assert (tmp_path / "vis.ply").read_bytes() == (tmp_path / "ref.ply").read_bytes(), variant
        check_lists(got, case.pairs)


@pytest.mark.parametrize("name", ["mixed_sizes", "blocks_641x409", "sources_31"])
def test_checker_with_options_and_normals(ob, vis, eth, tmp_path, name):
    """Option set "a" and the 27-byte records: the ETH checker's bytes."""
    case = fusion_cases.case(name)
    rule = E.OPTION_SETS["a"]
    want = E.fuse_case(eth, ob, case, tmp_path / "ref.ply", ply_normals=True, points=True, **rule)
    got = VC.fuse_case(vis, ob, "eth", case, tmp_path / "vis.ply", ply_normals=True, **rule)
    assert got.count == want.count > 0 and (tmp_path / "vis.ply").read_bytes() == (tmp_path / "ref.ply").read_bytes()
    assert got.support.min() >= 2
    check_lists(got, case.pairs)


def test_last_source_votes(ob, vis):
    """View 0 of the many-sources case lists 31 sources and every one of its points has the vote of the last: bit 30."""
    case = VC.last_source_case()
    assert len(case.pairs[0]) == 31
    for variant in VARIANTS:
        res = VC.fuse_case(vis, ob, variant, case)
        own = res.sources[res.view == 0]
        assert len(own) > 0 and ((own >> 30) & 1).all() and (own == (1 << 30 | 1 << 5)).all(), variant
        first = res.views[res.offsets[0]:res.offsets[1]]
        assert list(first) == [0, case.pairs[0][5], case.pairs[0][30]]


@pytest.mark.parametrize("label", sorted(VC.SCAN_EDGES))
def test_scan_edge_cases_have_the_counts_they_name(ob, vis, label):
    case, points = VC.scan_edge_case(label)
    res = VC.fuse_case(vis, ob, "eth", case)
    assert res.count == points and (res.view == 0).all()
    assert (points > VC.SCAN_SPAN) == (label == "span_plus")


def test_vis_file_round_trip(pkg, ob, vis, tmp_path):
    from apd_mvs_amd import pipeline
    case = fusion_cases.case("mixed_sizes")
    res = VC.fuse_case(vis, ob, "tat_intermediate", case, vis_path=tmp_path / "a.vis")
    raw = (tmp_path / "a.vis").read_bytes()
    assert res.count > 0 and len(raw) == 8 + 4 * (res.count + len(res.views)) and raw == VC.vis_bytes(res.offsets, res.views)
    offsets, views = pipeline.read_vis(tmp_path / "a.vis")
    assert offsets.dtype == np.int64 and views.dtype == np.int32
    assert np.array_equal(offsets, res.offsets) and np.array_equal(views, res.views)
    # no points: the count alone
    empty = VC.fuse_case(vis, ob, "eth", fusion_cases.case("all_blocked"), vis_path=tmp_path / "e.vis")
    assert empty.count == 0 and (tmp_path / "e.vis").read_bytes() == bytes(8) == VC.vis_bytes(empty.offsets, empty.views)
    offsets, views = pipeline.read_vis(tmp_path / "e.vis")
    assert list(offsets) == [0] and len(views) == 0
    for bad in (raw[:-4], raw + bytes(4), raw[:6], raw[:-3]):
        (tmp_path / "bad.vis").write_bytes(bad)
        with pytest.raises(ValueError):
            pipeline.read_vis(tmp_path / "bad.vis")


def test_header_declares_the_visibility_entry_points():
    text = open(os.path.join(ROOT, "include", "apd_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
    assert re.search(r"const\s+uint32_t\s*\*\s*apd_points_sources\s*\(\s*apd_points_t", text)
    assert re.search(r"int\s+apd_points_visibility\s*\(\s*apd_points_t\s+\w+\s*,\s*const\s+long\s+long\s*\*\*\s*\w+\s*,\s*const\s+int32_t\s*\*\*", text)
    assert re.search(r"int\s+apd_points_write_vis\s*\(\s*apd_points_t\s+\w+\s*,\s*const\s+char\s*\*", text)


def test_library_exports_and_guards_the_visibility_entry_points(pkg, tmp_path):
    """NULL is refused with APD_ERR_INVALID and a message, without a device; nothing is written."""
    L = pkg.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    L.apd_points_sources.restype = C.c_void_p
    assert L.apd_points_sources(None) is None
    offsets, views = C.c_void_p(), C.c_void_p()
    assert L.apd_points_visibility(None, C.byref(offsets), C.byref(views)) == -1
    assert L.apd_fusion_last_error().startswith(b"apd_points_visibility: ") and offsets.value is None and views.value is None
    out = tmp_path / "x.vis"
    assert L.apd_points_write_vis(None, str(out).encode()) == -1 and not out.exists()
    assert L.apd_fusion_last_error().startswith(b"apd_points_write_vis: ")
