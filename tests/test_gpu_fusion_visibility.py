"""The agreeing sources of every fused point and the visibility lists on the device (apd_points_sources, apd_points_visibility,
apd_points_write_vis; csrc/apd_points_vis.hip, csrc/apd_points.hip), bitwise against the sequential checker that keeps them
(tests/helpers/fusion_vis_ref.cpp): host- and device-resident points, all three loops and option set "a", the edges of the
64-bit scan behind the offsets, a view without points between two with points, a vote from source 30, the Python layer and the
drop-in binary's --ply-vis."""
import os
import shutil

import numpy as np
import pytest

import eth_fusion_checker as E
import fusion_cases
import vis_checker as VC
from test_fusion_cases import VARIANTS
from test_fusion_visibility import check_lists
from test_gpu_dropin_binary import _write_dense_folder
from test_gpu_fusion_options import _fuse, _fuse_saved_maps, _run, _scene

pytestmark = pytest.mark.gpu

RUNS = {"eth": ("eth", {}), "tat_intermediate": ("tat_intermediate", {}), "tat_advanced": ("tat_advanced", {}),
        "eth_a": ("eth", E.OPTION_SETS["a"])}
FIELDS = ("xyz", "normal", "bgr", "support", "view", "pixel")


@pytest.fixture(scope="module")
def vis(tmp_path_factory):
    return VC.build(tmp_path_factory.mktemp("vis_checker"))


class Lists:
    """The arrays of a Points object as numpy, whichever memory they are in."""

    def __init__(self, pts):
        host = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
        for f in FIELDS:
            setattr(self, f, host(getattr(pts, f)))
        self.sources = host(pts.sources).view(np.uint32)
        self.offsets, self.views = [host(a) for a in pts.visibility()]
        assert self.offsets.dtype == np.int64 and self.views.dtype == np.int32 and self.sources.dtype == np.uint32


def both(pkg, ob, vis, case, run, tmp_path):
    """The checker's result, and the device fusion's with host-resident and with device-resident points, compared bitwise: the
    arrays there were, sources, offsets, views, and the .vis bytes."""
    variant, rule = RUNS[run]
    want = VC.fuse_case(vis, ob, variant, case, vis_path=tmp_path / "ref.vis", **rule)
    ref_vis = (tmp_path / "ref.vis").read_bytes()
    options = dict(variant=VARIANTS.index(variant), **rule)
    out = []
    for on_device in (False, True):
        n, pts = _fuse(pkg, ob, case, pkg.default_fusion_options(result_on_device=int(on_device), **options), None, points=True,
                       on_device=on_device)
        assert n == want.count == pts.count and pts.on_device == on_device
        if on_device:
            assert pts.sources.is_cuda and all(a.is_cuda for a in pts.visibility())
        got = Lists(pts)
        for f in FIELDS + ("sources", "offsets", "views"):
            assert getattr(got, f).tobytes() == getattr(want, f).tobytes(), (f, on_device)
        assert pts.visibility()[0] is pts.visibility()[0]   # built once, kept
        path = tmp_path / ("dev.vis" if on_device else "host.vis")
        pts.write_vis(path)
        assert path.read_bytes() == ref_vis, on_device
        check_lists(got, case.pairs)
        out.append(got)
    return want, out


@pytest.mark.parametrize("run", sorted(RUNS))
@pytest.mark.parametrize("name", ["tiny_9x7", "mixed_sizes", "blocks_641x409", "all_blocked", "sources_31", "rolled_aniso", "source_behind"])
def test_sources_and_lists_equal_the_checker(gpu_pkg, ob, vis, tmp_path, name, run):
    """Fewer pixels than a wave; views of two sizes; 1024 * 256 + 25 pixels; no point at all (offsets == [0], a .vis file of eight
    zero bytes); 31 sources."""
    want, _ = both(gpu_pkg, ob, vis, fusion_cases.case(name), run, tmp_path)
    assert (want.count == 0) == (name == "all_blocked")
    if want.count == 0:
        assert list(want.offsets) == [0] and (tmp_path / "dev.vis").read_bytes() == bytes(8)


@pytest.mark.parametrize("run", sorted(RUNS))
def test_a_vote_from_the_last_of_31_sources(gpu_pkg, ob, vis, tmp_path, run):
    """View 0 of the many-sources case lists 31 sources; its points are accepted with the sources at positions 5 and 30."""
    case = VC.last_source_case()
    assert len(case.pairs[0]) == 31
    _, (host, dev) = both(gpu_pkg, ob, vis, case, run, tmp_path)
    for got in (host, dev):
        own = got.sources[got.view == 0]
        assert len(own) > 0 and (own == np.uint32(1 << 30 | 1 << 5)).all()
        assert list(got.views[:3]) == [0, case.pairs[0][5], case.pairs[0][30]]


@pytest.mark.parametrize("run", sorted(RUNS))
def test_lists_continue_across_a_view_without_points(gpu_pkg, ob, vis, tmp_path, run):
    """mixed_sizes with its second view blocked entirely: the views after it append at the running offset."""
    case = VC.first_pixels(fusion_cases.case("mixed_sizes"), "empty_between", [None, 0, None, None, None])
    want, (host, dev) = both(gpu_pkg, ob, vis, case, run, tmp_path)
    per_view = np.bincount(want.view, minlength=5)
    assert per_view[1] == 0 and (per_view[[0, 2, 3, 4]] > 0).all()
    first = int(np.searchsorted(dev.view, 2))
    assert dev.views[dev.offsets[first]] == 2 and dev.views[dev.offsets[first - 1]] == 0 and dev.offsets[first] > 0


@pytest.mark.parametrize("label", sorted(VC.SCAN_EDGES))
def test_scan_edges(gpu_pkg, ob, vis, tmp_path, label):
    """The offsets are a 64-bit scan over all points: per 256 points a block sum, then one workgroup of 1024 lanes over the block
    sums.  Point counts below a wave, on both sides of 64 and of 256, and on both sides of SCAN_SPAN = 1024 * 256 = 262144 points,
    the most for which every lane of that workgroup has at most one block sum (0 points: all_blocked above)."""
    case, points = VC.scan_edge_case(label)
    want, (host, dev) = both(gpu_pkg, ob, vis, case, "eth", tmp_path)
    assert want.count == points == len(dev.offsets) - 1
    assert (points > VC.SCAN_SPAN) == (label == "span_plus") and VC.SCAN_SPAN == 262144


def test_through_the_pipeline(gpu_pkg, ob, vis, tmp_path):
    """pipeline.fuse(vis_path=...): with the points (host and device) and as the only output."""
    from apd_mvs_amd import pipeline
    case = fusion_cases.case("mixed_sizes")
    want = VC.fuse_case(vis, ob, "eth", case, tmp_path / "ref.ply", vis_path=tmp_path / "ref.vis")
    scene, results = _scene(gpu_pkg, pipeline, case)
    n, pts = pipeline.fuse(scene, results, tmp_path / "a.ply", return_points=True, vis_path=tmp_path / "a.vis")
    assert n == want.count and isinstance(pts.sources, np.ndarray) and pts.sources.dtype == np.uint32
    assert np.array_equal(pts.sources, want.sources)
    offsets, views = pts.visibility()
    assert np.array_equal(offsets, want.offsets) and np.array_equal(views, want.views)
    assert (tmp_path / "a.ply").read_bytes() == (tmp_path / "ref.ply").read_bytes()
    assert (tmp_path / "a.vis").read_bytes() == (tmp_path / "ref.vis").read_bytes()
    got = pipeline.read_vis(tmp_path / "a.vis")
    assert np.array_equal(got[0], want.offsets) and np.array_equal(got[1], want.views)
    n, dev = pipeline.fuse(scene, results, None, return_points=True, options=gpu_pkg.default_fusion_options(result_on_device=1),
                           vis_path=tmp_path / "b.vis")
    assert n == want.count and dev.sources.is_cuda and (tmp_path / "b.vis").read_bytes() == (tmp_path / "ref.vis").read_bytes()
    assert pipeline.fuse(scene, results, None, vis_path=tmp_path / "c.vis") == want.count
    assert (tmp_path / "c.vis").read_bytes() == (tmp_path / "ref.vis").read_bytes()
    assert sorted(os.listdir(tmp_path)) == ["a.ply", "a.vis", "b.vis", "c.vis", "ref.ply", "ref.vis"]
    with pytest.raises(ValueError):
        pipeline.fuse(scene, results, None)


# --------------------------------------------------------------------------------------------------------------------
# the binary
# --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def folders(gpu_pkg, synth, tmp_path_factory):
    """One small synthetic dense folder run with --ply-vis in memory and through the files, and without the flag."""
    root = tmp_path_factory.mktemp("dense")
    a = root / "a"
    a.mkdir()
    _write_dense_folder(a, synth, 96, 72, 4)
    out = {}
    for name, extra in (("memory", ["--ply-vis", "--in-memory"]), ("files", ["--ply-vis", "--files"]), ("plain", [])):
        shutil.copytree(a, root / name)
        _run(root / name, *extra)
        out[name] = root / name
    return out


def _files(folder):
    return {os.path.relpath(os.path.join(d, f), folder): os.path.join(d, f) for d, _, fs in os.walk(folder) for f in fs}


def test_binary_writes_the_same_vis_in_memory_and_through_files(gpu_pkg, folders, tmp_path):
    memory = (folders["memory"] / "APD" / "APD.ply.vis").read_bytes()
    assert memory == (folders["files"] / "APD" / "APD.ply.vis").read_bytes()
    n = _fuse_saved_maps(gpu_pkg, folders["memory"], tmp_path / "pipe.ply", vis_path=tmp_path / "pipe.vis")
    assert n > 0 and (tmp_path / "pipe.vis").read_bytes() == memory
    assert (tmp_path / "pipe.ply").read_bytes() == (folders["memory"] / "APD" / "APD.ply").read_bytes()
    from apd_mvs_amd import pipeline
    offsets, views = pipeline.read_vis(folders["memory"] / "APD" / "APD.ply.vis")
    assert len(offsets) == n + 1 and views.min() >= 0 and views.max() < 4 and (np.diff(offsets) >= 2).all()


def test_binary_without_the_flag_keeps_its_files(gpu_pkg, folders, tmp_path):
    """No .vis file, and every file of the folder has the bytes it has with the flag: the flag adds one file and changes none.
    APD.ply is the one pipeline.fuse writes from the saved maps, which the existing tests pin to the sequential loops."""
    plain, memory = _files(folders["plain"]), _files(folders["memory"])
    assert not [f for f in plain if f.endswith(".vis")]
    assert set(memory) - set(plain) == {os.path.join("APD", "APD.ply.vis")} and set(plain) <= set(memory)
    for rel, path in plain.items():
        assert open(path, "rb").read() == open(memory[rel], "rb").read(), rel
    _fuse_saved_maps(gpu_pkg, folders["plain"], tmp_path / "pipe.ply")
    assert (tmp_path / "pipe.ply").read_bytes() == (folders["plain"] / "APD" / "APD.ply").read_bytes()
