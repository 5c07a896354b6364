"""The mean geometry of fused points on the device (apd_points_average, apd_points_write_ply; csrc/apd_points_average.hip, csrc/apd_points.hip), bitwise against
the sequential checker (tests/helpers/points_average_ref.cpp): host- and device-resident points, host and device maps, all three
loops, the skip path over filtered depth maps, the refusals that need a points object, the PLY writer against the file the same
fusion wrote, the Python layer and the drop-in binary's --ply-mean."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import eth_fusion_checker as E
import fusion_cases
import points_average_checker as PA
import vis_checker as VC
from test_fusion_cases import VARIANTS
from test_gpu_dropin_binary import _write_dense_folder
from test_gpu_fusion_options import _fuse, _fuse_saved_maps, _run, _scene
from test_points_average import SKIP_CASE, SKIP_RULE, popcount

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return PA.build(tmp_path_factory.mktemp("points_average_checker"))


class Arrays:
    """The arrays of a Points object as numpy, whichever memory they are in."""

    def __init__(self, pts):
        host = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
        for f in PA.FIELDS:
            setattr(self, f, host(getattr(pts, f)))
        self.sources = self.sources.view(np.uint32)


def fused(pkg, ob, case, variant, on_device, ply=None, **options):
    n, pts = _fuse(pkg, ob, case, pkg.default_fusion_options(variant=VARIANTS.index(variant), result_on_device=int(on_device), **options), ply,
                   points=True, on_device=on_device)
    assert n == pts.count and pts.on_device == on_device
    return pts


def averaged(pkg, case, pts, on_device, depths=None):
    """Points.average with the case's cameras and maps; on_device: the maps as torch tensors on the device."""
    deps, nors = case.depths if depths is None else depths, case.normals
    if on_device:
        import torch
        deps, nors = [torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() for a in deps], [torch.from_numpy(a).cuda() for a in nors]
    return pts.average(case.cameras(pkg.make_camera), deps, nors, maps_on_device=on_device)


def assert_equal(got, want, what):
    for f in PA.FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, f)
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        assert np.array_equal(a, b), (what, f)


# tiny: fewer points than a wave; blocks_641x409 / mixed_sizes: point counts that are no multiple of 256, over many blocks; views
# of two sizes; 31 and 32 sources (mask bits 30 and 31); non-finite depths and normals; no point at all; colour images
CASES = [("tiny_9x7", "eth"), ("tiny_1x300", "tat_advanced"), ("blocks_641x409", "eth"), ("mixed_sizes", "eth"), ("mixed_sizes", "tat_intermediate"),
         ("mixed_sizes", "tat_advanced"), ("sources_31", "tat_intermediate"), ("sources_32", "eth"), ("non_finite", "eth"), ("all_blocked", "eth"),
         ("source_lists", "eth")]


@pytest.mark.parametrize("name,variant", CASES)
def test_average_equals_the_checker(gpu_pkg, ob, checker, name, variant):
    """Host points with host maps and device points with device maps: every array has the checker's bits, the result lives where
    the points live, and the points themselves stay as they were."""
    case = fusion_cases.case(name)
    for on_device in (False, True):
        pts = fused(gpu_pkg, ob, case, variant, on_device)
        before = Arrays(pts)
        want = PA.average_case(checker, ob, case, before)
        mean = averaged(gpu_pkg, case, pts, on_device)
        assert mean.on_device == on_device and mean.count == pts.count == want.count
        if on_device and mean.count:
            assert mean.xyz.is_cuda and mean.sources.is_cuda
        got = Arrays(mean)
        assert_equal(got, want, (name, variant, on_device))
        assert_equal(Arrays(pts), before, "the input")
        assert np.array_equal(got.support.astype(np.int64), popcount(got.sources))
        if variant == "eth":   # with the fused maps no ETH vote is skipped
            assert np.array_equal(got.sources, before.sources) and np.array_equal(got.support, before.support)
    assert (want.count == 0) == (name == "all_blocked")
    assert name not in ("blocks_641x409", "mixed_sizes") or (want.count % 256 != 0 and want.count > 1024)
    assert name != "tiny_9x7" or 0 < want.count < 64
    if name == "sources_32":
        assert (got.sources[got.view == 0] == np.uint32(1 << 31 | 1 << 5)).all() and (got.view == 0).any()
    if name == "sources_31":
        assert (got.sources[got.view == 0] >> 30).all() and (got.view == 0).any()
    if name == "non_finite":
        assert not np.isnan(got.xyz).any() and not np.isnan(got.normal).any() and (np.abs(got.normal).sum(1) == 0).any()
    if name == "source_lists":
        assert "colour" in case.tags and len(np.unique(got.bgr, axis=0)) > 1


def test_host_points_with_device_maps_and_device_points_with_host_maps(gpu_pkg, ob, checker):
    case = fusion_cases.case("mixed_sizes")
    for points_on_device in (False, True):
        pts = fused(gpu_pkg, ob, case, "eth", points_on_device)
        want = PA.average_case(checker, ob, case, Arrays(pts))
        mean = averaged(gpu_pkg, case, pts, not points_on_device)
        assert mean.on_device == points_on_device
        assert_equal(Arrays(mean), want, points_on_device)


@pytest.fixture(scope="module")
def skip_run(gpu_pkg, ob, checker):
    """ETH points of SKIP_CASE (host- and device-resident) averaged over the depth maps of pipeline.filter_maps."""
    from apd_mvs_amd import pipeline
    case = fusion_cases.case(SKIP_CASE)
    scene, results = _scene(gpu_pkg, pipeline, case)
    depths = [m.depth for m in pipeline.filter_maps(scene, results, options=gpu_pkg.default_fusion_options(**SKIP_RULE))]
    out = []
    for on_device in (False, True):
        pts = fused(gpu_pkg, ob, case, "eth", on_device)
        before = Arrays(pts)
        out.append((before, PA.average_case(checker, ob, case, before, depths=depths), averaged(gpu_pkg, case, pts, on_device, depths=depths)))
    return case, out


def test_skipped_sources_leave_the_mean_the_mask_and_the_lists(skip_run):
    case, runs = skip_run
    for before, want, mean in runs:
        got = Arrays(mean)
        assert_equal(got, want, mean.on_device)
        lost, left = int(popcount(before.sources).sum()), int(popcount(want.sources).sum())
        assert 0 < left < lost and (want.sources & ~before.sources).max() == 0   # some sources are skipped, not all
        assert np.array_equal(popcount(got.sources), got.support.astype(np.int64))
        offsets, views = [a.cpu().numpy() if hasattr(a, "cpu") else a for a in mean.visibility()]
        assert np.array_equal(np.diff(offsets), got.support.astype(np.int64) + 1)
        table = np.full((case.num_views, 32), -1, np.int32)
        for v, p in enumerate(case.pairs):
            table[v, :len(p)] = p
        rows = np.concatenate([got.view[:, None], table[got.view]], axis=1)
        take = np.concatenate([np.ones((mean.count, 1), bool), ((got.sources[:, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool)], axis=1)
        assert np.array_equal(views, rows[take])   # exactly `view` plus the kept bits


def test_written_vis_is_that_of_the_averaged_points(skip_run, tmp_path):
    from apd_mvs_amd import pipeline
    _, runs = skip_run
    for before, want, mean in runs:
        mean.write_vis(tmp_path / "m.vis")
        offsets, views = pipeline.read_vis(tmp_path / "m.vis")
        assert np.array_equal(np.diff(offsets), want.support.astype(np.int64) + 1) and len(views) == want.count + int(want.support.sum())


# --------------------------------------------------------------------------------------------------------------------
# refusals that need a points object
# --------------------------------------------------------------------------------------------------------------------

def test_refusals(gpu_pkg, ob, tmp_path):
    case = fusion_cases.case("mixed_sizes")
    pts = fused(gpu_pkg, ob, case, "eth", False)
    L = gpu_pkg.lib()
    V = case.num_views
    cams = case.cameras(gpu_pkg.make_camera)
    deps = (C.c_void_p * V)(*[d.ctypes.data for d in case.depths])
    nors = (C.c_void_p * V)(*[n.ctypes.data for n in case.normals])
    rows = (C.c_int * V)(*[d.shape[0] for d in case.depths])
    cols = (C.c_int * V)(*[d.shape[1] for d in case.depths])
    out = C.c_void_p(77)

    def refused(*args):
        assert L.apd_points_average(pts._p, *args, C.byref(out)) == -1 and out.value == 77
        message = L.apd_fusion_last_error()
        assert message.startswith(b"apd_points_average: "), message
        return message

    assert b"views" in refused(V - 1, C.byref(cams), deps, nors, rows, cols, 0)
    wrong = (C.c_int * V)(*rows)
    wrong[1] += 1
    assert b"view 1" in refused(V, C.byref(cams), deps, nors, wrong, cols, 0)
    wrong = (C.c_int * V)(*cols)
    wrong[3] -= 1
    assert b"view 3" in refused(V, C.byref(cams), deps, nors, rows, wrong, 0)
    for table, kind in ((deps, b"depth"), (nors, b"normal")):
        holed = (C.c_void_p * V)(*table)
        holed[2] = None
        args = (deps, holed) if kind == b"normal" else (holed, nors)
        assert kind in refused(V, C.byref(cams), args[0], args[1], rows, cols, 0)
    assert refused(V, None, deps, nors, rows, cols, 0) == b"apd_points_average: null argument"
    assert L.apd_points_average(pts._p, V, C.byref(cams), deps, nors, rows, cols, 0, None) == -1
    # the PLY writer: a NULL path, and a path that cannot be written
    assert L.apd_points_write_ply(pts._p, None, 0) == -1 and L.apd_fusion_last_error() == b"apd_points_write_ply: null argument"
    assert L.apd_points_write_ply(pts._p, str(tmp_path / "no" / "such" / "dir.ply").encode(), 0) == -6
    assert L.apd_fusion_last_error().startswith(b"apd_points_write_ply: cannot write ")
    with pytest.raises(gpu_pkg.ApdError):
        pts.write_ply(tmp_path / "no" / "such" / "dir.ply")


# --------------------------------------------------------------------------------------------------------------------
# the PLY writer
# --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("normals", [0, 1])
@pytest.mark.parametrize("name,variant", [("mixed_sizes", "eth"), ("mixed_sizes", "tat_advanced"), ("all_blocked", "eth")])
def test_write_ply_gives_the_bytes_of_the_fusion_that_made_the_points(gpu_pkg, ob, tmp_path, name, variant, normals):
    """ply_path and the points from one fusion call; host- and device-resident points."""
    case = fusion_cases.case(name)
    for on_device in (False, True):
        pts = fused(gpu_pkg, ob, case, variant, on_device, ply=tmp_path / "fusion.ply", ply_normals=normals)
        pts.write_ply(tmp_path / "points.ply", normals=bool(normals))
        assert (tmp_path / "points.ply").read_bytes() == (tmp_path / "fusion.ply").read_bytes(), on_device
        assert (pts.count == 0) == (name == "all_blocked")
        # the other record size from the same object: the file of the fusion with the other option
        other = fused(gpu_pkg, ob, case, variant, False, ply=tmp_path / "other.ply", ply_normals=1 - normals)
        pts.write_ply(tmp_path / "points_other.ply", normals=not normals)
        assert (tmp_path / "points_other.ply").read_bytes() == (tmp_path / "other.ply").read_bytes() and other.count == pts.count


def test_ply_of_averaged_points_holds_their_arrays(gpu_pkg, ob, checker, tmp_path):
    case = fusion_cases.case("mixed_sizes")
    for on_device in (False, True):
        pts = fused(gpu_pkg, ob, case, "eth", on_device)
        mean = averaged(gpu_pkg, case, pts, on_device)
        got = Arrays(mean)
        for normals in (False, True):
            mean.write_ply(tmp_path / "mean.ply", normals=normals)
            lines, rec = E.read_ply(tmp_path / "mean.ply")
            assert "element vertex %d" % mean.count in lines and ("property float nx" in lines) == normals
            assert np.array_equal(rec["xyz"].view(np.uint32), got.xyz.view(np.uint32)) and np.array_equal(rec["bgr"], got.bgr)
            assert not normals or np.array_equal(rec["normal"].view(np.uint32), got.normal.view(np.uint32))
        assert not np.array_equal(got.xyz, Arrays(pts).xyz)


# --------------------------------------------------------------------------------------------------------------------
# the pipeline and the binary
# --------------------------------------------------------------------------------------------------------------------

def test_through_the_pipeline(gpu_pkg, ob, checker, tmp_path):
    """fuse(average=True) returns and writes the averaged points; average_points gives them from the points of a plain fuse()."""
    from apd_mvs_amd import pipeline
    case = fusion_cases.case("mixed_sizes")
    scene, results = _scene(gpu_pkg, pipeline, case)
    n, plain = pipeline.fuse(scene, results, tmp_path / "plain.ply", return_points=True)
    want = PA.average_case(checker, ob, case, Arrays(plain))
    assert_equal(Arrays(pipeline.average_points(scene, results, plain)), want, "average_points")
    options = gpu_pkg.default_fusion_options(ply_normals=1)
    m, mean = pipeline.fuse(scene, results, tmp_path / "mean.ply", return_points=True, vis_path=tmp_path / "mean.vis", average=True, options=options)
    assert m == n == want.count
    assert_equal(Arrays(mean), want, "fuse(average=True)")
    _, rec = E.read_ply(tmp_path / "mean.ply")
    assert np.array_equal(rec["xyz"].view(np.uint32), want.xyz.view(np.uint32)) and np.array_equal(rec["normal"].view(np.uint32), want.normal.view(np.uint32))
    mean.write_vis(tmp_path / "again.vis")
    assert (tmp_path / "mean.vis").read_bytes() == (tmp_path / "again.vis").read_bytes()
    assert pipeline.fuse(scene, results, tmp_path / "file_only.ply", average=True, options=options) == n
    assert (tmp_path / "file_only.ply").read_bytes() == (tmp_path / "mean.ply").read_bytes()
    # without the switch: the bytes there were
    assert pipeline.fuse(scene, results, tmp_path / "again.ply") == n
    assert (tmp_path / "again.ply").read_bytes() == (tmp_path / "plain.ply").read_bytes() != (tmp_path / "file_only.ply").read_bytes()


RUNS = {"mean": ["--ply-mean", "--in-memory"], "mean_files": ["--ply-mean", "--files"], "mean_all": ["--ply-mean", "--ply-normals", "--ply-vis"],
        "mean_tat": ["--ply-mean", "--fusion", "tat-intermediate"], "plain": []}


@pytest.fixture(scope="module")
def folders(gpu_pkg, synth, tmp_path_factory):
    """One small synthetic dense folder (the size of the drop-in tests) run with the flag in memory and through the files, with
    normals and lists, with a Tanks and Temples loop, and without the flag."""
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


def test_binary_writes_the_pipelines_averaged_file(gpu_pkg, folders, tmp_path):
    ply = (folders["mean"] / "APD" / "APD.ply").read_bytes()
    assert ply == (folders["mean_files"] / "APD" / "APD.ply").read_bytes()
    n = _fuse_saved_maps(gpu_pkg, folders["mean"], tmp_path / "pipe.ply", average=True)
    assert n > 0 and (tmp_path / "pipe.ply").read_bytes() == ply
    n = _fuse_saved_maps(gpu_pkg, folders["mean_all"], tmp_path / "all.ply", average=True, vis_path=tmp_path / "all.vis",
                         options=gpu_pkg.default_fusion_options(ply_normals=1))
    assert (tmp_path / "all.ply").read_bytes() == (folders["mean_all"] / "APD" / "APD.ply").read_bytes()
    assert (tmp_path / "all.vis").read_bytes() == (folders["mean_all"] / "APD" / "APD.ply.vis").read_bytes()
    n = _fuse_saved_maps(gpu_pkg, folders["mean_tat"], tmp_path / "tat.ply", average=True, variant="tat_intermediate")
    assert n > 0 and (tmp_path / "tat.ply").read_bytes() == (folders["mean_tat"] / "APD" / "APD.ply").read_bytes()


def test_binary_without_the_flag_keeps_its_bytes(gpu_pkg, folders, tmp_path):
    plain = (folders["plain"] / "APD" / "APD.ply").read_bytes()
    n = _fuse_saved_maps(gpu_pkg, folders["plain"], tmp_path / "pipe.ply")
    assert n > 0 and plain == (tmp_path / "pipe.ply").read_bytes()
    mean = (folders["mean"] / "APD" / "APD.ply").read_bytes()
    assert len(mean) == len(plain) and mean != plain
    assert not os.path.exists(folders["mean"] / "APD" / "APD.ply.vis")
