"""Fusion options on the device (apd_fuse_views_opt, csrc/apd_fusion.hip and csrc/apd_fusion_tat.hip): default options write the
bytes of apd_fuse_views_variant, the ETH loop with other thresholds equals the sequential checker with the same values
(tests/helpers/eth_fusion_opt_ref.cpp) byte for byte, the PLY with normals, the points in memory on the host and on the device,
the running offset of the structure-of-arrays compaction across views, the binary's flags, and the refusal of thresholds for
the T&T loops."""
import copy
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import eth_fusion_checker as E
import fusion_cases
import tat_checker
import vis_checker as VC
from test_fusion_cases import VARIANTS
from test_fusion_options import CASES_OF_SET
from test_gpu_dropin_binary import APD_BIN, _read_dmb, _write_dense_folder
from test_gpu_fusion_scale import _device

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return E.build(tmp_path_factory.mktemp("eth_checker"))


@pytest.fixture(scope="module")
def tat(ob, tmp_path_factory):
    return tat_checker.build(ob, tmp_path_factory.mktemp("tat_checker"))


def _fuse(pkg, ob, case, options, ply=None, points=False, on_device=False, expect=0):
    """apd_fuse_views_opt through ctypes; on_device: every map in a torch tensor on cuda:0.  Returns (count, Points or None)."""
    import torch
    L = pkg.lib()
    L.apd_fusion_last_error.restype = C.c_char_p
    V = case.num_views
    arrays = [[np.ascontiguousarray(a, dt) for a in arrs] for arrs, dt in ((case.images, np.float32), (case.depths, np.float32),
                                                                            (case.normals, np.float32), (case.weaks, np.uint8))]
    blocks = None if case.blocks is None else [None if b is None else np.ascontiguousarray(b, np.uint8) for b in case.blocks]
    if on_device:
        arrays = [[torch.from_numpy(a).cuda() for a in arrs] for arrs in arrays]
        blocks = None if blocks is None else [None if b is None else torch.from_numpy(b).cuda() for b in blocks]
        torch.cuda.synchronize()
        addr = lambda a: None if a is None else a.data_ptr()
    else:
        addr = lambda a: None if a is None else a.ctypes.data
    ptr = [(C.c_void_p * V)(*[addr(a) for a in arrs]) for arrs in arrays]
    bptr = None if blocks is None else (C.c_void_p * V)(*[addr(b) for b in blocks])
    rows = (C.c_int * V)(*[d.shape[0] for d in case.depths])
    cols = (C.c_int * V)(*[d.shape[1] for d in case.depths])
    flat = [s for p in case.pairs for s in p]
    offs = (C.c_int * (V + 1))(*np.cumsum([0] + [len(p) for p in case.pairs]).tolist())
    idx = (C.c_int * max(len(flat), 1))(*flat)
    channels = 3 if case.images[0].ndim == 3 else 1
    n, handle = C.c_longlong(-1), C.c_void_p()
    st = L.apd_fuse_views_opt(C.byref(options), 0, V, case.cameras(ob.make_camera), ptr[0], channels, ptr[1], ptr[2], ptr[3], bptr, rows, cols,
                              offs, idx, int(on_device), None if ply is None else str(ply).encode(), C.byref(n),
                              C.byref(handle) if points else None)
    assert st == expect, L.apd_fusion_last_error()
    return n.value, (pkg.Points(handle, 0) if points and st == 0 else None)


# --------------------------------------------------------------------------------------------------------------------
# default options == apd_fuse_views_variant
# --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", ["tiny_9x7", "blocks_641x409", "mixed_sizes", "all_blocked", "full_frame", "rolled_aniso", "source_behind"])
def test_default_options_write_the_bytes_of_the_variant_entry(gpu_pkg, ob, tmp_path, name, variant):
    """tiny: fewer pixels than a wave; 641 x 409 = 1024 * 256 + 25 pixels; views of two sizes; no point at all; a full frame."""
    case = fusion_cases.case(name)
    n_old = _device(gpu_pkg, ob, case, variant, tmp_path / "old.ply", False)
    n_new, _ = _fuse(gpu_pkg, ob, case, gpu_pkg.default_fusion_options(variant=VARIANTS.index(variant)), tmp_path / "new.ply")
    assert n_new == n_old
    assert (tmp_path / "new.ply").read_bytes() == (tmp_path / "old.ply").read_bytes()


# --------------------------------------------------------------------------------------------------------------------
# options == the sequential checker
# --------------------------------------------------------------------------------------------------------------------

OPTION_CASES = [(key, name) for key in sorted(CASES_OF_SET) for name in CASES_OF_SET[key]]


@pytest.mark.parametrize("key,name", OPTION_CASES)
def test_options_equal_the_sequential_checker(gpu_pkg, ob, checker, tmp_path, key, name):
    """Host maps and device maps through the C ABI, and through libapd_host.so (pipeline.fuse): the checker's bytes."""
    from apd_mvs_amd import pipeline
    case = fusion_cases.case(name)
    rule = E.OPTION_SETS[key]
    want = E.fuse_case(checker, ob, case, tmp_path / "ref.ply", **rule)
    default = E.fuse_case(checker, ob, case).count
    print(key, name, "default", default, "with options", want.count)
    assert want.count != default
    options = gpu_pkg.default_fusion_options(**rule)
    for on_device in (False, True):
        ply = tmp_path / ("dev.ply" if on_device else "host.ply")
        n, _ = _fuse(gpu_pkg, ob, case, options, ply, on_device=on_device)
        assert n == want.count, (key, name, on_device)
        assert ply.read_bytes() == (tmp_path / "ref.ply").read_bytes(), (key, name, on_device)
    scene, results = _scene(gpu_pkg, pipeline, case)
    colour = case.images if case.images[0].ndim == 3 else None
    assert pipeline.fuse(scene, results, tmp_path / "pipe.ply", options=options, block_masks=case.blocks, colour_images=colour) == want.count
    assert (tmp_path / "pipe.ply").read_bytes() == (tmp_path / "ref.ply").read_bytes()


def _scene(pkg, pipeline, case):
    grey = [im[..., 0] if im.ndim == 3 else im for im in case.images]
    scene = pipeline.MvsScene(list(case.cameras(pkg.make_camera)), grey, case.pairs)
    results = {v: pipeline.ViewState(case.depths[v], case.normals[v], case.weaks[v], np.zeros(case.depths[v].shape, np.uint32))
               for v in range(case.num_views)}
    return scene, results


def test_many_sources_with_three_votes(gpu_pkg, ob, checker, tmp_path):
    """33 views, view 0 with 32 sources: min_consistent = 3 against the checker."""
    case = fusion_cases.case("sources_32")
    want = E.fuse_case(checker, ob, case, tmp_path / "ref.ply", points=True, min_consistent=3)
    assert 0 < want.count < E.fuse_case(checker, ob, case).count
    n, pts = _fuse(gpu_pkg, ob, case, gpu_pkg.default_fusion_options(min_consistent=3), tmp_path / "dev.ply", points=True)
    assert n == want.count and (tmp_path / "dev.ply").read_bytes() == (tmp_path / "ref.ply").read_bytes()
    assert np.array_equal(pts.support, want.support) and pts.support.min() >= 3


# --------------------------------------------------------------------------------------------------------------------
# normals in the PLY
# --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", VARIANTS)
def test_ply_with_normals(gpu_pkg, ob, checker, tat, tmp_path, variant):
    case = fusion_cases.case("mixed_sizes")
    code = VARIANTS.index(variant)
    rule = dict(min_consistent=2) if variant == "eth" else {}
    n, pts = _fuse(gpu_pkg, ob, case, gpu_pkg.default_fusion_options(variant=code, ply_normals=1, **rule), tmp_path / "n.ply", points=True)
    n15, _ = _fuse(gpu_pkg, ob, case, gpu_pkg.default_fusion_options(variant=code, **rule), tmp_path / "p.ply")
    lines, rec = E.read_ply(tmp_path / "n.ply")
    props = [l for l in lines if l.startswith("property")]
    assert props == ["property float " + k for k in ("x", "y", "z", "nx", "ny", "nz")] + \
        ["property uchar diffuse_" + k for k in ("blue", "green", "red")]
    _, plain = E.read_ply(tmp_path / "p.ply")
    assert n == n15 == len(rec) > 0
    assert np.array_equal(plain["xyz"].view(np.uint32), rec["xyz"].view(np.uint32)) and np.array_equal(plain["bgr"], rec["bgr"])
    if variant == "eth":
        E.fuse_case(checker, ob, case, tmp_path / "ref.ply", ply_normals=True, **rule)
        assert (tmp_path / "n.ply").read_bytes() == (tmp_path / "ref.ply").read_bytes()
    else:  # the T&T checker's points, and the normal maps at the pixels they came from
        n_ref, _ = tat_checker.fuse(tat, variant, case.cameras(ob.make_camera), case.images, case.depths, case.normals, case.pairs,
                                    tmp_path / "ref.ply", blocks=case.blocks)
        xyz, bgr = tat_checker.read_ply(tmp_path / "ref.ply")
        assert n_ref == n and np.array_equal(xyz.view(np.uint32), rec["xyz"].view(np.uint32)) and np.array_equal(bgr, rec["bgr"])
        want = np.stack([case.normals[v].reshape(-1, 3)[p] for v, p in zip(pts.view, pts.pixel)])
        assert np.array_equal(want.view(np.uint32), rec["normal"].view(np.uint32))
        assert (np.diff(pts.view) >= 0).all() and (np.diff(pts.pixel)[np.diff(pts.view) == 0] > 0).all()
        assert pts.support.min() >= 2 and all(s <= len(case.pairs[v]) for s, v in zip(pts.support, pts.view))


# --------------------------------------------------------------------------------------------------------------------
# the points in memory
# --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["mixed_sizes", "blocks_641x409", "all_blocked"])
def test_points_equal_the_ply_and_the_checker(gpu_pkg, ob, checker, tmp_path, name):
    case = fusion_cases.case(name)
    rule = dict(min_consistent=2)
    want = E.fuse_case(checker, ob, case, points=True, **rule)
    n, host = _fuse(gpu_pkg, ob, case, gpu_pkg.default_fusion_options(ply_normals=1, **rule), tmp_path / "both.ply", points=True)
    _, rec = E.read_ply(tmp_path / "both.ply")
    assert n == want.count == host.count == len(rec) and not host.on_device
    assert (n == 0) == (name == "all_blocked")
    assert np.array_equal(host.xyz.view(np.uint32), rec["xyz"].view(np.uint32))
    assert np.array_equal(host.normal.view(np.uint32), rec["normal"].view(np.uint32)) and np.array_equal(host.bgr, rec["bgr"])
    for field in ("view", "pixel", "support"):
        assert np.array_equal(getattr(host, field), getattr(want, field)), field
    assert host.xyz.shape == (n, 3) and host.pixel.shape == (n,) and host.support.dtype == np.uint8 and host.view.dtype == np.int32
    assert (np.diff(host.view) >= 0).all() and (np.diff(host.pixel)[np.diff(host.view) == 0] > 0).all()
    # a device result without a file: torch tensors on the device, the same values, nothing written
    before = set(os.listdir(tmp_path))
    m, dev = _fuse(gpu_pkg, ob, case, gpu_pkg.default_fusion_options(result_on_device=1, **rule), None, points=True, on_device=True)
    assert m == n and dev.on_device and dev.count == n and set(os.listdir(tmp_path)) == before
    for field in ("xyz", "normal", "bgr", "support", "view", "pixel"):
        t = getattr(dev, field)
        assert t.is_cuda and t.device.index == 0
        a, b = t.cpu().numpy(), getattr(host, field)
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), field


def test_points_through_the_pipeline(gpu_pkg, ob, checker, tmp_path):
    """pipeline.fuse(..., return_points=True) with and without a file."""
    from apd_mvs_amd import pipeline
    case = fusion_cases.case("mixed_sizes")
    want = E.fuse_case(checker, ob, case, tmp_path / "ref.ply", points=True)
    scene, results = _scene(gpu_pkg, pipeline, case)
    n, pts = pipeline.fuse(scene, results, tmp_path / "pipe.ply", return_points=True)
    assert n == want.count == len(pts) and (tmp_path / "pipe.ply").read_bytes() == (tmp_path / "ref.ply").read_bytes()
    assert np.array_equal(pts.pixel, want.pixel) and np.array_equal(pts.normal.view(np.uint32), want.normal.view(np.uint32))
    n, dev = pipeline.fuse(scene, results, None, return_points=True, options=gpu_pkg.default_fusion_options(result_on_device=1))
    assert n == want.count and dev.xyz.is_cuda and dev.xyz.cpu().numpy().tobytes() == want.xyz.tobytes()
    with pytest.raises(ValueError):
        pipeline.fuse(scene, results, None)


def test_result_across_views_with_an_empty_view_between(gpu_pkg, ob, checker, tmp_path):
    """Five views of two sizes; the second is blocked entirely and emits nothing: the views after it append at the running
    count, on the host and on the device."""
    case = copy.deepcopy(fusion_cases.case("mixed_sizes"))
    case.blocks = [None, np.zeros(case.depths[1].shape, np.uint8), None, None, None]
    want = E.fuse_case(checker, ob, case, tmp_path / "ref.ply", points=True)
    per_view = np.bincount(want.view, minlength=5)
    assert per_view[1] == 0 and (per_view[[0, 2, 3, 4]] > 0).all() and len({d.shape for d in case.depths}) == 2
    n, host = _fuse(gpu_pkg, ob, case, gpu_pkg.default_fusion_options(), tmp_path / "dev.ply", points=True)
    assert n == want.count and (tmp_path / "dev.ply").read_bytes() == (tmp_path / "ref.ply").read_bytes()
    _, dev = _fuse(gpu_pkg, ob, case, gpu_pkg.default_fusion_options(result_on_device=1), None, points=True)
    for field in ("xyz", "normal", "bgr", "support", "view", "pixel"):
        assert getattr(host, field).tobytes() == getattr(want, field).tobytes(), field
        assert getattr(dev, field).cpu().numpy().tobytes() == getattr(want, field).tobytes(), field


# The first pixels of every view of full_frame kept as reference pixels, and the points the sequential ETH loop then makes per
# view (counted with the checker on the CPU before the cuts were chosen).  The points in memory start without room, and room for
# `need` points is max(need, twice the room, 4096): view 0 asks for none, view 1 gets the floor of 4096, view 2 passes it and
# doubles it to 8192, view 3 passes 8192 and 16384 at once and gets what it needs.
GROWTH_CUTS = [0, 40000, 1200000, 100000]
GROWTH_POINTS = [0, 3395, 1002, 17275]


def test_points_grow_across_views(gpu_pkg, ob, tmp_path):
    """The seven arrays, the visibility lists and the PLY bytes of a fusion whose device arrays grow three times, kept across
    every growth: host result and device result against the sequential checker, bit for bit."""
    case = VC.first_pixels(fusion_cases.case("full_frame"), "growth", GROWTH_CUTS)
    vis = VC.build(tmp_path)
    want = VC.fuse_case(vis, ob, "eth", case, tmp_path / "ref.ply", ply_normals=True, vis_path=tmp_path / "ref.vis")
    assert np.bincount(want.view, minlength=4).tolist() == GROWTH_POINTS
    totals = np.cumsum(GROWTH_POINTS)
    assert totals[0] == 0 and 0 < totals[1] < 4096 < totals[2] < 8192 and totals[3] > 16384
    for on_device in (False, True):
        tag = "dev" if on_device else "host"
        options = gpu_pkg.default_fusion_options(ply_normals=1, result_on_device=int(on_device))
        n, pts = _fuse(gpu_pkg, ob, case, options, tmp_path / (tag + ".ply"), points=True, on_device=on_device)
        assert n == want.count == pts.count and pts.on_device == on_device
        assert (tmp_path / (tag + ".ply")).read_bytes() == (tmp_path / "ref.ply").read_bytes(), tag
        host = lambda a: a.cpu().numpy() if on_device else np.asarray(a)
        for field in ("xyz", "normal", "bgr", "support", "view", "pixel", "sources"):
            assert host(getattr(pts, field)).tobytes() == getattr(want, field).tobytes(), (field, tag)
        offsets, views = [host(a) for a in pts.visibility()]
        assert offsets.tobytes() == want.offsets.tobytes() and views.tobytes() == want.views.tobytes(), tag
        pts.write_ply(tmp_path / (tag + "_points.ply"), normals=True)
        assert (tmp_path / (tag + "_points.ply")).read_bytes() == (tmp_path / "ref.ply").read_bytes(), tag
        pts.write_vis(tmp_path / (tag + ".vis"))
        assert (tmp_path / (tag + ".vis")).read_bytes() == (tmp_path / "ref.vis").read_bytes(), tag


# --------------------------------------------------------------------------------------------------------------------
# T&T variants keep their own thresholds
# --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", [1, 2])
def test_tat_variant_with_a_threshold_is_unsupported(gpu_pkg, ob, tmp_path, variant):
    case = fusion_cases.case("tiny_9x7")
    n, _ = _fuse(gpu_pkg, ob, case, gpu_pkg.default_fusion_options(variant=variant, max_reproj_error=1.0), tmp_path / "x.ply", expect=-5)
    assert n == -1 and not (tmp_path / "x.ply").exists()
    assert gpu_pkg.lib().apd_fusion_last_error().startswith(b"apd_fuse_views_opt: ")


# --------------------------------------------------------------------------------------------------------------------
# the binary
# --------------------------------------------------------------------------------------------------------------------

FLAGS = ["--fusion-min-consistent", "2", "--ply-normals"]


def _run(folder, *extra):
    r = subprocess.run([APD_BIN, str(folder), "0", "--seed", "21", "--iters", "1", "--keep-maps"] + list(extra), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "All done" in r.stdout, r.stdout[-2000:]
    return (folder / "APD" / "APD.ply").read_bytes()


@pytest.fixture(scope="module")
def folders(gpu_pkg, synth, tmp_path_factory):
    """One small synthetic dense folder (the size of the drop-in tests), run with the flags in memory and through the files,
    and without the flags."""
    root = tmp_path_factory.mktemp("dense")
    a = root / "a"
    a.mkdir()
    _write_dense_folder(a, synth, 96, 72, 4)
    out = {}
    for name, extra in (("memory", FLAGS + ["--in-memory"]), ("files", FLAGS + ["--files"]), ("plain", [])):
        shutil.copytree(a, root / name)
        out[name] = (root / name, _run(root / name, *extra))
    return out


def _fuse_saved_maps(pkg, folder, path, **kw):
    from apd_mvs_amd import pipeline
    scene = pipeline.load_dense_folder(str(folder), pkg.Camera)
    results = {}
    for v in range(scene.num_views):
        d = folder / "APD" / ("%08d" % v)
        results[v] = pipeline.ViewState(_read_dmb(d / "depths.dmb"), _read_dmb(d / "normals.dmb"), _read_dmb(d / "weak.bin"),
                                        _read_dmb(d / "selected_views.bin"))
    return pipeline.fuse(scene, results, path, **kw)


def test_binary_flags_equal_the_pipeline_with_options(gpu_pkg, folders, tmp_path):
    folder, ply = folders["memory"]
    n = _fuse_saved_maps(gpu_pkg, folder, tmp_path / "pipe.ply", options=gpu_pkg.default_fusion_options(min_consistent=2, ply_normals=1))
    assert n > 0 and ply == (tmp_path / "pipe.ply").read_bytes()
    lines, rec = E.read_ply(folder / "APD" / "APD.ply")
    assert "property float nz" in lines and len(rec) == n


def test_binary_flags_write_the_same_bytes_in_memory_and_through_files(folders):
    assert folders["memory"][1] == folders["files"][1]


def test_binary_without_the_flags_keeps_its_bytes(gpu_pkg, folders, tmp_path):
    folder, ply = folders["plain"]
    n = _fuse_saved_maps(gpu_pkg, folder, tmp_path / "pipe.ply")
    assert n > 0 and ply == (tmp_path / "pipe.ply").read_bytes() and ply != folders["memory"][1]
    lines, rec = E.read_ply(folder / "APD" / "APD.ply")
    assert "property float nx" not in lines and len(rec) == n


@pytest.mark.parametrize("flags", [["--fusion-min-consistent", "0"], ["--fusion-min-consistent", "33"], ["--fusion-reproj", "-1"],
                                   ["--fusion-depth", "nan"], ["--fusion-angle", "1e"], ["--fusion-factors", "0.3"],
                                   ["--fusion-factors", "0.3,x"], ["--fusion-reproj"],
                                   ["--fusion", "tat-advanced", "--fusion-min-consistent", "2"]])
def test_binary_refuses_bad_flag_values_before_anything_is_written(folders, tmp_path, flags):
    folder = tmp_path / "f"
    shutil.copytree(folders["plain"][0], folder, ignore=shutil.ignore_patterns("APD"))
    r = subprocess.run([APD_BIN, str(folder), "0"] + flags, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode != 0 and "USAGE: APD" in r.stdout and not (folder / "APD").exists(), r.stdout[-500:]
