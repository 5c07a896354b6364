"""`APD dense_folder ... --masks [DIR]`: per-view pixel masks through the drop-in binary's three drivers (the file-based one, the
in-memory scheduler in the reference's order, the device list) and against the Python scheduler, on folders of
tools/make_synthetic_dense.py --masks with two pyramid levels."""
import importlib.util
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_dropin_binary as T

pytestmark = pytest.mark.gpu

ROOT = T.ROOT
MAPS = ("depths.dmb", "normals.dmb", "weak.bin", "selected_views.bin")
W, H, V, SRC, SEED = 1040, 72, 4, 3, 21     # max(W, H) > 1000: two pyramid levels, 520 x 36 and 1040 x 72


def _tool():
    spec = importlib.util.spec_from_file_location("make_synthetic_dense", os.path.join(ROOT, "tools", "make_synthetic_dense.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _folder(path, synth, masks=True):
    tool = _tool()
    tool.write_dense_folder(str(path), synth, W, H, V, SRC, seed=2, textureless=0.2)
    if masks:
        tool.write_masks(str(path), W, H, V, 0.3, seed=2)
        os.remove(os.path.join(str(path), "masks", "%08d.pgm" % 1))   # a view without a file is unmasked
    return tool


def _apd(folder, dev, *flags):
    r = subprocess.run([T.APD_BIN, str(folder), dev, "--seed", str(SEED), "--iters", "1", "--keep-maps"] + list(flags), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=900)
    return r


def _bytes(folder):
    out = {(i, n): (folder / "APD" / ("%08d" % i) / n).read_bytes() for i in range(V) for n in MAPS}
    out["ply"] = (folder / "APD" / "APD.ply").read_bytes()
    return out


def _assert_same(a, b, what):
    for key in a:
        assert a[key] == b[key], (what, key)


def test_binary_masks_in_memory_equals_files_and_pipeline(gpu_pkg, synth, tmp_path):
    from apd_mvs_amd import pipeline
    mem, files, cli = tmp_path / "mem", tmp_path / "files", tmp_path / "cli"
    tool = _folder(mem, synth)
    shutil.copytree(mem, files)
    shutil.copytree(mem, cli)
    r = _apd(mem, "0", "--masks")
    assert r.returncode == 0 and "Round nums: 2" in r.stdout and "Processing image" not in r.stdout, r.stdout[-3000:]
    r = _apd(files, "0", "--masks", "--files")
    assert r.returncode == 0 and "Processing image: 00000000" in r.stdout, r.stdout[-3000:]
    got = _bytes(mem)
    _assert_same(got, _bytes(files), "in memory vs --files")

    # every masked pixel of every final map is empty; the live ones are estimated
    masks = [None if i == 1 else tool.synthetic_mask(W, H, 0.3, 2, i) for i in range(V)]
    for i in range(V):
        d = mem / "APD" / ("%08d" % i)
        depth, normal, weak, views = (T._read_dmb(d / n) for n in MAPS)
        assert depth.shape == (H, W)
        if masks[i] is None:
            assert (depth > 0).mean() > 0.5
            continue
        out = masks[i] == 0
        assert out.mean() > 0.15
        assert not depth[out].any() and not normal[out].any() and not views[out].any() and (weak[out] == 2).all()
        assert (depth[~out] > 0).mean() > 0.5

    # the Python scheduler on the same folder: the binary's four maps per view, bit for bit (file threshold and per-level resampling
    # of the masks included), through run_pipeline and through tools/mvs_pipeline.py --masks
    scene = pipeline.load_dense_folder(str(cli), gpu_pkg.Camera, masks_dir="masks")
    assert scene.masks[1] is None and all(np.array_equal(scene.masks[i], masks[i]) for i in (0, 2, 3))
    res = pipeline.run_pipeline(scene, pipeline.HipBackend(gpu_pkg, device=0), iters=1, seed=SEED)
    for i in range(V):
        d = mem / "APD" / ("%08d" % i)
        assert np.array_equal(T._read_dmb(d / "depths.dmb").view(np.uint32), res[i].depth.view(np.uint32)), i
        assert np.array_equal(T._read_dmb(d / "normals.dmb").view(np.uint32), res[i].normal.view(np.uint32)), i
        assert np.array_equal(T._read_dmb(d / "weak.bin"), res[i].weak), i
        assert np.array_equal(T._read_dmb(d / "selected_views.bin"), res[i].views), i
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mvs_pipeline.py"), str(cli), "--seed", str(SEED), "--iters", "1", "--masks"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    _assert_same(got, _bytes(cli), "tools/mvs_pipeline.py --masks vs the binary")

    # APD.ply holds no point of a masked reference pixel: fusing the same maps with the masks handed over as the fusion's own
    # block masks (reference pixels below 128 are skipped, APD.cpp:849-853) emits the same number of points
    n_ply = len(T._read_ply(mem / "APD" / "APD.ply")[0])
    assert n_ply > 0
    blocks = [np.full((H, W), 255, np.uint8) if m is None else m for m in masks]
    n_blocks = pipeline.fuse(scene, res, str(tmp_path / "blocks.ply"), device=0, block_masks=blocks)
    assert n_blocks == n_ply == pipeline.fuse(scene, res, str(tmp_path / "plain.ply"), device=0)


def test_device_list_with_masks_is_rank_count_invariant(gpu_pkg, synth, tmp_path):
    one, two, mem = tmp_path / "one", tmp_path / "two", tmp_path / "mem"
    _folder(one, synth)
    shutil.copytree(one, two)
    shutil.copytree(one, mem)
    r1 = _apd(one, "0", "--jacobi", "--masks")
    assert r1.returncode == 0 and "processed on 1 rank(s)" in r1.stdout, r1.stdout[-3000:]
    r2 = _apd(two, "0,0", "--masks")
    assert r2.returncode == 0 and "processed on 2 rank(s)" in r2.stdout, r2.stdout[-3000:]
    _assert_same(_bytes(one), _bytes(two), "0 --jacobi vs 0,0")
    depth = T._read_dmb(one / "APD" / "00000000" / "depths.dmb")
    out = _tool().synthetic_mask(W, H, 0.3, 2, 0) == 0
    assert not depth[out].any() and (depth[~out] > 0).mean() > 0.5


def test_masks_directory_is_ignored_without_the_option(gpu_pkg, synth, tmp_path):
    with_dir, without = tmp_path / "with", tmp_path / "without"
    _folder(with_dir, synth)
    _folder(without, synth, masks=False)
    for mode in ([], ["--files"]):
        for folder in (with_dir, without):
            shutil.rmtree(folder / "APD", ignore_errors=True)
            r = _apd(folder, "0", *mode)
            assert r.returncode == 0, r.stdout[-3000:]
        _assert_same(_bytes(with_dir), _bytes(without), mode)
    masked = tmp_path / "masked"
    shutil.copytree(with_dir, masked)
    shutil.rmtree(masked / "APD")
    assert _apd(masked, "0", "--masks").returncode == 0
    assert _bytes(masked)[(0, "depths.dmb")] != _bytes(with_dir)[(0, "depths.dmb")]


@pytest.mark.parametrize("mode", [[], ["--files"], ["--jacobi"]], ids=["in-memory", "files", "device-list"])
def test_mask_of_the_wrong_size_is_refused_before_any_output(gpu_pkg, synth, tmp_path, mode):
    _folder(tmp_path / "d", synth)
    bad = tmp_path / "d" / "masks" / "00000002.pgm"
    bad.write_bytes(b"P5\n%d %d\n255\n" % (W, H - 1) + bytes(W * (H - 1)))
    r = _apd(tmp_path / "d", "0", "--masks", *mode)
    assert r.returncode != 0
    assert "00000002.pgm" in r.stdout and "%dx%d" % (W, H - 1) in r.stdout, r.stdout[-2000:]
    assert not (tmp_path / "d" / "APD").exists()
    other = _apd(tmp_path / "d", "0", "--masks", "other_dir", *mode)       # a directory without files: every view unmasked
    assert other.returncode == 0, other.stdout[-2000:]
