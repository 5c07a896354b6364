"""Per-view pixel masks through the in-memory scheduler (apd-mvs_amd/pipeline.py) and tools/mvs_pipeline.py on the GPU: two
pyramid levels, masks resampled per level, masked pixels of every final map empty, an all-live mask and an ignored `masks`
directory change nothing."""
import importlib.util
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import common

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _maps_equal(a, b):
    return all(np.array_equal(common.bits(getattr(a, k)), common.bits(getattr(b, k))) for k in ("depth", "normal", "weak", "views"))


class _MaskLog:
    """HipBackend that notes which (width, view mask) pairs it was given."""
    accepts_tensors = True

    def __init__(self, inner):
        self.inner, self.device, self.seen = inner, inner.device, []

    @property
    def camera_type(self):
        return self.inner.camera_type

    def run_pass(self, width, height, params, cameras, images, depths, prior, mask=None):
        self.seen.append((width, height, None if mask is None else mask.cpu().numpy().copy()))
        return self.inner.run_pass(width, height, params, cameras, images, depths, prior, mask=mask)


def test_two_level_pipeline_with_masks(gpu_pkg, synth):
    from apd_mvs_amd import pipeline
    tool = _tool("make_synthetic_dense")
    W, H, V, S = 1040, 72, 3, 2   # max(W, H) > 1000 -> two levels: 520x36 and 1040x72 (main.cpp:72-88)
    scene = pipeline.synthetic_ring(synth, W, H, V, S, gpu_pkg.make_camera, seed=6, textureless=0.25)
    plain = pipeline.run_pipeline(scene, pipeline.HipBackend(gpu_pkg, device=0), iters=2, seed=91)
    scene.masks = [np.full((H, W), 255, np.uint8)] * V
    ones = pipeline.run_pipeline(scene, pipeline.HipBackend(gpu_pkg, device=0), iters=2, seed=91)
    for v in range(V):
        assert _maps_equal(plain[v], ones[v]), "a mask without a zero byte must change nothing (view %d)" % v
    scene.masks = [tool.synthetic_mask(W, H, 0.3, seed=4, view=0), None, tool.synthetic_mask(W, H, 0.3, seed=4, view=2)]
    backend = _MaskLog(pipeline.HipBackend(gpu_pkg, device=0))
    got = pipeline.run_pipeline(scene, backend, iters=2, seed=91)
    assert len(backend.seen) == 8 * V
    for k, (w, h, m) in enumerate(backend.seen):
        want = scene.masks[k % V]
        assert (m is None) == (want is None)
        if m is not None:
            assert np.array_equal(m, pipeline.level_mask(want, w, h)), "pass %d: not the level's nearest-neighbour mask" % k
    assert {w for w, _, _ in backend.seen} == {520, 1040}
    for v in (0, 2):
        out = scene.masks[v] == 0
        assert out.mean() > 0.15
        assert not got[v].depth[out].any() and not got[v].normal[out].any() and not got[v].views[out].any()
        assert (got[v].weak[out] == 2).all()
        assert (got[v].depth[~out] > 0).mean() > 0.5, "the live pixels must still be estimated"
        assert not _maps_equal(got[v], plain[v])
    assert (got[1].depth > 0).mean() > 0.5
    # the unmasked view has masked sources: their empty depth maps reach its geometric passes
    assert not np.array_equal(common.bits(got[1].depth), common.bits(plain[1].depth))


def _run_cli(folder, *extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mvs_pipeline.py"), str(folder), "--seed", "9", "--iters", "1", "--no-fusion"]
                       + list(extra), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    return r


def _files(folder, nviews):
    return [open(os.path.join(str(folder), "APD", "%08d" % i, name), "rb").read() for i in range(nviews)
            for name in ("depths.dmb", "normals.dmb", "weak.bin", "selected_views.bin")]


def test_pipeline_cli_masks(gpu_pkg, synth, tmp_path):
    """tools/mvs_pipeline.py --masks == run_pipeline on load_dense_folder(masks_dir=); without --masks the directory is ignored;
    a mask of the wrong size is refused with the file's name and nothing is written."""
    from apd_mvs_amd import pipeline
    tool = _tool("make_synthetic_dense")
    W, H, V = 72, 56, 3
    a, b, c, d = (tmp_path / n for n in "abcd")
    tool.write_dense_folder(str(a), synth, W, H, V, 2, seed=2)
    shutil.copytree(a, c)                       # no masks directory
    tool.write_masks(str(a), W, H, V, 0.3, seed=2)
    os.remove(os.path.join(str(a), "masks", "%08d.pgm" % 1))   # a view without a file is unmasked
    shutil.copytree(a, b)
    shutil.copytree(a, d)

    r = _run_cli(a, "--masks")
    assert r.returncode == 0, r.stdout[-2000:]
    scene = pipeline.load_dense_folder(str(a), gpu_pkg.Camera, masks_dir="masks")
    assert scene.masks[1] is None and scene.masks[0] is not None
    want = pipeline.run_pipeline(scene, pipeline.HipBackend(gpu_pkg, device=0), iters=1, seed=9)
    ref = tmp_path / "ref"
    shutil.copytree(c, ref)
    pipeline.save_results(str(ref), scene, want)
    assert _files(a, V) == _files(ref, V)
    for v in (0, 2):
        out = scene.masks[v] == 0
        assert out.any() and not want[v].depth[out].any() and (want[v].weak[out] == 2).all()

    for folder in (b, c):                       # masks directory present but not asked for / absent
        r = _run_cli(folder)
        assert r.returncode == 0, r.stdout[-2000:]
    assert _files(b, V) == _files(c, V)
    assert _files(b, V) != _files(a, V)

    with open(os.path.join(str(d), "masks", "%08d.pgm" % 2), "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (W, H - 1) + bytes(W * (H - 1)))
    r = _run_cli(d, "--masks")
    assert r.returncode != 0
    assert "00000002.pgm" in r.stdout and "%dx%d" % (W, H - 1) in r.stdout
    assert not os.path.exists(os.path.join(str(d), "APD"))
