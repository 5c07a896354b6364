"""Host side of the per-view pixel masks (no GPU): the header, mask files and their threshold, per-level resampling, the
synthetic-folder tool, and how the pipeline hands masks to its backend."""
import importlib.util
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _write_pgm(path, a):
    a = np.ascontiguousarray(a, np.uint8)
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (a.shape[1], a.shape[0]) + a.tobytes())


def test_header_declares_the_mask_entry_points():
    text = open(os.path.join(ROOT, "include", "apd_mi355x.h")).read()
    assert re.search(r"\bint\s+apd_upload_mask\s*\(\s*apd_handle\s+h\s*,\s*const\s+uint8_t\s*\*\s*mask\s*\)\s*;", text)
    assert re.search(r"\bint\s+apd_masked_count\s*\(\s*apd_handle\s+h\s*\)\s*;", text)
    assert "APD.cpp:849-853" in text[:text.index("apd_upload_mask(")][-2500:]   # cites what the masks stand beside


def test_library_exports_the_mask_entry_points(pkg):
    import ctypes as C
    L = C.CDLL(pkg.library_path())
    assert hasattr(L, "apd_upload_mask") and hasattr(L, "apd_masked_count")
    assert L.apd_masked_count(None) == 0


def test_mask_threshold(pkg):
    from apd_mvs_amd import pipeline
    grey = np.arange(256, dtype=np.float32).reshape(16, 16)
    m = pipeline.mask_from_grey(grey)
    assert m.dtype == np.uint8
    assert (m.reshape(-1)[:128] == 0).all() and (m.reshape(-1)[128:] != 0).all()


def test_mask_files_of_a_dense_folder(pkg, synth, tmp_path):
    """masks/%08d.pgm: grey < 128 masked out, a view without a file unmasked, nothing read without masks_dir, a file of another
    size refused with its name."""
    from apd_mvs_amd import pipeline
    tool = _tool("make_synthetic_dense")
    folder = str(tmp_path / "dense")
    W, H, V = 48, 36, 3
    tool.write_dense_folder(folder, synth, W, H, V, 2, seed=1)
    os.makedirs(os.path.join(folder, "masks"))
    grey = (np.arange(W * H).reshape(H, W) * 7 % 256).astype(np.uint8)
    _write_pgm(os.path.join(folder, "masks", "%08d.pgm" % 0), grey)
    _write_pgm(os.path.join(folder, "masks", "%08d.pgm" % 2), np.full((H, W), 127, np.uint8))
    scene = pipeline.load_dense_folder(folder, pkg.Camera)
    assert scene.masks is None                                   # directory ignored without masks_dir
    scene = pipeline.load_dense_folder(folder, pkg.Camera, masks_dir="masks")
    assert len(scene.masks) == V and scene.masks[1] is None
    assert np.array_equal(scene.masks[0] != 0, grey >= 128) and scene.masks[0].dtype == np.uint8
    assert not scene.masks[2].any()
    _write_pgm(os.path.join(folder, "masks", "%08d.pgm" % 1), np.zeros((H, W + 1), np.uint8))
    with pytest.raises(ValueError, match=r"masks.00000001\.pgm is %dx%d" % (W + 1, H)):
        pipeline.load_dense_folder(folder, pkg.Camera, masks_dir="masks")
    assert not os.path.exists(os.path.join(folder, "APD"))       # refused before any work: no output


def test_positional_scene_construction_still_works(pkg):
    from apd_mvs_amd import pipeline
    sc = pipeline.MvsScene([1], [2], [[0]])
    assert sc.masks is None and sc.num_views == 1
    assert pipeline.MvsScene([1], [2], [[0]], [None]).masks == [None]


@pytest.mark.parametrize("rows,cols,tr,tc", [(36, 48, 18, 24), (35, 47, 18, 24), (18, 24, 35, 47), (151, 203, 76, 102), (76, 102, 151, 203)])
def test_level_mask_is_rescale_mat_to_target_size(pkg, rows, cols, tr, tc):
    """RescaleMatToTargetSize (APD.cpp:752-774) stated in numpy, swapped factors included: dst(r, c) = src((int)(r / scale_x),
    (int)(c / scale_y)) with scale_x = dst_cols / src_cols, scale_y = dst_rows / src_rows in float; outside -> 0."""
    from apd_mvs_amd import pipeline
    rng = np.random.RandomState(rows * 1000 + cols)
    src = np.where(rng.rand(rows, cols) < 0.4, 0, 255).astype(np.uint8)
    want = np.zeros((tr, tc), np.uint8)
    sx, sy = np.float32(tc) / np.float32(cols), np.float32(tr) / np.float32(rows)
    for r in range(tr):
        o_r = int(np.float32(r) / sx)
        for c in range(tc):
            o_c = int(np.float32(c) / sy)
            if o_r < rows and o_c < cols:
                want[r, c] = src[o_r, o_c]
    got = pipeline.level_mask(src, tc, tr)
    assert got.dtype == np.uint8 and got.flags["C_CONTIGUOUS"]
    assert np.array_equal(got, want)
    assert pipeline.level_mask(src, cols, rows) is not None and np.array_equal(pipeline.level_mask(src, cols, rows), src)


def test_synthetic_masks_are_seeded_and_reproducible(tmp_path):
    tool = _tool("make_synthetic_dense")
    W, H = 160, 120
    a = tool.synthetic_mask(W, H, 0.3, seed=5, view=2)
    assert np.array_equal(a, tool.synthetic_mask(W, H, 0.3, seed=5, view=2))
    assert not np.array_equal(a, tool.synthetic_mask(W, H, 0.3, seed=6, view=2))
    assert not np.array_equal(a, tool.synthetic_mask(W, H, 0.3, seed=5, view=3))
    assert set(np.unique(a)) == {0, 255}
    assert 0.15 < (a == 0).mean() < 0.45                        # about the fraction asked for
    assert (a[0] == 0).all() and (a[-1] != 0).sum() > 0        # the band of "sky" lies along the top
    for d in ("a", "b"):
        tool.write_masks(str(tmp_path / d), W, H, 3, 0.3, seed=5)
    for i in range(3):
        fa, fb = (open(str(tmp_path / d / "masks" / ("%08d.pgm" % i)), "rb").read() for d in ("a", "b"))
        assert fa == fb and fa.startswith(b"P5\n160 120\n255\n")


def test_cli_tools_take_masks(pkg, tmp_path):
    """The two command lines, run: make_synthetic_dense.py --masks writes the seeded masks, and tools/mvs_pipeline.py --masks refuses a
    mask of the wrong size with the file's name before any output (the refusal comes before the first device call)."""
    import subprocess
    import sys
    tool = _tool("make_synthetic_dense")
    folder = tmp_path / "dense"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synthetic_dense.py"), str(folder), "--width", "64", "--height", "48",
                        "--views", "3", "--src", "2", "--seed", "3", "--masks", "0.3"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    for i in range(3):
        raw = (folder / "masks" / ("%08d.pgm" % i)).read_bytes()
        assert raw == b"P5\n64 48\n255\n" + tool.synthetic_mask(64, 48, 0.3, 3, i).tobytes()
    _write_pgm(str(folder / "masks" / "00000001.pgm"), np.zeros((47, 64), np.uint8))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mvs_pipeline.py"), str(folder), "--masks", "--iters", "1"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode != 0
    assert "00000001.pgm is 64x47" in r.stdout, r.stdout[-2000:]
    assert not (folder / "APD").exists()


class _RecordingBackend:
    """Stands in for a compute backend: records what run_pipeline hands over, returns an empty estimate."""
    device = None

    def __init__(self, camera_type, with_mask_keyword):
        self.camera_type = camera_type
        self.calls = []
        if with_mask_keyword:
            self.run_pass = self._run_pass_masked
        else:
            self.run_pass = self._run_pass_plain

    def _out(self, width, height):
        planes = np.zeros((height, width, 4), np.float32)
        planes[..., 2] = 1
        planes[..., 3] = 2.0
        return planes, np.ones((height, width), np.uint8), np.zeros((height, width), np.uint32)

    def _run_pass_plain(self, width, height, params, cameras, images, depths, prior):
        self.calls.append((width, height, None))
        return self._out(width, height)

    def _run_pass_masked(self, width, height, params, cameras, images, depths, prior, mask=None):
        self.calls.append((width, height, None if mask is None else np.array(mask)))
        return self._out(width, height)


def test_pipeline_hands_level_masks_to_the_backend_only_for_masked_views(pkg, synth):
    from apd_mvs_amd import pipeline
    W, H, V = 48, 36, 3
    scene = pipeline.synthetic_ring(synth, W, H, V, 2, pkg.make_camera, seed=2)
    # a backend that does not know the keyword keeps working for unmasked scenes (masks None, and a list of None)
    for masks in (None, [None] * V):
        scene.masks = masks
        plain = _RecordingBackend(pkg.Camera, with_mask_keyword=False)
        pipeline.run_pipeline(scene, plain, iters=1, max_passes=1, single_level=True)
        assert len(plain.calls) == V
    m = np.where(np.arange(W * H).reshape(H, W) % 5 < 2, 0, 255).astype(np.uint8)
    scene.masks = [None, m, None]
    rec = _RecordingBackend(pkg.Camera, with_mask_keyword=True)
    pipeline.run_pipeline(scene, rec, iters=1, max_passes=2, single_level=True)
    assert len(rec.calls) == 2 * V
    for k, (w, h, got) in enumerate(rec.calls):
        if k % V == 1:
            assert got is not None and got.dtype == np.uint8 and np.array_equal(got, pipeline.level_mask(m, w, h))
        else:
            assert got is None
    with pytest.raises(TypeError):    # a masked view needs a backend that takes the mask: no silent unmasked run
        pipeline.run_pipeline(scene, _RecordingBackend(pkg.Camera, with_mask_keyword=False), iters=1, max_passes=1, single_level=True)
