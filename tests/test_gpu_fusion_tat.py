"""The Tanks and Temples fusions on the device (apd_fuse_views_variant, csrc/apd_fusion_tat.hip) against the sequential checker
(tests/helpers/tat_fusion_ref.cpp: RunFusion_TAT_Intermediate / RunFusion_TAT_advanced, APD.cpp:979-1296): byte-identical PLY
files through every layer -- C ABI (host and device maps), pipeline.fuse, and the drop-in binary's --fusion."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import tat_checker
import test_gpu_dropin_binary as T

pytestmark = pytest.mark.gpu

VARIANTS = ("tat_intermediate", "tat_advanced")


@pytest.fixture(scope="module")
def checker(ob, tmp_path_factory):
    return tat_checker.build(ob, tmp_path_factory.mktemp("tat_checker"))


def _ring(gpu_pkg, synth, W, H, nviews, nsrc, noise):
    """The ETH fusion tests' ring (exact surface + noise, 5 % holes) with three zeroed depth patches per view: out-of-bounds (the
    image borders), masked (pixels earlier views emitted) and zero-depth invalidity all occur."""
    from apd_mvs_amd import pipeline
    scene, results = T._fusion_inputs(synth, pipeline, gpu_pkg, W, H, nviews, nsrc, noise, seed=5)
    rng = np.random.RandomState(7)
    for v in range(nviews):
        for _ in range(3):
            r0, c0 = rng.randint(0, H - H // 5), rng.randint(0, W - W // 5)
            results[v].depth[r0:r0 + H // 5, c0:c0 + W // 5] = 0.0
    return pipeline, scene, results


def _check(checker, scene, results, variant, path, colour=None, blocks=None):
    V = scene.num_views
    cams = (type(scene.cameras[0]) * V)(*scene.cameras)
    imgs = scene.images if colour is None else colour
    return tat_checker.fuse(checker, variant, cams, imgs, [results[v].depth for v in range(V)], [results[v].normal for v in range(V)],
                            scene.pairs, path, blocks=blocks)


def _abi(gpu_pkg, variant, scene, results, path, on_device, pairs=None):
    """apd_fuse_views_variant straight through ctypes, maps on the host or in torch tensors on cuda:0 (maps_on_device = 1)."""
    import torch
    L = gpu_pkg.lib()
    L.apd_fusion_last_error.restype = C.c_char_p
    V = scene.num_views
    pairs = scene.pairs if pairs is None else pairs
    cams = (type(scene.cameras[0]) * V)(*scene.cameras)
    arrays = [[np.ascontiguousarray(scene.images[v], np.float32) for v in range(V)],
              [np.ascontiguousarray(results[v].depth, np.float32) for v in range(V)],
              [np.ascontiguousarray(results[v].normal, np.float32) for v in range(V)]]
    if on_device:
        arrays = [[torch.from_numpy(a).cuda() for a in arrs] for arrs in arrays]
        torch.cuda.synchronize()
        ptr = [(C.c_void_p * V)(*[a.data_ptr() for a in arrs]) for arrs in arrays]
    else:
        ptr = [(C.c_void_p * V)(*[a.ctypes.data for a in arrs]) for arrs in arrays]
    rows = (C.c_int * V)(*[results[v].depth.shape[0] for v in range(V)])
    cols = (C.c_int * V)(*[results[v].depth.shape[1] for v in range(V)])
    flat = [s for p in pairs for s in p]
    offs = (C.c_int * (V + 1))(*np.cumsum([0] + [len(p) for p in pairs]).tolist())
    idx = (C.c_int * max(len(flat), 1))(*flat)
    n = C.c_longlong(-1)
    code = {"eth": 0, "tat_intermediate": 1, "tat_advanced": 2}.get(variant, variant)
    st = L.apd_fuse_views_variant(code, 0, V, cams, ptr[0], 1, ptr[1], ptr[2], None, None, rows, cols, offs, idx, int(on_device),
                                  str(path).encode(), C.byref(n))
    return st, n.value, L.apd_fusion_last_error()


@pytest.mark.parametrize("W,H,nviews,nsrc,noise", [(160, 120, 5, 4, 0.0004), (333, 217, 7, 6, 0.0008)])
@pytest.mark.parametrize("variant", VARIANTS)
def test_device_tat_fusion_equals_the_sequential_loop(gpu_pkg, synth, checker, tmp_path, W, H, nviews, nsrc, noise, variant):
    pipeline, scene, results = _ring(gpu_pkg, synth, W, H, nviews, nsrc, noise)
    n_ref, stale = _check(checker, scene, results, variant, tmp_path / "ref.ply")
    assert n_ref > 0.1 * W * H * nviews and stale > 0   # the quirk of the per-view diff entries is exercised
    n = pipeline.fuse(scene, results, tmp_path / "gpu.ply", variant=variant)
    assert n == n_ref and (tmp_path / "gpu.ply").read_bytes() == (tmp_path / "ref.ply").read_bytes()
    for on_device in (False, True):   # the C ABI itself, host maps and device maps
        st, n_abi, err = _abi(gpu_pkg, variant, scene, results, tmp_path / "abi.ply", on_device)
        assert st == 0 and n_abi == n_ref, err
        assert (tmp_path / "abi.ply").read_bytes() == (tmp_path / "ref.ply").read_bytes(), on_device
    # colour images (blue, green, red): Intermediate averages them over the used sources, advanced keeps the reference's
    rng = np.random.RandomState(9)
    colour = [np.ascontiguousarray(np.stack([im, np.roll(im, 3, 1), 255.0 - im], -1) + rng.randint(0, 3, im.shape + (3,)), np.float32)
              .clip(0, 255) for im in scene.images]
    n_c, _ = _check(checker, scene, results, variant, tmp_path / "ref_c.ply", colour=colour)
    assert pipeline.fuse(scene, results, tmp_path / "gpu_c.ply", colour_images=colour, variant=variant) == n_c == n_ref
    assert (tmp_path / "gpu_c.ply").read_bytes() == (tmp_path / "ref_c.ply").read_bytes()
    # blocks/ masks: reference pixels below 128 are skipped and leave the diff entries alone
    masks = [np.full((H, W), 255, np.uint8) for _ in range(nviews)]
    masks[0][:, : W // 2] = 0
    masks[2][H // 3:, :] = 100
    n_b, _ = _check(checker, scene, results, variant, tmp_path / "ref_b.ply", blocks=masks)
    assert pipeline.fuse(scene, results, tmp_path / "gpu_b.ply", block_masks=masks, variant=variant) == n_b != n_ref
    assert (tmp_path / "gpu_b.ply").read_bytes() == (tmp_path / "ref_b.ply").read_bytes()
    # not the ETH loop
    assert pipeline.fuse(scene, results, tmp_path / "eth.ply") != n_ref


def test_unknown_variant_and_self_source_are_refused(gpu_pkg, synth, tmp_path):
    pipeline, scene, results = _ring(gpu_pkg, synth, 64, 48, 3, 2, 0.0004)
    for bad in (3, -1):
        st, _, err = _abi(gpu_pkg, bad, scene, results, tmp_path / "x.ply", False)
        assert st == -1 and b"unknown variant" in err and not (tmp_path / "x.ply").exists()
    with pytest.raises(ValueError):
        pipeline.fuse(scene, results, tmp_path / "x.ply", variant="tat")
    pairs = [list(p) for p in scene.pairs]
    pairs[1] = [1, 0]
    for variant in VARIANTS:
        st, _, err = _abi(gpu_pkg, variant, scene, results, tmp_path / "x.ply", False, pairs=pairs)
        assert st == -1 and b"itself" in err and not (tmp_path / "x.ply").exists()


def test_drop_in_binary_fusion_flag(gpu_pkg, synth, checker, tmp_path):
    """`APD folder 0 --keep-maps --fusion tat-intermediate` (in memory and --files) and `APD folder 0,0 --keep-maps --fusion
    tat-advanced` write the checker's APD.ply for the maps they kept; `--fusion eth` is the default."""
    W, H, nviews = 96, 72, 4
    base = tmp_path / "base"
    base.mkdir()
    T._write_dense_folder(base, synth, W, H, nviews)
    runs = {}
    for name, dev, extra in (("plain", "0", []), ("eth", "0", ["--fusion", "eth"]), ("inter", "0", ["--fusion", "tat-intermediate"]),
                             ("inter_files", "0", ["--files", "--fusion", "tat-intermediate"]), ("adv_two", "0,0", ["--fusion", "tat-advanced"])):
        d = tmp_path / name
        shutil.copytree(base, d)
        r = subprocess.run([T.APD_BIN, str(d), dev, "--seed", "5", "--iters", "1", "--keep-maps"] + extra, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=600)
        assert r.returncode == 0 and "All done" in r.stdout, (name, r.stdout[-2000:])
        runs[name] = d
    assert (runs["eth"] / "APD" / "APD.ply").read_bytes() == (runs["plain"] / "APD" / "APD.ply").read_bytes()
    pairs = [[j for j in range(nviews) if j != i] for i in range(nviews)]
    for name, variant in (("inter", "tat_intermediate"), ("inter_files", "tat_intermediate"), ("adv_two", "tat_advanced")):
        d = runs[name]
        cams = (gpu_pkg.Camera * nviews)(*[T._read_cam(d / "cams" / ("%08d_cam.txt" % i), gpu_pkg, W, H) for i in range(nviews)])
        depths = [np.ascontiguousarray(T._read_dmb(d / "APD" / ("%08d" % i) / "depths.dmb")) for i in range(nviews)]
        normals = [np.ascontiguousarray(T._read_dmb(d / "APD" / ("%08d" % i) / "normals.dmb")) for i in range(nviews)]
        images = [T._read_image(d, i, False) for i in range(nviews)]
        assert all(dm.shape == (H, W) for dm in depths)
        n, _ = tat_checker.fuse(checker, variant, cams, images, depths, normals, pairs, tmp_path / (name + ".ply"))
        assert n > 0.1 * W * H, (name, n)
        assert (d / "APD" / "APD.ply").read_bytes() == (tmp_path / (name + ".ply")).read_bytes(), name
    assert (runs["inter"] / "APD" / "APD.ply").read_bytes() != (runs["plain"] / "APD" / "APD.ply").read_bytes()
    r = subprocess.run([T.APD_BIN, str(runs["plain"]), "0", "--fusion", "tat"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode != 0 and "USAGE" in r.stdout
    assert os.path.exists(T.APD_BIN)
