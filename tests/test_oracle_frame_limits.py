"""The oracle ALONE at the tiny frames of tests/test_gpu_frame_limits.py.  Bit equality with the oracle means nothing where the
oracle itself is not well defined -- the reference reads next to its arrays at some borders, and the oracle cites it line by
line -- so before the HIP path is compared with it at 1 x 1 ... 33 x 17:

  * oracle/frame_limits_driver.c runs orc_run through the three pass kinds at every tiny shape (N = 2, and N = 17 at 24 x 20;
    8-bit and non-integer images; the crafted WEAK map) in a build of the oracle under the host sanitizers
    (-fsanitize=address,undefined, `make -C oracle frame_limits_asan`): exit status 0 and no report;
  * the per-pixel restatements of tests/test_oracle_second_entry.py -- view selection, K3, K14 -- reproduce the oracle bit for bit
    at 12 x 10 and 31 x 32 as well: a second witness of its behaviour where every arm, ray and margin is cut by the frame."""
import os
import subprocess

import numpy as np
import pytest

import common
import frame_limits_cases as fl
import test_oracle_second_entry as second

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_oracle_is_sanitizer_clean_at_the_tiny_shapes():
    exe = os.path.join(ROOT, "oracle", "_build", "frame_limits_asan")
    made = subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "frame_limits_asan"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert made.returncode == 0 and os.path.exists(exe), made.stdout
    env = dict(os.environ)
    # leaks are not the subject (and the leak checker needs ptrace rights a test box may lack): reads and writes outside arrays,
    # and undefined behaviour, abort the program with a report
    env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=0"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1"
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=600)
    assert run.returncode == 0, run.stderr[-4000:]
    assert run.stderr.strip() == "", run.stderr[-4000:]
    runs = 2 * len(fl.TINY_SHAPES) + 2
    assert "frame_limits_driver: %d runs of three passes, no report" % runs in run.stdout, run.stdout


def _first_pass_prior(synth, ob, W, H, N, seed):
    sc, imgs = common.scene_inputs(synth, W, H, N, seed=seed, textureless=0.25)
    p0 = common.base_params(sc, N, seed=5, max_iterations=2, **fl.PASSES[0])
    o0 = common.make_oracle(ob, sc, imgs, N, p0)
    o0.run()
    planes, views, _ = common.postprocess(o0.planes.copy(), o0.weak_info.copy(), o0.selected_views.copy(), f32(p0["depth_min"]), f32(p0["depth_max"]))
    o0.close()
    return sc, imgs, (planes, views, fl.crafted_weak_map(W, H))


@pytest.mark.parametrize("W,H", [(12, 10), (31, 32)])
def test_view_selection_at_the_frame_border(synth, ob, W, H):
    """Arm search + joint view selection of K6 / K7 (APD.cu:1012-1259) at every pixel: at 12 x 10 no arm of any pixel has its
    full length."""
    N = 2
    sc, imgs = common.scene_inputs(synth, W, H, N, seed=21)
    o = common.make_oracle(ob, sc, imgs, N, common.base_params(sc, N, seed=77, max_iterations=2))
    for kid in (1, 2, 5):
        o.run_kernel(kid)
    checked = 0
    for it in (0, 1):
        for colour, kid in ((0, 6), (1, 7)):
            snap = (o.costs.copy(), o.planes.copy(), o.selected_views.copy(), o.rng.copy())
            o.run_kernel(kid, it)
            got = o.view_weight
            for py in range(H):
                for px in range(W):
                    if (px + py) % 2 != colour:
                        continue
                    want = second.view_weights_of_pixel(ob, o, snap, W, H, N, px, py, it)
                    assert np.array_equal(got[py, px], want), (it, colour, px, py, got[py, px][:N], want[:N])
                    checked += 1
    assert checked == 2 * W * H
    o.close()


@pytest.mark.parametrize("W,H", [(12, 10), (31, 32)])
def test_gen_neighbours_on_the_crafted_map(synth, ob, W, H):
    """K3 (APD.cu:1750-1969) on the crafted WEAK block: every ray leaves the frame within a few steps of the radius sequence."""
    N = 2
    sc, imgs, prior = _first_pass_prior(synth, ob, W, H, N, seed=12)
    p1 = common.base_params(sc, N, seed=6, max_iterations=1, **fl.PASSES[1])
    o = common.make_oracle(ob, sc, imgs, N, p1, prior=prior)
    for kid in (1, 2):
        o.run_kernel(kid)
    weak = o.weak_info.copy()
    x0, y0, x1, y1 = fl.weak_block(W, H)
    assert o.weak_count == (x1 - x0) * (y1 - y0) > 0
    snap = dict(weak=weak, nearest=o.nearest_strong.copy(), planes=o.planes.copy(), rng=o.rng.copy())
    nmap = o.neighbours_map.copy()
    o.run_kernel(3)
    K = [f32(v) for v in sc.K[0].reshape(-1)]
    nb, reliable, rng_after = o.neighbours, o.weak_reliable, o.rng
    for py in range(H):
        for px in range(W):
            if weak[py, px] != fl.WEAK:
                assert np.array_equal(rng_after[py, px], snap["rng"][py, px]) and reliable[py, px] == 0
                continue
            want_nb, want_rel, want_rng = second.gen_neighbours_pixel(ob, W, H, K, p1, snap["weak"], snap["nearest"], snap["planes"], snap["rng"], px, py)
            row = nb[nmap[py, px]]
            assert [tuple(int(v) for v in q) for q in row] == want_nb, (px, py, row.tolist(), want_nb)
            assert int(reliable[py, px]) == want_rel, (px, py)
            assert np.array_equal(rng_after[py, px], want_rng), (px, py)
    o.close()


@pytest.mark.parametrize("W,H", [(12, 10), (31, 32)])
def test_depth_to_weak_inside_and_outside_the_margin(synth, ob, W, H):
    """K14 (APD.cu:1990-2143) at every pixel, photometric and with the geometric term: 12 x 10 lies entirely inside the 6-px
    margin (all UNKNOWN), 31 x 32 has a 19 x 20 interior."""
    N = 2
    sc, imgs, prior = _first_pass_prior(synth, ob, W, H, N, seed=14)
    for geom in (0, 1):
        params = common.base_params(sc, N, seed=9, max_iterations=2, **fl.PASSES[2 if geom else 0])
        params["geom_factor"] = ob.default_params(**params).geom_factor
        depths = common.fake_depth_maps(W, H, N + 1) if geom else None
        o = common.make_oracle(ob, sc, imgs, N, params, depths=depths, prior=prior if geom else None)
        o.run_kernel(1)
        o.run_kernel(2)
        if geom:
            o.run_kernel(3)
            o.run_kernel(4)
        o.run_kernel(5)
        o.run_sweeps(0, 2)
        for kid in (11, 12, 13):
            o.run_kernel(kid)
        planes, sel, vw = o.planes.copy(), o.selected_views.copy(), o.view_weight.copy()
        o.run_kernel(14)
        got = o.weak_info
        K = [f32(v) for v in sc.K[0].reshape(-1)]
        R = [f32(v) for v in sc.R[0].reshape(-1)]
        cams_c = [[f32(v) for v in ob.make_camera(sc.K[i], sc.R[i], sc.t[i], W, H, sc.depth_min, sc.depth_max).c] for i in range(N + 1)]
        counts = [0, 0, 0]
        for py in range(H):
            for px in range(W):
                want = second.depth_to_weak_pixel(o, cams_c, K, R, params, planes, sel, vw, N, W, H, px, py, geom)
                assert int(got[py, px]) == want, (geom, px, py, int(got[py, px]), want)
                counts[want] += 1
        if W < 13 or H < 13:
            assert counts[fl.UNKNOWN] == W * H
        else:
            assert counts[fl.UNKNOWN] >= W * H - (W - 12) * (H - 12) and counts[fl.UNKNOWN] < W * H, counts
        o.close()
