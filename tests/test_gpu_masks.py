"""Per-view pixel masks (apd_upload_mask), bit for bit.

The reference of the masked path is an emulation built from the unmasked, oracle-verified kernels: a handle WITHOUT a mask
whose prior weak map has APD_UNKNOWN at the masked pixels is single-stepped, and after every kernel from K6 on the values K5
left at the masked pixels are written back over them ("masked pixels are frozen").  The kernels are race-free (a colour reads
only the other colour, per-pixel RNG), so that is exactly what skipping the masked pixels must give.  After EVERY kernel all
APD_STATE_* arrays of the masked handle and of the emulation are compared bitwise at every pixel."""
import numpy as np
import pytest

import common

pytestmark = pytest.mark.gpu

UNKNOWN, STRONG, WEAK = 2, 1, 0
FROZEN = ["STATE_PLANES", "STATE_FIT_PLANES", "STATE_COSTS", "STATE_RNG", "STATE_SELECTED_VIEWS", "STATE_VIEW_WEIGHT",
          "STATE_WEAK_INFO"]
ALL_STATES = FROZEN + ["STATE_WEAK_RELIABLE", "STATE_NEAREST_STRONG", "STATE_NEIGHBOURS_MAP", "STATE_NEIGHBOURS"]
KINDS = {
    "first_init": dict(state=0, use_APD=0, weak_peak_radius=6),
    "refine_init_apd": dict(state=1, use_APD=1, weak_peak_radius=6, rotate_time=2, ransac_threshold=0.00875),
    "refine_iter_geom": dict(state=2, use_APD=1, weak_peak_radius=4, rotate_time=4, ransac_threshold=0.0075, geom_consistency=1),
}
ORDER = ["first_init", "refine_init_apd", "refine_iter_geom"]
SIZES = [(40, 33, 2), (33, 35, 3), (203, 151, 4)]
ITERS = 2


def make_mask(name, W, H):
    """uint8 [H, W], non-zero = process."""
    ys, xs = np.mgrid[0:H, 0:W]
    if name == "half_plane":      # an oblique edge: cuts through the 32 x 4 footprints of the waves
        out = (0.61 * xs + ys) < 0.47 * (0.61 * W + H)
    elif name == "speckle":       # no wave is masked entirely
        out = (xs * xs + 3 * ys + (xs ^ ys)) % 3 == 0
    elif name == "blob_with_hole":
        r2 = ((xs - 0.52 * W) / (0.45 * W)) ** 2 + ((ys - 0.48 * H) / (0.45 * H)) ** 2
        out = (r2 < 1.0) & (r2 > 0.1)
    else:
        raise KeyError(name)
    return np.where(out, 0, 255).astype(np.uint8)


def _schedule(iters, weak):
    s = [1, 2] + ([3, 4] if weak else []) + [5]
    for i in range(iters):
        s += [(6, i), (7, i), (8, i)] + ([(9, i), (10, i)] if weak else [])
    s += [11, 12, 13, 14, 15]
    return [(k, 0) if isinstance(k, int) else k for k in s]


_inputs_cache = {}


def case_inputs(pkg, synth, kind, W, H, N):
    """Scene, parameters, depth maps and prior of one pass kind; the priors come from unmasked passes of the kinds before it."""
    key = (W, H, N)
    if key not in _inputs_cache:
        sc, imgs = common.scene_inputs(synth, W, H, N, seed=3, textureless=0.25)
        deps = common.fake_depth_maps(W, H, N + 1)
        priors, prior = {}, None
        for k in ORDER:
            p = common.base_params(sc, N, seed=11, max_iterations=ITERS, **KINDS[k])
            priors[k] = prior
            geom = bool(p.get("geom_consistency"))
            h = common.make_handle(pkg, sc, imgs, N, p, depths=deps if geom else None, prior=prior)
            h.run()
            planes, weak, views = h.download()
            h.close()
            prior = common.postprocess(planes, weak, views, p["depth_min"], p["depth_max"])
        _inputs_cache[key] = (sc, imgs, deps, priors)
    sc, imgs, deps, priors = _inputs_cache[key]
    p = common.base_params(sc, N, seed=11, max_iterations=ITERS, **KINDS[kind])
    return sc, imgs, (deps if p.get("geom_consistency") else None), p, priors[kind]


def states(pkg, h):
    out = {}
    for name in ALL_STATES:
        if name == "STATE_NEIGHBOURS" and h.weak_count == 0:
            continue
        out[name] = h.state(getattr(pkg, name))
    return out


def assert_handles_equal(pkg, a, b, where):
    assert a.weak_count == b.weak_count, "%s: WEAK counts %d / %d" % (where, a.weak_count, b.weak_count)
    sa, sb = states(pkg, a), states(pkg, b)
    for name in sa:
        if not np.array_equal(common.bits(sa[name]), common.bits(sb[name])):
            diff = common.bits(sa[name]).reshape(sa[name].shape[0], -1) != common.bits(sb[name]).reshape(sa[name].shape[0], -1)
            raise AssertionError("%s: `%s` differs in %d bytes" % (where, name, int(diff.sum())))


def step_pair(pkg, a, b, sched, label):
    for kid, it in sched:
        a.run_kernel(kid, it)
        b.run_kernel(kid, it)
        assert_handles_equal(pkg, a, b, "%s after K%d(iter %d)" % (label, kid, it))


def emulation_prior(prior, mask, H, W):
    planes, views, weak = prior if prior is not None else (None, None, None)
    weak = np.full((H, W), STRONG, np.uint8) if weak is None else weak.copy()
    weak[mask == 0] = UNKNOWN
    return planes, views, weak


@pytest.mark.parametrize("shape", ["half_plane", "speckle", "blob_with_hole"])
@pytest.mark.parametrize("W,H,N", SIZES)
@pytest.mark.parametrize("kind", ORDER)
def test_masked_pass_equals_frozen_pixel_emulation(gpu_pkg, synth, kind, W, H, N, shape):
    import torch
    pkg = gpu_pkg
    sc, imgs, deps, p, prior = case_inputs(pkg, synth, kind, W, H, N)
    mask = make_mask(shape, W, H)
    out = mask == 0
    assert out.mean() >= 0.2, "at least 20 %% of the pixels must be masked, got %.1f %%" % (100 * out.mean())
    assert (~out).mean() >= 0.2
    if kind != "first_init":
        assert all((prior[2] == s).any() for s in (WEAK, STRONG, UNKNOWN)), "the prior must hold WEAK, STRONG and UNKNOWN pixels"
    label = "%s %dx%d %s" % (kind, W, H, shape)

    a = common.make_handle(pkg, sc, imgs, N, p, depths=deps, prior=prior)
    a.upload_mask(mask)
    assert a.masked_count() == int(out.sum())
    b = common.make_handle(pkg, sc, imgs, N, p, depths=deps, prior=emulation_prior(prior, mask, H, W))
    if kind != "first_init":
        assert b.weak_count > 0, "the case must drive pixels through the weak path"
    frozen = None
    for kid, it in _schedule(ITERS, b.weak_count > 0):
        a.run_kernel(kid, it)
        b.run_kernel(kid, it)
        if kid == 5:
            frozen = {name: b.state(getattr(pkg, name))[out] for name in FROZEN}
        elif kid >= 6:
            for name in FROZEN:
                if name == "STATE_WEAK_INFO" and kid < 14:   # no kernel before K14 changes it at a non-WEAK pixel; an upload disarms K8..K10
                    assert np.array_equal(b.state(pkg.STATE_WEAK_INFO)[out], frozen[name])
                    continue
                arr = b.state(getattr(pkg, name))
                arr[out] = frozen[name]
                b.set_state(getattr(pkg, name), arr)
        assert_handles_equal(pkg, a, b, "%s after K%d(iter %d)" % (label, kid, it))
    final = states(pkg, a)
    for name in FROZEN:   # point 3 of the contract, stated directly
        assert np.array_equal(common.bits(final[name][out]), common.bits(frozen[name])), name

    # not vacuous: masked neighbours change what propagates to live pixels
    u = common.make_handle(pkg, sc, imgs, N, p, depths=deps, prior=prior)
    u.run()
    pu = u.state(pkg.STATE_PLANES)
    u.close()
    live_diff = (common.bits(pu).reshape(H, W, 16) != common.bits(final["STATE_PLANES"]).reshape(H, W, 16)).any(-1) & ~out
    assert live_diff.any(), "no live pixel differs from the unmasked run: the case shows nothing"

    # one apd_run == the stepped pass
    r = common.make_handle(pkg, sc, imgs, N, p, depths=deps, prior=prior)
    r.upload_mask(mask)
    r.run()
    assert_handles_equal(pkg, r, a, label + ": apd_run vs stepped")
    r.close()

    # before_depths + after_depths, the mask uploaded BEFORE the prior this time
    cams = [pkg.make_camera(sc.K[i], sc.R[i], sc.t[i], W, H, sc.depth_min, sc.depth_max) for i in range(N + 1)]
    s = pkg.Handle(W, H, pkg.default_params(**p), device=0)
    s.upload_mask(mask)
    s.upload_views_split(cams, imgs)
    if prior is not None:
        s.upload_prior(*prior)
    s.run_before_depths()
    if deps is not None:
        s.upload_depths(deps)
    s.run_after_depths()
    assert_handles_equal(pkg, s, a, label + ": split run vs stepped")
    s.close()

    # exports: ProcessProblem's post-processing of the emulation's final state, masked pixels cleared
    rp, rv, rw = common.postprocess(b.state(pkg.STATE_PLANES), b.state(pkg.STATE_WEAK_INFO), b.state(pkg.STATE_SELECTED_VIEWS),
                                    p["depth_min"], p["depth_max"])
    rp[out], rv[out], rw[out] = 0, 0, UNKNOWN
    planes = torch.empty((H, W, 4), device="cuda", dtype=torch.float32)
    weak = torch.empty((H, W), device="cuda", dtype=torch.uint8)
    views = torch.empty((H, W), device="cuda", dtype=torch.int32)
    depth = torch.empty((H, W), device="cuda", dtype=torch.float32)
    a.export_state(planes, weak, views, depth)
    assert np.array_equal(planes.cpu().numpy().view(np.uint32), rp.view(np.uint32))
    assert np.array_equal(weak.cpu().numpy(), rw)
    assert np.array_equal(views.cpu().numpy().view(np.uint32), rv)
    assert np.array_equal(depth.cpu().numpy().view(np.uint32), np.ascontiguousarray(rp[..., 3]).view(np.uint32))
    normal = torch.empty((H, W, 3), device="cuda", dtype=torch.float32)
    depth.zero_()
    torch.cuda.synchronize()   # the export runs on the handle's own non-blocking stream: torch's fill must have ended before it
    a.export_depth_normal(depth, normal)
    assert np.array_equal(depth.cpu().numpy().view(np.uint32), np.ascontiguousarray(rp[..., 3]).view(np.uint32))
    assert np.array_equal(normal.cpu().numpy().view(np.uint32), np.ascontiguousarray(rp[..., :3]).view(np.uint32))
    dp, dw, dv = a.download()   # the raw arrays (no range test), masked pixels cleared
    for got, name, zero in ((dp, "STATE_PLANES", 0), (dw, "STATE_WEAK_INFO", UNKNOWN), (dv, "STATE_SELECTED_VIEWS", 0)):
        want = b.state(getattr(pkg, name))
        want[out] = zero
        assert np.array_equal(common.bits(got), common.bits(want)), name
    tp, tw, tv = a.download_device()
    assert np.array_equal(common.bits(tp.cpu().numpy()), common.bits(dp)) and np.array_equal(tw.cpu().numpy(), dw)
    assert np.array_equal(tv.cpu().numpy().view(np.uint32), dv)
    a.close()
    b.close()


@pytest.mark.parametrize("kind", ORDER)
def test_no_mask_means_no_change(gpu_pkg, synth, kind):
    """A mask of all ones, and apd_upload_mask(NULL) after a real mask: every state array after every kernel is the one of a handle
    that never saw a mask."""
    pkg = gpu_pkg
    W, H, N = 40, 33, 2
    sc, imgs, deps, p, prior = case_inputs(pkg, synth, kind, W, H, N)
    for variant in ("ones", "cleared"):
        plain = common.make_handle(pkg, sc, imgs, N, p, depths=deps, prior=prior)
        h = common.make_handle(pkg, sc, imgs, N, p, depths=deps, prior=prior)
        if variant == "ones":
            h.upload_mask(np.ones((H, W), np.uint8))
        else:
            h.upload_mask(make_mask("blob_with_hole", W, H))
            assert h.masked_count() > 0
            h.upload_mask(None)
        assert h.masked_count() == 0
        step_pair(pkg, h, plain, _schedule(ITERS, plain.weak_count > 0), "%s, %s mask" % (kind, variant))
        for got, want in zip(h.download(), plain.download()):
            assert np.array_equal(common.bits(got), common.bits(want))
        h.close()
        plain.close()


@pytest.mark.parametrize("kind", ["first_init", "refine_init_apd"])
def test_all_ones_mask_in_lockstep_with_the_oracle(gpu_pkg, ob, synth, kind):
    """The masked code path itself (mask pointer set, every byte non-zero) against the CPU oracle, kernel by kernel."""
    pkg = gpu_pkg
    W, H, N = 40, 33, 2
    sc, imgs, deps, p, prior = case_inputs(pkg, synth, kind, W, H, N)
    h = common.make_handle(pkg, sc, imgs, N, p, depths=deps, prior=prior)
    h.upload_mask(np.full((H, W), 7, np.uint8))
    o = common.make_oracle(ob, sc, imgs, N, p, depths=deps, prior=prior)
    for kid, it in _schedule(ITERS, o.weak_count > 0):
        h.run_kernel(kid, it)
        o.run_kernel(kid, it)
        common.assert_state_equal(pkg, h, o, "%s, all-ones mask, after K%d(iter %d)" % (kind, kid, it))
    h.close()
    o.close()


def test_mask_call_order_count_reset_and_device_pointer(gpu_pkg, synth):
    import torch
    pkg = gpu_pkg
    W, H, N = 40, 33, 2
    sc, imgs, deps, p, prior = case_inputs(pkg, synth, "first_init", W, H, N)
    mask = make_mask("half_plane", W, H)
    h = common.make_handle(pkg, sc, imgs, N, p)
    assert h.masked_count() == 0
    h.upload_mask(mask)
    assert h.masked_count() == int((mask == 0).sum())
    h.run_kernel(1, 0)
    with pytest.raises(pkg.ApdError, match="apd error -4"):   # APD_ERR_STATE: a kernel of the pass has run
        h.upload_mask(mask)
    with pytest.raises(pkg.ApdError, match="apd error -4"):
        h.upload_mask(None)
    for kid, it in _schedule(ITERS, False)[1:]:
        h.run_kernel(kid, it)
    host = states(pkg, h)
    host_dl = h.download()

    # a device-pointer mask (bool tensor -> bytes) gives the bits of the host-pointer one
    d = common.make_handle(pkg, sc, imgs, N, p)
    d.upload_mask(torch.from_numpy(mask).cuda() != 0)
    assert d.masked_count() == h.masked_count()
    d.run()
    dev = states(pkg, d)
    for name in host:
        assert np.array_equal(common.bits(host[name]), common.bits(dev[name])), name
    for got, want in zip(d.download(), host_dl):
        assert np.array_equal(common.bits(got), common.bits(want))
    d.close()

    # apd_reset forgets the mask: the recycled handle is an unmasked one
    cams = [pkg.make_camera(sc.K[i], sc.R[i], sc.t[i], W, H, sc.depth_min, sc.depth_max) for i in range(N + 1)]
    h.reset(pkg.default_params(**p))
    assert h.masked_count() == 0
    h.upload_views(cams, imgs)
    h.run()
    plain = common.make_handle(pkg, sc, imgs, N, p)
    plain.run()
    assert_handles_equal(pkg, h, plain, "after apd_reset")
    assert not np.array_equal(common.bits(plain.state(pkg.STATE_PLANES)), common.bits(host["STATE_PLANES"]))
    for got, want in zip(h.download(), plain.download()):
        assert np.array_equal(common.bits(got), common.bits(want))
    # ... and takes a new mask again
    h.reset(pkg.default_params(**p))
    h.upload_mask(mask)
    h.upload_views(cams, imgs)
    h.run()
    again = states(pkg, h)
    for name in host:
        assert np.array_equal(common.bits(host[name]), common.bits(again[name])), name
    h.close()
    plain.close()
