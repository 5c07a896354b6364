"""Named cases off the camera ring synth.make_scene builds (one K with fx == fy and a centred principal point, upright cameras on a
tight ring in the plane z ~ 0): sources rolled about their optical axis, zoomed in and out, with fx != fy and principal points off
the centre and outside the frame, moved along the reference's optical axis, converging at 40 to 50 degrees, seeing half of the
reference frame, and with the surface (or all of it) behind them.  tests/test_camera_space_cases.py runs the ORACLE ALONE on every
case and asserts that the case contains what its name says; tests/test_gpu_camera_space.py compares the HIP path with the oracle on
the same cases after every kernel of three passes.

The renderer is here and not in synth: per-view (K, R, c), the same two slanted planes and sinusoid-product texture, exact ray /
plane intersection in float64, 8-bit quantisation, and the exact depth map of EVERY view -- the geometric pass reads those and not
common.fake_depth_maps, so its forward-backward projection has small, non-trivial residuals.

A case is a rig (a function returning the views, the reference first), a frame, a scene seed and a textureless share; every case
runs the passes FIRST, APD and GEOM of param_space_cases, each from common.postprocess of the one before, every kernel stepped."""
import math

import numpy as np
import torch

import common
import frame_limits_cases as fl
import param_space_cases as pc

TARGET = np.array([0.0, 0.0, 2.2])
# the surface of synth.make_scene: n.P + d = 0; every camera of every rig lies inside both half spaces n.P + d < 0, so the nearest
# intersection along a ray is the same surface for all of them (the images are photo-consistent)
PLANES = [(np.array([-0.15, -0.10, 1.0]), -2.0), (np.array([0.25, 0.05, 1.0]), -2.6)]
SCENE_DEPTH = 2.2


# ---- cameras ----------------------------------------------------------------------------------------------------------------

def focal(W):
    return 0.9 * W


def intrinsics(W, H, fx=None, fy=None, cx=None, cy=None):
    """K as 9 values; the defaults are synth's: f = 0.9 W, the principal point at the frame centre."""
    f = focal(W)
    return np.array([f if fx is None else fx, 0, 0.5 * W if cx is None else cx, 0, f if fy is None else fy, 0.5 * H if cy is None else cy,
                     0, 0, 1], np.float64)


def _lookat(center, target):
    z = np.asarray(target, np.float64) - np.asarray(center, np.float64)
    z = z / np.linalg.norm(z)
    x = np.cross(np.array([0.0, 1.0, 0.0]), z)
    x = x / np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z], 0)


def aim(K, c, point, pixel=None, roll=0.0):
    """World -> camera rotation of a camera at `c` that sees the world point `point` at `pixel` (default: its principal point),
    rolled `roll` degrees about that line of sight."""
    a = math.radians(roll)
    Rz = np.array([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
    R = Rz @ _lookat(c, point)
    if pixel is not None:
        d = np.array([(pixel[0] - K[2]) / K[0], (pixel[1] - K[5]) / K[4], 1.0])
        R = _lookat(np.zeros(3), d).T @ R   # takes the optical axis to the ray of `pixel`
    return R


def ring_centre(j, baseline=0.06):
    """Centre j >= 1 of synth.make_scene's ring."""
    ang = 2.399963 * j
    rad = baseline * (1 + (j % 3))
    return np.array([rad * math.cos(ang), rad * math.sin(ang), 0.02 * math.sin(1.3 * j)])


def reference_view(W, H, K=None, roll=0.0):
    K = intrinsics(W, H) if K is None else K
    return K, aim(K, np.zeros(3), TARGET, roll=roll), np.zeros(3)


def ring_source(W, H, j, K=None, roll=0.0, baseline=0.06, point=TARGET, pixel=None, offset=(0.0, 0.0, 0.0)):
    K = intrinsics(W, H) if K is None else K
    c = ring_centre(j, baseline) + np.asarray(offset, np.float64)
    return K, aim(K, c, point, pixel=pixel, roll=roll), c


# ---- rigs: (W, H) -> [(K, R, c)], the reference first -----------------------------------------------------------------------------

def rig_ring(W, H, N=3):
    return [reference_view(W, H)] + [ring_source(W, H, j) for j in range(1, N + 1)]


def rig_roll(deg):
    def rig(W, H, N=3):
        return [reference_view(W, H)] + [ring_source(W, H, j, roll=deg) for j in range(1, N + 1)]
    return rig


def rig_roll90_ref(W, H):
    return [reference_view(W, H, roll=90.0)] + [ring_source(W, H, j) for j in (1, 2, 3)]


# where the zoomed-in sources look: a source at twice the focal length sees a quarter of the reference frame
_ZOOM_AIMS = [(-0.30, -0.22), (0.30, 0.22), (0.0, 0.0), (0.30, -0.22)]


def rig_zoom(ratios, spread=False):
    def rig(W, H):
        views = [reference_view(W, H)]
        for j, r in enumerate(ratios, 1):
            K = intrinsics(W, H, fx=r * focal(W), fy=r * focal(W))
            ax, ay = _ZOOM_AIMS[(j - 1) % 4] if (spread and r > 1) else (0.0, 0.0)
            views.append(ring_source(W, H, j, K=K, point=TARGET + np.array([ax, ay, 0.0])))
        return views
    return rig


def _aniso_ref(W, H):
    return intrinsics(W, H, fx=0.6 * focal(W), fy=1.2 * focal(W))     # fx = 0.5 fy


def _aniso_src(W, H, **kw):
    return intrinsics(W, H, fx=1.2 * focal(W), fy=0.6 * focal(W), **kw)     # fy = 0.5 fx


def rig_aniso(W, H, N=3):
    return [reference_view(W, H, K=_aniso_ref(W, H))] + [ring_source(W, H, j, K=_aniso_src(W, H)) for j in range(1, N + 1)]


# principal points as shares of (W, H): the reference's and three sources'
_PP = [(0.2, 0.8), (0.8, 0.2), (0.35, 0.3), (0.7, 0.75)]


def _scene_point(W, H, K):
    """The surface point the reference sees at its frame centre (a camera with the principal point off the centre that looks AT the
    target shows the scene off its frame; the off-centre views are aimed so that this point lands on their frame centre)."""
    d = np.array([(0.5 * W - K[2]) / K[0], (0.5 * H - K[5]) / K[4], 1.0])
    return d * SCENE_DEPTH


def rig_offcentre(W, H, N=3):
    Kr = intrinsics(W, H, cx=_PP[0][0] * W, cy=_PP[0][1] * H)
    P0 = _scene_point(W, H, Kr)
    views = [(Kr, np.eye(3), np.zeros(3))]
    for j in range(1, N + 1):
        pp = _PP[1 + (j - 1) % 3]     # past three sources the principal points repeat, the centres do not
        K = intrinsics(W, H, cx=pp[0] * W, cy=pp[1] * H)
        views.append(ring_source(W, H, j, K=K, point=P0, pixel=(0.5 * W, 0.5 * H)))
    return views


def general_rig(name, W, H, N):
    """`aniso`, `offcentre` or `roll37` with N sources: the rigs on which the oracle's own checks run again."""
    return {"aniso": rig_aniso, "offcentre": rig_offcentre, "roll37": rig_roll(37.0)}[name](W, H, N)


def rig_pp_outside(W, H):
    """Source 1 is the crop of a wider frame: cx = -0.25 W."""
    views = rig_offcentre(W, H)
    P0 = _scene_point(W, H, views[0][0])
    K = intrinsics(W, H, cx=-0.25 * W, cy=0.4 * H)
    views[1] = ring_source(W, H, 1, K=K, point=P0, pixel=(0.5 * W, 0.5 * H))
    return views


def rig_forward(W, H):
    """Sources 30 % of the scene depth in front of and behind the reference, a ring radius to the side: the epipole lies inside
    the frame and the scale changes across it."""
    dz = 0.3 * SCENE_DEPTH
    return [reference_view(W, H)] + [ring_source(W, H, j, offset=(0, 0, s * dz)) for j, s in ((1, 1), (2, -1), (3, 1), (4, -1))]


def rig_wide(W, H):
    """Convergence of 42, 49 and 45 degrees: sources left, right and above (y points down)."""
    K = intrinsics(W, H)
    views = [reference_view(W, H)]
    for c in ((-2.0, 0.1, 0.0), (2.5, -0.1, 0.05), (0.1, -2.2, 0.0)):
        c = np.array(c)
        views.append((K, aim(K, c, TARGET), c))
    return views


def rig_partial(W, H):
    """Four sources that see the target on the middle of their left, right, top and bottom edge: the reference's projections fall
    left of, right of, above and below them."""
    views = [reference_view(W, H)]
    for j, pixel in enumerate(((0.0, 0.5 * H), (float(W), 0.5 * H), (0.5 * W, 0.0), (0.5 * W, float(H))), 1):
        views.append(ring_source(W, H, j, baseline=0.1, point=TARGET, pixel=pixel))
    return views


PARTIAL_SIDES = ["left", "right", "above", "below"]   # of source 1, 2, 3, 4: where the reference's pixels fall outside it
BEHIND_NEAR, BEHIND_AWAY = 2, 3                       # view indices in rig_behind


def rig_behind(W, H):
    """Source 1 on the ring; source 2 between the ring and the nearer plane, looking along the surface so that the part of it at
    x > ~0.7 lies behind its image plane; source 3 turned 124 degrees upward: the whole surface is behind it and every projection
    (a point reflection through the principal point) falls outside its frame."""
    K = intrinsics(W, H)
    views = [reference_view(W, H), ring_source(W, H, 1)]
    c = np.array([0.5, 0.0, 1.2])
    views.append((K, aim(K, c, c + np.array([-1.0, 0.0, 0.3])), c))
    c = ring_centre(3)
    a = math.radians(124.0)
    views.append((K, aim(K, c, c + np.array([0.0, math.sin(a), math.cos(a)])), c))
    return views


def rig_mixed(W, H):
    """One source each of roll90, zoom_in2, aniso + offcentre, forward, wide and partial."""
    K = intrinsics(W, H)
    views = [reference_view(W, H), ring_source(W, H, 1, roll=90.0)]
    views.append(ring_source(W, H, 2, K=intrinsics(W, H, fx=2 * focal(W), fy=2 * focal(W))))
    views.append(ring_source(W, H, 3, K=_aniso_src(W, H, cx=0.3 * W, cy=0.7 * H), pixel=(0.5 * W, 0.5 * H)))
    views.append(ring_source(W, H, 4, offset=(0, 0, 0.3 * SCENE_DEPTH)))
    c = np.array([2.0, -0.1, 0.0])
    views.append((K, aim(K, c, TARGET), c))
    views.append(ring_source(W, H, 6, baseline=0.1, pixel=(0.0, 0.5 * H)))
    return views


def random_rig(rng, W, H, N):
    """(views, kind of every source) of tools/parity_fuzz.py's rig family, drawn from `rng` (a numpy RandomState)."""
    views, kinds = [reference_view(W, H)], []
    for j in range(1, N + 1):
        roll = [0.0, 90.0, 180.0, float(rng.uniform(0.0, 360.0))][int(rng.randint(4))]
        fx = focal(W) * float(np.exp(rng.uniform(math.log(0.5), math.log(3.0))))
        fy = fx * float(np.exp(rng.uniform(math.log(0.5), math.log(2.0))))
        K = intrinsics(W, H, fx=fx, fy=fy, cx=float(rng.uniform(0, W)), cy=float(rng.uniform(0, H)))
        pose = ["ring", "forward", "wide", "partial"][int(rng.randint(4))]
        pixel, c = (0.5 * W, 0.5 * H), ring_centre(j, 0.1 if pose == "partial" else 0.06)
        if pose == "forward":
            c = c + np.array([0.0, 0.0, float(rng.choice([-0.3, 0.3])) * SCENE_DEPTH])
        elif pose == "wide":
            a = float(rng.uniform(0, 2 * math.pi))
            c = float(rng.uniform(1.5, 2.5)) * np.array([math.cos(a), math.sin(a), 0.0])
        elif pose == "partial":
            pixel = [(0.0, 0.5 * H), (float(W), 0.5 * H), (0.5 * W, 0.0), (0.5 * W, float(H))][int(rng.randint(4))]
        views.append((K, aim(K, c, TARGET, pixel=pixel, roll=roll), c))
        kinds.append("%s roll %.0f f %.2f fy/fx %.2f" % (pose, roll, fx / focal(W), fy / fx))
    return views, kinds


# ---- renderer ---------------------------------------------------------------------------------------------------------------

def render(W, H, views, seed=0, textureless=0.0, noise=1.5):
    """(images, depths): per view the 8-bit grey image as float32 [H, W] and the exact z-depth of the surface (0 where a ray meets
    no surface in front of the camera).  The texture is synth's, a function of the world x and y of the surface point."""
    rng = np.random.RandomState(seed)
    f = focal(W)
    lam = np.array([5.0, 9.0, 17.0, 31.0]) * (2.0 / f)     # wavelengths in reference pixels at depth 2
    phi = rng.uniform(0, math.pi, 4)
    psi = rng.uniform(0, 2 * math.pi, (4, 2))
    amp = np.array([38.0, 30.0, 24.0, 18.0])
    rects = []
    if textureless > 0:
        side = math.sqrt(textureless / 3) * 2.0 * (W / f)
        for _ in range(3):
            x0 = rng.uniform(-0.8, 0.8 - side) * (W / f)
            y0 = rng.uniform(-0.8, 0.8 - side) * (H / f)
            rects.append((x0, y0, x0 + side, y0 + side * H / W))
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    images, depths = [], []
    for k, (K, R, c) in enumerate(views):
        d = np.stack([(xs - K[2]) / K[0], (ys - K[5]) / K[4], np.ones_like(xs)], -1) @ R     # world direction R^T d, z = 1 in the camera
        best = np.full((H, W), np.inf)
        for n, off in PLANES:
            with np.errstate(divide="ignore", invalid="ignore"):
                s = -(float(n @ c) + off) / (d @ n)
            best = np.minimum(best, np.where(s > 1e-6, s, np.inf))
        hit = np.isfinite(best)
        s = np.where(hit, best, 0.0)
        X, Y = c[0] + s * d[..., 0], c[1] + s * d[..., 1]
        tex = np.zeros((H, W))
        for q in range(4):
            u = X * math.cos(phi[q]) + Y * math.sin(phi[q])
            v = -X * math.sin(phi[q]) + Y * math.cos(phi[q])
            w = 2 * math.pi / lam[q]
            tex += amp[q] * np.sin(w * u + psi[q, 0]) * np.sin(w * v + psi[q, 1])
        scale = np.ones((H, W))
        for (x0, y0, x1, y1) in rects:
            scale[(X >= x0) & (X <= x1) & (Y >= y0) & (Y <= y1)] = 0.03
        img = 128.0 + np.where(hit, tex * scale, 0.0)
        if noise > 0:
            img = img + (np.random.RandomState(1000 * seed + 17 * k + 5).rand(H, W) - 0.5) * (2 * noise)
        images.append(np.clip(np.round(img), 0, 255).astype(np.float32))
        depths.append(s.astype(np.float32))
    return images, depths


def make_scene(synth, W, H, views, seed=0, textureless=0.0):
    """A synth.Scene of the rendered views (so that common.make_handle / make_oracle take it) and the depth map of every view."""
    images, depths = render(W, H, views, seed=seed, textureless=textureless)
    Ks = [K.astype(np.float32) for K, _, _ in views]
    Rs = [R.reshape(9).astype(np.float32) for _, R, _ in views]
    ts = [(-R @ c).astype(np.float32) for _, R, c in views]
    sc = synth.Scene(W, H, len(views) - 1, [torch.from_numpy(im) for im in images], Ks, Rs, ts, 1.0, 4.0, torch.from_numpy(depths[0]),
                     [torch.from_numpy(d) for d in depths])
    return sc, depths


# ---- case table -------------------------------------------------------------------------------------------------------------------

class Case:
    def __init__(self, name, rig, W=80, H=60, seed=2, textureless=0.25, floats=False, nans=False, converged=0.0, pass_seed=61):
        self.name, self.rig, self.W, self.H = name, rig, W, H
        self.N = len(rig(W, H)) - 1
        self.scene_seed, self.textureless, self.floats = seed, textureless, floats
        self.passes = [dict(pc.FIRST, seed=pass_seed, max_iterations=2), dict(pc.APD, seed=pass_seed, max_iterations=2),
                       dict(pc.GEOM, seed=pass_seed, max_iterations=2)]
        # the oracle leaves NaN words (a pixel no source sees sums no view: 0 / 0 in the sweep); measured by
        # tests/test_camera_space_cases.py, which holds the flag to what the oracle does
        self.nans = nans
        # share of the interior pixels within 1 % of the rendered depth after the three passes on the oracle, as measured; the host
        # test asserts it minus 2 points
        self.converged = converged

    def __repr__(self):
        return self.name


_SCENES = {}


def scene(synth, case):
    """(scene, images, depth maps of every view), made once per case and never written to."""
    key = (case.name, case.W, case.H)
    if key not in _SCENES:
        sc, deps = make_scene(synth, case.W, case.H, case.rig(case.W, case.H), seed=case.scene_seed, textureless=case.textureless)
        imgs = sc.images_numpy()
        if case.floats:
            imgs = fl.float_images(imgs)
        for a in imgs + deps:
            a.setflags(write=False)
        _SCENES[key] = (sc, imgs, deps)
    return _SCENES[key]


def scene_views(case):
    """[(K, R, c)] of the case's rig, the reference first."""
    return case.rig(case.W, case.H)


def pass_params(case, sc, pi):
    return common.base_params(sc, case.N, **case.passes[pi])


def steps(params, weak_count):
    return fl.schedule(params["max_iterations"], weak_count > 0)


RING = Case("ring", rig_ring)   # the control: what the suite covered until now, at the same size
# nans / converged: as tests/test_camera_space_cases.py measures them on the oracle (a pixel that no source sees sums no view, and the
# sweep divides 0 by 0 there: most rigs that lose part of the frame leave NaN costs)
CASES = [
    Case("roll90", rig_roll(90.0), nans=True, converged=0.797), Case("roll180", rig_roll(180.0), converged=0.964),
    Case("roll37", rig_roll(37.0), nans=True, converged=0.947), Case("roll90_ref", rig_roll90_ref, nans=True, converged=0.837),
    Case("zoom_in2", rig_zoom([2, 2, 2], spread=True), nans=True, converged=0.594),
    Case("zoom_out_half", rig_zoom([0.5, 0.5, 0.5]), converged=0.799),
    Case("zoom_mixed", rig_zoom([0.5, 1, 2, 3]), nans=True, converged=0.858),
    Case("aniso", rig_aniso, nans=True, converged=0.541),
    # the reference's off-centre frame shows less of the low-texture rectangles: a larger share keeps more than 50 pixels WEAK
    Case("offcentre", rig_offcentre, textureless=0.3, nans=True, converged=0.931),
    Case("pp_outside", rig_pp_outside, textureless=0.3, nans=True, converged=0.933),
    Case("forward", rig_forward, converged=0.935), Case("wide", rig_wide, nans=True, converged=0.996),
    Case("partial", rig_partial, nans=True, converged=0.968), Case("behind", rig_behind, nans=True, converged=0.955),
    Case("mixed", rig_mixed, nans=True, converged=0.987),
    Case("roll90_float", rig_roll(90.0), floats=True, nans=True, converged=0.791),
    Case("mixed_float", rig_mixed, floats=True, nans=True, converged=0.987),
]
BY_NAME = {c.name: c for c in CASES}
