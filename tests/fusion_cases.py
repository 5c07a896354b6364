"""Deterministic inputs of the three fusion loops (ETH: RunFusion; Tanks and Temples: RunFusion_TAT_Intermediate /
RunFusion_TAT_advanced), numpy only, no device.  A case is cameras, per-view images, depths, normals, weak maps, optional block
masks and source lists, plus tags naming the edges it exercises.  Most tags are read off the arrays (`_derived_tags`), so a
later edit of a builder cannot claim an edge its data lost.

CASES names the committed cases (builder, seed); test_fusion_cases.py runs the sequential checkers on every one of them and
test_gpu_fusion_scale.py compares the device fusions with them.  random_case(seed) draws small cases for tools/fusion_fuzz.py."""
import math

import numpy as np

from test_gpu_dropin_binary import _ring_depth

FLT_MIN = np.float32(1.1754944e-38)

# every tag of every class must occur in a committed case (test_fusion_cases.py)
TAG_CLASSES = {
    "sizes": ["n<64", "n=256", "blocks=1024", "blocks=1025", "blocks=2052", "1920x1080", "1px_wide", "1px_tall"],
    "view_sizes": ["mixed_sizes"],
    "sources": ["src=0", "src=1", "src=2", "src=31", "src=32", "shuffled", "asymmetric", "duplicated", "unlisted_view"],
    "invalid": ["holes", "zero_band", "long_carry", "all_zero_view", "all_blocked_view"],
    "images": ["grey", "colour", "near_255", "blocks", "blocks_none"],
    "maps": ["maps_host", "maps_device", "blocks_device"],
    "cameras": ["rolled", "aniso", "offcentre", "source_behind"],
    "non_finite": ["nan_depth", "inf_depth", "neg_inf_depth", "neg_zero_depth", "denormal_depth", "huge_depth", "nan_normal"],
}


class Case:
    """views: list of dicts K (9,), R (9,), t (3,) float32, W, H; images float32 [H, W] or [H, W, 3]; depths float32 [H, W];
    normals float32 [H, W, 3]; weaks uint8 [H, W]; blocks None or a list of uint8 [H, W] / None; pairs: source lists."""

    def __init__(self, name, views, images, depths, normals, weaks, pairs, blocks=None, tags=()):
        self.name, self.views, self.images, self.depths, self.normals, self.weaks = name, views, images, depths, normals, weaks
        self.pairs = [list(p) for p in pairs]
        self.blocks = blocks
        self.declared = set(tags)   # the edges the arrays cannot show (a zero band, a long carry, empty by construction)
        self.retag()

    def retag(self):
        """Tags of the arrays as they are now: the declared ones and those read off the arrays."""
        self.tags = self.declared | _derived_tags(self)

    @property
    def num_views(self):
        return len(self.views)

    def cameras(self, make_camera):
        """ctypes array of the reference's Camera (make_camera: the package's or the oracle's)."""
        cams = [make_camera(v["K"], v["R"], v["t"], v["W"], v["H"], 1.0, 100.0) for v in self.views]
        return (type(cams[0]) * len(cams))(*cams)

    def block_arrays(self):
        """The block masks with None replaced by an all-255 mask (what a missing mask means), for the host checkers."""
        if self.blocks is None:
            return None
        return [np.full(d.shape, 255, np.uint8) if b is None else b for b, d in zip(self.blocks, self.depths)]


def _derived_tags(c):
    tags = {"maps_host", "maps_device"}   # test_gpu_fusion_scale.py runs every case with both
    sizes = [d.shape for d in c.depths]
    for h, w in sizes:
        n = h * w
        nb = (n + 255) // 256
        tags |= {t for t, ok in (("n<64", 0 < n < 64), ("n=256", n == 256), ("blocks=1024", nb == 1024), ("blocks=1025", nb == 1025),
                                 ("blocks=2052", nb == 2052), ("1920x1080", (h, w) == (1080, 1920)), ("1px_wide", w == 1 and h > 1),
                                 ("1px_tall", h == 1 and w > 1)) if ok}
    if len(set(sizes)) > 1:
        tags.add("mixed_sizes")
    listed = set()
    for i, p in enumerate(c.pairs):
        listed |= set(p)
        if len(p) in (0, 1, 2, 31, 32):
            tags.add("src=%d" % len(p))
        if list(p) != sorted(p):
            tags.add("shuffled")
        if len(set(p)) < len(p):
            tags.add("duplicated")
        if any(i not in c.pairs[j] for j in p):
            tags.add("asymmetric")
    if any(v not in listed for v in range(c.num_views)) and listed:
        tags.add("unlisted_view")
    for v in c.views:
        tags |= {t for t, ok in (("rolled", abs(float(v["R"][1])) > 0.5), ("aniso", float(v["K"][0]) != float(v["K"][4])),
                                 ("offcentre", float(v["K"][2]) != 0.5 * v["W"] and float(v["K"][2]) != (v["W"] - 1) / 2.0)) if ok}
    for d in c.depths:
        if (d == 0).mean() >= 0.01 and (d != 0).any():
            tags.add("holes")
        if d.size and (d == 0).all():
            tags.add("all_zero_view")
        tags |= {t for t, ok in (("nan_depth", np.isnan(d).any()), ("inf_depth", np.isposinf(d).any()), ("neg_inf_depth", np.isneginf(d).any()),
                                 ("neg_zero_depth", ((d == 0) & np.signbit(d)).any()),
                                 ("denormal_depth", ((d != 0) & (np.abs(d) < FLT_MIN)).any()),
                                 ("huge_depth", (np.abs(d) >= 1e30).any())) if ok}
    if any(np.isnan(nm).any() for nm in c.normals):
        tags.add("nan_normal")
    tags.add("colour" if c.images[0].ndim == 3 else "grey")
    if any((im >= 250).any() for im in c.images):
        tags.add("near_255")
    if c.blocks is not None:
        tags |= {"blocks", "blocks_device"}
        if any(b is None for b in c.blocks):
            tags.add("blocks_none")
        if any(b is not None and b.size and (b < 128).all() for b in c.blocks):
            tags.add("all_blocked_view")
    return tags


# --------------------------------------------------------------------------------------------------------------------
# scenes
# --------------------------------------------------------------------------------------------------------------------

def _lookat(c, target):
    z = target - c
    z = z / np.linalg.norm(z)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z], 0)


def ring_views(W, H, nviews):
    """The synthetic generator's camera ring (apd-mvs_amd/synth.py make_scene, reference view 0, baseline 0.06), in numpy."""
    f = 0.9 * W
    K = np.array([f, 0, 0.5 * W, 0, f, 0.5 * H, 0, 0, 1], np.float64)
    target = np.array([0.0, 0.0, 2.2])
    views = []
    for k in range(nviews):
        if k == 0:
            c, R = np.zeros(3), np.eye(3)
        else:
            ang, rad = 2.399963 * k, 0.06 * (1 + (k % 3))
            c = np.array([rad * math.cos(ang), rad * math.sin(ang), 0.02 * math.sin(1.3 * k)])
            R = _lookat(c, target)
        views.append(dict(K=K.astype(np.float32), R=R.reshape(9).astype(np.float32), t=(-R @ c).astype(np.float32), W=W, H=H))
    return views


def ring_pairs(nviews, nsrc):
    """Every view paired with its nsrc nearest ring neighbours (pipeline.synthetic_ring)."""
    return [sorted((j for j in range(nviews) if j != i), key=lambda j: (abs(j - i), j))[:nsrc] for i in range(nviews)]


def _ring_maps(view, rng, noise, holes=0.05):
    """Depth (exact surface + noise, holes), normal and weak maps of one ring view, as test_gpu_dropin_binary._fusion_inputs."""
    W, H = view["W"], view["H"]
    gt, Rw = _ring_depth(view["K"], view["R"], view["t"], W, H)
    d = (gt * (1.0 + noise * rng.standard_normal(gt.shape))).astype(np.float32)
    d[rng.rand(H, W) < holes] = 0.0
    n = np.zeros((H, W, 3), np.float64)
    n[..., 2] = -1.0
    n[..., 0] = 0.01 * rng.standard_normal((H, W))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    n = np.ascontiguousarray((n @ Rw).astype(np.float32))
    weak = (rng.rand(H, W) < 0.2).astype(np.uint8)
    return d, n, weak


def _grey(rng, H, W, lo=0, hi=256):
    return rng.randint(lo, hi, (H, W)).astype(np.float32)


def ring_case(name, seed, W, H, nviews, nsrc, noise=0.0004, views=None, pairs=None, tags=()):
    rng = np.random.RandomState(seed)
    views = ring_views(W, H, nviews) if views is None else views
    depths, normals, weaks, images = [], [], [], []
    for v in views:
        d, n, w = _ring_maps(v, rng, noise)
        depths.append(d)
        normals.append(n)
        weaks.append(w)
        images.append(_grey(rng, v["H"], v["W"]))
    return Case(name, views, images, depths, normals, weaks, ring_pairs(nviews, nsrc) if pairs is None else pairs, tags=tags)


def plane_case(name, seed, W, H, nviews, pairs, bad=(), noise=1e-4):
    """A fronto-parallel plane at depth 10 seen with f = 10 (test_tat_fusion_checker._scene) by cameras R = I shifted by less than
    0.45 pixel in x and y: every pixel of a view lands on the same pixel of every other view, the reprojection error is the
    shift difference.  Views in `bad` have their depths 5 % too far: they fail every depth test of every loop."""
    rng = np.random.RandomState(seed)
    F, Z = 10.0, 10.0
    K = np.array([F, 0, (W - 1) / 2.0, 0, F, (H - 1) / 2.0, 0, 0, 1], np.float32)
    views, depths, normals, weaks, images = [], [], [], [], []
    for v in range(nviews):
        s = rng.uniform(-0.2, 0.2, 2) if v else np.zeros(2)
        views.append(dict(K=K, R=np.eye(3, dtype=np.float32).reshape(9), t=np.array([-s[0], -s[1], 0.0], np.float32), W=W, H=H))
        d = Z * (1.0 + noise * rng.standard_normal((H, W)))
        depths.append((d * (1.05 if v in bad else 1.0)).astype(np.float32))
        n = np.zeros((H, W, 3), np.float64)
        n[..., 2] = -1.0
        n[..., :2] = 0.01 * rng.standard_normal((H, W, 2))
        normals.append(np.ascontiguousarray((n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32)))
        weaks.append((rng.rand(H, W) < 0.2).astype(np.uint8))
        images.append(_grey(rng, H, W))
    return Case(name, views, images, depths, normals, weaks, pairs)


# --------------------------------------------------------------------------------------------------------------------
# the committed cases
# --------------------------------------------------------------------------------------------------------------------

def full_frame(seed, long_carry=False):
    """1920 x 1080, 4 views, 3 sources; long_carry: source pairs[0][0] keeps depth in rows 0-2 only, so view 0 carries that
    source's entry from there over most of the frame."""
    c = ring_case("full_frame" + ("_long_carry" if long_carry else ""), seed, 1920, 1080, 4, 3, tags=("long_carry",) if long_carry else ())
    if long_carry:
        c.depths[c.pairs[0][0]][3:] = 0.0
        c.retag()
    return c


def block_boundary(seed, W, H):
    """A 3-view ring at a size whose block count is a boundary of the scans' partitions, a zero band over the middle rows of
    view 0's first source (carries across partitions) and blocks in place for view 1 only."""
    c = ring_case("blocks_%dx%d" % (W, H), seed, W, H, 3, 2, tags=("zero_band",))
    c.depths[c.pairs[0][0]][H // 3: 2 * H // 3] = 0.0
    rng = np.random.RandomState(seed + 1)
    c.blocks = [None, (rng.rand(H, W) < 0.9).astype(np.uint8) * 255, None]
    c.retag()
    return c


def tiny(seed, W, H):
    """Degenerate frame sizes on the plane scene: 4 views, every view lists two or three others."""
    pairs = [[1, 2, 3], [2, 0], [3, 1], [0, 1]]
    return plane_case("tiny_%dx%d" % (W, H), seed, W, H, 4, pairs)


def many_sources(seed, S):
    """S + 1 views of 40 x 30; view 0 lists the S others shuffled, and only the sources at positions S - 1 (bit S - 1 of the
    validity word) and 5 agree with it: every point of view 0 needs both.  View 1 lists 2 sources, one of them twice."""
    rng = np.random.RandomState(seed)
    order = list(rng.permutation(np.arange(1, S + 1)))
    good = {int(order[S - 1]), int(order[5])}
    pairs = [[int(x) for x in order], [2, 3, 2]] + [[] for _ in range(S - 1)]
    pairs[2] = [1, 0]
    c = plane_case("sources_%d" % S, seed, 40, 30, S + 1, pairs, bad=[v for v in range(1, S + 1) if v not in good])
    return c


def few_sources(seed, S):
    """Plane scene, 3 views, every view with S sources (S = 0: nothing to fuse in any loop)."""
    pairs = [[(i + 1 + k) % 3 for k in range(S)] for i in range(3)]
    c = plane_case("sources_%d" % S, seed, 24, 20, 3, pairs)
    if S == 0:
        c.declared.add("empty")
        c.retag()
    return c


def source_lists(seed):
    """A 6-view ring: shuffled, asymmetric and duplicated lists; view 5 is nobody's source; view 2's depths are all zero, view 3
    is entirely blocked, view 4 has no block mask, the others' masks straddle 128; colour images near 255."""
    pairs = [[2, 1, 3], [0, 0, 2, 4], [3, 1], [4, 2, 1, 0], [3, 2, 1], [4, 3, 0, 1]]
    c = ring_case("source_lists", seed, 200, 150, 6, 0, pairs=pairs)
    rng = np.random.RandomState(seed + 1)
    c.depths[2][:] = 0.0
    c.images = [np.ascontiguousarray(np.stack([im, 255.0 - im, np.full_like(im, 250.0) + rng.randint(0, 6, im.shape)], -1), np.float32)
                for im in c.images]
    c.blocks = [np.where(rng.rand(150, 200) < 0.5, 127, 128).astype(np.uint8) for _ in range(6)]
    c.blocks[3][:] = 0
    c.blocks[4] = None
    c.retag()
    return c


def mixed_sizes(seed):
    """A 5-view 240 x 180 ring whose views 1 and 3 are at half resolution (K scaled), holes and zero bands in rows."""
    views = ring_views(240, 180, 5)
    for v in (1, 3):
        K = views[v]["K"].copy()
        K[[0, 2, 4, 5]] *= np.float32(0.5)
        views[v] = dict(views[v], K=K, W=120, H=90)
    c = ring_case("mixed_sizes", seed, 240, 180, 5, 3, views=views, tags=("zero_band",))
    c.depths[1][30:60] = 0.0
    c.depths[4][:, 100:140] = 0.0
    c.retag()
    return c


def all_blocked(seed):
    """Every view of a 3-view ring is entirely blocked: empty by construction."""
    c = ring_case("all_blocked", seed, 64, 48, 3, 2, tags=("empty",))
    c.blocks = [np.zeros((48, 64), np.uint8) for _ in range(3)]
    c.retag()
    return c


def non_finite(seed):
    """The 160 x 120 ring (5 views, 4 sources) with 1 % NaN depths, 0.5 % each of +inf, -inf, -0.0, 1e-40 (denormal) and 1e30
    depths (projections past the int range), and 1 % NaN normals."""
    c = ring_case("non_finite", seed, 160, 120, 5, 4)
    rng = np.random.RandomState(seed + 1)
    for v in range(5):
        d, n = c.depths[v], c.normals[v]
        u = rng.rand(*d.shape)
        for lo, hi, val in ((0.0, 0.01, np.nan), (0.01, 0.015, np.inf), (0.015, 0.02, -np.inf), (0.02, 0.025, -0.0),
                            (0.025, 0.03, 1e-40), (0.03, 0.035, 1e30)):
            d[(u >= lo) & (u < hi)] = np.float32(val)
        n[rng.rand(*d.shape) < 0.01] = np.nan
    c.retag()
    return c


def _rig_views(W, H, rig):
    """[(K, R, c)] of tests/camera_space_cases.py as the view dicts of this module."""
    return [dict(K=K.astype(np.float32), R=R.reshape(9).astype(np.float32), t=(-R @ c).astype(np.float32), W=W, H=H) for K, R, c in rig]


def _world_normals(c, seed):
    """_ring_maps turns (0, 0, -1) of each CAMERA into the world frame, which agrees between views only while their optical axes are
    near parallel (the ring).  Here every view gets the normal of one world direction, the ring's optical axis, with the same noise."""
    rng = np.random.RandomState(seed)
    for v in range(c.num_views):
        n = np.zeros(c.depths[v].shape + (3,), np.float64)
        n[..., 2] = -1.0
        n[..., 0] = 0.01 * rng.standard_normal(c.depths[v].shape)
        c.normals[v] = np.ascontiguousarray((n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32))


def projected_z(c, i, j):
    """Camera-frame z in view j of every pixel of view i with a depth above zero (float64)."""
    vi, vj = c.views[i], c.views[j]
    K, R, t = vi["K"].astype(np.float64), vi["R"].astype(np.float64).reshape(3, 3), vi["t"].astype(np.float64)
    ys, xs = np.nonzero(c.depths[i] > 0)
    d = c.depths[i][ys, xs].astype(np.float64)
    world = (np.stack([(xs - K[2]) / K[0] * d, (ys - K[5]) / K[4] * d, d], -1) - t) @ R
    return world @ vj["R"].astype(np.float64).reshape(3, 3)[2] + float(vj["t"][2])


ROLLED_VIEWS = (0, 1)   # of rolled_aniso; first in the list, so that no other view has consumed their pixels before them


def rolled_aniso(seed):
    """96 x 72, 5 views of the ring's scene, every view a source of every other: view 0 rolled by 90 degrees, view 1 rolled with
    fy = 0.5 fx and the principal point at (0.3 W, 0.7 H), view 2 the upright ring camera, view 3 fy = 0.5 fx, view 4 the principal
    point at (0.7 W, 0.25 H).  The off-centre views are aimed so that the target still lands on their frame centre."""
    import camera_space_cases as cc
    W, H = 96, 72
    mid = (0.5 * W, 0.5 * H)
    f = cc.focal(W)
    rig = [cc.ring_source(W, H, 1, roll=90.0),
           cc.ring_source(W, H, 2, K=cc.intrinsics(W, H, fx=1.2 * f, fy=0.6 * f, cx=0.3 * W, cy=0.7 * H), roll=90.0, pixel=mid),
           cc.reference_view(W, H),
           cc.ring_source(W, H, 3, K=cc.intrinsics(W, H, fx=1.2 * f, fy=0.6 * f)),
           cc.ring_source(W, H, 4, K=cc.intrinsics(W, H, cx=0.7 * W, cy=0.25 * H), pixel=mid)]
    c = ring_case("rolled_aniso", seed, W, H, 5, 4, views=_rig_views(W, H, rig))
    _world_normals(c, seed + 1)
    return c


BEHIND_PART, BEHIND_ALL = 3, 4   # of source_behind: the views that have part of the cloud, and all of it, behind them


def source_behind(seed):
    """96 x 72, 5 views, every view a source of every other: three ring cameras, one camera between the ring and the nearer plane that
    looks along the surface (part of the others' points have z <= 0 in it) and one that faces away (every point has z < 0 in it, and
    its own rays meet no surface: its depth map is zero)."""
    import camera_space_cases as cc
    W, H = 96, 72
    rig = cc.rig_behind(W, H)
    rig = rig[:2] + [cc.ring_source(W, H, 2)] + rig[2:]
    c = ring_case("source_behind", seed, W, H, 5, 4, views=_rig_views(W, H, rig), tags=("source_behind",))
    _world_normals(c, seed + 1)
    for d in c.depths:
        d[d > 1e6] = 0.0   # rays that meet no surface
    c.retag()
    return c


# group: which test of test_gpu_fusion_scale.py runs the case
CASES = {
    "full_frame": ("full_frame", lambda: full_frame(5)),
    "full_frame_long_carry": ("full_frame", lambda: full_frame(5, long_carry=True)),
    "blocks_512x512": ("boundary", lambda: block_boundary(11, 512, 512)),
    "blocks_641x409": ("boundary", lambda: block_boundary(12, 641, 409)),
    "blocks_1024x513": ("boundary", lambda: block_boundary(13, 1024, 513)),
    "tiny_1x1": ("generated", lambda: tiny(21, 1, 1)),
    "tiny_300x1": ("generated", lambda: tiny(22, 300, 1)),
    "tiny_1x300": ("generated", lambda: tiny(23, 1, 300)),
    "tiny_9x7": ("generated", lambda: tiny(24, 9, 7)),
    "tiny_16x16": ("generated", lambda: tiny(25, 16, 16)),
    "sources_0": ("generated", lambda: few_sources(31, 0)),
    "sources_1": ("generated", lambda: few_sources(32, 1)),
    "sources_2": ("generated", lambda: few_sources(33, 2)),
    "sources_31": ("generated", lambda: many_sources(34, 31)),
    "sources_32": ("generated", lambda: many_sources(35, 32)),
    "source_lists": ("generated", lambda: source_lists(41)),
    "mixed_sizes": ("generated", lambda: mixed_sizes(42)),
    "all_blocked": ("generated", lambda: all_blocked(43)),
    "rolled_aniso": ("generated", lambda: rolled_aniso(44)),
    "source_behind": ("generated", lambda: source_behind(45)),
    "non_finite": ("non_finite", lambda: non_finite(5)),
}

_cache = {}


def case(name):
    """The committed case `name` (built once per process)."""
    if name not in _cache:
        _cache[name] = CASES[name][1]()
    return _cache[name]


def names(group=None):
    return [k for k, (g, _) in CASES.items() if group is None or g == group]


def random_case(seed):
    """A small random case for tools/fusion_fuzz.py: a ring of random size, view count and source lists (shuffled, at times
    duplicated), extra holes and zero bands, colour or grey images, block masks or none, now and then a half-resolution view
    or non-finite depths."""
    rng = np.random.RandomState(5000 + seed)
    W, H = int(rng.randint(1, 400)), int(rng.randint(1, 300))
    V = int(rng.randint(2, 9))
    views = ring_views(W, H, V)
    if rng.rand() < 0.25 and V > 2 and W > 3 and H > 3:
        K = views[1]["K"].copy()
        K[[0, 2, 4, 5]] *= np.float32(0.5)
        views[1] = dict(views[1], K=K, W=W // 2, H=H // 2)
    pairs = []
    for i in range(V):
        p = [int(j) for j in rng.permutation([j for j in range(V) if j != i])[:int(rng.randint(0, V))]]
        if p and rng.rand() < 0.2:
            p.append(p[0])
        pairs.append(p)
    c = ring_case("random_%d" % seed, seed, W, H, V, 0, noise=float(rng.choice([0.0, 0.0003, 0.001, 0.004])), views=views, pairs=pairs)
    for v in range(V):
        d = c.depths[v]
        d[rng.rand(*d.shape) < rng.choice([0.0, 0.1, 0.4])] = 0.0
        if rng.rand() < 0.3:
            r0 = int(rng.randint(0, d.shape[0]))
            d[r0: r0 + int(rng.randint(1, d.shape[0] + 1))] = 0.0
        if rng.rand() < 0.15:
            u = rng.rand(*d.shape)
            d[u < 0.01] = np.nan
            d[(u >= 0.01) & (u < 0.02)] = np.inf
            d[(u >= 0.02) & (u < 0.03)] = 1e-40
    if rng.rand() < 0.5:
        c.images = [np.ascontiguousarray(np.stack([im, 255.0 - im, np.roll(im, 5, 0)], -1), np.float32) for im in c.images]
    if rng.rand() < 0.4:
        c.blocks = [None if rng.rand() < 0.3 else (rng.rand(*d.shape) < 0.7).astype(np.uint8) * 255 for d in c.depths]
    c.retag()
    return c
