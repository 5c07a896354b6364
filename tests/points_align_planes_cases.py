"""The clouds of the point-to-plane alignment tests (test_points_align_planes.py, test_gpu_points_align_planes.py): surfaces with
analytic normals, sampled twice, and the pairs of test_points_align.py dressed with normals.  Everything is made in binary64
and rounded to binary32 once."""
import numpy as np

from test_points_align import PLANTED_RADIUS, align_cases, moved_back, rotation

SURFACE_RADIUS = 0.5
BUMPS = np.float64([[2.0, 0.0, 0.0, 0.10], [0.0, -1.5, 0.0, -0.08], [0.0, 0.0, 1.2, 0.12], [1.2, 1.0, 0.4, 0.07], [-1.3, 0.6, -0.7, -0.06]])
AXES = np.float64([2.0, 1.5, 1.2])
BUMP_WIDTH = 0.6


def surface_value(x):
    """F of the implicit surface F(x) = 1: the ellipsoid with the half-axes 2, 1.5, 1.2 plus five Gaussian bumps and dents of
    width 0.6; and its gradient."""
    value = ((x / AXES) ** 2).sum(axis=1)
    gradient = 2.0 * x / AXES ** 2
    for cx, cy, cz, height in BUMPS:
        d = x - np.float64([cx, cy, cz])
        bell = height * np.exp(-(d * d).sum(axis=1) / BUMP_WIDTH ** 2)
        value = value - bell                      # a positive height pushes the surface outwards
        gradient = gradient + (2.0 / BUMP_WIDTH ** 2) * d * bell[:, None]
    return value, gradient


def surface_sample(n, seed):
    """n points of the surface along random directions from the origin -- F grows along every ray, so bisection finds the one
    crossing -- and their unit normals: (xyz float32 [n, 3], normal float32 [n, 3]).  The normal is that of the binary64 point."""
    rng = np.random.default_rng(seed)
    direction = rng.normal(size=(n, 3))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    lo, hi = np.full(n, 0.5), np.full(n, 3.0)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        inside = surface_value(direction * mid[:, None])[0] < 1.0
        lo, hi = np.where(inside, mid, lo), np.where(inside, hi, mid)
    x = direction * (0.5 * (lo + hi))[:, None]
    gradient = surface_value(x)[1]
    return x.astype(np.float32), (gradient / np.linalg.norm(gradient, axis=1, keepdims=True)).astype(np.float32)


def ellipsoid_case(n_q=800, n_p=700, degrees=2.0, shift=0.05):
    """Q: n_q points of the surface with their normals; P: ANOTHER sample of n_p points of it, moved by the inverse of R (`degrees`
    about (1, 2, 3)) and t (`shift` per axis), so that (R, t) brings P back onto the surface.  (P, Q, Q's normals, radius, R, t)."""
    q, normal = surface_sample(n_q, 11)
    x = surface_sample(n_p, 12)[0]
    R, t = rotation(degrees), np.full(3, shift)
    return moved_back(x, 1.0, R, t), q, normal, SURFACE_RADIUS, R, t


def plane_case():
    """A sampled plane z = 0 with the normal (0, 0, 1): the columns of rotation about z and of the two translations in the plane
    are exactly zero.  P is another sample, 0.02 above it."""
    rng = np.random.default_rng(13)
    q = np.concatenate([rng.uniform(-2, 2, (500, 2)), np.zeros((500, 1))], axis=1).astype(np.float32)
    p = np.concatenate([rng.uniform(-2, 2, (400, 2)), np.full((400, 1), 0.02)], axis=1).astype(np.float32)
    return p, q, np.tile(np.float32([0, 0, 1]), (500, 1)), 0.5


def sphere_case():
    """A sphere of radius 1.5 about the origin, sampled in antipodal pairs so that the centre of the matches is the sphere's, with
    radial normals; P is Q blown up by 2 %: every point is matched to the one it came from and lies on its normal, so that no
    rotation changes a residual."""
    rng = np.random.default_rng(14)
    d = rng.normal(size=(300, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    half = (1.5 * d).astype(np.float32)
    q = np.concatenate([half, -half])
    normal = np.concatenate([d, -d]).astype(np.float32)
    return (q.astype(np.float64) * 1.02).astype(np.float32), q, normal, 0.5


def cylinder_case():
    """A cylinder of radius 1 along z, 3 long, with its radial normals: the column of the translation along z is exactly zero.  P is
    another sample of a cylinder of radius 1.01, shifted by 0.03 along x."""
    rng = np.random.default_rng(15)

    def sample(n, radius):
        phi, z = rng.uniform(0, 2 * np.pi, n), rng.uniform(-1.5, 1.5, n)
        return np.stack([radius * np.cos(phi), radius * np.sin(phi), z], axis=1), np.stack([np.cos(phi), np.sin(phi), np.zeros(n)], axis=1)
    q, normal = sample(700, 1.0)
    p = sample(600, 1.01)[0] + np.float64([0.03, 0, 0])
    return p.astype(np.float32), q.astype(np.float32), normal.astype(np.float32), 0.5


DEGENERATE_CASES = {"plane": plane_case, "sphere": sphere_case, "cylinder": cylinder_case}


def bad_normals_case():
    """The ellipsoid pair with every fifth normal of Q replaced in turn by zero, NaN, +Inf, -Inf in one component, and a normal of
    length 1e-20 (usable: its square is a positive binary64 number) and of length 1e18 (usable too)."""
    p, q, normal, radius = ellipsoid_case()[:4]
    normal = normal.copy()
    bad = np.float32([[0, 0, 0], [np.nan, 0, 1], [np.inf, 0, 0], [0, -np.inf, 0]])
    for k, j in enumerate(range(0, len(q), 5)):
        if k % 6 < 4:
            normal[j] = bad[k % 6]
        else:
            normal[j] = normal[j] * np.float32(1e-20 if k % 6 == 4 else 1e18)
    return p, q, normal, radius


def usable(normal):
    """Which stored normals the contract takes: a squared length, in binary64, that is finite and > 0."""
    with np.errstate(invalid="ignore", over="ignore"):
        s = (normal.astype(np.float64) ** 2).sum(axis=1)
    return np.isfinite(s) & (s > 0.0)


def few_usable_case(count):
    """Eight points of the surface, spread over it, each matched by a point 0.05 along its normal; `count` of the eight normals
    are usable, the others zero."""
    q, normal = surface_sample(8, 16)
    p = (q.astype(np.float64) + 0.05 * normal.astype(np.float64)).astype(np.float32)
    normal = normal.copy()
    normal[count:] = 0.0
    return p, q, normal, SURFACE_RADIUS


def last_chunk_case():
    """257 points of which only the last, alone in the second chunk of 256, is matched -- and a second P of 264 whose last eight
    are: the only usable matches stand in the last chunk."""
    q, normal = surface_sample(800, 11)
    far = np.full((264, 3), 40, np.float32) + np.arange(264, dtype=np.float32)[:, None]
    one, eight = far[:257].copy(), far.copy()
    one[256] = q[5] + np.float32(0.05)
    eight[256:] = q[[5, 100, 333, 400, 512, 640, 700, 777]] + np.float32([0.05, -0.05, 0.1])
    return one, eight, q, normal


def dressed_normals(q, seed):
    """Normals for a cloud that has none: random directions, every seventh of them zero and every eleventh NaN."""
    rng = np.random.default_rng(seed)
    normal = rng.normal(size=(len(q), 3)).astype(np.float32)
    normal[::7] = 0.0
    normal[3::11, 1] = np.nan
    return normal


def plane_cases(pkg):
    """name -> (P, Q, Q's normals, radius, origin): the pairs of align_cases(pkg) dressed with normals, and the ones made here."""
    out = {}
    for k, (name, (p, q, radius, origin)) in enumerate(align_cases(pkg).items()):
        out[name] = (p, q, dressed_normals(q, 100 + k), radius, origin)
    p, q, normal, radius = ellipsoid_case()[:4]
    out["ellipsoid"] = (p, q, normal, radius, None)
    out["ellipsoid onto itself"] = (q, q, normal, radius, None)
    out["ellipsoid, another origin"] = (p, q, normal, 0.45, [0.1, -0.2, 0.05])
    for name, make in DEGENERATE_CASES.items():
        out[name] = make() + (None,)
    out["bad normals"] = bad_normals_case() + (None,)
    one, eight, q, normal = last_chunk_case()
    out["one match in the last chunk, planes"] = (one, q, normal, SURFACE_RADIUS, None)
    out["eight matches in the last chunk"] = (eight, q, normal, SURFACE_RADIUS, None)
    for count in (5, 6):
        out["%d usable" % count] = few_usable_case(count) + (None,)
    return out
