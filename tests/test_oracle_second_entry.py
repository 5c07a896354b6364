"""Double entry for the control-flow-heavy stages of the path.  The reference ships no tests or vectors and cannot be built
here, so the oracle (oracle/apd_oracle.c) is pinned by inspection only.  This file is a SECOND restatement of eleven stages,
written from the reference's text (APD.cu line numbers below) and not from the oracle's: plain Python over numpy binary32
scalars, one statement per statement.  It shares with the oracle only leaf functions that have their own independent checks --
the NCC / geometric cost of one (pixel, view, plane) (tests/test_oracle_float64.py), the XORWOW stream (tests/test_rng.py,
pinned to rocRAND) and the polynomial exp of the arithmetic contract -- and must reproduce the oracle's state BIT FOR BIT:

  * adaptive checkerboard arm search + multi-hypothesis joint view selection of CheckerboardPropagationStrong
    (APD.cu:1012-1259): the view weights of every pixel of a colour;
  * GenNeighbours, K3 (APD.cu:1750-1969): neighbour table, reliability flags and the random state it leaves behind, and
    NeigbourUpdate, K4 (:1971-1987);
  * the peak classifier of DepthToWeak, K14 (APD.cu:1990-2143): the weak map;
  * RANSACToGetFitPlane, K8 (APD.cu:2272-2384): the fit planes and the random state it leaves behind;
  * LocalRefine, K15 (APD.cu:2146-2232): the depths it adopts;
  * FindNearestStrongPoint, K2 (APD.cu:2234-2270), and GetDepthandNormal + the two median-filter launches, K11-K13
    (APD.cu:1587-1748) with the HALF launch geometry of RunPatchMatch (:2400-2407) on a frame of odd height;
  * the rest of CheckerboardPropagationStrong (APD.cu:1260-1321) with PlaneHypothesisRefinementStrong and its random and
    perturbed hypotheses (:211-273, :837-890): planes, costs, selected views and random streams after K6 / K7;
  * RandomInitialization, K5 (APD.cu:807-835) with both initial-cost functions (:616-693; `unSetBit` clears the bit and
    everything below it, :46-49);
  * CheckerboardPropagationWeak with PlaneHypothesisRefinementWeak, K9 / K10 (APD.cu:1323-1508, :892-980), photometric and with
    the geometric term: planes, costs, view weights, selected views and random streams of the WEAK pixels.

Two independent transcriptions that agree on every bit do not prove either right, but a slip in one of them (a swapped arm,
a `<` for a `<=`, a draw out of order) shows up here."""
import ctypes as C
import math

import numpy as np

import pytest

import camera_space_cases as cc
import common

f32 = np.float32


def ring_scene(synth):
    """scene(W, H, N, seed, textureless) -> (scene, images) on synth's ring: what every stage's own test runs on."""
    return lambda W, H, N, seed=1, textureless=0.0: common.scene_inputs(synth, W, H, N, seed=seed, textureless=textureless)


def rig_scene(synth, rig):
    """The same on a rig of tests/camera_space_cases.py with N sources, rendered at the size, seed and textureless share asked for."""
    def scene(W, H, N, seed=1, textureless=0.0):
        sc, _ = cc.make_scene(synth, W, H, cc.general_rig(rig, W, H, N), seed=seed, textureless=textureless)
        return sc, sc.images_numpy()
    return scene


def populated(strict, ring_bounds, some):
    """The non-vacuity of a stage: on the ring (strict) the counts meet the bounds set for synth's scenes; on another rig, whose
    scenes hold other shares of WEAK and moving pixels, each branch the bounds are about must still occur at all."""
    return ring_bounds if strict else some


FLT_EPSILON = f32(1.1920929e-07)
FLT_MAX = f32(3.4028234663852886e38)
WEAK, STRONG, UNKNOWN = 0, 1, 2


# ---- leaves shared with the oracle (each has its own independent test) ----------------------------------------------------

class Rng:
    """curand / curand_uniform on one pixel's XORWOW state (6 words: x0..x4, d)."""

    def __init__(self, ob, words):
        self.L = ob.lib()
        self.state = (C.c_uint32 * 6)(*[int(w) for w in words])

    def next(self):
        return int(self.L.orc_xorwow_next(self.state))

    def uniform(self):
        return f32(self.L.orc_xorwow_uniform(self.state))

    def words(self):
        return np.array(list(self.state), np.uint32)


def expf(ob, x):
    return f32(ob.lib().orc_expf(C.c_float(float(x))))


# ---- small device helpers, APD.cu:29-142 ----------------------------------------------------------------------------------

def is_set(v, n):  # :52-55
    return (int(v) >> n) & 1


def normalize2(x, y):  # :136-142, rsqrtf := 1 / sqrtf (contract C4)
    inv = f32(1.0) / np.sqrt(f32(x * x + y * y))
    return f32(x * inv), f32(y * inv)


def normalize3(x, y, z):  # :128-134
    inv = f32(1.0) / np.sqrt(f32(f32(x * x + y * y) + z * z))
    return f32(x * inv), f32(y * inv), f32(z * inv)


def point_in_triangle(A, B, Cc, P):  # :91-112, short2 / int2 arguments
    ABx, ABy = f32(B[0] - A[0]), f32(B[1] - A[1])
    BCx, BCy = f32(Cc[0] - B[0]), f32(Cc[1] - B[1])
    CAx, CAy = f32(A[0] - Cc[0]), f32(A[1] - Cc[1])
    ab = np.sqrt(f32(ABx * ABx + ABy * ABy))
    bc = np.sqrt(f32(BCx * BCx + BCy * BCy))
    ca = np.sqrt(f32(CAx * CAx + CAy * CAy))
    if ab <= 2 or bc <= 2 or ca <= 2:
        return False
    if not (f32(ab + bc) > ca and f32(bc + ca) > ab and f32(ab + ca) > bc):
        return False
    PAx, PAy = f32(A[0] - P[0]), f32(A[1] - P[1])
    PBx, PBy = f32(B[0] - P[0]), f32(B[1] - P[1])
    PCx, PCy = f32(Cc[0] - P[0]), f32(Cc[1] - P[1])
    t1 = f32(PAx * PBy - PAy * PBx)
    t2 = f32(PBx * PCy - PBy * PCx)
    t3 = f32(PCx * PAy - PCy * PAx)
    return bool(f32(t1 * t2) >= 0 and f32(t1 * t3) >= 0)


def get_3d_point(K, px, py, depth):  # :159-172
    depth = f32(depth)
    return (f32(f32(depth * f32(f32(px) - K[2])) / K[0]), f32(f32(depth * f32(f32(py) - K[5])) / K[4]), depth)


def distance_to_origin(K, px, py, depth, n):  # :186-192
    X = get_3d_point(K, px, py, depth)
    return f32(-f32(f32(f32(n[0] * X[0]) + f32(n[1] * X[1])) + f32(n[2] * X[2])))


def normal_to_ref_cam(R, p):  # TransformNormal2RefCam, :383-392
    return (f32(f32(f32(R[0] * p[0]) + f32(R[1] * p[1])) + f32(R[2] * p[2])),
            f32(f32(f32(R[3] * p[0]) + f32(R[4] * p[1])) + f32(R[5] * p[2])),
            f32(f32(f32(R[6] * p[0]) + f32(R[7] * p[1])) + f32(R[8] * p[2])), f32(p[3]))


# ---- stage 1: arm search + joint view selection, APD.cu:1012-1259 ---------------------------------------------------------

def arm_search(costs, W, H, px, py):
    """positions[8] and flag[8] in the reference's order: 0 up_near, 1 up_far, 2 down_near, 3 down_far, 4 left_near,
    5 left_far, 6 right_near, 7 right_far (:1020); every probe is `costs[q] < costMin` on the flat index."""
    c = costs.reshape(-1)
    center = py * W + px
    pos = [center - W, center - 3 * W, center + W, center + 3 * W, center - 1, center - 3, center + 1, center + 3]
    flag = [False] * 8

    def scan(first, probes):
        best, cmin = first, c[first]
        for ok, q in probes:
            if ok and c[q] < cmin:
                cmin, best = c[q], q
        return best

    if py > 2:  # up_far :1021-1038
        flag[1] = True
        pos[1] = scan(pos[1], [(py > 2 + 2 * i, center - 3 * W - 2 * i * W) for i in range(1, 11)])
    if py < H - 3:  # down_far :1040-1057
        flag[3] = True
        pos[3] = scan(pos[3], [(py < H - 3 - 2 * i, center + 3 * W + 2 * i * W) for i in range(1, 11)])
    if px > 2:  # left_far :1059-1076
        flag[5] = True
        pos[5] = scan(pos[5], [(px > 2 + 2 * i, center - 3 - 2 * i) for i in range(1, 11)])
    if px < W - 3:  # right_far :1078-1095
        flag[7] = True
        pos[7] = scan(pos[7], [(px < W - 3 - 2 * i, center + 3 + 2 * i) for i in range(1, 11)])
    if py > 0:  # up_near :1097-1121
        flag[0] = True
        probes = []
        for i in range(3):
            probes.append((py > 1 + i and px > i, center - W - (1 + i) * W - (1 + i)))
            probes.append((py > 1 + i and px < W - 1 - i, center - W - (1 + i) * W + (1 + i)))
        pos[0] = scan(pos[0], probes)
    if py < H - 1:  # down_near :1123-1147
        flag[2] = True
        probes = []
        for i in range(3):
            probes.append((py < H - 2 - i and px > i, center + W + (1 + i) * W - (1 + i)))
            probes.append((py < H - 2 - i and px < W - 1 - i, center + W + (1 + i) * W + (1 + i)))
        pos[2] = scan(pos[2], probes)
    if px > 0:  # left_near :1149-1173
        flag[4] = True
        probes = []
        for i in range(3):
            probes.append((px > 1 + i and py > i, center - 1 - (1 + i) - (1 + i) * W))
            probes.append((px > 1 + i and py < H - 1 - i, center - 1 - (1 + i) + (1 + i) * W))
        pos[4] = scan(pos[4], probes)
    if px < W - 1:  # right_near :1175-1199
        flag[6] = True
        probes = []
        for i in range(3):
            probes.append((px < W - 2 - i and py > i, center + 1 + (1 + i) - (1 + i) * W))
            probes.append((px < W - 2 - i and py < H - 1 - i, center + 1 + (1 + i) + (1 + i) * W))
        pos[6] = scan(pos[6], probes)
    return pos, flag


def view_weights_of_pixel(ob, o, snap, W, H, nsrc, px, py, it):
    return view_selection_of_pixel(ob, o, snap, W, H, nsrc, px, py, it)[0]


def view_selection_of_pixel(ob, o, snap, W, H, nsrc, px, py, it):
    """(view weights, arm positions, arm flags, the 8 x 32 cost table, the pixel's random stream after its 15 draws)"""
    costs, planes, sel, rng_words = snap
    pos, flag = arm_search(costs, W, H, px, py)
    cost_array = np.zeros((8, 32), np.float32)
    cost_array[0, 0] = f32(2.0)  # `= { 2.0f }` sets one element (:1004)
    flat_planes = planes.reshape(-1, 4)
    for a in range(8):
        if flag[a]:
            for v in range(nsrc):  # ComputeMultiViewCostVectorOld :696-705
                cost_array[a, v] = f32(o.ncc_old(px, py, v + 1, flat_planes[pos[a]]))
    center = py * W + px
    priors = np.zeros(32, np.float32)
    nb = [center - W, center + W, center - 1, center + 1]
    flat_sel = sel.reshape(-1)
    for i in range(4):  # :1210-1222
        if flag[2 * i]:
            for j in range(nsrc):
                priors[j] = f32(priors[j] + (f32(0.9) if is_set(flat_sel[nb[i]], j) == 1 else f32(0.1)))
    probs = np.zeros(32, np.float32)
    thr = f32(0.8 * float(expf(ob, f32(it * it) / f32(-90.0))))  # double product, then float (:1225)
    for i in range(nsrc):
        count, count_false, tmpw = f32(0), 0, f32(0)
        for j in range(8):
            cij = cost_array[j, i]
            if cij < thr:
                tmpw = f32(tmpw + expf(ob, f32(f32(cij * cij) / f32(-0.18))))
                count = f32(count + f32(1))
            if cij > f32(1.2):
                count_false += 1
        if count > 2 and count_false < 3:
            probs[i] = f32(tmpw / count)
        elif count_false < 3:
            probs[i] = expf(ob, f32(f32(thr * thr) / f32(-0.32)))
        probs[i] = f32(probs[i] * priors[i])
    with np.errstate(divide="ignore", invalid="ignore"):  # TransformPDFToCDF :143-157; a zero sum gives inf / NaN like the device
        s = f32(0)
        for i in range(nsrc):
            s = f32(s + probs[i])
        inv = f32(1.0) / s
        cum = f32(0)
        for i in range(nsrc):
            cum = f32(cum + f32(probs[i] * inv))
            probs[i] = cum
    rng = Rng(ob, rng_words[py, px])
    weights = np.zeros(32, np.uint8)
    for _ in range(15):  # :1249-1259
        rand_prob = f32(rng.uniform() - FLT_EPSILON)
        for v in range(nsrc):
            if probs[v] > rand_prob:
                weights[v] += 1
                break
    return weights, pos, flag, cost_array, rng


def test_arm_search_and_view_selection(synth, ob):
    _check_arm_search_and_view_selection(ob, ring_scene(synth))


def _check_arm_search_and_view_selection(ob, scene, strict=True):
    W, H, N = 40, 30, 3
    sc, imgs = scene(W, H, N, seed=21)
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
                    want = view_weights_of_pixel(ob, o, snap, W, H, N, px, py, it)
                    assert np.array_equal(got[py, px], want), (it, colour, px, py, got[py, px][:N], want[:N])
                    checked += 1
    assert checked == 2 * W * H
    o.close()


# ---- stage 2: GenNeighbours, APD.cu:1750-1969 -----------------------------------------------------------------------------

def to_short(v):
    """float -> short2 member: truncation toward zero (values stay far inside the short range here)."""
    return int(np.trunc(v))


def gen_neighbours_pixel(ob, W, H, K, params, weak, nearest, planes, rng_words, px, py):
    """Returns (neighbours[9] as (x, y), reliable, rng words after) for one WEAK pixel."""
    rng = Rng(ob, rng_words[py, px])
    min_margin = 6
    depth_diff = f32(f32(params["depth_max"]) - f32(params["depth_min"]))
    rotate_time = params["rotate_time"]
    angle = f32(f32(45.0) / f32(rotate_time))
    cos_angle = f32(math.cos(float(angle) * math.pi / float(f32(180.0))))
    sin_angle = f32(math.sin(float(angle) * math.pi / float(f32(180.0))))
    threshold = f32(math.cos(float(f32(angle / f32(2.0))) * math.pi / float(f32(180.0))))
    shift_range = max(int(math.tan(float(f32(angle / f32(2.0))) * math.pi / float(f32(180.0))) * 20), 1)
    ransac_threshold = f32(params["ransac_threshold"])
    strong = [(-1, -1)] * 32
    valid = [False] * 32
    dir_index0 = -1
    found = 0

    def shift():  # (curand() % 2 == 0 ? 1 : -1) * curand() % shift_range, unsigned; sign draw first (contract C8)
        sign = 1 if rng.next() % 2 == 0 else 0xFFFFFFFF
        mag = rng.next()
        return ((sign * mag) & 0xFFFFFFFF) % shift_range

    for ox in (-1, 0, 1):
        for oy in (-1, 0, 1):
            if ox == 0 and oy == 0:
                continue
            dx, dy = normalize2(f32(ox), f32(oy))
            dir_index0 += 1
            for rot in range(rotate_time):
                slot = dir_index0 * 4 + rot
                radius = 2
                while radius <= 4096:
                    tx, ty = f32(f32(px) + f32(dx * f32(radius))), f32(f32(py) + f32(dy * f32(radius)))
                    if tx < 0 or ty < 0 or tx >= W or ty >= H:
                        break
                    for _ in range(4):
                        sx = shift()
                        sy = shift()
                        ddx, ddy = normalize2(f32(f32(dx * f32(20)) + f32(sx)), f32(f32(dy * f32(20)) + f32(sy)))
                        qx, qy = to_short(f32(f32(px) + f32(ddx * f32(radius)))), to_short(f32(f32(py) + f32(ddy * f32(radius))))
                        if qx < min_margin or qy < min_margin or qx >= W - min_margin or qy >= H - min_margin:
                            continue
                        if weak[qy, qx] != STRONG:
                            qx, qy = int(nearest[qy, qx, 0]), int(nearest[qy, qx, 1])
                            if qx == -1 or qy == -1:
                                continue
                        tdx, tdy = normalize2(f32(qx - px), f32(qy - py))
                        ca = f32(f32(tdx * dx) + f32(tdy * dy))
                        if ca > threshold:
                            strong[slot] = (qx, qy)
                            valid[slot] = True
                            found += 1
                            break
                    if valid[slot]:
                        break
                    radius = min(radius * 2, radius + 25)
                rx = f32(f32(dx * cos_angle) - f32(dy * sin_angle))
                ry = f32(f32(dx * sin_angle) + f32(dy * cos_angle))
                dx, dy = normalize2(rx, ry)
    out = [(-1, -1)] * 9
    out[0] = (px, py)
    if found <= 3:
        return out, 0, rng.words()
    center3 = get_3d_point(K, px, py, planes[py, px, 3])  # .w still holds the DEPTH before K5 (:1866)
    pts, pts3 = [], []
    for i in range(32):
        if valid[i]:
            q = strong[i]
            pts.append(q)
            pts3.append(get_3d_point(K, q[0], q[1], planes[q[1], q[0], 3]))
    n = len(pts)
    pts = pts + [(-1, -1)] * (32 - n)
    best, use, has_plane = None, (-1, -1, -1), False
    min_cost, max_count = FLT_MAX, 3

    def plane_dist(pl, P):
        return np.abs(f32(f32(f32(f32(pl[0] * P[0]) + f32(pl[1] * P[1])) + f32(pl[2] * P[2])) + pl[3]))

    for _ in range(50):
        a = rng.next() % n
        b = rng.next() % n
        c = rng.next() % n
        if a == b or b == c or a == c:
            continue
        if not point_in_triangle(pts[a], pts[b], pts[c], (px, py)):
            continue
        A, B, Cc = pts3[a], pts3[b], pts3[c]
        ACx, ACy, ACz = f32(A[0] - Cc[0]), f32(A[1] - Cc[1]), f32(A[2] - Cc[2])
        BCx, BCy, BCz = f32(B[0] - Cc[0]), f32(B[1] - Cc[1]), f32(B[2] - Cc[2])
        nx = f32(f32(ACy * BCz) - f32(BCy * ACz))
        ny = f32(-f32(f32(ACx * BCz) - f32(BCx * ACz)))
        nz = f32(f32(ACx * BCy) - f32(BCx * ACy))
        if (nx == 0 and ny == 0 and nz == 0) or np.isnan(nx) or np.isnan(ny) or np.isnan(nz):
            continue
        nx, ny, nz = normalize3(nx, ny, nz)
        nw = f32(-f32(f32(f32(nx * A[0]) + f32(ny * A[1])) + f32(nz * A[2])))
        pl = (nx, ny, nz, nw)
        count = 0
        for k in range(n):
            if f32(plane_dist(pl, pts3[k]) / depth_diff) < ransac_threshold:
                count += 1
        if count < 6:
            continue
        if count > max_count:
            max_count = count
            min_cost = plane_dist(pl, center3)
            best, use, has_plane = pl, (a, b, c), True
        elif count == max_count:
            cd = plane_dist(pl, center3)
            if cd < min_cost:
                min_cost = cd
                best, use = pl, (a, b, c)
    if not has_plane:
        return out, 0, rng.words()
    weight = [f32(0)] * n
    for i in range(n):
        d = plane_dist(best, pts3[i])
        if f32(d / depth_diff) >= ransac_threshold:
            pts[i] = (-1, -1)
            weight[i] = FLT_MAX
            continue
        if i in use:
            d = f32(d - f32(1))
        weight[i] = d
    for i in range(1, n):  # sort_small_weighted :14-27
        tmp, tw = pts[i], weight[i]
        j = i
        while j >= 1 and tw < weight[j - 1]:
            pts[j], weight[j] = pts[j - 1], weight[j - 1]
            j -= 1
        pts[j], weight[j] = tmp, tw
    for i in range(1, 9):
        out[i] = pts[i - 1]
    return out, 1, rng.words()


def _apd_oracle(scene, ob, W, H, N, seed):
    """A REFINE_INIT + APD oracle whose prior comes from a complete FIRST_INIT pass of the same scene."""
    sc, imgs = scene(W, H, N, seed=seed, textureless=0.3)
    p0 = common.base_params(sc, N, seed=5, max_iterations=2, weak_peak_radius=6)
    o0 = common.make_oracle(ob, sc, imgs, N, p0)
    o0.run()
    prior = common.postprocess(o0.planes.copy(), o0.weak_info.copy(), o0.selected_views.copy(), f32(p0["depth_min"]), f32(p0["depth_max"]))
    o0.close()
    p1 = common.base_params(sc, N, seed=6, max_iterations=1, state=1, use_APD=1, weak_peak_radius=6, rotate_time=2, ransac_threshold=0.00875)
    return sc, p1, common.make_oracle(ob, sc, imgs, N, p1, prior=prior)


def test_gen_neighbours(synth, ob):
    _check_gen_neighbours(ob, ring_scene(synth))


def _check_gen_neighbours(ob, scene, strict=True):
    W, H, N = 128, 96, 3   # a textureless region wide enough for the radius sequence to leave its doubling phase (57, 82, ...)
    sc, p1, o = _apd_oracle(scene, ob, W, H, N, seed=12)
    for kid in (1, 2):
        o.run_kernel(kid)
    weak = o.weak_info.copy()
    assert (weak == WEAK).sum() > populated(strict, 40, 0), "the scene must have a textureless region"
    snap = dict(weak=weak, nearest=o.nearest_strong.copy(), planes=o.planes.copy(), rng=o.rng.copy())
    nmap = o.neighbours_map.copy()
    o.run_kernel(3)
    K = [f32(v) for v in sc.K[0].reshape(-1)]
    nb, reliable, rng_after = o.neighbours, o.weak_reliable, o.rng
    n_reliable = 0
    for py in range(H):
        for px in range(W):
            if weak[py, px] != WEAK:
                assert np.array_equal(rng_after[py, px], snap["rng"][py, px])
                continue
            want_nb, want_rel, want_rng = gen_neighbours_pixel(ob, W, H, K, p1, snap["weak"], snap["nearest"], snap["planes"], snap["rng"], px, py)
            row = nb[nmap[py, px]]
            assert [tuple(int(v) for v in q) for q in row] == want_nb, (px, py, row.tolist(), want_nb)
            assert int(reliable[py, px]) == want_rel, (px, py)
            assert np.array_equal(rng_after[py, px], want_rng), (px, py)
            n_reliable += want_rel
    assert n_reliable > populated(strict, 10, 0), "some pixels must get a full neighbour set, or the RANSAC half is not exercised"
    # NeigbourUpdate, K4 (:1971-1987): a WEAK pixel that K3 did not mark reliable becomes UNKNOWN
    ys, xs = np.nonzero(weak == WEAK)
    o.weak_reliable[ys[::3], xs[::3]] = 0   # every pixel of this scene found its neighbours: make a third of them unreliable
    rel = o.weak_reliable.copy()
    o.run_kernel(4)
    want_weak = np.where((weak == WEAK) & (rel != 1), UNKNOWN, weak).astype(np.uint8)
    assert np.array_equal(o.weak_info, want_weak) and (want_weak != weak).any()
    o.close()


def test_gen_neighbours_long_rays(synth, ob):
    """The same on a hand-made WEAK block 150 px wide: the rays leave the doubling phase of the radius sequence
    (2, 4, 8, 16, 32, 57, 82, ...; :1807) and run into the substitution by the nearest STRONG pixel; every 7th WEAK pixel."""
    _check_gen_neighbours_long_rays(ob, ring_scene(synth))


def _check_gen_neighbours_long_rays(ob, scene, strict=True):
    W, H, N = 200, 140, 2
    sc, imgs = scene(W, H, N, seed=4)
    p0 = common.base_params(sc, N, seed=5, max_iterations=1, weak_peak_radius=6)
    o0 = common.make_oracle(ob, sc, imgs, N, p0)
    o0.run()
    planes, views, weak0 = common.postprocess(o0.planes.copy(), o0.weak_info.copy(), o0.selected_views.copy(), f32(p0["depth_min"]), f32(p0["depth_max"]))
    o0.close()
    weak = np.where(weak0 == UNKNOWN, UNKNOWN, STRONG).astype(np.uint8)
    weak[20:120, 25:175] = WEAK
    weak[60:64, 90:96] = STRONG   # an island inside the block
    p1 = common.base_params(sc, N, seed=6, max_iterations=1, state=1, use_APD=1, weak_peak_radius=6, rotate_time=4, ransac_threshold=0.0075)
    o = common.make_oracle(ob, sc, imgs, N, p1, prior=(planes, views, weak))
    for kid in (1, 2):
        o.run_kernel(kid)
    snap = dict(weak=o.weak_info.copy(), nearest=o.nearest_strong.copy(), planes=o.planes.copy(), rng=o.rng.copy())
    nmap = o.neighbours_map.copy()
    o.run_kernel(3)
    K = [f32(v) for v in sc.K[0].reshape(-1)]
    nb, reliable, rng_after = o.neighbours, o.weak_reliable, o.rng
    checked = far = 0
    for py in range(H):
        for px in range(W):
            if snap["weak"][py, px] != WEAK or (px * 31 + py * 17) % 7 != 0:
                continue
            want_nb, want_rel, want_rng = gen_neighbours_pixel(ob, W, H, K, p1, snap["weak"], snap["nearest"], snap["planes"], snap["rng"], px, py)
            row = nb[nmap[py, px]]
            assert [tuple(int(v) for v in q) for q in row] == want_nb, (px, py, row.tolist(), want_nb)
            assert int(reliable[py, px]) == want_rel and np.array_equal(rng_after[py, px], want_rng), (px, py)
            checked += 1
            far += any(q[0] >= 0 and max(abs(q[0] - px), abs(q[1] - py)) > 45 for q in want_nb[1:])
    assert checked > 1500 and far > 100, (checked, far)
    o.close()


# ---- stage 3: DepthToWeak, APD.cu:1990-2143 -------------------------------------------------------------------------------

def depth_to_weak_pixel(o, cams_c, K, R, params, planes, sel, vweight, nsrc, W, H, px, py, geom):
    min_margin = 6
    if px < min_margin or py < min_margin or px >= W - min_margin or py >= H - min_margin:
        return UNKNOWN
    origin = normal_to_ref_cam(R, planes[py, px])
    origin_depth = origin[3]
    if origin_depth == 0:
        return UNKNOWN
    s = int(sel[py, px])
    vw = vweight[py, px]
    base_line, valid, weight_normal = f32(0), 0, f32(0)
    for v in range(nsrc):
        if is_set(s, v):
            cd = [f32(cams_c[0][k] - cams_c[v + 1][k]) for k in range(3)]
            tv = float(f32(f32(f32(cd[0] * cd[0]) + f32(cd[1] * cd[1])) + f32(cd[2] * cd[2])))  # float expression stored in a double (:2043)
            base_line = f32(base_line + f32(np.sqrt(f32(tv))))   # sqrtf(double) converts back to float first
            weight_normal = f32(weight_normal + f32(vw[v]))
            valid += 1
    if valid == 0:
        return UNKNOWN
    base_line = f32(base_line / f32(valid))
    disp = f32(f32(K[0] * base_line) / origin_depth)
    radius, n = 30, 61
    p_costs = [f32(0)] * n
    for p_disp in range(-radius, radius + 1):
        p_depth = f32(f32(K[0] * base_line) / f32(disp + f32(p_disp)))
        if p_depth < f32(params["depth_min"]) or p_depth > f32(params["depth_max"]):
            p_costs[p_disp + radius] = f32(2.0)
            continue
        pl = np.array([origin[0], origin[1], origin[2], distance_to_origin(K, px, py, p_depth, origin)], np.float32)
        p_cost = f32(0)
        for v in range(nsrc):
            if is_set(s, v):
                t = f32(0)
                t = f32(t + f32(o.ncc_old(px, py, v + 1, pl)))
                if geom:
                    t = f32(t + f32(f32(params["geom_factor"]) * f32(o.geom_cost(px, py, v + 1, pl))))
                p_cost = f32(p_cost + f32(t * f32(vw[v])))
        with np.errstate(divide="ignore", invalid="ignore"):
            p_cost = f32(p_cost / weight_normal)
        p_costs[p_disp + radius] = f32(2.0) if f32(2.0) < p_cost else p_cost   # MIN(2.0f, p_cost) = (a < b) ? a : b
    is_peak = [False] * n
    peak_count, min_peak, min_cost = 0, 0, f32(2.0)
    for i in range(2, n - 2):  # :2101-2110
        if p_costs[i - 1] > p_costs[i] and p_costs[i + 1] > p_costs[i]:
            is_peak[i] = True
            peak_count += 1
            if p_costs[i] < min_cost:
                min_peak, min_cost = i, p_costs[i]
    if abs(min_peak - radius) > params["weak_peak_radius"] or p_costs[min_peak] > f32(0.5):
        return WEAK
    if peak_count == 1:
        return STRONG if p_costs[min_peak] <= f32(0.15) else WEAK
    var = f32(0)
    for i in range(2, n - 2):
        if is_peak[i] and i != min_peak:
            d = f32(p_costs[i] - min_cost)
            var = f32(var + f32(d * d))
    var = f32(np.sqrt(var))
    var = f32(var / f32(peak_count - 1))
    return STRONG if var > f32(0.2) else WEAK


def test_depth_to_weak_classifier(synth, ob):
    _check_depth_to_weak_classifier(ob, ring_scene(synth))


def _check_depth_to_weak_classifier(ob, scene, strict=True):
    W, H, N = 56, 40, 3
    sc, imgs = scene(W, H, N, seed=14, textureless=0.25)
    for geom in (0, 1):
        kw = dict(seed=9, max_iterations=2, weak_peak_radius=4 if geom else 6)
        depths = None
        prior = None
        if geom:
            kw.update(state=2, geom_consistency=1)
            depths = common.fake_depth_maps(W, H, N + 1)
            o0 = common.make_oracle(ob, sc, imgs, N, common.base_params(sc, N, seed=3, max_iterations=2, weak_peak_radius=6))
            o0.run()
            p0 = common.base_params(sc, N)
            prior = common.postprocess(o0.planes.copy(), o0.weak_info.copy(), o0.selected_views.copy(), f32(p0["depth_min"]), f32(p0["depth_max"]))
            o0.close()
        params = common.base_params(sc, N, **kw)
        full = ob.default_params(**params)
        params["geom_factor"] = full.geom_factor
        o = common.make_oracle(ob, sc, imgs, N, params, depths=depths, prior=prior)
        for kid in (1, 2, 5):
            o.run_kernel(kid)
        o.run_sweeps(0, 2)
        for kid in (11, 12, 13):
            o.run_kernel(kid)
        planes, sel, vw = o.planes.copy(), o.selected_views.copy(), o.view_weight.copy()
        o.run_kernel(14)
        got = o.weak_info
        K = [f32(v) for v in sc.K[0].reshape(-1)]
        R = [f32(v) for v in sc.R[0].reshape(-1)]
        # Camera::c = -R^T t accumulated in double, stored as float (APD.cpp:75-77); ob.make_camera does the same
        cams_c = [[f32(v) for v in ob.make_camera(sc.K[i], sc.R[i], sc.t[i], W, H, sc.depth_min, sc.depth_max).c] for i in range(N + 1)]
        counts = [0, 0, 0]
        for py in range(H):
            for px in range(W):
                want = depth_to_weak_pixel(o, cams_c, K, R, params, planes, sel, vw, N, W, H, px, py, geom)
                assert int(got[py, px]) == want, (geom, px, py, int(got[py, px]), want)
                counts[want] += 1
        assert min(counts) > 0, counts   # all three classes occur
        o.close()


# ---- stage 4: RANSACToGetFitPlane, K8 (APD.cu:2272-2384) --------------------------------------------------------------------

def depth_from_plane(K, pl, px, py):  # ComputeDepthfromPlaneHypothesis, :206-209
    num = f32(f32(-pl[3]) * K[0])
    a = f32(f32(f32(px) - K[2]) * pl[0])
    b = f32(f32(f32(K[0] / K[4]) * f32(f32(py) - K[5])) * pl[1])
    c = f32(K[0] * pl[2])
    return f32(num / f32(f32(a + b) + c))


def view_direction(K, px, py, depth):  # GetViewDirection, :174-184
    X = get_3d_point(K, px, py, depth)
    norm = np.sqrt(f32(f32(f32(X[0] * X[0]) + f32(X[1] * X[1])) + f32(X[2] * X[2])))
    return f32(X[0] / norm), f32(X[1] / norm), f32(X[2] / norm)


def ransac_fit_plane_pixel(ob, W, K, weak, planes, neighbours_row, rng_words, px, py):
    """One pixel of K8: returns (fit plane as 4 binary32, random state afterwards)."""
    pl_c = tuple(f32(v) for v in planes[py, px])
    if weak[py, px] != WEAK:  # :2283-2286
        return pl_c, np.array(rng_words, np.uint32)
    rng = Rng(ob, rng_words)
    pts, pts3 = [], []
    for i in range(1, 9):  # :2296-2311, NEIGHBOUR_NUM = 9
        qx, qy = int(neighbours_row[i][0]), int(neighbours_row[i][1])
        if qx == -1 or qy == -1:
            continue
        pts.append((qx, qy))
        d = depth_from_plane(K, tuple(f32(v) for v in planes[qy, qx]), qx, qy)
        pts3.append(get_3d_point(K, qx, qy, d))
    n = len(pts)
    if n < 3:  # :2312-2315
        return pl_c, rng.words()
    min_cost, best = FLT_MAX, None
    for _ in range(50):  # :2317-2370, `while (iteration--)`
        a = rng.next() % n   # unsigned remainder (curand returns unsigned int, the int operand is converted)
        b = rng.next() % n
        c = rng.next() % n
        if a == b or b == c or a == c:
            continue
        if not point_in_triangle(pts[a], pts[b], pts[c], (px, py)):
            continue
        A, B, Cp = pts3[a], pts3[b], pts3[c]
        ac = (f32(A[0] - Cp[0]), f32(A[1] - Cp[1]), f32(A[2] - Cp[2]))
        bc = (f32(B[0] - Cp[0]), f32(B[1] - Cp[1]), f32(B[2] - Cp[2]))
        cx = f32(f32(ac[1] * bc[2]) - f32(bc[1] * ac[2]))
        cy = f32(-f32(f32(ac[0] * bc[2]) - f32(bc[0] * ac[2])))
        cz = f32(f32(ac[0] * bc[1]) - f32(bc[0] * ac[1]))
        if (cx == 0 and cy == 0 and cz == 0) or math.isnan(cx) or math.isnan(cy) or math.isnan(cz):
            continue
        inv = f32(f32(1.0) / np.sqrt(f32(f32(f32(cx * cx) + f32(cy * cy)) + f32(cz * cz))))  # NormalizeVec3, rsqrtf := 1 / sqrtf (C4)
        cx, cy, cz = f32(cx * inv), f32(cy * inv), f32(cz * inv)
        cw = f32(-f32(f32(f32(cx * A[0]) + f32(cy * A[1])) + f32(cz * A[2])))
        cost = f32(0.0)
        for k in range(n):
            if k in (a, b, c):
                continue
            t = pts3[k]
            cost = f32(cost + f32(abs(f32(f32(f32(f32(cx * t[0]) + f32(cy * t[1])) + f32(cz * t[2])) + cw))))
        if cost < min_cost:
            min_cost, best = cost, (cx, cy, cz, cw)
        if min_cost == 0:
            break
    if best is None:  # :2381-2383
        return (f32(0), f32(0), f32(0), f32(0)), rng.words()
    d = depth_from_plane(K, pl_c, px, py)  # :2372-2379: flip to face the camera
    vd = view_direction(K, px, py, d)
    dot = f32(f32(f32(best[0] * vd[0]) + f32(best[1] * vd[1])) + f32(best[2] * vd[2]))
    if dot > 0:
        best = (f32(-best[0]), f32(-best[1]), f32(-best[2]), f32(-best[3]))
    return best, rng.words()


def test_ransac_fit_plane(synth, ob):
    _check_ransac_fit_plane(ob, ring_scene(synth))


def _check_ransac_fit_plane(ob, scene, strict=True):
    W, H, N = 128, 96, 3
    sc, p1, o = _apd_oracle(scene, ob, W, H, N, seed=12)
    for kid in (1, 2, 3, 4, 5, 6, 7):   # RunPatchMatch's order up to the first K8 (:2407-2451)
        o.run_kernel(kid, 0)
    weak, planes, rng0 = o.weak_info.copy(), o.planes.copy(), o.rng.copy()
    nmap, nb = o.neighbours_map.copy(), o.neighbours.copy()
    o.run_kernel(8, 0)
    fit, rng1 = o.fit_planes, o.rng
    K = [f32(v) for v in sc.K[0].reshape(-1)]
    fitted = zeroed = 0
    with np.errstate(all="ignore"):
        for py in range(H):
            for px in range(W):
                want, want_rng = ransac_fit_plane_pixel(ob, W, K, weak, planes, nb[nmap[py, px]], rng0[py, px], px, py)
                got = fit[py, px]
                assert np.array_equal(np.array(want, np.float32).view(np.uint32), got.view(np.uint32)), (px, py, want, got.tolist())
                assert np.array_equal(rng1[py, px], want_rng), (px, py)
                if weak[py, px] == WEAK:
                    zero = not np.any(got.view(np.uint32) & 0x7FFFFFFF)
                    zeroed += int(zero)
                    fitted += int(not zero and not np.array_equal(got.view(np.uint32), planes[py, px].view(np.uint32)))
    assert fitted > populated(strict, 20, 0) and zeroed > populated(strict, 0, -1), (fitted, zeroed)   # both outcomes of the RANSAC loop occur
    o.close()


# ---- stage 5: LocalRefine, K15 (APD.cu:2146-2232) ---------------------------------------------------------------------------

def local_refine_pixel(o, cams_c, K, R, params, planes, sel, vweight, nsrc, px, py, geom):
    """One pixel of K15: the w component its plane has afterwards (binary32)."""
    origin = normal_to_ref_cam(R, planes[py, px])
    origin_depth = origin[3]
    if origin_depth == 0:
        return f32(planes[py, px][3])
    s = int(sel[py, px])
    vw = vweight[py, px]
    gf = f32(params["geom_factor"])
    cost_now, base_line, valid, weight_normal = f32(0), f32(0), 0, f32(0)
    for v in range(nsrc):  # :2170-2190
        if is_set(s, v):
            pl = np.array([origin[0], origin[1], origin[2], distance_to_origin(K, px, py, origin_depth, origin)], np.float32)
            t = f32(o.ncc_old(px, py, v + 1, pl))
            if geom:
                t = f32(t + f32(gf * f32(o.geom_cost(px, py, v + 1, pl))))
            cost_now = f32(cost_now + f32(t * f32(vw[v])))
            weight_normal = f32(weight_normal + f32(vw[v]))
            cd = [f32(cams_c[0][k] - cams_c[v + 1][k]) for k in range(3)]
            tv = float(f32(f32(f32(cd[0] * cd[0]) + f32(cd[1] * cd[1])) + f32(cd[2] * cd[2])))  # float expression into a double
            base_line = f32(base_line + f32(np.sqrt(f32(tv))))
            valid += 1
    if weight_normal == 0 or valid == 0:
        return f32(planes[py, px][3])
    cost_now = f32(cost_now / weight_normal)
    base_line = f32(base_line / f32(valid))
    disp = f32(f32(K[0] * base_line) / origin_depth)
    min_cost, best_depth = f32(2.0), origin_depth
    for p_disp in range(-5, 6):  # :2201-2226
        p_depth = f32(f32(K[0] * base_line) / f32(disp + f32(p_disp)))
        if p_depth < f32(params["depth_min"]) or p_depth > f32(params["depth_max"]):
            continue
        pl = np.array([origin[0], origin[1], origin[2], distance_to_origin(K, px, py, p_depth, origin)], np.float32)
        t = f32(0)
        for v in range(nsrc):
            if is_set(s, v):
                t = f32(t + f32(f32(o.ncc_old(px, py, v + 1, pl)) * f32(vw[v])))
                if geom:
                    t = f32(t + f32(f32(gf * f32(o.geom_cost(px, py, v + 1, pl))) * f32(vw[v])))
        t = f32(t / weight_normal)
        if t < min_cost:
            min_cost, best_depth = t, p_depth
    if float(f32(cost_now - min_cost)) > 0.1:  # :2229, a float difference against a double constant
        return best_depth
    return f32(planes[py, px][3])


def test_local_refine(synth, ob):
    _check_local_refine(ob, ring_scene(synth))


def _check_local_refine(ob, scene, strict=True):
    W, H, N = 56, 40, 3
    sc, imgs = scene(W, H, N, seed=14, textureless=0.25)
    for geom in (0, 1):
        kw = dict(seed=9, max_iterations=1, weak_peak_radius=4 if geom else 6)   # one iteration: planes far enough from converged to move
        depths = None
        prior = None
        if geom:
            kw.update(state=2, geom_consistency=1)
            depths = common.fake_depth_maps(W, H, N + 1)
            o0 = common.make_oracle(ob, sc, imgs, N, common.base_params(sc, N, seed=3, max_iterations=2, weak_peak_radius=6))
            o0.run()
            p0 = common.base_params(sc, N)
            prior = common.postprocess(o0.planes.copy(), o0.weak_info.copy(), o0.selected_views.copy(), f32(p0["depth_min"]), f32(p0["depth_max"]))
            o0.close()
        params = common.base_params(sc, N, **kw)
        params["geom_factor"] = ob.default_params(**params).geom_factor
        o = common.make_oracle(ob, sc, imgs, N, params, depths=depths, prior=prior)
        for kid in (1, 2, 5):
            o.run_kernel(kid)
        o.run_sweeps(0, 1)
        for kid in (11, 12, 13, 14):   # the post-loop kernels in RunPatchMatch's order (:2459-2490)
            o.run_kernel(kid)
        planes, sel, vw = o.planes.copy(), o.selected_views.copy(), o.view_weight.copy()
        o.run_kernel(15)
        got = o.planes
        K = [f32(v) for v in sc.K[0].reshape(-1)]
        R = [f32(v) for v in sc.R[0].reshape(-1)]
        cams_c = [[f32(v) for v in ob.make_camera(sc.K[i], sc.R[i], sc.t[i], W, H, sc.depth_min, sc.depth_max).c] for i in range(N + 1)]
        moved = 0
        with np.errstate(all="ignore"):
            for py in range(H):
                for px in range(W):
                    want = local_refine_pixel(o, cams_c, K, R, params, planes, sel, vw, N, px, py, geom)
                    assert np.array_equal(got[py, px, :3].view(np.uint32), planes[py, px, :3].view(np.uint32)), (geom, px, py)  # only w is written
                    assert np.float32(want).view(np.uint32) == got[py, px, 3].view(np.uint32), (geom, px, py, float(want), float(got[py, px, 3]))
                    moved += int(got[py, px, 3].view(np.uint32) != planes[py, px, 3].view(np.uint32))
        assert moved > populated(strict, 5, 0), (geom, moved)   # some depths are adopted
        o.close()


# ---- stage 6: FindNearestStrongPoint, K2 (APD.cu:2234-2270) -----------------------------------------------------------------

def nearest_strong_pixel(weak, W, H, px, py):
    if weak[py, px] != WEAK:
        return (-1, -1)
    best, min_dist = (-1, -1), f32(255.0)
    for x in range(-100, 101):          # x is the OUTER loop (:2252-2253): ties go to the first hit in that order
        for y in range(-100, 101):
            qx, qy = px + x, py + y
            if qx < 0 or qy < 0 or qx >= W or qy >= H:
                continue
            if weak[qy, qx] == STRONG:
                dist = np.sqrt(f32(x * x + y * y))   # integer expression converted to float, then sqrtf
                if dist < min_dist:
                    min_dist, best = dist, (qx, qy)
    return best


def test_find_nearest_strong_point(synth, ob):
    _check_find_nearest_strong_point(ob, ring_scene(synth))


def _check_find_nearest_strong_point(ob, scene, strict=True):
    W, H, N = 128, 96, 2
    sc, p1, o = _apd_oracle(scene, ob, W, H, N, seed=12)
    o.run_kernel(1)
    weak = o.weak_info.copy()
    # a hand-made WEAK block wider than the search radius, with UNKNOWN pixels on part of its border: pixels without any STRONG
    # pixel within 100, ties between equidistant candidates, candidates hidden behind non-STRONG ones
    weak[:, :] = STRONG
    weak[10:90, 4:124] = WEAK
    weak[9, 30:60] = UNKNOWN
    weak[40:44, 3] = UNKNOWN
    weak[50, 60] = STRONG
    o.weak_info[:, :] = weak
    o.run_kernel(2)
    got = o.nearest_strong
    ys, xs = np.nonzero(weak == WEAK)
    pick = np.random.RandomState(0).choice(len(ys), 350, replace=False)
    none = 0
    for py, px in [(int(ys[i]), int(xs[i])) for i in pick] + [(0, 0), (9, 40), (50, 60), (49, 60), (50, 59)]:
        want = nearest_strong_pixel(weak, W, H, px, py)
        assert (int(got[py, px][0]), int(got[py, px][1])) == want, (px, py, got[py, px].tolist(), want)
        none += int(want == (-1, -1) and weak[py, px] == WEAK)
    o.close()


# ---- stage 7: GetDepthandNormal, Black/RedPixelFilterStrong, K11-K13 (APD.cu:1587-1748) -------------------------------------

def normal_to_world(R, p):  # TransformNormal, :374-381: R^T n
    return (f32(f32(f32(R[0] * p[0]) + f32(R[3] * p[1])) + f32(R[6] * p[2])),
            f32(f32(f32(R[1] * p[0]) + f32(R[4] * p[1])) + f32(R[7] * p[2])),
            f32(f32(f32(R[2] * p[0]) + f32(R[5] * p[1])) + f32(R[8] * p[2])), f32(p[3]))


def filter_strong_pixel(planes, costs, weak, W, H, px, py):
    """CheckerboardFilterStrong (:1602-1714) on pixel (px, py): the depth it leaves in planes[py, px][3]."""
    w = planes[..., 3]
    vals = [f32(w[py, px])]
    if costs[py, px] < f32(0.001):
        return f32(w[py, px])

    def take(cond, dx, dy):
        if cond and weak[py + dy, px + dx] == STRONG:
            vals.append(f32(w[py + dy, px + dx]))

    take(py > 0, 0, -1)
    take(py > 2, 0, -3)
    take(py > 4, 0, -5)
    take(py < H - 1, 0, 1)
    take(py < H - 3, 0, 3)
    take(py < H - 5, 0, 5)
    take(px > 0, -1, 0)
    take(px > 2, -3, 0)
    take(px > 4, -5, 0)
    take(px < W - 1, 1, 0)
    take(px < W - 3, 3, 0)
    take(px < W - 5, 5, 0)
    take(py > 0 and px < W - 2, 2, -1)
    take(py < H - 1 and px < W - 2, 2, 1)
    take(py > 0 and px > 1, -2, -1)
    take(py < H - 1 and px > 1, -2, 1)
    take(px > 0 and py > 2, -1, -2)
    take(px < W - 1 and py > 2, 1, -2)
    take(px > 0 and py < H - 2, -1, 2)
    take(px < W - 1 and py < H - 2, 1, 2)
    d = list(vals)   # sort_small (:3-12): insertion sort, strict `<`
    for i in range(1, len(d)):
        tmp, j = d[i], i
        while j >= 1 and tmp < d[j - 1]:
            d[j] = d[j - 1]
            j -= 1
        d[j] = tmp
    m = len(d) // 2
    if len(d) % 2 == 0:
        return f32(f32(d[m - 1] + d[m]) / f32(2))
    return d[m]


def test_depth_normal_and_median_filter(synth, ob):
    _check_depth_normal_and_median_filter(ob, ring_scene(synth))


def _check_depth_normal_and_median_filter(ob, scene, strict=True):
    W, H, N = 89, 65, 3   # odd height: grid_size_half.y = ((65 / 2) + 15) / 16 = 2 blocks of 16 row pairs -> row 64 is never filtered
    sc, imgs = scene(W, H, N, seed=21, textureless=0.3)
    o0 = common.make_oracle(ob, sc, imgs, N, common.base_params(sc, N, seed=3, max_iterations=2, weak_peak_radius=6))
    o0.run()
    p0 = common.base_params(sc, N)
    prior = common.postprocess(o0.planes.copy(), o0.weak_info.copy(), o0.selected_views.copy(), f32(p0["depth_min"]), f32(p0["depth_max"]))
    o0.close()
    params = common.base_params(sc, N, seed=9, max_iterations=1, state=1, use_APD=1, weak_peak_radius=6, rotate_time=2, ransac_threshold=0.00875)
    o = common.make_oracle(ob, sc, imgs, N, params, prior=prior)
    for kid in (1, 2, 3, 4, 5):
        o.run_kernel(kid)
    o.run_sweeps(0, 1)
    before, costs, weak = o.planes.copy(), o.costs.copy(), o.weak_info.copy()
    assert (weak == WEAK).sum() > populated(strict, 20, 0) and (weak == STRONG).sum() > 200
    K = [f32(v) for v in sc.K[0].reshape(-1)]
    R = [f32(v) for v in sc.R[0].reshape(-1)]
    # K11, :1587-1600: depth first, then the normal to the world frame (w keeps the depth)
    o.run_kernel(11)
    want = np.empty_like(before)
    for py in range(H):
        for px in range(W):
            pl = [f32(v) for v in before[py, px]]
            pl[3] = depth_from_plane(K, pl, px, py)
            want[py, px] = normal_to_world(R, pl)
    assert np.array_equal(o.planes.view(np.uint32), want.view(np.uint32))
    # K12 then K13: HALF launches of 32 x 16 threads, p.y = 2 * p.y (+ 1) by the parity of threadIdx.x (:1716-1748)
    rows = 2 * (((H // 2) + 15) // 16) * 16
    changed = 0
    for colour in (0, 1):
        o.run_kernel(12 + colour)
        snap = want.copy()
        for py in range(min(rows, H)):
            for px in range(W):
                black = (py % 2) == (px % 2)   # threadIdx.x even <-> px even (block width 32): black rows are even there
                if black != (colour == 0) or weak[py, px] == WEAK:
                    continue
                v = filter_strong_pixel(snap, costs, weak, W, H, px, py)
                changed += int(np.float32(v).view(np.uint32) != snap[py, px, 3].view(np.uint32))
                want[py, px, 3] = v
        assert np.array_equal(o.planes.view(np.uint32), want.view(np.uint32)), colour
    assert changed > populated(strict, 50, 0), changed
    assert rows == H - 1   # the last row of the odd-height frame stays as K11 left it
    o.close()


# ---- stage 8: the tail of CheckerboardPropagationStrong (APD.cu:1260-1321) + PlaneHypothesisRefinementStrong (:837-890) -----

def sinf(ob, x):
    return f32(ob.lib().orc_sinf(C.c_float(float(x))))


def cosf(ob, x):
    return f32(ob.lib().orc_cosf(C.c_float(float(x))))


def random_normal(K, px, py, rng, depth):  # GenerateRandomNormal, :211-237
    q1, q2, s = f32(1), f32(1), f32(2)
    while s >= f32(1):
        q1 = f32(f32(f32(2) * rng.uniform()) - f32(1))
        q2 = f32(f32(f32(2) * rng.uniform()) - f32(1))
        s = f32(f32(q1 * q1) + f32(q2 * q2))
    sq = np.sqrt(f32(f32(1) - s))
    n = [f32(f32(f32(2) * q1) * sq), f32(f32(f32(2) * q2) * sq), f32(f32(1) - f32(f32(2) * s))]
    vd = view_direction(K, px, py, depth)
    if f32(f32(f32(n[0] * vd[0]) + f32(n[1] * vd[1])) + f32(n[2] * vd[2])) > 0:
        n = [f32(-n[0]), f32(-n[1]), f32(-n[2])]
    return normalize3(*n)


def perturbed_normal(ob, K, px, py, normal, rng, perturbation):  # GeneratePerturbedNormal, :239-273
    vd = view_direction(K, px, py, f32(1))
    a1 = f32(f32(rng.uniform() - f32(0.5)) * perturbation)
    a2 = f32(f32(rng.uniform() - f32(0.5)) * perturbation)
    a3 = f32(f32(rng.uniform() - f32(0.5)) * perturbation)
    s1, s2, s3 = sinf(ob, a1), sinf(ob, a2), sinf(ob, a3)
    c1, c2, c3 = cosf(ob, a1), cosf(ob, a2), cosf(ob, a3)
    R = [f32(c2 * c3),
         f32(f32(f32(c3 * s1) * s2) - f32(c1 * s3)),
         f32(f32(s1 * s3) + f32(f32(c1 * c3) * s2)),
         f32(c2 * s3),
         f32(f32(c1 * c3) + f32(f32(s1 * s2) * s3)),
         f32(f32(f32(c1 * s2) * s3) - f32(c3 * s1)),
         f32(-s2),
         f32(c2 * s1),
         f32(c1 * c2)]
    p = [f32(f32(f32(R[3 * r] * normal[0]) + f32(R[3 * r + 1] * normal[1])) + f32(R[3 * r + 2] * normal[2])) for r in range(3)]
    if f32(f32(f32(p[0] * vd[0]) + f32(p[1] * vd[1])) + f32(p[2] * vd[2])) >= 0:
        p = [f32(normal[0]), f32(normal[1]), f32(normal[2])]
    return normalize3(*p)


def strong_update_pixel(ob, o, snap, W, H, nsrc, params, K, px, py, it):
    """(plane, cost, selected views, random state) of pixel (px, py) after its K6 / K7 update."""
    costs, planes, sel, rng_words = snap
    weights, pos, flag, cost_array, rng = view_selection_of_pixel(ob, o, snap, W, H, nsrc, px, py, it)
    flat_planes = planes.reshape(-1, 4)
    center = py * W + px
    dmin, dmax = f32(params["depth_min"]), f32(params["depth_max"])
    temp_sel, weight_norm = 0, f32(0)
    for i in range(nsrc):  # :1260-1270
        if weights[i] > 0:
            temp_sel |= 1 << i
            weight_norm = f32(weight_norm + f32(weights[i]))
    with np.errstate(all="ignore"):
        final = []
        for i in range(8):  # :1272-1282
            acc = f32(0)
            for j in range(nsrc):
                if weights[j] > 0:
                    acc = f32(acc + f32(f32(weights[j]) * cost_array[i, j]))
            final.append(f32(acc / weight_norm))
        best = 0   # FindMinCostIndex, :29-40: `<=`, the last minimum wins
        cmin = final[0]
        for i in range(1, 8):
            if final[i] <= cmin:
                cmin, best = final[i], i
        plane_c = np.array(flat_planes[center], np.float32)
        cost_now = f32(0)
        for i in range(nsrc):  # :1286-1293: every view, selected or not
            cost_now = f32(cost_now + f32(f32(weights[i]) * f32(o.ncc_old(px, py, i + 1, plane_c))))
        cost_now = f32(cost_now / weight_norm)
        committed = cost_now   # costs[center] = cost_now (:1294)
        depth_now = depth_from_plane(K, plane_c, px, py)
        plane_now = plane_c.copy()
        new_sel = int(sel[py, px])
        if flag[best]:  # :1298-1307
            cand = np.array(flat_planes[pos[best]], np.float32)
            d = depth_from_plane(K, cand, px, py)
            if d >= dmin and d <= dmax and final[best] < cost_now:
                depth_now, plane_now, cost_now, new_sel = d, cand.copy(), final[best], temp_sel
        # PlaneHypothesisRefinementStrong, :837-890
        depth_rand = f32(f32(rng.uniform() * f32(dmax - dmin)) + dmin)
        n_rand = random_normal(K, px, py, rng, depth_now)
        lo, hi = f32(f32(f32(1) - f32(0.02)) * depth_now), f32(f32(f32(1) + f32(0.02)) * depth_now)
        depth_pert = f32(f32(rng.uniform() * f32(hi - lo)) + lo)   # `do ... while (a < min && a > max)` runs once
        n_pert = perturbed_normal(ob, K, px, py, plane_now, rng, f32(float(f32(0.02)) * math.pi))
        depths = [depth_rand, depth_now, depth_rand, depth_now, depth_pert]
        normals = [tuple(plane_now[:3]), n_rand, n_rand, n_pert, tuple(plane_now[:3])]
        for dk, nk in zip(depths, normals):
            pl = np.array([nk[0], nk[1], nk[2], distance_to_origin(K, px, py, dk, nk)], np.float32)
            t = f32(0)
            for j in range(nsrc):
                if weights[j] > 0:
                    t = f32(t + f32(f32(weights[j]) * f32(o.ncc_old(px, py, j + 1, pl))))
            t = f32(t / weight_norm)
            d = depth_from_plane(K, pl, px, py)
            if d >= dmin and d <= dmax and t < cost_now:
                depth_now, plane_now, cost_now = d, pl.copy(), t
        if params.get("state", 0) == 1:  # REFINE_INIT, :1311-1316: float < float - double
            if float(cost_now) < float(committed) - 0.1:
                return plane_now, cost_now, new_sel, rng.words()
            return plane_c, committed, new_sel, rng.words()
        return plane_now, cost_now, new_sel, rng.words()


def test_strong_update(synth, ob):
    _check_strong_update(ob, ring_scene(synth))


def _check_strong_update(ob, scene, strict=True):
    W, H, N = 36, 28, 3
    sc, imgs = scene(W, H, N, seed=23)
    for state in (0, 1):
        prior = None
        params = common.base_params(sc, N, seed=41 + state, max_iterations=2, state=state)
        if state == 1:
            o0 = common.make_oracle(ob, sc, imgs, N, common.base_params(sc, N, seed=3, max_iterations=1, weak_peak_radius=6))
            o0.run()
            p0 = common.base_params(sc, N)
            prior = common.postprocess(o0.planes.copy(), o0.weak_info.copy(), o0.selected_views.copy(), f32(p0["depth_min"]), f32(p0["depth_max"]))
            o0.close()
        o = common.make_oracle(ob, sc, imgs, N, params, prior=prior)
        for kid in (1, 2, 5):
            o.run_kernel(kid)
        K = [f32(v) for v in sc.K[0].reshape(-1)]
        adopted = refined = 0
        for it in (0, 1):
            for colour, kid in ((0, 6), (1, 7)):
                snap = (o.costs.copy(), o.planes.copy(), o.selected_views.copy(), o.rng.copy())
                weak = o.weak_info.copy()
                o.run_kernel(kid, it)
                planes, costs, sel, rng = o.planes, o.costs, o.selected_views, o.rng
                for py in range(H):
                    for px in range(W):
                        if (px + py) % 2 != colour or weak[py, px] == WEAK:
                            continue
                        wp, wc, ws, wr = strong_update_pixel(ob, o, snap, W, H, N, params, K, px, py, it)
                        assert np.array_equal(np.asarray(wp, np.float32).view(np.uint32), planes[py, px].view(np.uint32)), (state, it, colour, px, py)
                        assert np.float32(wc).view(np.uint32) == costs[py, px].view(np.uint32), (state, it, colour, px, py)
                        assert int(sel[py, px]) == ws and np.array_equal(rng[py, px], wr), (state, it, colour, px, py)
                        adopted += int(ws != int(snap[2][py, px]))
                        refined += int(not np.array_equal(planes[py, px].view(np.uint32), snap[1][py, px].view(np.uint32)))
        # REFINE_INIT only commits an improvement of more than 0.1 (:1312): few pixels move, both branches occur
        assert ((adopted > 20 and refined > 100) if state == 0 else (adopted > 3 and refined > 20)) if strict else (adopted > 0 and refined > 0), (state, adopted, refined)
        o.close()


# ---- stage 9: RandomInitialization, K5 (APD.cu:807-835, :275-282, :616-693) -------------------------------------------------

def random_initialization_pixel(ob, o, K, R, params, planes, sel, rng_words, nsrc, px, py):
    """(plane, cost, selected views, random state) of pixel (px, py) after K5."""
    dmin, dmax = f32(params["depth_min"]), f32(params["depth_max"])
    if params.get("state", 0) == 0:  # FIRST_INIT
        rng = Rng(ob, rng_words)
        depth = f32(f32(rng.uniform() * f32(dmax - dmin)) + dmin)   # GenerateRandomPlaneHypothesis, :275-282
        n = random_normal(K, px, py, rng, depth)
        pl = np.array([n[0], n[1], n[2], distance_to_origin(K, px, py, depth, n)], np.float32)
        # ComputeMultiViewInitialCostandSelectedViews, :616-662
        cost_vector = [f32(o.ncc_old(px, py, i + 1, pl)) for i in range(nsrc)]
        copy = list(cost_vector)
        valid = sum(1 for c in cost_vector if c < f32(2.0))
        d = list(cost_vector)   # sort_small over cost_count entries
        for i in range(1, len(d)):
            tmp, j = d[i], i
            while j >= 1 and tmp < d[j - 1]:
                d[j] = d[j - 1]
                j -= 1
            d[j] = tmp
        top_k = min(valid, int(params.get("top_k", 4)))
        new_sel = 0
        if top_k > 0:
            cost = f32(0)
            for i in range(top_k):
                cost = f32(cost + d[i])
            thr = d[top_k - 1]
            for i in range(nsrc):
                if copy[i] <= thr:
                    new_sel |= 1 << i
            return pl, f32(cost / f32(top_k)), new_sel, rng.words()
        return pl, f32(2.0), new_sel, rng.words()
    # REFINE_*: the prior plane (world normal, depth) back into the camera frame (:823-833); no draw
    q = normal_to_ref_cam(R, planes[py, px])
    pl = np.array([q[0], q[1], q[2], distance_to_origin(K, px, py, q[3], q)], np.float32)
    s, count, cost = int(sel[py, px]), 0, f32(0)
    for i in range(nsrc):  # ComputeMultiViewInitialCost, :664-693
        if is_set(s, i):
            c = f32(o.ncc_old(px, py, i + 1, pl))
            if c < f32(2.0):
                count += 1
                cost = f32(cost + c)
            else:
                s &= (0xFFFFFFFE << i) & 0xFFFFFFFF   # unSetBit (:46-49): bit i AND every bit below it
    return pl, (f32(2.0) if count == 0 else f32(cost / f32(count))), s, np.array(rng_words, np.uint32)


def test_random_initialization(synth, ob):
    _check_random_initialization(ob, ring_scene(synth))


def _check_random_initialization(ob, scene, strict=True):
    W, H, N = 48, 36, 5
    sc, imgs = scene(W, H, N, seed=31, textureless=0.2)
    K = [f32(v) for v in sc.K[0].reshape(-1)]
    R = [f32(v) for v in sc.R[0].reshape(-1)]
    prior = None
    for state in (0, 2):
        params = common.base_params(sc, N, seed=51 + state, max_iterations=1, state=state, weak_peak_radius=6)
        if "top_k" not in params:
            params["top_k"] = ob.default_params(**params).top_k
        o = common.make_oracle(ob, sc, imgs, N, params, prior=prior)
        for kid in (1, 2):
            o.run_kernel(kid)
        planes, sel, rng0 = o.planes.copy(), o.selected_views.copy(), o.rng.copy()
        o.run_kernel(5)
        cleared = 0
        with np.errstate(all="ignore"):
            for py in range(H):
                for px in range(W):
                    wp, wc, ws, wr = random_initialization_pixel(ob, o, K, R, params, planes, sel, rng0[py, px], N, px, py)
                    assert np.array_equal(np.asarray(wp, np.float32).view(np.uint32), o.planes[py, px].view(np.uint32)), (state, px, py)
                    assert np.float32(wc).view(np.uint32) == o.costs[py, px].view(np.uint32), (state, px, py)
                    assert int(o.selected_views[py, px]) == ws, (state, px, py, int(o.selected_views[py, px]), ws)
                    assert np.array_equal(o.rng[py, px], wr), (state, px, py)
                    cleared += int(state != 0 and ws != int(sel[py, px]))
        if state == 0:
            o.run()   # the FIRST_INIT pass gives the prior of the second round
            p0 = common.base_params(sc, N)
            prior = common.postprocess(o.planes.copy(), o.weak_info.copy(), o.selected_views.copy(), f32(p0["depth_min"]), f32(p0["depth_max"]))
        else:
            assert cleared > 0, "no view failed: the unSetBit path is not exercised"
        o.close()


# ---- stage 10: CheckerboardPropagationWeak + PlaneHypothesisRefinementWeak, K9 / K10 (APD.cu:1323-1508, :892-980) -----------

def weak_update_pixel(ob, o, snap, nb_row, fit_plane, W, H, nsrc, params, K, px, py, it, geom):
    """(plane, cost, view weights, selected views, random state) of WEAK pixel (px, py) after its K9 / K10 update."""
    planes, sel, weak, rng_words = snap
    dmin, dmax = f32(params["depth_min"]), f32(params["depth_max"])
    gf = f32(params["geom_factor"])
    cost_array = np.zeros((8, 32), np.float32)
    cost_array[0, 0] = f32(2.0)   # `= { 2.0f }` (:1345)
    flag, cand = [False] * 8, [None] * 8
    for i in range(8):  # :1352-1363
        qx, qy = int(nb_row[i + 1][0]), int(nb_row[i + 1][1])
        if qx == -1 or qy == -1 or weak[qy, qx] != STRONG:
            continue
        flag[i] = True
        cand[i] = np.array(planes[qy, qx], np.float32)
        for v in range(nsrc):
            cost_array[i, v] = f32(o.ncc_new(px, py, v + 1, cand[i]))
    priors = np.zeros(32, np.float32)
    for i in range(8):  # :1371-1385: every neighbour that exists, STRONG or not
        qx, qy = int(nb_row[i + 1][0]), int(nb_row[i + 1][1])
        if qx == -1 or qy == -1:
            continue
        for j in range(nsrc):
            priors[j] = f32(priors[j] + (f32(0.9) if is_set(sel[qy, qx], j) == 1 else f32(0.1)))
    probs = np.zeros(32, np.float32)
    thr = f32(0.8 * float(expf(ob, f32(it * it) / f32(-90.0))))
    for i in range(nsrc):
        count, count_false, tmpw = f32(0), 0, f32(0)
        for j in range(8):
            cij = cost_array[j, i]
            if cij < thr:
                tmpw = f32(tmpw + expf(ob, f32(f32(cij * cij) / f32(-0.18))))
                count = f32(count + f32(1))
            if cij > f32(1.2):
                count_false += 1
        if count > 2 and count_false < 3:
            probs[i] = f32(tmpw / count)
        elif count_false < 3:
            probs[i] = expf(ob, f32(f32(thr * thr) / f32(-0.32)))
        probs[i] = f32(probs[i] * priors[i])
    s = f32(0)
    for i in range(nsrc):
        s = f32(s + probs[i])
    inv = f32(1.0) / s
    cum = f32(0)
    for i in range(nsrc):
        cum = f32(cum + f32(probs[i] * inv))
        probs[i] = cum
    rng = Rng(ob, rng_words[py, px])
    weights = np.zeros(32, np.uint8)
    for _ in range(15):
        rand_prob = f32(rng.uniform() - FLT_EPSILON)
        for v in range(nsrc):
            if probs[v] > rand_prob:
                weights[v] += 1
                break
    temp_sel, weight_norm = 0, f32(0)
    for i in range(nsrc):
        if weights[i] > 0:
            temp_sel |= 1 << i
            weight_norm = f32(weight_norm + f32(weights[i]))

    def weighted(plane, cost_of_view, only_selected):
        """sum_j w_j * (cost_j [+ geom_factor * geometric cost_j]) in view order"""
        acc = f32(0)
        for j in range(nsrc):
            if only_selected and not weights[j] > 0:
                continue
            c = cost_of_view(j)
            if geom:
                c = f32(c + f32(gf * (f32(o.geom_cost(px, py, j + 1, plane)) if plane is not None else f32(3.0))))
            acc = f32(acc + f32(f32(weights[j]) * c))
        return acc

    final = []
    for i in range(8):  # :1441-1460
        acc = weighted(cand[i] if flag[i] else None, lambda j, i=i: cost_array[i, j], True)
        final.append(f32(acc / weight_norm))
    best, cmin = 0, final[0]
    for i in range(1, 8):
        if final[i] <= cmin:
            cmin, best = final[i], i
    plane_c = np.array(planes[py, px], np.float32)
    cost_now = f32(weighted(plane_c, lambda j: f32(o.ncc_new(px, py, j + 1, plane_c)), False) / weight_norm)  # :1464-1476, every view
    committed = cost_now
    depth_now, plane_now, new_sel = depth_from_plane(K, plane_c, px, py), plane_c.copy(), int(sel[py, px])
    if flag[best]:  # :1480-1488
        d = depth_from_plane(K, cand[best], px, py)
        if d >= dmin and d <= dmax and final[best] < cost_now:
            depth_now, plane_now, cost_now, new_sel = d, cand[best].copy(), final[best], temp_sel

    def try_plane(pl):
        nonlocal depth_now, plane_now, cost_now
        t = f32(weighted(pl, lambda j: f32(o.ncc_new(px, py, j + 1, pl)), True) / weight_norm)
        d = depth_from_plane(K, pl, px, py)
        if d >= dmin and d <= dmax and t < cost_now:
            depth_now, plane_now, cost_now = d, pl.copy(), t

    fit = np.array(fit_plane, np.float32)
    if not (fit[0] == 0 and fit[1] == 0 and fit[2] == 0):  # PlaneHypothesisRefinementWeak, :910-980; no fit plane: no refinement at all
        try_plane(fit)
        depth_rand = f32(f32(rng.uniform() * f32(dmax - dmin)) + dmin)
        n_rand = random_normal(K, px, py, rng, depth_now)
        lo, hi = f32(f32(f32(1) - f32(0.02)) * depth_now), f32(f32(f32(1) + f32(0.02)) * depth_now)
        depth_pert = f32(f32(rng.uniform() * f32(hi - lo)) + lo)
        n_pert = perturbed_normal(ob, K, px, py, plane_now, rng, f32(float(f32(0.02)) * math.pi))
        depths = [depth_rand, depth_now, depth_rand, depth_now, depth_pert]
        normals = [tuple(plane_now[:3]), n_rand, n_rand, n_pert, tuple(plane_now[:3])]
        for dk, nk in zip(depths, normals):
            try_plane(np.array([nk[0], nk[1], nk[2], distance_to_origin(K, px, py, dk, nk)], np.float32))
    if params.get("state", 0) == 1:  # REFINE_INIT, :1490-1495
        plane_final = plane_now if float(cost_now) < float(committed) - 0.1 else plane_c
    else:
        plane_final = plane_now
    rescore = f32(0)  # :1499-1507: the stored cost is the fixed-patch cost of the committed plane over every view
    for i in range(nsrc):
        rescore = f32(rescore + f32(f32(weights[i]) * f32(o.ncc_old(px, py, i + 1, plane_final))))
    return plane_final, f32(rescore / weight_norm), weights, new_sel, rng.words()


def test_weak_update(synth, ob):
    _check_weak_update(ob, ring_scene(synth))


def _check_weak_update(ob, scene, strict=True):
    W, H, N = 96, 72, 3
    sc, imgs = scene(W, H, N, seed=12, textureless=0.3)
    o0 = common.make_oracle(ob, sc, imgs, N, common.base_params(sc, N, seed=5, max_iterations=2, weak_peak_radius=6))
    o0.run()
    p0 = common.base_params(sc, N)
    prior = common.postprocess(o0.planes.copy(), o0.weak_info.copy(), o0.selected_views.copy(), f32(p0["depth_min"]), f32(p0["depth_max"]))
    o0.close()
    K = [f32(v) for v in sc.K[0].reshape(-1)]
    nofit_total = 0
    for state, geom in ((1, 0), (2, 1)):
        params = common.base_params(sc, N, seed=60 + state, max_iterations=1, state=state, use_APD=1, weak_peak_radius=6, rotate_time=2,
                                    ransac_threshold=0.00875, geom_consistency=geom)
        params["geom_factor"] = ob.default_params(**params).geom_factor
        depths = common.fake_depth_maps(W, H, N + 1) if geom else None
        o = common.make_oracle(ob, sc, imgs, N, params, depths=depths, prior=prior)
        for kid in (1, 2, 3, 4, 5, 6, 7, 8):   # RunPatchMatch's order up to the first weak launch
            o.run_kernel(kid, 0)
        nmap, nb, fit = o.neighbours_map.copy(), o.neighbours.copy(), o.fit_planes.copy()
        moved = refined = nofit = 0
        for colour, kid in ((0, 9), (1, 10)):
            snap = (o.planes.copy(), o.selected_views.copy(), o.weak_info.copy(), o.rng.copy())
            o.run_kernel(kid, 0)
            with np.errstate(all="ignore"):
                for py in range(H):
                    for px in range(W):
                        if snap[2][py, px] != WEAK:
                            continue
                        if (px + py) % 2 != colour:
                            continue
                        wp, wc, ww, ws, wr = weak_update_pixel(ob, o, snap, nb[nmap[py, px]], fit[py, px], W, H, N, params, K, px, py, 0, geom)
                        where = (state, colour, px, py)
                        assert np.array_equal(np.asarray(wp, np.float32).view(np.uint32), o.planes[py, px].view(np.uint32)), where
                        assert np.float32(wc).view(np.uint32) == o.costs[py, px].view(np.uint32), where
                        assert np.array_equal(o.view_weight[py, px], ww), where
                        assert int(o.selected_views[py, px]) == ws and np.array_equal(o.rng[py, px], wr), where
                        moved += int(ws != int(snap[1][py, px]))
                        refined += int(not np.array_equal(o.planes[py, px].view(np.uint32), snap[0][py, px].view(np.uint32)))
                        nofit += int(not np.any(fit[py, px, :3]))
        checked = int((snap[2] == WEAK).sum())
        # REFINE_INIT only commits an improvement of more than 0.1: few planes move there
        assert (checked > 150 and refined > (3 if state == 1 else 20)) if strict else (checked > 50 and refined > 0), (state, checked, moved, refined, nofit)
        nofit_total += nofit
        o.close()
    assert nofit_total > 0, "no WEAK pixel without a fit plane: the early return of the refinement is not exercised"


# ---- every stage again on general cameras -----------------------------------------------------------------------------------------
# fx != fy, principal points off the centre and different per view, a roll that is no multiple of 90 degrees: on synth's ring an
# fx-for-fy or a cx-for-cy slip in either entry changes nothing.  Same frame sizes, seeds and passes as each stage's own test; the
# bit comparisons are the same, the population counts are held to `populated`.

STAGES = [_check_arm_search_and_view_selection, _check_gen_neighbours, _check_gen_neighbours_long_rays, _check_depth_to_weak_classifier,
          _check_ransac_fit_plane, _check_local_refine, _check_find_nearest_strong_point, _check_depth_normal_and_median_filter,
          _check_strong_update, _check_random_initialization, _check_weak_update]


@pytest.mark.parametrize("rig", ["aniso", "offcentre", "roll37"])
@pytest.mark.parametrize("stage", STAGES, ids=[f.__name__[7:] for f in STAGES])
def test_stage_on_general_cameras(synth, ob, stage, rig):
    stage(ob, rig_scene(synth, rig), strict=False)
