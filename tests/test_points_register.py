"""Global registration by FPFH descriptors, matches and RANSAC (arithmetic contract C19; csrc/apd_register_math.h) on the CPU: the
sequential checker (tests/helpers/points_register_ref.cpp) in its two modes on every case of the device tests, the properties of
the descriptors, the binning of theta by comparisons against a binary64 atan2, the generator, a planted transform recovered by
the checker alone, every way the registration ends, and the C ABI's refusals, which need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from common import kernel_resources
import points_align_checker as PA
import points_nearest_checker as PX
import points_normals_checker as PN
import points_register_checker as RC
from test_points_align import rotation
from test_points_nearest import bits32, pair_cases
from test_points_radius import BAD as BAD_RADIUS
from test_points_voxel import cloud, from_cloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("apd_points_features", "apd_points_match_features", "apd_points_match_features_bounded", "apd_points_register")
SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257)
MATCH_TILE = 128                                        # kMatchTile of csrc/apd_points_register.hip
PLANTED_RADIUS, PLANTED_NORMALS, PLANTED_INLIER, PLANTED_ICP, PLANTED_TAU = 1.0, 0.8, 0.3, 0.5, 0.01
PLANTED_R, PLANTED_T = rotation(130.0), np.float64([40.0, -25.0, 30.0])


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return RC.build(tmp_path_factory.mktemp("points_register_checker"))


@pytest.fixture(scope="module")
def align_checker(tmp_path_factory):
    return PA.build(tmp_path_factory.mktemp("points_align_checker"))


@pytest.fixture(scope="module")
def score_checker(tmp_path_factory):
    return PX.build(tmp_path_factory.mktemp("points_nearest_checker"))


@pytest.fixture(scope="module")
def normals_checker(tmp_path_factory):
    return PN.build(tmp_path_factory.mktemp("points_normals_checker"))


# --------------------------------------------------------------------------------------------------------------------
# the clouds
# --------------------------------------------------------------------------------------------------------------------

def surface(n=2000, seed=11):
    """n points scattered -- no lattice -- on a surface of varied shape over [0, 10]^2: a height field of four bumps and, for a
    quarter of them, three faces of a box corner."""
    rng = np.random.default_rng(seed)
    n_box = n // 4
    xy = rng.uniform(0, 10, (n - n_box, 2))
    bumps = [(2.5, 2.5, 1.5, 1.2), (7, 3, -1.0, 0.9), (3, 7.5, 0.8, 0.6), (5, 5, 0.6, 2.0)]
    z = sum(h * np.exp(-((xy[:, 0] - cx) ** 2 + (xy[:, 1] - cy) ** 2) / (2 * s * s)) for cx, cy, h, s in bumps)
    face, u = rng.integers(0, 3, n_box), rng.uniform(0, 2.5, (n_box, 2))
    top = np.column_stack([7 + u[:, 0], 7 + u[:, 1], np.full(n_box, 3.0)])
    wall_x = np.column_stack([np.full(n_box, 7.0), 7 + u[:, 0], 0.5 + u[:, 1]])
    wall_y = np.column_stack([7 + u[:, 0], np.full(n_box, 7.0), 0.5 + u[:, 1]])
    box = np.where((face == 0)[:, None], top, np.where((face == 1)[:, None], wall_x, wall_y))
    return np.concatenate([np.column_stack([xy, z]), box]).astype(np.float32)


def planted_case(normals_checker, align_checker):
    """Q: the surface with the normals the normals checker estimates -- what with_estimated_normals gives; P: two of every three
    of its points, positions and normals moved by the inverse of x' = R x + t, R 130 degrees about (1, 2, 3) and t several cloud
    diameters.  (P, P's normals, Q, Q's normals, the indices P was made from)."""
    q = surface()
    qn = PN.run(normals_checker, cloud(q), PLANTED_NORMALS, 5).normal
    chosen = np.flatnonzero(np.arange(len(q)) % 3 != 0)
    p, pn = PA.transformed(align_checker, q[chosen], qn[chosen], 1.0, PLANTED_R.T, -PLANTED_R.T @ PLANTED_T)
    return p, pn, q, qn, chosen


def random_normals(rng, n):
    """Normals of every length, the first two of a cloud with the two kinds that give no frame."""
    normal = rng.normal(size=(n, 3)).astype(np.float32)
    normal[0:1] = 0.0
    normal[1:2, 1] = np.nan
    if n > 7:
        normal[7, 2] = np.inf
    return normal


def star(centre, rng, reach=0.9):
    """Four points of which only the first has three neighbours within 1: three leaves at `reach` from it, 120 degrees apart."""
    angles = rng.uniform(0, 2 * np.pi) + np.arange(3) * 2 * np.pi / 3
    leaves = np.column_stack([np.cos(angles), np.sin(angles), rng.uniform(-0.2, 0.2, 3)]) * reach
    return np.float32(centre) + np.concatenate([np.zeros((1, 3)), leaves]).astype(np.float32)


def stars_case(count, seed=3):
    """A cloud in which exactly `count` points get a descriptor at radius 1 and min_neighbours 3: the centres of that many stars,
    ten cells apart."""
    rng = np.random.default_rng(seed)
    xyz = np.concatenate([star([10.0 * s + 0.5, 0.5, 0.5], rng) for s in range(count)] + [np.zeros((0, 3), np.float32)])
    return xyz, rng.normal(size=(len(xyz), 3)).astype(np.float32)


def register_cases(pkg):
    """name -> (P, P's normals, Q, Q's normals, radius, origin, min_neighbours): the pairs of test_points_nearest.py with random
    normals -- points outside the grid, a crowded cell, another origin, zero and non-finite normals -- and dense patches of the
    surface at every size around a wave and a block."""
    out = {}
    rng = np.random.default_rng(77)
    for name, (p, q, radius, origin) in pair_cases(pkg).items():
        out[name] = (p, random_normals(rng, len(p)), q, random_normals(rng, len(q)), radius, origin, 3)
    s = surface()
    s = s[np.argsort(s[:, 0] + s[:, 1], kind="stable")]          # a patch: dense at every size
    for k, n in enumerate(SIZES):
        m = SIZES[(k + 4) % len(SIZES)]
        out["patch %d in %d" % (n, m)] = (s[:n], random_normals(rng, n), s[100:100 + m], random_normals(rng, m), 1.0, None, 3)
    few, few_normals = stars_case(6)
    out["no point reaches min_neighbours"] = (few, few_normals, s[:300], random_normals(rng, 300), 1.0, None, 4)
    for count in range(4):
        xyz, normal = stars_case(count)
        out["%d matches" % count] = (xyz, normal, s[:300], random_normals(rng, 300), 1.0, None, 3)
    return out


# --------------------------------------------------------------------------------------------------------------------
# the checker: its two modes and the descriptors
# --------------------------------------------------------------------------------------------------------------------

def test_brute_force_and_grid_agree_on_every_device_case(pkg, checker):
    """Descriptors, flags, matches with and without the mutual test and every field of the registration: the same bits from the
    loop over all pairs and from the 27 lookups."""
    described = 0
    for name, (p, pn, q, qn, radius, origin, least) in register_cases(pkg).items():
        for xyz, normal in ((p, pn), (q, qn)):
            grid, brute = (RC.features(checker, xyz, normal, radius, origin, least, mode) for mode in (RC.GRID, RC.BRUTE))
            assert np.array_equal(bits32(grid[0]), bits32(brute[0])) and np.array_equal(grid[1], brute[1]), name
            assert np.isfinite(grid[0]).all() and not grid[0][grid[1] == 0].any(), name
            described += int(grid[1].sum())
        for mutual in (False, True):
            grid, brute = (RC.match_features(checker, p, pn, q, qn, radius, origin, least, mutual, mode) for mode in (RC.GRID, RC.BRUTE))
            assert np.array_equal(grid[0], brute[0]) and np.array_equal(bits32(grid[1]), bits32(brute[1])), (name, mutual)
            assert np.array_equal(grid[0] >= 0, np.isfinite(grid[1])), name
        kw = dict(trials=65, min_neighbours=least, mutual=False, inlier_distance=0.5)
        grid, brute = (RC.register(checker, p, pn, q, qn, radius, origin, mode=mode, **kw) for mode in (RC.GRID, RC.BRUTE))
        assert RC.bits(grid) == RC.bits(brute), (name, grid, brute)
    assert described > 5000


def test_each_block_of_a_descriptor_sums_to_one(checker, normals_checker, align_checker):
    """Eleven binary32 terms, each the rounding of a share of a block that sums to 1 in binary64 up to its own eleven roundings:
    the sum taken in binary64 is within 11 half-ulps of binary32 at 1 plus the binary64 slack, 11 * 2^-24 + 2^-40."""
    p, pn, q, qn, _ = planted_case(normals_checker, align_checker)
    for xyz, normal in ((p, pn), (q, qn)):
        f, has = RC.features(checker, xyz, normal, PLANTED_RADIUS)
        assert has.sum() > 0.9 * len(xyz)
        blocks = f[has == 1].astype(np.float64).reshape(-1, 3, 11).sum(axis=2)
        worst = np.abs(blocks - 1.0).max()
        print("largest |block sum - 1|", worst)
        assert worst <= 11 * 2.0 ** -24 + 2.0 ** -40 and (f >= 0).all()
        assert not f[has == 0].any()


def test_a_pair_on_a_known_frame(checker):
    """Centre at the origin with normal +z, neighbour at (1, 0, 0) with a normal tilted from +z towards +y: the centre is the source
    (both dots with the line are 0: no swap), v = d x n1 = -y, w = n1 x v = +x; alpha = v . n2 = -sin, phi = 0, theta =
    atan2(w . n2, n1 . n2) = atan2(0, cos) = 0."""
    tilt = np.deg2rad(30.0)
    rc, d2, bins = RC.pair(checker, [0, 0, 0], [0, 0, 2], [1, 0, 0], [0, np.sin(tilt), np.cos(tilt)])
    assert rc == 1 and d2 == 1.0
    assert bins == [int(np.floor(11 * (1 - np.sin(tilt)) / 2)), 5, 5]
    assert RC.pair(checker, [0, 0, 0], [0, 0, 1], [0, 0, 0], [0, 1, 0])[0] == 0            # the same position: skipped
    assert RC.pair(checker, [0, 0, 0], [0, 0, 1], [0, 0, 3], [0, 0, 1])[0] == 0            # the line along the source normal: skipped
    assert RC.pair(checker, [0, 0, 0], [0, 0, 0], [1, 0, 0], [0, 0, 1])[0] == -1           # no frame
    assert RC.pair(checker, [0, 0, 0], [0, np.inf, 0], [1, 0, 0], [0, 0, 1])[0] == -1


# --------------------------------------------------------------------------------------------------------------------
# theta by comparisons
# --------------------------------------------------------------------------------------------------------------------

EDGE_MARGIN = 1e-9          # radians kept between a tested direction and an edge: a cross product of unit-scale numbers carries about
                            # 2^-52 of error, and so do the literals; 1e-9 is seven orders above both


def test_theta_bin_is_the_floor_of_atan2_away_from_the_edges(checker):
    rng = np.random.default_rng(9)
    angles = np.concatenate([rng.uniform(-np.pi, np.pi, 20000), np.linspace(-np.pi, np.pi, 2311)[1:-1]])
    edges = -np.pi + 2 * np.pi * np.arange(0, 12) / 11
    for sign in (-1e-7, -1e-9 * 1.5, 1e-9 * 1.5, 1e-7):                       # just beside every edge, on either side
        angles = np.concatenate([angles, edges[1:11] + sign])
    length = rng.uniform(1e-3, 1e3, len(angles))
    y, x = length * np.sin(angles), length * np.cos(angles)
    theta = np.arctan2(y, x)
    keep = np.abs(theta[:, None] - edges[None, :]).min(axis=1) > EDGE_MARGIN
    assert keep.sum() > 22000
    want = np.floor(11 * (theta + np.pi) / (2 * np.pi)).astype(int)
    got = np.array([checker.points_register_theta_bin(float(b), float(a)) for b, a in zip(y, x)])
    assert np.array_equal(got[keep], want[keep]) and set(got[keep]) == set(range(11))


def test_theta_on_an_edge_at_the_ends_and_at_zero_is_what_the_header_states(checker):
    text = open(os.path.join(ROOT, "apd-mvs_amd", "csrc", "apd_register_math.h")).read()
    literals = [(float(c), float(s)) for c, s in re.findall(r"^\s+F\((-?[0-9.]+), (-?[0-9.]+)\)", text, flags=re.M)]
    assert len(literals) == 10
    for k, (c, s) in enumerate(literals, start=1):
        angle = -np.pi + 2 * np.pi * k / 11
        # the angle itself is rounded here, by up to 2^-52 * pi: 2^-50 covers that and the literal's own half ulp
        assert abs(c - np.cos(angle)) <= 2.0 ** -50 and abs(s - np.sin(angle)) <= 2.0 ** -50, k
        assert checker.points_register_theta_bin(s, c) == k, "exactly on edge %d: the upper bin" % k            # cross == 0.0
        assert checker.points_register_theta_bin(4.0 * s, 4.0 * c) == k
    assert checker.points_register_theta_bin(0.0, 0.0) == 5 and checker.points_register_theta_bin(-0.0, 0.0) == 5
    assert checker.points_register_theta_bin(0.0, -1.0) == 10                 # theta = +pi, clamped
    assert checker.points_register_theta_bin(-0.0, -1.0) == 10                # -0.0 is not the lower half plane
    assert checker.points_register_theta_bin(-1e-300, -1.0) == 0              # just below -pi's ray: the first bin
    assert checker.points_register_theta_bin(0.0, 1.0) == 5 and checker.points_register_theta_bin(-1e-300, 1.0) == 5
    assert [checker.points_register_linear_bin(v) for v in (-1.0, -1.0000001, 1.0, 1.0000001, 0.0, -0.82, 0.82)] == [0, 0, 10, 10, 5, 0, 10]
    assert checker.points_register_linear_bin(float("nan")) == 0


# --------------------------------------------------------------------------------------------------------------------
# the generator
# --------------------------------------------------------------------------------------------------------------------

def draw(seed, t, c, M):
    """The generator of the header, restated with Python's integers."""
    mask = (1 << 64) - 1
    z = (seed + (t + 1) * 0x9E3779B97F4A7C15 + c * 0xD1B54A32D192ED03) & mask
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & mask
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & mask
    z ^= z >> 31
    return ((z >> 32) * M) >> 32


def test_the_generator_gives_three_distinct_reachable_positions_and_known_answers(checker):
    for seed, t, c, M in ((0, 0, 0, 1000), (1, 2, 3, 7), (2 ** 64 - 1, 65535, 15, 2 ** 31 - 1), (12345, 99, 1, 3)):
        assert checker.points_register_draw(seed, t, c, M) == draw(seed, t, c, M)
    assert [RC.three(checker, 0, t, 1000) for t in range(3)] == [(883, 176, 235), (431, 459, 352), (26, 525, 102)]
    assert RC.three(checker, 2 ** 64 - 1, 7, 5) == (1, 4, 2) and RC.three(checker, 42, 0, 3) == (2, 1, 0)
    for M in (3, 4, 5, 17, 1000):
        seen = set()
        for t in range(40 * M):
            at = RC.three(checker, 7, t, M)
            assert len(set(at)) == 3 and all(0 <= a < M for a in at), (M, t, at)
            seen.update(at)
            first = draw(7, t, 0, M)
            assert at[0] == first
        assert seen == set(range(M)), M


# --------------------------------------------------------------------------------------------------------------------
# the planted case
# --------------------------------------------------------------------------------------------------------------------

def test_the_planted_transform_is_recovered_by_the_checker_alone(checker, normals_checker, align_checker, score_checker):
    """A rotation of 130 degrees and a shift of several diameters: ICP alone matches nothing; the registration finds the transform
    with at least half of its matches as inliers of the best trial; after it ICP ends with every point of P within tau of Q."""
    p, pn, q, qn, chosen = planted_case(normals_checker, align_checker)
    assert len(q) == 2000 and len(p) == 1333 and np.linalg.norm(PLANTED_T) > 3 * np.linalg.norm(q.max(axis=0) - q.min(axis=0))
    alone = PA.align(align_checker, p, q, PLANTED_ICP)
    assert (alone.stopped, alone.matched_before, alone.steps) == (PA.TOO_FEW, 0, 0)
    r = RC.register(checker, p, pn, q, qn, PLANTED_RADIUS, inlier_distance=PLANTED_INLIER)
    print(r)
    assert r.stopped == RC.OK and r.matches >= 3 and 2 * r.inliers >= r.matches and r.inliers_after >= r.inliers // 2 and r.scale == 1.0
    assert r.features_p > 0.9 * len(p) and r.features_q > 0.9 * len(q) and 0 <= r.best_trial < 4096 and 0 < r.trials_admitted <= 4096
    R = np.asarray(r.rotation).reshape(3, 3)
    assert np.abs(R - PLANTED_R).max() < 0.01 and np.abs(np.asarray(r.translation) - PLANTED_T).max() < 0.2 and r.rms_after < PLANTED_INLIER
    index, _ = RC.match_features(checker, p, pn, q, qn, PLANTED_RADIUS)
    assert (index >= 0).sum() == r.matches and 2 * (index == chosen).sum() >= r.matches
    moved, _ = PA.transformed(align_checker, p, pn, r.scale, r.rotation, r.translation)
    refined = PA.align(align_checker, moved, q, PLANTED_ICP, iterations=32)
    assert refined.matched_after == len(p) and refined.rms_after < PLANTED_TAU / 10
    final, _ = PA.transformed(align_checker, moved, pn, refined.scale, refined.rotation, refined.translation)
    score = PX.score(score_checker, final, q, PLANTED_TAU)
    assert score.p_within == len(p), score
    scaled = RC.register(checker, p, pn, q, qn, PLANTED_RADIUS, inlier_distance=PLANTED_INLIER, with_scale=True)
    assert scaled.stopped == RC.OK and abs(scaled.scale - 1.0) < 0.01 and scaled.scale != 1.0 and scaled.best_trial == r.best_trial


# --------------------------------------------------------------------------------------------------------------------
# every way it ends
# --------------------------------------------------------------------------------------------------------------------

IDENTITY = (1.0, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0))


def test_every_stop_is_reached_by_a_hand_made_case(checker):
    rng = np.random.default_rng(4)
    q = rng.uniform(-3, 3, (40, 3)).astype(np.float32)
    R, t = rotation(100.0), np.float64([5, 6, 7])
    p = ((q.astype(np.float64) - t) @ R).astype(np.float32)
    pairs = np.column_stack([np.arange(40), np.arange(40)])
    for M in range(3):
        r = RC.register_matches(checker, p, q, pairs[:M], 0.01)
        assert r[:3] == IDENTITY and (r.stopped, r.matches, r.trials_admitted, r.best_trial, r.inliers) == (RC.TOO_FEW_MATCHES, M, 0, -1, 0), r
    r = RC.register_matches(checker, p, q, pairs[:3], 0.01, trials=1)
    assert (r.stopped, r.matches, r.trials_admitted, r.best_trial, r.inliers, r.inliers_after) == (RC.OK, 3, 1, 0, 3, 3), r
    assert np.abs(np.asarray(r.rotation).reshape(3, 3) - R).max() < 1e-6 and r.rms_after < 1e-5
    r = RC.register_matches(checker, p, q, pairs, 0.01)
    assert (r.stopped, r.inliers, r.inliers_after) == (RC.OK, 40, 40) and np.abs(np.asarray(r.translation) - t).max() < 1e-5
    # no trial is admitted: one side three times the size of the other
    r = RC.register_matches(checker, 3 * p, q, pairs, 0.01)
    assert r[:3] == IDENTITY and (r.stopped, r.trials_admitted, r.best_trial, r.inliers) == (RC.NO_TRIAL, 0, -1, 0), r
    r = RC.register_matches(checker, 3 * p, q, pairs, 0.01, edge_ratio=0.3)
    assert r.trials_admitted == 4096 and r.stopped == RC.NO_TRIAL and r.inliers < 3 and r.best_trial >= 0 and r[:3] == IDENTITY
    # degenerate triangles: every point of one side at one position
    r = RC.register_matches(checker, np.zeros_like(p), q, pairs, 0.01, edge_ratio=1e-30)
    assert (r.stopped, r.trials_admitted) == (RC.NO_TRIAL, 0)
    # admitted, but nothing lands within the distance: wrong partners, triangles alike within the ratio by chance alone
    shuffled = np.column_stack([np.arange(40), rng.permutation(40)])
    r = RC.register_matches(checker, p, q, shuffled, 1e-4, edge_ratio=0.5)
    assert r.trials_admitted > 0 and r.stopped == RC.NO_TRIAL and r.inliers < 3 and r[:3] == IDENTITY, r


def test_trials_that_tie_on_inliers_leave_the_lowest(checker):
    """Exact partners: every admitted trial has all the matches as inliers, and the first admitted one is the best."""
    rng = np.random.default_rng(6)
    q = rng.integers(-8, 8, (30, 3)).astype(np.float32)
    p = q[:, [1, 2, 0]].copy()                                  # a rotation that binary32 holds exactly
    pairs = np.column_stack([np.arange(30), np.arange(30)])
    first = None
    for trials in (1, 2, 3, 63, 64, 65, 257):
        r = RC.register_matches(checker, p, q, pairs, 0.5, trials=trials)
        if r.trials_admitted > 0:
            first = r.best_trial if first is None else first
            assert r.best_trial == first and r.inliers == 30 and r.stopped == RC.OK, (trials, r)
            assert r.trials_admitted > 1 or trials < 3
    assert first is not None


# --------------------------------------------------------------------------------------------------------------------
# the C ABI without a device
# --------------------------------------------------------------------------------------------------------------------

def test_header_declares_the_entry_points_as_ctypes_calls_them(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "apd_mi355x.h")).read(), flags=re.S)
    common = r"\s*float\s+\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,"
    assert re.search(r"int\s+apd_points_features\s*\(\s*apd_points_t\s+\w+\s*," + common + r"\s*unsigned\s+\w+\s*,\s*float\s*\*\s*\w+\s*,"
                     r"\s*unsigned\s+char\s*\*\s*\w+\s*\)", text)
    assert re.search(r"int\s+apd_points_match_features\s*\(\s*apd_points_t\s+\w+\s*,\s*apd_points_t\s+\w+\s*," + common +
                     r"\s*unsigned\s+\w+\s*,\s*int\s+\w+\s*,\s*int32_t\s*\*\s*\w+\s*,\s*float\s*\*\s*\w+\s*\)", text)
    assert re.search(r"int\s+apd_points_register\s*\(\s*apd_points_t\s+\w+\s*,\s*apd_points_t\s+\w+\s*," + common +
                     r"\s*const\s+apd_points_register_options\s*\*\s*\w+\s*,\s*apd_points_registration_t\s*\*\s*\w+\s*\)", text)
    assert re.search(r"typedef\s+struct\s*\{\s*unsigned\s+trials\s*;\s*unsigned\s+long\s+long\s+seed\s*;\s*float\s+inlier_distance\s*;\s*float\s+edge_ratio\s*;"
                     r"\s*unsigned\s+min_neighbours\s*;\s*int\s+mutual\s*;\s*int\s+with_scale\s*;\s*\}\s*apd_points_register_options\s*;", text)
    assert re.search(r"typedef\s+struct\s*\{\s*double\s+scale\s*,\s*rotation\[9\]\s*,\s*translation\[3\]\s*;\s*long\s+long\s+features_p\s*,\s*features_q\s*,"
                     r"\s*matches\s*,\s*trials_admitted\s*,\s*best_trial\s*,\s*inliers\s*,\s*inliers_after\s*;\s*double\s+rms_after\s*;\s*int\s+stopped\s*;"
                     r"\s*\}\s*apd_points_registration_t\s*;", text)
    assert re.search(r"APD_REGISTER_OK\s*=\s*0\s*,\s*APD_REGISTER_TOO_FEW_MATCHES\s*=\s*1\s*,\s*APD_REGISTER_NO_TRIAL\s*=\s*2", text)
    L = pkg.lib()
    assert L.apd_points_features.argtypes == [C.c_void_p, C.c_float, C.POINTER(C.c_float), C.c_uint, C.c_void_p, C.c_void_p]
    assert L.apd_points_match_features.argtypes == [C.c_void_p, C.c_void_p, C.c_float, C.POINTER(C.c_float), C.c_uint, C.c_int, C.c_void_p, C.c_void_p]
    assert L.apd_points_register.argtypes == [C.c_void_p, C.c_void_p, C.c_float, C.POINTER(C.c_float), C.POINTER(pkg.PointsRegisterOptions),
                                              C.POINTER(pkg.PointsRegistration)]
    assert [n for n, _ in pkg.PointsRegistration._fields_] == list(RC.FIELDS) == list(pkg.Registration._fields)
    assert [(n, t) for n, t in pkg.PointsRegisterOptions._fields_] == [(n, t) for n, t in RC._Options._fields_]
    assert C.sizeof(pkg.PointsRegistration) == 176 and C.sizeof(pkg.PointsRegisterOptions) == 40
    assert (pkg.REGISTER_OK, pkg.REGISTER_TOO_FEW_MATCHES, pkg.REGISTER_NO_TRIAL) == (RC.OK, RC.TOO_FEW_MATCHES, RC.NO_TRIAL)
    assert pkg.FEATURE_WIDTH == RC.WIDTH == 33


def test_library_exports_the_entry_points(pkg):
    for name in NEW_SYMBOLS:
        assert hasattr(pkg.lib(), name), name


def test_refusals_that_need_no_device(pkg):
    """Every bad argument answers with its code and a message that starts with the call's name and leaves the outputs as they
    were: no device is touched, so this passes on a machine without one."""
    L = pkg.lib()
    pts = from_cloud(pkg, cloud([[0.5, 0, 0], [0.6, 0, 0]]), [4], [5], [[]])
    other = from_cloud(pkg, cloud([[0.5, 0, 0], [0.6, 0, 0], [0.7, 0, 0]]), [4], [5], [[]])
    out = pkg.PointsRegistration()
    out.scale, out.stopped = -7.0, -7
    features, has = np.full(66, -7.0, np.float32), np.full(2, 7, np.uint8)
    index, distance = np.full(2, -7, np.int32), np.full(2, -7.0, np.float32)
    good = (64, 0, 0.5, 0.9, 3, 1, 0)

    def refused(call, message, *, p=pts._p, q=other._p, radius=1.0, origin=None, least=3, options=good, null_output=False, code=-1, bound=None):
        org = None if origin is None else (C.c_float * 3)(*origin)
        if call == "apd_points_features":
            rc = L.apd_points_features(p, radius, org, least, None if null_output else C.c_void_p(features.ctypes.data), C.c_void_p(has.ctypes.data))
        elif call == "apd_points_match_features":
            outputs = (None, None) if null_output else (C.c_void_p(index.ctypes.data), C.c_void_p(distance.ctypes.data))
            rc = (L.apd_points_match_features(p, q, radius, org, least, 1, *outputs) if bound is None else
                  L.apd_points_match_features_bounded(p, q, radius, org, least, 1, bound, *outputs))
        else:
            opt = None if options is None else C.byref(pkg.PointsRegisterOptions(*options))
            rc = L.apd_points_register(p, q, radius, org, opt, None if null_output else C.byref(out))
        assert rc == code, (call, message, rc)
        assert L.apd_fusion_last_error().decode() == call + ": " + message
        assert out.scale == -7.0 and out.stopped == -7 and (features == -7.0).all() and (has == 7).all() and (index == -7).all() and (distance == -7.0).all()

    for call in ("apd_points_features", "apd_points_match_features", "apd_points_register"):
        refused(call, "null argument", p=None)
        refused(call, "null argument", null_output=True)
        for (radius, origin), message in BAD_RADIUS:
            refused(call, message, radius=radius, origin=origin)
        if call != "apd_points_register":
            refused(call, "min_neighbours = 2, below 3", least=2)
            refused(call, "min_neighbours = 0, below 3", least=0)
        if call != "apd_points_features":
            refused(call, "null argument", q=None)
    refused("apd_points_match_features", "a launch bound of 0 pairs", bound=0)
    refused("apd_points_register", "min_neighbours = 2, below 3", options=(64, 0, 0.5, 0.9, 2, 1, 0))
    refused("apd_points_register", "trials = 0, not in 1 .. 65536", options=(0,) + good[1:])
    refused("apd_points_register", "trials = 65537, not in 1 .. 65536", options=(65537,) + good[1:])
    for bad, text in ((0.0, "0"), (-1.0, "-1"), (float("nan"), "nan"), (float("inf"), "inf"), (1e30, "1e+30"), (1e-30, "1e-30")):
        refused("apd_points_register", "an inlier distance of %s, not a positive finite number with such a square" % text, options=good[:2] + (bad,) + good[3:])
    for bad, text in ((0.0, "0"), (-0.5, "-0.5"), (1.5, "1.5"), (float("nan"), "nan")):
        refused("apd_points_register", "an edge ratio of %s, not in (0, 1]" % text, options=good[:3] + (bad,) + good[4:])
    many = from_cloud(pkg, cloud(np.zeros((2 ** 18 + 1, 3), np.float32)), [4], [5], [[]])
    message = ("262145 points, more than 262144: matching costs the product of the two counts; thin the cloud first (apd_points_merge_voxels)")
    refused("apd_points_register", message, p=many._p, code=-5)
    refused("apd_points_register", message, q=many._p, code=-5)
    refused("apd_points_match_features", message, q=many._p, code=-5)
    with pytest.raises(pkg.ApdError, match="apd_points_register: trials = 0"):
        pts.register(other, 1.0, trials=0)
    with pytest.raises(pkg.ApdError, match="apd_points_register: an edge ratio of 2"):
        pts.register(other, 1.0, edge_ratio=2.0)
    with pytest.raises(pkg.ApdError, match="apd_points_features: min_neighbours = 1"):
        pts.features(1.0, min_neighbours=1)
    with pytest.raises(pkg.ApdError, match="apd_points_match_features: a radius of 0"):
        pts.match_features(other, 0.0)
    with pytest.raises(pkg.ApdError, match="Points.register: the other points are closed or not a Points"):
        pts.register(None, 1.0)


def test_objects_without_points_give_their_answers_without_a_device(pkg):
    empty = from_cloud(pkg, cloud(np.zeros((0, 3), np.float32)), [4], [5], [[]])
    some = from_cloud(pkg, cloud([[0.5, 0, 0], [0.6, 0, 0]]), [4], [5], [[]])
    for p, q in ((empty, some), (some, empty), (empty, empty)):
        r = p.register(q, 1.0, with_scale=True)
        assert r._fields == RC.FIELDS and RC.bits(r) == RC.bits(RC.Registration(*IDENTITY, 0, 0, 0, 0, -1, 0, 0, 0.0, RC.TOO_FEW_MATCHES)), r
        assert r.rotation.shape == (3, 3) and r.translation.shape == (3,) and isinstance(r.matches, int)
    f, has = empty.features(1.0)
    assert f.shape == (0, 33) and f.dtype == np.float32 and has.shape == (0,) and has.dtype == np.uint8
    index, distance = empty.match_features(some, 1.0)
    assert index.shape == (0,) and index.dtype == np.int32 and distance.dtype == np.float32
    index, distance = some.match_features(empty, 1.0)
    assert index.tolist() == [-1, -1] and np.isposinf(distance).all()
    assert empty.transformed(empty.register(some, 1.0)).count == 0


def test_no_gpu_means_the_registration_fails_loudly(pkg):
    """There is no host implementation: without a device non-empty host objects are refused with a message."""
    if pkg.device_count() > 0:
        pytest.skip("a GPU is visible")
    pts = from_cloud(pkg, cloud([[0.5, 0, 0], [0.6, 0, 0]]), [4], [5], [[]])
    with pytest.raises(pkg.ApdError, match=r"apd_points_features: hipSetDevice\("):
        pts.features(1.0)
    with pytest.raises(pkg.ApdError, match=r"apd_points_match_features: hipSetDevice\("):
        pts.match_features(pts, 1.0)
    with pytest.raises(pkg.ApdError, match=r"apd_points_register: hipSetDevice\("):
        pts.register(pts, 1.0)


# --------------------------------------------------------------------------------------------------------------------
# the kernels' resources
# --------------------------------------------------------------------------------------------------------------------

NEW_KERNELS = {"k_register_frames": "0", "k_register_spfh": "8448", "k_register_fpfh": "0", "k_register_flags": "0", "k_register_compact": "0",
               "k_register_match": str(MATCH_TILE * 33 * 4), "k_register_matches": "0", "k_register_count": "6144", "k_register_gather": "0", "k_register_mark": "0"}


def test_no_new_kernel_uses_scratch_memory(tmp_path):
    """Every kernel of apd_points_register.hip: 0 bytes of scratch per lane and no spilled register; the LDS each one declares --
    33 counters for 64 lanes, a tile of 128 descriptors, a tile of 256 matches.  Registers and occupancy are printed."""
    found = kernel_resources("apd_points_register.hip", tmp_path)
    for kernel, lds in NEW_KERNELS.items():
        mine = [v for k, v in found.items() if kernel + "E" in k]
        assert len(mine) == 1, (kernel, sorted(found))
        print(kernel, "VGPRs", mine[0]["VGPRs"], "SGPRs", mine[0]["TotalSGPRs"], "LDS", mine[0]["LDS Size [bytes/block]"], "occupancy",
              mine[0]["Occupancy [waves/SIMD]"])
        assert mine[0]["ScratchSize [bytes/lane]"] == "0" and mine[0]["VGPRs Spill"] == "0" and mine[0]["SGPRs Spill"] == "0", (kernel, mine[0])
        assert mine[0]["LDS Size [bytes/block]"] == lds, (kernel, mine[0])
    for name, v in found.items():
        assert v["ScratchSize [bytes/lane]"] == "0", name
