"""FPFH descriptors, their matches and the registration to another cloud on the device (apd_points_features,
apd_points_match_features, apd_points_register; csrc/apd_points_register.hip), bitwise against the grid mode of the sequential
checker (tests/helpers/points_register_ref.cpp): descriptors and distances as uint32, indices, every field of the Registration
with the doubles as uint64, for host- and device-resident points on either side.  The clouds are made in test_points_register.py,
where the checker's two modes are held against each other on them; here also: the match kernel's tile and launch bound, ties,
the numbers of trials, a planted transform through register, transformed, align and score, two runs, the same object on both
sides, the pipeline, the drop-in binary and a real fused cloud turned far away and brought back."""
import shutil
import subprocess

import numpy as np
import pytest

import fusion_cases
import points_align_checker as PA
import points_normals_checker as PN
import points_radius_checker as PR
import points_register_checker as RC
from test_gpu_dropin_binary import _write_dense_folder
from test_gpu_fusion_options import APD_BIN, _run, _scene
from test_gpu_points_average import fused
from test_gpu_points_nearest import RESIDENCIES, host, run_binary
from test_points_align import rotation
from test_points_nearest import bits32
from test_points_normals import REAL_CLOUD
from test_points_radius import real_cloud_radius
from test_points_register import (MATCH_TILE, PLANTED_ICP, PLANTED_INLIER, PLANTED_NORMALS, PLANTED_R, PLANTED_RADIUS, PLANTED_T, PLANTED_TAU, SIZES, planted_case,
                                  register_cases, surface)
from test_points_voxel import arrays_of, cloud, from_cloud

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return RC.build(tmp_path_factory.mktemp("points_register_checker"))


@pytest.fixture(scope="module")
def align_checker(tmp_path_factory):
    return PA.build(tmp_path_factory.mktemp("points_align_checker"))


@pytest.fixture(scope="module")
def normals_checker(tmp_path_factory):
    return PN.build(tmp_path_factory.mktemp("points_normals_checker"))


@pytest.fixture(scope="module")
def planted(normals_checker, align_checker):
    return planted_case(normals_checker, align_checker)


def points_with(pkg, xyz, normal, on_device):
    return from_cloud(pkg, cloud(xyz, normal=np.ascontiguousarray(normal, np.float32)), [4], [5], [[]], on_device=on_device)


def assert_features(got, want, what):
    f, has = host(got[0]), host(got[1])
    assert f.dtype == np.float32 and has.dtype == np.uint8 and f.shape == want[0].shape and has.shape == want[1].shape, what
    assert np.array_equal(has, want[1]), (what, np.flatnonzero(has != want[1])[:5])
    differ = np.flatnonzero((bits32(f) != bits32(want[0])).any(axis=1)) if len(f) else np.zeros(0, int)
    assert differ.size == 0, (what, differ[:5], f[differ[:1]], want[0][differ[:1]])


def assert_matches(got, want, what):
    index, distance = host(got[0]), host(got[1])
    assert index.dtype == np.int32 and distance.dtype == np.float32 and index.shape == distance.shape == want[0].shape, what
    differ = np.flatnonzero((index != want[0]) | (bits32(distance) != bits32(want[1])))
    assert differ.size == 0, (what, differ[:5], index[differ[:5]], want[0][differ[:5]], distance[differ[:5]], want[1][differ[:5]])


def assert_registration(got, want, what):
    assert got._fields == RC.FIELDS and got.rotation.shape == (3, 3) and got.rotation.dtype == np.float64 and got.translation.shape == (3,), what
    assert RC.bits(got) == RC.bits(want), (what, got, want)


# --------------------------------------------------------------------------------------------------------------------
# every pair of clouds
# --------------------------------------------------------------------------------------------------------------------

def test_every_pair_of_clouds(gpu_pkg, checker):
    """Sizes 0, 1, 2 and around a wave and a block on either side, points outside the grid, a crowded cell, another origin, zero
    and non-finite normals, a cloud in which no point reaches min_neighbours, 0 .. 3 matches: descriptors of both clouds in both
    memories, matches with and without the mutual test and the registration at 65 trials in all four residencies."""
    stops, sizes = set(), set()
    for name, (p, pn, q, qn, radius, origin, least) in register_cases(gpu_pkg).items():
        points = {(side, dev): points_with(gpu_pkg, xyz, normal, dev) for side, xyz, normal in (("p", p, pn), ("q", q, qn)) for dev in (False, True)}
        for side, xyz, normal in (("p", p, pn), ("q", q, qn)):
            want = RC.features(checker, xyz, normal, radius, origin, least)
            for dev in (False, True):
                assert_features(points[side, dev].features(radius, least, origin), want, (name, side, dev))
        matches = {mutual: RC.match_features(checker, p, pn, q, qn, radius, origin, least, mutual) for mutual in (False, True)}
        kw = dict(trials=65, min_neighbours=least, mutual=False, inlier_distance=0.5)
        want = RC.register(checker, p, pn, q, qn, radius, origin, **kw)
        stops.add(want.stopped)
        sizes.add(len(p))
        for p_dev, q_dev in RESIDENCIES:
            for mutual in (False, True):
                got = points["p", p_dev].match_features(points["q", q_dev], radius, least, mutual, origin)
                assert_matches(got, matches[mutual], (name, p_dev, q_dev, mutual))
            assert_registration(points["p", p_dev].register(points["q", q_dev], radius, origin=origin, **kw), want, (name, p_dev, q_dev))
        if name.endswith(" matches"):
            assert want.matches == int(name.split()[0]) == (matches[False][0] >= 0).sum(), (name, want)
        if name == "no point reaches min_neighbours":
            assert want.features_p == 0 and want.stopped == RC.TOO_FEW_MATCHES
    assert sizes >= set(SIZES) and stops >= {RC.OK, RC.TOO_FEW_MATCHES}


# --------------------------------------------------------------------------------------------------------------------
# the match kernel
# --------------------------------------------------------------------------------------------------------------------

def patch_with(checker, target, seed):
    """The shortest leading patch of the surface in which exactly `target` points have a descriptor at radius 1, min_neighbours 3,
    with random normals: (positions, normals)."""
    s = surface()
    s = s[np.argsort(s[:, 0] + s[:, 1], kind="stable")]
    normal = np.random.default_rng(seed).normal(size=(len(s), 3)).astype(np.float32)
    for n in range(target, len(s)):
        if int(RC.features(checker, s[:n], normal[:n], 1.0, None, 3)[1].sum()) == target:
            return s[:n], normal[:n]
    raise AssertionError("no patch with %d descriptors" % target)


def test_candidates_around_the_tile_and_the_launch_bound(gpu_pkg, checker):
    """Q with one descriptor fewer than, exactly and one more than the LDS tile holds; and launches bounded so that Q has one
    candidate more than a launch takes, so that a launch takes fewer pairs than there are queries, and one pair at a time: the
    results do not depend on the bound."""
    p, pn = patch_with(checker, 70, 1)
    P = {dev: points_with(gpu_pkg, p, pn, dev) for dev in (False, True)}
    for count in (MATCH_TILE - 1, MATCH_TILE, MATCH_TILE + 1):
        q, qn = patch_with(checker, count, 2)
        Q = {dev: points_with(gpu_pkg, q, qn, dev) for dev in (False, True)}
        for mutual in (False, True):
            want = RC.match_features(checker, p, pn, q, qn, 1.0, None, 3, mutual)
            assert (want[0] >= 0).sum() > 0
            for p_dev, q_dev in RESIDENCIES:
                assert_matches(P[p_dev].match_features(Q[q_dev], 1.0, 3, mutual), want, (count, mutual, p_dev, q_dev))
            for bound in (70 * (count - 1), 70 * count, 69, 1):
                assert_matches(P[True].match_features(Q[True], 1.0, 3, mutual, _pair_bound=bound), want, (count, mutual, bound))


def test_equal_descriptors_go_to_the_smallest_index(gpu_pkg, checker):
    """Q twice over: a point and its copy have the same neighbours but each other, which a pair at distance 0 skips, so many
    descriptors tie bit for bit, and the match of every point of P is then in the first copy."""
    q, qn = patch_with(checker, 150, 3)
    twice, twice_normals = np.concatenate([q, q]), np.concatenate([qn, qn])
    f, has = RC.features(checker, twice, twice_normals, 1.0, None, 3)
    tied = has[:len(q)].astype(bool) & (bits32(f[:len(q)]) == bits32(f[len(q):])).all(axis=1)
    assert tied.sum() > 50
    want = RC.match_features(checker, q, qn, twice, twice_normals, 1.0, None, 3, False)
    assert (want[0][tied] >= 0).all() and (want[0][tied] < len(q)).all()
    for p_dev, q_dev in RESIDENCIES:
        got = points_with(gpu_pkg, q, qn, p_dev).match_features(points_with(gpu_pkg, twice, twice_normals, q_dev), 1.0, 3, False)
        assert_matches(got, want, (p_dev, q_dev))


# --------------------------------------------------------------------------------------------------------------------
# the trials
# --------------------------------------------------------------------------------------------------------------------

def small_planted(planted, count=500):
    p, pn, q, qn, chosen = planted
    return p[:count], pn[:count], q[:int(chosen[count - 1]) + 1], qn[:int(chosen[count - 1]) + 1]


def test_numbers_of_trials_and_an_edge_ratio_that_admits_none(gpu_pkg, checker, planted):
    """1, 63, 64, 65 and 257 trials -- around a wave of the count kernel, and several workgroups -- rigid and with scale, in all
    four residencies; edge ratios off the default: a loose one, a tight one, and 1, which asks for equal squared lengths and so
    admits no trial on positions that a rotation has rounded; one side three times the size of the other admits none either."""
    p, pn, q, qn = small_planted(planted)
    P = {dev: points_with(gpu_pkg, p, pn, dev) for dev in (False, True)}
    Q = {dev: points_with(gpu_pkg, q, qn, dev) for dev in (False, True)}
    admitted = {}
    for trials in (1, 63, 64, 65, 257):
        for with_scale in (False, True):
            kw = dict(inlier_distance=PLANTED_INLIER, trials=trials, seed=trials, with_scale=with_scale)
            want = RC.register(checker, p, pn, q, qn, PLANTED_RADIUS, **kw)
            for p_dev, q_dev in RESIDENCIES:
                assert_registration(P[p_dev].register(Q[q_dev], PLANTED_RADIUS, **kw), want, (trials, with_scale, p_dev, q_dev))
            admitted[trials] = want.trials_admitted
            assert want.matches > 100 and want.trials_admitted <= trials
    assert max(admitted.values()) > 64
    by_ratio = {}
    for edge_ratio in (0.5, 0.97, 1.0):
        kw = dict(inlier_distance=PLANTED_INLIER, trials=257, seed=257, edge_ratio=edge_ratio)
        want = RC.register(checker, p, pn, q, qn, PLANTED_RADIUS, **kw)
        by_ratio[edge_ratio] = want.trials_admitted
        for p_dev, q_dev in RESIDENCIES:
            assert_registration(P[p_dev].register(Q[q_dev], PLANTED_RADIUS, **kw), want, (edge_ratio, p_dev, q_dev))
        if edge_ratio == 1.0:
            assert (want.stopped, want.trials_admitted, want.best_trial, want.scale) == (RC.NO_TRIAL, 0, -1, 1.0), want
    assert by_ratio[0.5] > admitted[257] > by_ratio[0.97] > by_ratio[1.0] == 0, (by_ratio, admitted)
    big = (3 * p.astype(np.float64)).astype(np.float32)
    want = RC.register(checker, big, pn, q, qn, PLANTED_RADIUS, inlier_distance=PLANTED_INLIER, min_neighbours=3, mutual=False)
    assert want.matches >= 3 and (want.stopped, want.trials_admitted, want.best_trial) == (RC.NO_TRIAL, 0, -1), want
    got = points_with(gpu_pkg, big, pn, False).register(Q[False], PLANTED_RADIUS, PLANTED_INLIER, min_neighbours=3, mutual=False)
    assert_registration(got, want, "no trial")
    assert got.scale == 1.0 and np.array_equal(got.rotation, np.eye(3)) and not got.translation.any()


def test_the_same_object_on_both_sides_and_trials_that_tie(gpu_pkg, checker, planted):
    """With the mutual test every match is a point with itself at distance 0 -- of several points with one descriptor, the flat
    parts of the surface have such, only the first stays --, so every admitted trial has every match as an inlier and the first
    admitted one is the best; the identity comes back as the refit returns it: the checker's bits, within rounding of the identity."""
    _, _, q, qn = small_planted(planted)
    for dev in (False, True):
        pts = points_with(gpu_pkg, q, qn, dev)
        index, distance = (host(a) for a in pts.match_features(pts, PLANTED_RADIUS))
        loose = host(pts.match_features(pts, PLANTED_RADIUS, mutual=False)[0])
        has = host(pts.features(PLANTED_RADIUS)[1]).astype(bool)
        kept = index >= 0
        assert np.array_equal(index[kept], np.flatnonzero(kept)) and not distance[kept].any() and not kept[~has].any() and kept.sum() > 100
        assert np.array_equal(loose >= 0, has) and (loose <= np.arange(len(q)))[has].all() and np.array_equal(loose[kept], index[kept])
        results = {}
        for trials in (8, 64):
            want = RC.register(checker, q, qn, q, qn, PLANTED_RADIUS, inlier_distance=PLANTED_INLIER, trials=trials)
            got = pts.register(pts, PLANTED_RADIUS, PLANTED_INLIER, trials=trials)
            assert_registration(got, want, (dev, trials))
            results[trials] = got
            assert got.stopped == gpu_pkg.REGISTER_OK and got.inliers == got.matches == got.inliers_after == kept.sum() and got.trials_admitted > 1
            assert np.abs(got.rotation - np.eye(3)).max() < 1e-12 and np.abs(got.translation).max() < 1e-10 and got.rms_after < 1e-6
        assert results[8].best_trial == results[64].best_trial          # every admitted trial ties: the lowest stays


def test_two_calls_give_identical_bits(gpu_pkg, checker, planted):
    p, pn, q, qn = small_planted(planted)
    for p_dev, q_dev in RESIDENCIES:
        P, Q = points_with(gpu_pkg, p, pn, p_dev), points_with(gpu_pkg, q, qn, q_dev)
        runs = [RC.bits(P.register(Q, PLANTED_RADIUS, PLANTED_INLIER, trials=300, seed=9)) for _ in range(2)]
        assert runs[0] == runs[1]
    f = [bits32(host(P.features(PLANTED_RADIUS)[0])) for _ in range(2)]
    assert np.array_equal(f[0], f[1])
    other = RC.bits(P.register(Q, PLANTED_RADIUS, PLANTED_INLIER, trials=300, seed=10))
    assert other != runs[0]                                             # the seed is used


# --------------------------------------------------------------------------------------------------------------------
# the planted case
# --------------------------------------------------------------------------------------------------------------------

def test_the_planted_transform_through_register_transformed_align_and_score(gpu_pkg, checker, planted):
    """Q's normals from with_estimated_normals on the device; ICP alone matches nothing; the registration is the checker's in every
    bit, so it registers what the checker registers (test_points_register.py asserts that it does); the chain ends with every
    point of P within tau of Q."""
    p, pn, q, qn, chosen = planted
    want = RC.register(checker, p, pn, q, qn, PLANTED_RADIUS, inlier_distance=PLANTED_INLIER)
    assert want.stopped == RC.OK and 2 * want.inliers >= want.matches
    for p_dev, q_dev in RESIDENCIES:
        Q, estimated = from_cloud(gpu_pkg, cloud(q), [4], [5], [[]], on_device=q_dev).with_estimated_normals(PLANTED_NORMALS, 5)
        assert estimated == len(q) and np.array_equal(bits32(host(Q.normal)), bits32(qn))
        P = points_with(gpu_pkg, p, pn, p_dev)
        alone = P.align(Q, PLANTED_ICP)
        assert (alone.stopped, alone.matched_before) == (gpu_pkg.ALIGN_TOO_FEW, 0)
        got = P.register(Q, PLANTED_RADIUS, PLANTED_INLIER)
        assert_registration(got, want, (p_dev, q_dev))
        assert np.abs(got.rotation - PLANTED_R).max() < 0.01 and np.abs(got.translation - PLANTED_T).max() < 0.2
        moved = P.transformed(got)
        refined = moved.align(Q, PLANTED_ICP, iterations=32)
        final = moved.transformed(refined)
        score = final.score(Q, PLANTED_TAU)
        assert refined.matched_after == len(p) and score.p_within == len(p) == score.n_p, (refined, score)
        assert P.score(Q, PLANTED_TAU).p_within == 0


# --------------------------------------------------------------------------------------------------------------------
# the pipeline and a real cloud
# --------------------------------------------------------------------------------------------------------------------

def far_away(pkg, pts, path=None):
    """`pts` under 170 degrees about (1, 2, 3) through its centre and a shift of ten times its extent, as a host-resident truth."""
    xyz = host(pts.xyz)
    finite = xyz[np.isfinite(xyz).all(axis=1)].astype(np.float64)
    R, centre = rotation(170.0), finite.mean(axis=0)
    t = centre - R @ centre + 10.0 * (finite.max(axis=0) - finite.min(axis=0))
    moved = pts.transformed(1.0, R, t)
    if path is not None:
        moved.write_ply(path, normals=True)
        return pkg.Points.read_ply(path), R, t
    return moved, R, t


def test_through_the_pipeline(gpu_pkg, ob, checker, align_checker, tmp_path):
    """fuse(register=...) moves the points every other option has produced: the returned points, the file and the registration are
    those of Points.register and Points.transformed on the result without the option, which the checker confirms; align= and
    score= follow on the moved points; without the option every file keeps its bytes."""
    from apd_mvs_amd import pipeline
    case = fusion_cases.case("mixed_sizes")
    scene, results = _scene(gpu_pkg, pipeline, case)
    kw = dict(average=True, voxel=0.05)
    n, whole = pipeline.fuse(scene, results, tmp_path / "plain.ply", return_points=True, vis_path=tmp_path / "plain.vis", **kw)
    w = arrays_of(whole)
    radius = float(np.float32(4.0 * real_cloud_radius(PR.build(tmp_path), w)))
    truth, R, t = far_away(gpu_pkg, whole, tmp_path / "truth.ply")
    t_xyz, t_normal = np.asarray(truth.xyz), np.asarray(truth.normal)
    want = RC.register(checker, w.xyz, w.normal, t_xyz, t_normal, radius, inlier_distance=radius / 2, trials=512, seed=3)
    print(n, "points, radius", radius, want)
    got = whole.register(truth, radius, radius / 2, trials=512, seed=3)
    assert_registration(got, want, "by hand")
    by_hand = whole.transformed(got)
    by_hand.write_ply(tmp_path / "by_hand.ply")
    m, pts, r = pipeline.fuse(scene, results, tmp_path / "m.ply", return_points=True, vis_path=tmp_path / "m.vis", register=(truth, radius, radius / 2, 512, 3), **kw)
    assert m == n == pts.count
    assert_registration(r, want, "pipeline")
    want_xyz, want_normal = PA.transformed(align_checker, w.xyz, w.normal, want.scale, want.rotation, want.translation)
    after = arrays_of(pts)
    assert np.array_equal(bits32(after.xyz), bits32(want_xyz)) and np.array_equal(bits32(after.normal), bits32(want_normal))
    assert (tmp_path / "m.ply").read_bytes() == (tmp_path / "by_hand.ply").read_bytes()
    assert (tmp_path / "m.vis").read_bytes() == (tmp_path / "plain.vis").read_bytes()
    m, r = pipeline.fuse(scene, results, tmp_path / "file_only.ply", register=(truth, radius, radius / 2, 512, 3), **kw)
    assert m == n and RC.bits(r) == RC.bits(want) and (tmp_path / "file_only.ply").read_bytes() == (tmp_path / "by_hand.ply").read_bytes()
    m, r, a, s = pipeline.fuse(scene, results, tmp_path / "all.ply", register=(truth, radius, radius / 2, 512, 3), align=(truth, radius, 4), score=(truth, radius / 4), **kw)
    assert RC.bits(r) == RC.bits(want)
    by_both = by_hand.align(truth, radius, iterations=4)
    assert PA.bits(a) == PA.bits(by_both) and s == by_hand.transformed(by_both).score(truth, radius / 4)
    with pytest.raises(ValueError, match="register="):
        pipeline.fuse(scene, results, tmp_path / "bad.ply", register=(truth, radius, radius / 2, 512, 3, 4), **kw)
    pipeline.fuse(scene, results, tmp_path / "again.ply", vis_path=tmp_path / "again.vis", **kw)
    assert (tmp_path / "again.ply").read_bytes() == (tmp_path / "plain.ply").read_bytes()
    assert (tmp_path / "again.vis").read_bytes() == (tmp_path / "plain.vis").read_bytes()


def test_a_real_cloud_turned_far_away_and_brought_back(gpu_pkg, ob, checker, tmp_path_factory):
    """A fused cloud thinned by merge_voxels, with its own normals, under 170 degrees and a shift of ten extents: ICP alone finds
    nothing; the registration is the checker's in every bit in all four residencies and brings the cloud back onto itself."""
    radius_checker = PR.build(tmp_path_factory.mktemp("points_radius_checker"))
    name, variant, _ = REAL_CLOUD
    case = fusion_cases.case(name)
    whole = fused(gpu_pkg, ob, case, variant, False)
    voxel = real_cloud_radius(radius_checker, arrays_of(whole))
    thin, _ = whole.merge_voxels(voxel)
    while thin.count > 3000:
        voxel *= 1.5
        thin, _ = whole.merge_voxels(voxel)
    radius, distance = float(np.float32(5.0 * voxel)), float(np.float32(1.5 * voxel))
    a = arrays_of(thin)
    moved = {False: far_away(gpu_pkg, thin)[0]}
    R, t = far_away(gpu_pkg, thin)[1:]
    b = arrays_of(moved[False])
    moved[True] = from_cloud(gpu_pkg, cloud(b.xyz, normal=b.normal), [4], [5], [[]], on_device=True)
    here = {dev: from_cloud(gpu_pkg, cloud(a.xyz, normal=a.normal), [4], [5], [[]], on_device=dev) for dev in (False, True)}
    want = RC.register(checker, b.xyz, b.normal, a.xyz, a.normal, radius, inlier_distance=distance, trials=1024)
    print("real cloud", name, thin.count, "points, radius", radius, want)
    assert moved[False].align(here[False], radius).matched_before == 0
    for p_dev, q_dev in RESIDENCIES:
        assert_registration(moved[p_dev].register(here[q_dev], radius, distance, trials=1024), want, (name, p_dev, q_dev))
    # brought back: an inlier distance of 1.5 cells over a cloud of many cells bounds the angle far below 0.1
    back = np.asarray(want.rotation).reshape(3, 3)
    assert want.stopped == RC.OK and np.abs(back @ R - np.eye(3)).max() < 0.1 and want.rms_after < distance


# --------------------------------------------------------------------------------------------------------------------
# the binary
# --------------------------------------------------------------------------------------------------------------------

FLAGS_BEFORE = {"register": ["--ply-normals"], "register_all": ["--ply-mean", "--ply-voxel", "0.25", "--ply-vis", "--ply-normals", "--ply-radius-filter", "2,1"]}
REGISTRATION_NAMES = (["scale"] + ["rotation%d" % e for e in range(9)] + ["translation%d" % e for e in range(3)] + list(RC.FIELDS[3:]))
BINARY_TRIALS, BINARY_SEED = 512, 3


@pytest.fixture(scope="module")
def folders(gpu_pkg, synth, tmp_path_factory):
    """One small synthetic dense folder (the size of the drop-in tests): per set of flags a run without --ply-register, a ground
    truth made from that run's APD.ply turned far away, and a run with --ply-register, --ply-align and --ply-score after the others.
    name -> (plain folder, registered folder, the truth file, radius, inlier distance, the registered run's output)."""
    root = tmp_path_factory.mktemp("dense")
    radius_checker = PR.build(tmp_path_factory.mktemp("points_radius_checker"))
    a = root / "a"
    a.mkdir()
    _write_dense_folder(a, synth, 96, 72, 4)
    out = {}
    for name, flags in FLAGS_BEFORE.items():
        plain, registered = root / (name + "_plain"), root / name
        shutil.copytree(a, plain)
        _run(plain, *flags)
        made = gpu_pkg.Points.read_ply(plain / "APD" / "APD.ply")
        radius = float(np.float32(4.0 * real_cloud_radius(radius_checker, arrays_of(made))))
        distance = float(np.float32(radius / 2.0))
        truth = root / (name + ",truth,1.ply")       # commas in the path: the value is read from its end
        far_away(gpu_pkg, made, truth)
        shutil.copytree(a, registered)
        value = "%s,%.9g,%.9g,%d,%d" % (truth, radius, distance, BINARY_TRIALS, BINARY_SEED)
        out[name] = (plain, registered, truth, radius, distance,
                     run_binary(registered, *flags, "--ply-register", value, "--ply-align", "%s,%.9g,4" % (truth, radius), "--ply-score",
                                "%s,%.9g" % (truth, distance)))
    return out


def test_binary_prints_and_writes_the_registration(gpu_pkg, checker, align_checker, folders):
    """The printed line, APD.ply.register and the checker agree in every bit; --ply-align and --ply-score after it work on the moved
    points, and APD.ply holds them; APD.ply.vis is byte-identical to the run without the flag, which writes no APD.ply.register."""
    for name, (plain, registered, truth, radius, distance, output) in folders.items():
        with_vis = "--ply-vis" in FLAGS_BEFORE[name]
        assert (plain / "APD" / "APD.ply.vis").exists() == (registered / "APD" / "APD.ply.vis").exists() == with_vis, name
        if with_vis:
            assert (plain / "APD" / "APD.ply.vis").read_bytes() == (registered / "APD" / "APD.ply.vis").read_bytes(), name
        assert not (plain / "APD" / "APD.ply.register").exists() and not (plain / "APD" / "APD.ply.align").exists()
        before, truth_points = gpu_pkg.Points.read_ply(plain / "APD" / "APD.ply"), gpu_pkg.Points.read_ply(truth)
        after = gpu_pkg.Points.read_ply(registered / "APD" / "APD.ply")
        b_xyz, b_normal, t_xyz, t_normal = (np.asarray(v) for v in (before.xyz, before.normal, truth_points.xyz, truth_points.normal))
        assert np.abs(b_normal).max() > 0 and np.abs(t_normal).max() > 0
        want = RC.register(checker, b_xyz, b_normal, t_xyz, t_normal, radius, inlier_distance=distance, trials=BINARY_TRIALS, seed=BINARY_SEED)
        print(name, before.count, "points", want)
        lines = [ln for ln in output.splitlines() if ln.startswith("Registered to ")]
        assert len(lines) == 1 and lines[0].startswith("Registered to %s at " % truth), (name, lines)
        words = lines[0].split(":")[-1].split()
        printed = dict(zip(words[0::2], words[1::2]))
        written = dict(ln.split(" ") for ln in (registered / "APD" / "APD.ply.register").read_text().splitlines())
        assert list(written) == REGISTRATION_NAMES and printed == written, (name, printed, written)
        got = RC.Registration(float(written["scale"]), tuple(float(written["rotation%d" % e]) for e in range(9)),
                              tuple(float(written["translation%d" % e]) for e in range(3)), *[int(written[f]) for f in RC.FIELDS[3:10]],
                              float(written["rms_after"]), int(written["stopped"]))
        assert RC.bits(got) == RC.bits(want), (name, got, want)
        assert output.index("Registered to ") < output.index("Aligned to ") < output.index("Score against ")
        moved_xyz, moved_normal = PA.transformed(align_checker, b_xyz, b_normal, want.scale, want.rotation, want.translation)
        refined = PA.align(align_checker, moved_xyz, t_xyz, radius, iterations=4)
        want_xyz, want_normal = PA.transformed(align_checker, moved_xyz, moved_normal, refined.scale, refined.rotation, refined.translation)
        assert np.array_equal(bits32(np.asarray(after.xyz)), bits32(want_xyz)) and np.array_equal(bits32(np.asarray(after.normal)), bits32(want_normal)), name
        assert np.array_equal(np.asarray(after.bgr), np.asarray(before.bgr)), name
        aligned = dict(ln.split(" ") for ln in (registered / "APD" / "APD.ply.align").read_text().splitlines())
        assert int(aligned["matched_before"]) == refined.matched_before and float(aligned["rms_after"]) == refined.rms_after, name
        assert (registered / "APD" / "APD.ply.score").exists()


def test_binary_refuses_a_bad_value_before_anything_is_read(tmp_path):
    for bad in ("", "truth.ply", "truth.ply,", "truth.ply,1", ",1,1", "truth.ply,0,1", "truth.ply,1,0", "truth.ply,-1,1", "truth.ply,nan,1", "truth.ply,1,inf",
                "truth.ply,1e30,1", "truth.ply,1,1e-30", "truth.ply,1x,1", "truth.ply,1,1,0", "truth.ply,1,1,", "truth.ply,1,0,7", "truth.ply,1,1,scale",
                "truth.ply,1,1,8,", "truth.ply,1,1,8,-1", "truth.ply,1,1,8,99999999999999999999"):
        r = subprocess.run([APD_BIN, str(tmp_path / "no_such_folder"), "0", "--ply-register", bad], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=60)
        assert r.returncode != 0 and "bad value '%s' of --ply-register" % bad in r.stdout and "USAGE" in r.stdout, (bad, r.stdout[-500:])
    for good in ("truth.ply,1,0.5", "a,b.ply,0.5,0.25", "truth.ply,0.5,0.25,8", "truth.ply,0.5,0.25,65536,18446744073709551615", "a,1,0.5,0.3"):
        r = subprocess.run([APD_BIN, str(tmp_path / "no_such_folder"), "0", "--ply-register", good], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=60)
        assert r.returncode != 0 and "bad value" not in r.stdout and "USAGE" not in r.stdout, (good, r.stdout[-500:])
