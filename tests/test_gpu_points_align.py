"""The alignment to another cloud and the move by a transform on the device (apd_points_align, apd_points_transformed;
csrc/apd_points_align.hip), bitwise against the grid mode of the sequential checker (tests/helpers/points_align_ref.cpp): every
field of the Alignment with the doubles as uint64, for host- and device-resident points on either side in all four combinations,
at 1 and 5 iterations, rigid and with scale.  The pairs of clouds are made in test_points_align.py and test_points_nearest.py,
where the checker's brute-force mode and numpy are held against the grid mode on them; here also: the planted transform from
the device itself, the moved object against the checker and its untouched arrays and lists, a real fused cloud brought back onto
itself, two runs, the pipeline and the drop-in binary."""
import shutil
import subprocess

import numpy as np
import pytest

import fusion_cases
import points_align_checker as PA
import points_nearest_checker as PX
import points_radius_checker as PR
from test_gpu_dropin_binary import _write_dense_folder
from test_gpu_fusion_options import APD_BIN, _run, _scene
from test_gpu_points_average import fused
from test_gpu_points_nearest import RESIDENCIES, assert_score, host, points_at, run_binary
from test_points_align import PLANTED_RADIUS, SETTINGS, align_cases, as_matrix, far_start_case, planted_case, rotation
from test_points_nearest import bits32
from test_points_normals import REAL_CLOUD
from test_points_radius import determinism_case, dressed, merged_many_views_case, real_cloud_radius
from test_points_voxel import arrays_of, from_cloud

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return PA.build(tmp_path_factory.mktemp("points_align_checker"))


@pytest.fixture(scope="module")
def score_checker(tmp_path_factory):
    return PX.build(tmp_path_factory.mktemp("points_nearest_checker"))


@pytest.fixture(scope="module")
def radius_checker(tmp_path_factory):
    return PR.build(tmp_path_factory.mktemp("points_radius_checker"))


@pytest.fixture(scope="module")
def made(gpu_pkg):
    """name -> (P, Q, radius, origin, {(side, on_device): Points}), made once for the four settings."""
    out = {}
    for name, (p, q, radius, origin) in align_cases(gpu_pkg).items():
        out[name] = (p, q, radius, origin, {(side, dev): points_at(gpu_pkg, xyz, dev) for side, xyz in (("p", p), ("q", q)) for dev in (False, True)})
    return out


def assert_alignment(got, want, what):
    assert got._fields == PA.FIELDS and got.rotation.shape == (3, 3) and got.rotation.dtype == np.float64 and got.translation.shape == (3,), what
    assert PA.bits(got) == PA.bits(want), (what, got, want)


# --------------------------------------------------------------------------------------------------------------------
# every pair of clouds
# --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("iterations,with_scale", SETTINGS)
def test_every_pair_of_clouds(gpu_pkg, checker, made, iterations, with_scale):
    """Sizes 0, 1, 2, around a wave and a chunk and the sort-tile sizes on either side, n_P != n_Q, points outside the grid and a
    cloud entirely outside, ties, a crowded cell, another origin and radius; the planted pairs, the far start, 0 .. 3 matches, a P
    of 257 points whose only matches stand in the last, one-slot chunk, coincident points."""
    stops = set()
    for name, (p, q, radius, origin, points) in made.items():
        want = PA.align(checker, p, q, radius, origin, iterations, 1e-6, with_scale)
        stops.add(want.stopped)
        for p_dev, q_dev in RESIDENCIES:
            got = points["p", p_dev].align(points["q", q_dev], radius, origin, iterations, 1e-6, with_scale)
            assert_alignment(got, want, (name, p_dev, q_dev))
        assert np.array_equal(bits32(host(points["p", True].xyz)), bits32(p)), (name, "nothing is moved")
    assert {len(p) for p, _, _, _, _ in made.values()} >= {0, 1, 2, 63, 64, 65, 255, 256, 257}
    assert stops >= {PA.ITERATIONS, PA.TOO_FEW} and (iterations == 1 or PA.CONVERGED in stops)


def test_the_planted_transform_comes_back_from_the_device(gpu_pkg):
    for scale in (1.0, 1.03):
        p, q, _, scale, R, t = planted_case(scale)
        for dev in (False, True):
            a = points_at(gpu_pkg, p, dev).align(points_at(gpu_pkg, q, dev), PLANTED_RADIUS, iterations=1, with_scale=scale != 1.0)
            assert (a.steps, a.stopped, a.matched_before, a.matched_after) == (1, gpu_pkg.ALIGN_ITERATIONS, len(p), len(p))
            assert abs(a.scale - scale) < 1e-8 and np.abs(a.rotation - R).max() < 1e-8 and np.abs(a.translation - t).max() < 1e-7
            assert a.rms_after < 1e-6 < 0.3 < a.rms_before
    p, q, radius, R, t = far_start_case()
    a = points_at(gpu_pkg, p, True).align(points_at(gpu_pkg, q, False), radius, iterations=64)
    assert a.stopped == gpu_pkg.ALIGN_CONVERGED and 5 < a.steps < 20 and np.abs(a.rotation - R).max() < 1e-3 and np.abs(a.translation - t).max() < 1e-2


def test_the_same_object_on_both_sides(gpu_pkg, checker):
    q = planted_case()[1]
    for dev in (False, True):
        pts = points_at(gpu_pkg, q, dev)
        a = pts.align(pts, PLANTED_RADIUS)
        assert_alignment(a, PA.align(checker, q, q, PLANTED_RADIUS), dev)
        assert a.scale == 1.0 and np.array_equal(a.rotation, np.eye(3)) and not a.translation.any() and a.rms_after == 0.0
        assert (a.matched_after, a.steps, a.stopped) == (len(q), 1, gpu_pkg.ALIGN_CONVERGED)


def test_two_calls_give_identical_bits(gpu_pkg, checker):
    c, _ = determinism_case()
    q = c.xyz
    R, t = rotation(3.0), np.float64([0.2, -0.1, 0.15])
    p = ((q[::2].astype(np.float64) - t) @ R).astype(np.float32)
    origin = [0.25, -0.5, 0.125]
    P, Q = points_at(gpu_pkg, p, True), points_at(gpu_pkg, q, True)
    runs = [PA.bits(P.align(Q, 1.0, origin, iterations=4, with_scale=True)) for _ in range(2)]
    assert runs[0] == runs[1]
    want = PA.align(checker, p, q, 1.0, origin, iterations=4, with_scale=True)
    assert runs[0] == PA.bits(want) and 3 < want.matched_before < want.matched_after <= len(p) and want.steps > 1


# --------------------------------------------------------------------------------------------------------------------
# the moved object
# --------------------------------------------------------------------------------------------------------------------

def assert_moved(moved, before, want_xyz, want_normal, what):
    after = arrays_of(moved)
    assert np.array_equal(bits32(after.xyz), bits32(want_xyz)) and np.array_equal(bits32(after.normal), bits32(want_normal)), what
    for field in ("bgr", "support", "view", "pixel", "sources", "offsets", "views"):
        a, b = np.asarray(getattr(after, field)), np.asarray(getattr(before, field))
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (what, field)


def test_transformed_points_keep_everything_but_positions_and_normals(gpu_pkg, checker, score_checker):
    """xyz and normal bitwise as the checker moves them; colours, support, view, pixel, sources and the lists byte for byte; the
    input untouched; the object lives where its input lives; the score of the moved object is the checker's score of the moved
    positions.  Sizes around a block, and a merged object, which stays merged with its lists."""
    rng = np.random.default_rng(21)
    p, q, _, scale, R, t = planted_case(1.03)
    for n in (1, 255, 256, 257, len(p)):
        c, (rows, cols, pairs) = dressed(rng, p[:n])
        want_xyz, want_normal = PA.transformed(checker, c.xyz, c.normal, scale, R, t)
        assert not np.array_equal(want_xyz, c.xyz) and not np.array_equal(want_normal, c.normal)
        for dev in (False, True):
            pts = from_cloud(gpu_pkg, c, rows, cols, pairs, on_device=dev)
            before = arrays_of(pts)
            moved = pts.transformed(scale, R, t)
            assert moved.on_device == dev and moved.count == n
            assert_moved(moved, before, want_xyz, want_normal, (n, dev))
            assert_moved(pts, before, c.xyz, c.normal, (n, dev, "the input"))
            if n == len(p):
                a = pts.align(points_at(gpu_pkg, q, dev), PLANTED_RADIUS, with_scale=True)
                by_alignment = pts.transformed(a)
                ax, an = PA.transformed(checker, c.xyz, c.normal, a.scale, a.rotation, a.translation)
                assert_moved(by_alignment, before, ax, an, (n, dev, "by an Alignment"))
                tau = 0.01
                truth = points_at(gpu_pkg, q, not dev)
                assert_score(by_alignment.score(truth, tau), PX.score(score_checker, ax, q, tau), (n, dev))
                assert by_alignment.score(truth, tau).p_within == n and pts.score(truth, tau).p_within == 0


def test_a_merged_object_stays_merged_with_its_lists(gpu_pkg, checker, tmp_path_factory):
    import points_voxel_checker as PV
    voxel_checker = PV.build(tmp_path_factory.mktemp("points_voxel_checker"))
    c, (rows, cols, pairs), _ = merged_many_views_case(voxel_checker)
    R, t = rotation(25.0, (0, 1, 1)), np.float64([1, -2, 3])
    for dev in (False, True):
        merged, _ = from_cloud(gpu_pkg, c, rows, cols, pairs, on_device=dev).merge_voxels(1.0)
        before = arrays_of(merged)
        assert len(before.views) > 0
        want_xyz, want_normal = PA.transformed(checker, before.xyz, before.normal, 0.5, R, t)
        assert_moved(merged.transformed(0.5, R, t), before, want_xyz, want_normal, dev)


def test_a_moved_real_cloud_aligns_back_to_itself(gpu_pkg, ob, radius_checker, checker):
    """A fused cloud rotated by 3 degrees and shifted by half the radius, aligned to the cloud it came from: more matches, a
    smaller rms distance, and every bit the checker's, in all four residencies."""
    name, variant, _ = REAL_CLOUD
    case = fusion_cases.case(name)
    pts = {dev: fused(gpu_pkg, ob, case, variant, dev) for dev in (False, True)}
    before = arrays_of(pts[False])
    radius = real_cloud_radius(radius_checker, before)
    R = rotation(3.0)
    centre = before.xyz[np.isfinite(before.xyz).all(axis=1)].astype(np.float64).mean(axis=0)
    t = centre - R @ centre + 0.5 * radius / np.sqrt(3.0)            # about the cloud's centre, then half a radius away
    moved = {dev: pts[dev].transformed(1.0, R, t) for dev in (False, True)}
    moved_xyz = host(moved[False].xyz)
    assert np.array_equal(bits32(moved_xyz), bits32(host(moved[True].xyz)))
    want = PA.align(checker, moved_xyz, before.xyz, radius, iterations=8)
    print("real cloud", name, len(moved_xyz), "points, radius", radius, want)
    assert want.rms_after < want.rms_before and want.matched_after >= want.matched_before > 3 and want.steps > 1
    for p_dev, q_dev in RESIDENCIES:
        assert_alignment(moved[p_dev].align(pts[q_dev], radius, iterations=8), want, (name, p_dev, q_dev))


# --------------------------------------------------------------------------------------------------------------------
# the pipeline and the binary
# --------------------------------------------------------------------------------------------------------------------

def moved_truth(pkg, xyz, radius, path):
    """A ground truth for the cloud at xyz, written to `path`: two of every three of its points under 2 degrees about the cloud's
    centre and a shift of a quarter of the radius.  Returns its positions."""
    keep = np.arange(len(xyz)) % 3 != 0
    R = rotation(2.0)
    centre = xyz.astype(np.float64).mean(axis=0)
    truth = ((xyz[keep].astype(np.float64) - centre) @ R.T + centre + 0.25 * radius / np.sqrt(3.0)).astype(np.float32)
    points_at(pkg, truth, False).write_ply(path)
    return truth


def test_through_the_pipeline(gpu_pkg, ob, radius_checker, checker, score_checker, tmp_path):
    """fuse(align=...) moves the points every other option has produced: the returned points, the file and the alignment are those
    of Points.align and Points.transformed on the result without the option, which the checker confirms; the score that follows is
    that of the moved points; without the option every file keeps its bytes."""
    from apd_mvs_amd import pipeline
    case = fusion_cases.case("mixed_sizes")
    scene, results = _scene(gpu_pkg, pipeline, case)
    for kw in (dict(), dict(average=True, voxel=0.05, component_filter=(0.2, 2))):
        n, whole = pipeline.fuse(scene, results, tmp_path / "plain.ply", return_points=True, vis_path=tmp_path / "plain.vis", **kw)
        w = arrays_of(whole)
        radius = real_cloud_radius(radius_checker, w)
        truth_xyz = moved_truth(gpu_pkg, w.xyz, radius, tmp_path / "truth.ply")
        want = PA.align(checker, w.xyz, truth_xyz, radius, iterations=6)
        assert want.steps > 1 and want.rms_after < want.rms_before and want.matched_after > 3
        want_xyz, want_normal = PA.transformed(checker, w.xyz, w.normal, want.scale, want.rotation, want.translation)
        for on_device in (False, True):
            truth = gpu_pkg.Points.read_ply(tmp_path / "truth.ply", on_device=on_device)
            a = whole.align(truth, radius, iterations=6)
            assert_alignment(a, want, kw)
            by_hand = whole.transformed(a)
            by_hand.write_ply(tmp_path / "by_hand.ply")
            m, pts, got = pipeline.fuse(scene, results, tmp_path / "m.ply", return_points=True, vis_path=tmp_path / "m.vis", align=(truth, radius, 6), **kw)
            assert m == n == pts.count
            assert_alignment(got, want, kw)
            assert_moved(pts, w, want_xyz, want_normal, kw)
            assert (tmp_path / "m.ply").read_bytes() == (tmp_path / "by_hand.ply").read_bytes() != (tmp_path / "plain.ply").read_bytes()
            assert (tmp_path / "m.vis").read_bytes() == (tmp_path / "plain.vis").read_bytes()
            m, got = pipeline.fuse(scene, results, tmp_path / "file_only.ply", align=(truth, radius, 6, False), **kw)
            assert m == n and (tmp_path / "file_only.ply").read_bytes() == (tmp_path / "by_hand.ply").read_bytes()
            assert_alignment(got, want, kw)
            tau = float(np.float32(radius / 4.0))
            m, pts, got, s = pipeline.fuse(scene, results, None, return_points=True, align=(truth, radius, 6), score=(truth, tau), **kw)
            assert_alignment(got, want, kw)
            assert_score(s, PX.score(score_checker, want_xyz, truth_xyz, tau), kw)
            assert s.p_within > whole.score(truth, tau).p_within
            m, got, s2 = pipeline.fuse(scene, results, tmp_path / "both.ply", align=(truth, radius, 6), score=(truth, tau), **kw)
            assert PA.bits(got) == PA.bits(want) and s2 == s
            # without the option nothing changes
            m = pipeline.fuse(scene, results, tmp_path / "again.ply", vis_path=tmp_path / "again.vis", **kw)
            assert (tmp_path / "again.ply").read_bytes() == (tmp_path / "plain.ply").read_bytes()
            assert (tmp_path / "again.vis").read_bytes() == (tmp_path / "plain.vis").read_bytes()


FLAGS_BEFORE = {"align": [], "align_all": ["--ply-mean", "--ply-voxel", "0.25", "--ply-vis", "--ply-normals", "--ply-radius-filter", "2,1"]}
ALIGNMENT_NAMES = (["scale"] + ["rotation%d" % e for e in range(9)] + ["translation%d" % e for e in range(3)] +
                   ["matched_before", "matched_after", "rms_before", "rms_after", "steps", "stopped"])


@pytest.fixture(scope="module")
def folders(gpu_pkg, synth, radius_checker, tmp_path_factory):
    """One small synthetic dense folder (the size of the drop-in tests): per set of flags a run without --ply-align, a ground truth
    made from that run's APD.ply, and a run with --ply-align and --ply-score after the others.  name -> (plain folder, aligned
    folder, the truth file, radius, tau, the aligned run's output)."""
    root = tmp_path_factory.mktemp("dense")
    a = root / "a"
    a.mkdir()
    _write_dense_folder(a, synth, 96, 72, 4)
    out = {}
    for name, flags in FLAGS_BEFORE.items():
        plain, aligned = root / (name + "_plain"), root / name
        shutil.copytree(a, plain)
        _run(plain, *flags)
        made = gpu_pkg.Points.read_ply(plain / "APD" / "APD.ply")
        radius = real_cloud_radius(radius_checker, arrays_of(made))
        tau = float(np.float32(radius / 4.0))
        truth = root / (name + ",truth.ply")       # a comma in the path: the value is read from its end
        moved_truth(gpu_pkg, np.asarray(made.xyz), radius, truth)
        shutil.copytree(a, aligned)
        value = "%s,%.9g,6" % (truth, radius) + (",scale" if flags else "")
        out[name] = (plain, aligned, truth, radius, tau, run_binary(aligned, *flags, "--ply-align", value, "--ply-score", "%s,%.9g" % (truth, tau)))
    return out


def test_binary_prints_and_writes_the_alignment(gpu_pkg, checker, score_checker, folders):
    """The printed line, APD.ply.align and the checker agree in every bit; APD.ply holds the moved points; --ply-score after it
    scores them; APD.ply.vis is byte-identical to the run without the flag."""
    for name, (plain, aligned, truth, radius, tau, output) in folders.items():
        with_scale = bool(FLAGS_BEFORE[name])
        assert (plain / "APD" / "APD.ply.vis").exists() == (aligned / "APD" / "APD.ply.vis").exists() == with_scale, name
        if with_scale:
            assert (plain / "APD" / "APD.ply.vis").read_bytes() == (aligned / "APD" / "APD.ply.vis").read_bytes(), name
        assert not (plain / "APD" / "APD.ply.align").exists()
        before, truth_points = gpu_pkg.Points.read_ply(plain / "APD" / "APD.ply"), gpu_pkg.Points.read_ply(truth)
        after = gpu_pkg.Points.read_ply(aligned / "APD" / "APD.ply")
        want = PA.align(checker, np.asarray(before.xyz), np.asarray(truth_points.xyz), radius, iterations=6, with_scale=with_scale)
        assert want.steps > 1 and want.rms_after < want.rms_before, (name, want)
        lines = [ln for ln in output.splitlines() if ln.startswith("Aligned to ")]
        assert len(lines) == 1 and lines[0].startswith("Aligned to %s within " % truth), (name, lines)
        words = lines[0].split(":")[-1].split()
        printed = dict(zip(words[0::2], words[1::2]))
        written = dict(ln.split(" ") for ln in (aligned / "APD" / "APD.ply.align").read_text().splitlines())
        assert list(written) == ALIGNMENT_NAMES and printed == written, (name, printed, written)
        got = PA.Alignment(float(written["scale"]), tuple(float(written["rotation%d" % e]) for e in range(9)),
                           tuple(float(written["translation%d" % e]) for e in range(3)), int(written["matched_before"]), int(written["matched_after"]),
                           float(written["rms_before"]), float(written["rms_after"]), int(written["steps"]), int(written["stopped"]))
        assert PA.bits(got) == PA.bits(want), (name, got, want)
        want_xyz, want_normal = PA.transformed(checker, np.asarray(before.xyz), np.asarray(before.normal), want.scale, want.rotation, want.translation)
        assert np.array_equal(bits32(np.asarray(after.xyz)), bits32(want_xyz)) and np.array_equal(np.asarray(after.bgr), np.asarray(before.bgr)), name
        if with_scale:      # --ply-normals: the file holds them
            assert np.array_equal(bits32(np.asarray(after.normal)), bits32(want_normal)), name
        score = dict(ln.split(" ") for ln in (aligned / "APD" / "APD.ply.score").read_text().splitlines())
        want_score = PX.score(score_checker, want_xyz, np.asarray(truth_points.xyz), tau)
        got_score = PX.Score(*[int(score[f]) for f in PX.FIELDS[:4]], *[float(score[f]) for f in PX.FIELDS[4:]])
        assert PX.score_bits(got_score) == PX.score_bits(want_score) and want_score.p_within > 0, (name, got_score, want_score)


def test_binary_refuses_a_bad_value_before_anything_is_read(tmp_path):
    for bad in ("", "truth.ply", "truth.ply,", ",1", "truth.ply,0", "truth.ply,-1", "truth.ply,nan", "truth.ply,inf", "truth.ply,1e30", "truth.ply,1e-30",
                "truth.ply,1x", "truth.ply,1,0", "truth.ply,1,2,scal", "truth.ply,1,2,", "scale", ",scale", "truth.ply,scale"):
        r = subprocess.run([APD_BIN, str(tmp_path / "no_such_folder"), "0", "--ply-align", bad], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=60)
        assert r.returncode != 0 and "bad value '%s' of --ply-align" % bad in r.stdout and "USAGE" in r.stdout, (bad, r.stdout[-500:])
    for good in ("truth.ply,1", "a,b.ply,0.5", "truth.ply,0.5,8", "truth.ply,0.5,64,scale", "truth.ply,0.5,scale"):
        r = subprocess.run([APD_BIN, str(tmp_path / "no_such_folder"), "0", "--ply-align", good], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=60)
        assert r.returncode != 0 and "bad value" not in r.stdout and "USAGE" not in r.stdout, (good, r.stdout[-500:])
