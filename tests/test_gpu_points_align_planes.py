"""The alignment to another cloud's tangent planes on the device (apd_points_align_planes; csrc/apd_points_align_planes.hip),
bitwise against the grid mode of the sequential checker (tests/helpers/points_align_planes_ref.cpp): every field of the
PlaneAlignment with the doubles as uint64, for host- and device-resident points on either side in all four combinations, at 1 and
5 iterations.  The pairs of clouds are made in points_align_planes_cases.py; test_points_align_planes.py holds the checker's
brute-force mode and numpy against its grid mode on them.  Here also: the planted transform from the device itself, untouched
inputs, two runs, a real fused cloud brought back onto itself, the pipeline and the drop-in binary."""
import shutil
import subprocess

import numpy as np
import pytest

import fusion_cases
import points_align_checker as PA
import points_align_planes_cases as K
import points_align_planes_checker as PP
import points_nearest_checker as PX
import points_radius_checker as PR
from test_gpu_dropin_binary import _write_dense_folder
from test_gpu_fusion_options import APD_BIN, _run, _scene
from test_gpu_points_average import fused
from test_gpu_points_nearest import RESIDENCIES, assert_score, host, run_binary
from test_points_align import rotation
from test_points_align_planes import SETTINGS, errors
from test_points_nearest import bits32
from test_points_normals import REAL_CLOUD, REAL_MIN
from test_points_radius import real_cloud_radius
from test_points_voxel import arrays_of, cloud, from_cloud

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return PP.build(tmp_path_factory.mktemp("points_align_planes_checker"))


@pytest.fixture(scope="module")
def point_checker(tmp_path_factory):
    return PA.build(tmp_path_factory.mktemp("points_align_checker"))


@pytest.fixture(scope="module")
def score_checker(tmp_path_factory):
    return PX.build(tmp_path_factory.mktemp("points_nearest_checker"))


@pytest.fixture(scope="module")
def radius_checker(tmp_path_factory):
    return PR.build(tmp_path_factory.mktemp("points_radius_checker"))


def points_at(pkg, xyz, normal, on_device):
    return from_cloud(pkg, cloud(xyz, normal=None if normal is None else np.ascontiguousarray(normal, np.float32)), [4], [5], [[]], on_device=on_device)


@pytest.fixture(scope="module")
def made(gpu_pkg):
    """name -> (P, Q, Q's normals, radius, origin, {(side, on_device): Points}), made once for both settings."""
    out = {}
    for name, (p, q, normal, radius, origin) in K.plane_cases(gpu_pkg).items():
        sides = (("p", p, None), ("q", q, normal))
        out[name] = (p, q, normal, radius, origin, {(side, dev): points_at(gpu_pkg, xyz, n, dev) for side, xyz, n in sides for dev in (False, True)})
    return out


def assert_alignment(got, want, what):
    assert got._fields == PP.FIELDS and got.rotation.shape == (3, 3) and got.rotation.dtype == np.float64 and got.translation.shape == (3,), what
    assert PP.bits(got) == PP.bits(want), (what, got, want)


# --------------------------------------------------------------------------------------------------------------------
# every pair of clouds
# --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("iterations", SETTINGS)
def test_every_pair_of_clouds(gpu_pkg, checker, made, iterations):
    """The pairs of the point-to-point tests dressed with normals of which some are zero or NaN -- sizes 0, 1, 2, around a wave
    and a chunk on either side, points outside the grid, ties, another origin and radius --, the ellipsoid, onto itself and on
    another grid, the plane, the sphere and the cylinder, the bad normals, 5 and 6 usable matches, and a P of 257 and one of 264
    points whose only usable matches stand in the last, short chunk."""
    stops = set()
    for name, (p, q, normal, radius, origin, points) in made.items():
        want = PP.align_planes(checker, p, q, normal, radius, origin, iterations)
        stops.add(want.stopped)
        for p_dev, q_dev in RESIDENCIES:
            got = points["p", p_dev].align_planes(points["q", q_dev], radius, origin, iterations)
            assert_alignment(got, want, (name, p_dev, q_dev))
        assert np.array_equal(bits32(host(points["p", True].xyz)), bits32(p)), (name, "nothing is moved")
        for dev in (False, True):
            assert np.array_equal(bits32(host(points["q", dev].xyz)), bits32(q)) and np.array_equal(bits32(host(points["q", dev].normal)), bits32(normal)), name
    assert {len(p) for p, _, _, _, _, _ in made.values()} >= {0, 1, 2, 63, 64, 65, 255, 256, 257}
    assert stops == {PP.ITERATIONS, PP.TOO_FEW, PP.DEGENERATE} | ({PP.CONVERGED} if iterations > 1 else set())      # all four codes at 5 iterations


def test_the_same_object_on_both_sides(gpu_pkg, checker):
    q, normal = K.surface_sample(800, 11)
    for dev in (False, True):
        pts = points_at(gpu_pkg, q, normal, dev)
        a = pts.align_planes(pts, K.SURFACE_RADIUS)
        assert_alignment(a, PP.align_planes(checker, q, q, normal, K.SURFACE_RADIUS), dev)
        assert a.scale == 1.0 and np.array_equal(a.rotation, np.eye(3)) and not a.translation.any() and a.rms_after == 0.0 and a.plane_rms_after == 0.0
        assert (a.matched_after, a.planes_after, a.steps, a.stopped) == (len(q), len(q), 1, gpu_pkg.ALIGN_CONVERGED)


def test_the_planted_transform_comes_back_from_the_device(gpu_pkg):
    """What test_points_align_planes.py established on the checker: nearer to the planted transform than the point-to-point call
    from the same start and with the same cap, in rotation and translation, and a smaller plane rms."""
    p, q, normal, radius, R, t = K.ellipsoid_case()
    for dev in (False, True):
        P, Q = points_at(gpu_pkg, p, None, dev), points_at(gpu_pkg, q, normal, not dev)
        for cap in (1, 16):
            planes, points = P.align_planes(Q, radius, iterations=cap), P.align(Q, radius, iterations=cap)
            e_planes, e_points = errors(planes, R, t), errors(points, R, t)
            assert e_planes[0] < e_points[0] and e_planes[1] < e_points[1], (cap, e_planes, e_points)
            assert planes.plane_rms_after < planes.plane_rms_before and planes.planes_before == len(p)
        assert planes.stopped == gpu_pkg.ALIGN_CONVERGED and planes.steps == 5 and e_planes[0] < 0.2 and e_planes[1] < 0.002
        moved = P.transformed(planes)
        assert np.abs(host(moved.xyz).astype(np.float64) - (p.astype(np.float64) @ planes.rotation.T + planes.translation)).max() < 1e-6


def test_two_calls_give_identical_bits(gpu_pkg, checker):
    p, q, normal, radius = K.bad_normals_case()
    origin = [0.25, -0.5, 0.125]
    P, Q = points_at(gpu_pkg, p, None, True), points_at(gpu_pkg, q, normal, True)
    runs = [PP.bits(P.align_planes(Q, radius, origin, iterations=4)) for _ in range(2)]
    assert runs[0] == runs[1]
    want = PP.align_planes(checker, p, q, normal, radius, origin, iterations=4)
    assert runs[0] == PP.bits(want) and want.steps == 4 and 6 < want.planes_before < want.matched_before


def test_a_moved_real_cloud_aligns_back_to_itself(gpu_pkg, ob, radius_checker, checker):
    """A fused cloud with its normals re-estimated, rotated by 3 degrees and shifted by half the radius, aligned to the planes of
    the cloud it came from: a smaller plane rms, no degenerate geometry, and every bit the checker's, in all four residencies."""
    name, variant, _ = REAL_CLOUD
    case = fusion_cases.case(name)
    raw = {dev: fused(gpu_pkg, ob, case, variant, dev) for dev in (False, True)}
    radius = real_cloud_radius(radius_checker, arrays_of(raw[False]))
    pts = {dev: raw[dev].with_estimated_normals(radius, REAL_MIN)[0] for dev in (False, True)}
    before = arrays_of(pts[False])
    assert np.array_equal(bits32(before.normal), bits32(host(pts[True].normal))) and not np.array_equal(before.normal, arrays_of(raw[False]).normal)
    R = rotation(3.0)
    centre = before.xyz[np.isfinite(before.xyz).all(axis=1)].astype(np.float64).mean(axis=0)
    t = centre - R @ centre + 0.5 * radius / np.sqrt(3.0)            # about the cloud's centre, then half a radius away
    moved = {dev: pts[dev].transformed(1.0, R, t) for dev in (False, True)}
    moved_xyz = host(moved[False].xyz)
    assert np.array_equal(bits32(moved_xyz), bits32(host(moved[True].xyz)))
    want = PP.align_planes(checker, moved_xyz, before.xyz, before.normal, radius, iterations=8)
    print("real cloud", name, len(moved_xyz), "points, radius", radius, want)
    assert want.plane_rms_after < want.plane_rms_before and want.planes_before > 6 and want.steps > 1 and want.stopped != PP.DEGENERATE
    for p_dev, q_dev in RESIDENCIES:
        assert_alignment(moved[p_dev].align_planes(pts[q_dev], radius, iterations=8), want, (name, p_dev, q_dev))


# --------------------------------------------------------------------------------------------------------------------
# the pipeline and the binary
# --------------------------------------------------------------------------------------------------------------------

def moved_truth(pkg, c, radius, path):
    """A ground truth with normals for the cloud c, written to `path`: two of every three of its points under 2 degrees about the
    cloud's centre and a shift of a quarter of the radius, normals turned with them.  Returns its positions and normals."""
    keep = np.arange(c.count) % 3 != 0
    R = rotation(2.0)
    centre = c.xyz.astype(np.float64).mean(axis=0)
    xyz = ((c.xyz[keep].astype(np.float64) - centre) @ R.T + centre + 0.25 * radius / np.sqrt(3.0)).astype(np.float32)
    normal = (c.normal[keep].astype(np.float64) @ R.T).astype(np.float32)
    points_at(pkg, xyz, normal, False).write_ply(path, normals=True)
    return xyz, normal


def test_through_the_pipeline(gpu_pkg, ob, radius_checker, checker, point_checker, score_checker, tmp_path):
    """fuse(align_planes=...) moves the points every other option has produced: the returned points, the file and the
    PlaneAlignment are those of Points.align_planes and Points.transformed on the result without the option, which the checker
    confirms; the score that follows is that of the moved points; the .vis file and, without the option, every file keep their
    bytes."""
    from apd_mvs_amd import pipeline
    case = fusion_cases.case("mixed_sizes")
    scene, results = _scene(gpu_pkg, pipeline, case)
    kw = dict(average=True, voxel=0.05, component_filter=(0.2, 2))
    n, whole = pipeline.fuse(scene, results, tmp_path / "plain.ply", return_points=True, vis_path=tmp_path / "plain.vis", **kw)
    w = arrays_of(whole)
    radius = real_cloud_radius(radius_checker, w)
    truth_xyz, truth_normal = moved_truth(gpu_pkg, w, radius, tmp_path / "truth.ply")
    want = PP.align_planes(checker, w.xyz, truth_xyz, truth_normal, radius, iterations=6)
    assert want.steps > 1 and want.plane_rms_after < want.plane_rms_before and want.planes_after > 6
    want_xyz, want_normal = PA.transformed(point_checker, w.xyz, w.normal, want.scale, want.rotation, want.translation)
    for on_device in (False, True):
        truth = gpu_pkg.Points.read_ply(tmp_path / "truth.ply", on_device=on_device)
        assert np.array_equal(bits32(host(truth.normal)), bits32(truth_normal))
        a = whole.align_planes(truth, radius, iterations=6)
        assert_alignment(a, want, on_device)
        by_hand = whole.transformed(a)
        by_hand.write_ply(tmp_path / "by_hand.ply")
        m, pts, got = pipeline.fuse(scene, results, tmp_path / "m.ply", return_points=True, vis_path=tmp_path / "m.vis", align_planes=(truth, radius, 6), **kw)
        assert m == n == pts.count
        assert_alignment(got, want, on_device)
        after = arrays_of(pts)
        assert np.array_equal(bits32(after.xyz), bits32(want_xyz)) and np.array_equal(bits32(after.normal), bits32(want_normal))
        assert (tmp_path / "m.ply").read_bytes() == (tmp_path / "by_hand.ply").read_bytes() != (tmp_path / "plain.ply").read_bytes()
        assert (tmp_path / "m.vis").read_bytes() == (tmp_path / "plain.vis").read_bytes()
        tau = float(np.float32(radius / 4.0))
        m, got, s = pipeline.fuse(scene, results, tmp_path / "both.ply", align_planes=(truth, radius, 6), score=(truth, tau), **kw)
        assert PP.bits(got) == PP.bits(want) and (tmp_path / "both.ply").read_bytes() == (tmp_path / "by_hand.ply").read_bytes()
        assert_score(s, PX.score(score_checker, want_xyz, truth_xyz, tau), on_device)
        assert s.p_within > whole.score(truth, tau).p_within
        # after align, the Alignment comes first
        m, first, second = pipeline.fuse(scene, results, tmp_path / "two.ply", align=(truth, radius, 2), align_planes=(truth, radius, 6), **kw)
        assert first._fields == PA.FIELDS and second._fields == PP.FIELDS and first.steps == 2
        # without the option nothing changes
        pipeline.fuse(scene, results, tmp_path / "again.ply", vis_path=tmp_path / "again.vis", **kw)
        assert (tmp_path / "again.ply").read_bytes() == (tmp_path / "plain.ply").read_bytes()
        assert (tmp_path / "again.vis").read_bytes() == (tmp_path / "plain.vis").read_bytes()


FLAGS_BEFORE = ["--ply-mean", "--ply-voxel", "0.25", "--ply-vis", "--ply-normals", "--ply-radius-filter", "2,1"]
NAMES = (["scale"] + ["rotation%d" % e for e in range(9)] + ["translation%d" % e for e in range(3)] +
         ["matched_before", "matched_after", "rms_before", "rms_after", "steps", "stopped", "planes_before", "planes_after", "plane_rms_before",
          "plane_rms_after"])


def test_binary_prints_and_writes_the_alignment(gpu_pkg, synth, radius_checker, checker, point_checker, tmp_path):
    """One small synthetic dense folder: a run without the flag, a ground truth with normals made from that run's APD.ply, and a
    run with --ply-align-planes after the others.  The printed line, APD.ply.align_planes and the checker agree in every bit;
    APD.ply holds the moved points and normals; APD.ply.vis is byte-identical to the run without the flag."""
    a = tmp_path / "a"
    a.mkdir()
    _write_dense_folder(a, synth, 96, 72, 4)
    plain, aligned = tmp_path / "plain", tmp_path / "aligned"
    shutil.copytree(a, plain)
    _run(plain, *FLAGS_BEFORE)
    before = gpu_pkg.Points.read_ply(plain / "APD" / "APD.ply")
    c = arrays_of(before)
    radius = real_cloud_radius(radius_checker, c)
    truth = tmp_path / "planes,truth.ply"       # a comma in the path: the value is read from its end
    truth_xyz, truth_normal = moved_truth(gpu_pkg, c, radius, truth)
    shutil.copytree(a, aligned)
    output = run_binary(aligned, *FLAGS_BEFORE, "--ply-align-planes", "%s,%.9g,6" % (truth, radius))
    want = PP.align_planes(checker, c.xyz, truth_xyz, truth_normal, radius, iterations=6)
    assert want.steps > 1 and want.plane_rms_after < want.plane_rms_before, want
    lines = [ln for ln in output.splitlines() if ln.startswith("Aligned to ")]
    assert len(lines) == 1 and lines[0].startswith("Aligned to planes of %s within " % truth), lines
    words = lines[0].split(":")[-1].split()
    printed = dict(zip(words[0::2], words[1::2]))
    written = dict(ln.split(" ") for ln in (aligned / "APD" / "APD.ply.align_planes").read_text().splitlines())
    assert list(written) == list(NAMES) and printed == written, (printed, written)
    got = PP.PlaneAlignment(float(written["scale"]), tuple(float(written["rotation%d" % e]) for e in range(9)),
                            tuple(float(written["translation%d" % e]) for e in range(3)), int(written["matched_before"]), int(written["matched_after"]),
                            float(written["rms_before"]), float(written["rms_after"]), int(written["steps"]), int(written["stopped"]),
                            int(written["planes_before"]), int(written["planes_after"]), float(written["plane_rms_before"]), float(written["plane_rms_after"]))
    assert PP.bits(got) == PP.bits(want), (got, want)
    after = gpu_pkg.Points.read_ply(aligned / "APD" / "APD.ply")
    want_xyz, want_normal = PA.transformed(point_checker, c.xyz, c.normal, want.scale, want.rotation, want.translation)
    assert np.array_equal(bits32(np.asarray(after.xyz)), bits32(want_xyz)) and np.array_equal(bits32(np.asarray(after.normal)), bits32(want_normal))
    assert np.array_equal(np.asarray(after.bgr), c.bgr)
    assert (plain / "APD" / "APD.ply.vis").read_bytes() == (aligned / "APD" / "APD.ply.vis").read_bytes()
    assert not (plain / "APD" / "APD.ply.align_planes").exists() and not (aligned / "APD" / "APD.ply.align").exists()


def test_binary_refuses_a_bad_value_before_anything_is_read(tmp_path):
    for bad in ("", "truth.ply", "truth.ply,0", "truth.ply,nan", "truth.ply,1,0", "truth.ply,0.5,scale"):
        r = subprocess.run([APD_BIN, str(tmp_path / "no_such_folder"), "0", "--ply-align-planes", bad], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=60)
        assert r.returncode != 0 and "bad value '%s' of --ply-align-planes" % bad in r.stdout and "USAGE" in r.stdout, (bad, r.stdout[-500:])
    for good in ("truth.ply,1", "a,b.ply,0.5", "truth.ply,0.5,64"):
        r = subprocess.run([APD_BIN, str(tmp_path / "no_such_folder"), "0", "--ply-align-planes", good], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=60)
        assert r.returncode != 0 and "bad value" not in r.stdout and "USAGE" not in r.stdout, (good, r.stdout[-500:])
