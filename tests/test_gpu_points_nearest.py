"""The nearest point of another cloud and the score on the device (apd_points_nearest, apd_points_score;
csrc/apd_points_nearest.hip), bitwise against the grid mode of the sequential checker (tests/helpers/points_nearest_ref.cpp):
distances as uint32 (so that inf counts), indices, and the nine fields of the score with the doubles as uint64, in both directions,
for host- and device-resident points on either side in all four combinations.  The pairs of clouds are made in
test_points_nearest.py, where the checker's brute-force mode and a numpy search are held against the grid mode on them; here
also: the same object on both sides, real fused clouds against what the filters and the smoothing make of them, two runs, the
pipeline and the drop-in binary."""
import shutil
import subprocess

import numpy as np
import pytest

import fusion_cases
import points_nearest_checker as PX
import points_radius_checker as PR
from test_gpu_dropin_binary import _write_dense_folder
from test_gpu_fusion_options import APD_BIN, _run, _scene
from test_gpu_points_average import fused
from test_points_nearest import bits32, pair_cases, planted_case, tie_case
from test_points_normals import REAL_CLOUD, REAL_MIN
from test_points_radius import determinism_case, real_cloud_radius
from test_points_voxel import arrays_of, cloud, from_cloud

pytestmark = pytest.mark.gpu
RESIDENCIES = [(False, False), (False, True), (True, False), (True, True)]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return PX.build(tmp_path_factory.mktemp("points_nearest_checker"))


@pytest.fixture(scope="module")
def radius_checker(tmp_path_factory):
    return PR.build(tmp_path_factory.mktemp("points_radius_checker"))


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def points_at(pkg, xyz, on_device):
    return from_cloud(pkg, cloud(xyz), [4], [5], [[]], on_device=on_device)


def assert_nearest(got, want, what):
    distance, index = host(got[0]), host(got[1])
    assert distance.dtype == np.float32 and index.dtype == np.int32 and distance.shape == index.shape == want[1].shape, what
    differ = np.flatnonzero((bits32(distance) != bits32(want[0])) | (index != want[1]))
    assert differ.size == 0, (what, differ[:5], distance[differ[:5]], want[0][differ[:5]], index[differ[:5]], want[1][differ[:5]])


def assert_score(got, want, what):
    assert got._fields == PX.FIELDS and all(isinstance(v, int) for v in got[:4]) and all(isinstance(v, float) for v in got[4:]), what
    assert PX.score_bits(got) == PX.score_bits(want), (what, got, want)


def check_objects(p, q, p_xyz, q_xyz, want, radius, origin, what):
    """nearest in both directions and the score of the Points p and q, which hold the positions p_xyz and q_xyz, against
    want = ((distance, index) p in q, (distance, index) q in p, the score); the inputs are unchanged afterwards."""
    got = p.nearest(q, radius, origin)
    assert (hasattr(got[0], "cpu"), hasattr(got[1], "cpu")) == (p.on_device, p.on_device), what
    assert_nearest(got, want[0], (what, "p in q"))
    assert_nearest(q.nearest(p, radius, origin), want[1], (what, "q in p"))
    assert_score(p.score(q, radius, origin), want[2], what)
    assert np.array_equal(bits32(host(p.xyz)), bits32(p_xyz)) and np.array_equal(bits32(host(q.xyz)), bits32(q_xyz)), (what, "the inputs")


def check(pkg, checker, p_xyz, q_xyz, radius, origin=None, what=""):
    """The pair of clouds as host- and as device-resident points on either side.  Returns the checker's three results."""
    want = (PX.nearest(checker, p_xyz, q_xyz, radius, origin), PX.nearest(checker, q_xyz, p_xyz, radius, origin),
            PX.score(checker, p_xyz, q_xyz, radius, origin))
    made = {(side, dev): points_at(pkg, xyz, dev) for side, xyz in (("p", p_xyz), ("q", q_xyz)) for dev in (False, True)}
    for p_dev, q_dev in RESIDENCIES:
        check_objects(made["p", p_dev], made["q", q_dev], p_xyz, q_xyz, want, radius, origin, (what, p_dev, q_dev))
    for pts in made.values():
        pts.close()
    return want


# --------------------------------------------------------------------------------------------------------------------
# the pairs of test_points_nearest.py
# --------------------------------------------------------------------------------------------------------------------

def test_every_pair_of_clouds(gpu_pkg, checker):
    """Sizes 0, 1, 2, around a wave and a block and the sort-tile sizes on either side, n_P != n_Q, about three points per cell; the
    cell borders, the edges of the grid, points outside it in either cloud and a cloud entirely outside; the planted lattices;
    ties across cells; a crowded cell with queries in it and in its 26 neighbours, and an empty neighbourhood; another origin and
    radius."""
    cases = pair_cases(gpu_pkg)
    for name, (p, q, radius, origin) in cases.items():
        (_, index), _, score = check(gpu_pkg, checker, p, q, radius, origin, what=name)
        if name.startswith("n=") and min(len(p), len(q)) >= 63:
            assert 0 < score.p_within < len(p) and 0 < score.q_within, name     # some queries have a target in reach and some have not
    assert {len(p) for p, _, _, _ in cases.values()} >= {0, 1, 2, 63, 64, 65, 255, 256, 257}


def test_planted_answers_on_the_device(gpu_pkg, checker):
    """The exact distances, indices and rationals of test_points_nearest.py, from the device itself."""
    p, q, chosen = planted_case()
    for dev in (False, True):
        distance, index = points_at(gpu_pkg, p, dev).nearest(points_at(gpu_pkg, q, dev), 1.0)
        assert (host(distance) == np.float32(0.25)).all() and np.array_equal(host(index), chosen)
    p, q, chosen = planted_case(moved=19)
    s = points_at(gpu_pkg, p, True).score(points_at(gpu_pkg, q, False), 0.25)
    assert s[:4] == (171, 512, 152, s.q_within) and s.precision == 152 / 171 and s.recall == s.q_within / 512 and s.mean_p == 0.25 and s.mean_q == 0.25
    assert s.fscore == 2.0 * s.precision * s.recall / (s.precision + s.recall)
    for seed in (None, 6, 7, 8):
        p, q, want = tie_case(seed)
        assert host(points_at(gpu_pkg, p, True).nearest(points_at(gpu_pkg, q, True), 1.0)[1]).tolist() == [want]


def test_the_same_object_on_both_sides(gpu_pkg, checker):
    """Every point inside the grid finds itself at distance 0, or the first of the points that coincide with it; the cloud is
    sorted once."""
    xyz = pair_cases(gpu_pkg)["outside in both"][0]
    xyz = np.concatenate([xyz, xyz[100:130]])           # thirty coincident pairs
    want = (PX.nearest(checker, xyz, xyz, 1.0), PX.nearest(checker, xyz, xyz, 1.0), PX.score(checker, xyz, xyz, 1.0))
    inside = want[0][1] >= 0
    assert np.array_equal(want[0][1][:600][inside[:600]], np.arange(600)[inside[:600]]) and np.array_equal(want[0][1][600:], np.arange(100, 130))
    assert 0 < want[2].p_within < len(xyz) and want[2].precision == want[2].recall and want[2].mean_p == 0.0
    for dev in (False, True):
        pts = points_at(gpu_pkg, xyz, dev)
        check_objects(pts, pts, xyz, xyz, want, 1.0, None, dev)
        # one output alone
        only_index = np.zeros(len(xyz), np.int32)
        if not dev:
            assert gpu_pkg.lib().apd_points_nearest(pts._p, pts._p, 1.0, None, None, only_index.ctypes.data) == 0
            assert np.array_equal(only_index, want[0][1])


def test_two_calls_give_identical_bits(gpu_pkg, checker):
    c, _ = determinism_case()
    q = c.xyz
    p = (q[::2].astype(np.float64) + np.random.default_rng(15).normal(size=(len(q[::2]), 3)) * 0.4).astype(np.float32)
    origin = [0.25, -0.5, 0.125]
    P, Q = points_at(gpu_pkg, p, True), points_at(gpu_pkg, q, True)
    runs = []
    for run in range(2):
        distance, index = P.nearest(Q, 1.0, origin)
        runs.append((bits32(host(distance)).tobytes(), host(index).tobytes(), PX.score_bits(P.score(Q, 1.0, origin))))
    assert runs[0] == runs[1]
    want = PX.nearest(checker, p, q, 1.0, origin)
    assert runs[0][0] == bits32(want[0]).tobytes() and runs[0][1] == want[1].tobytes()
    assert runs[0][2] == PX.score_bits(PX.score(checker, p, q, 1.0, origin)) and 0 < (want[1] >= 0).sum() < len(p)


# --------------------------------------------------------------------------------------------------------------------
# real clouds
# --------------------------------------------------------------------------------------------------------------------

def test_a_real_cloud_against_what_remove_sparse_keeps(gpu_pkg, ob, radius_checker, checker):
    """A fused cloud and the points of it that have at least one other point within a radius, scored at that radius on the same
    grid: every kept point finds itself, so precision is 1 exactly; a removed point has no other point within the radius -- the
    neighbours of contract C11 are the candidates of C17 -- so the points with a kept point in reach are the kept ones, and
    recall is kept / n."""
    name, variant, _ = REAL_CLOUD
    case = fusion_cases.case(name)
    radius = None
    for dev in (False, True):
        pts = fused(gpu_pkg, ob, case, variant, dev)
        before = arrays_of(pts)
        radius = radius or float(np.float32(real_cloud_radius(radius_checker, before) / 3.0))   # the median nearest spacing: about half stay
        kept, removed = pts.remove_sparse(radius, 1)
        n, k = pts.count, kept.count
        assert 0 < removed and 0 < k < n
        s = kept.score(pts, radius)
        assert_score(s, PX.score(checker, host(kept.xyz), before.xyz, radius), (name, dev))
        assert (s.n_p, s.n_q, s.p_within, s.q_within) == (k, n, k, k) and s.precision == 1.0 and s.recall == k / n
        assert s.mean_p == 0.0 and s.mean_q == 0.0 and s.fscore == 2.0 * 1.0 * (k / n) / (1.0 + k / n)
        assert_nearest(pts.nearest(kept, radius), PX.nearest(checker, before.xyz, host(kept.xyz), radius), (name, dev))


def test_a_real_cloud_against_its_smoothed_self(gpu_pkg, ob, radius_checker, checker):
    """Distances that are neither 0 nor planted: against the checker only, in all four residencies."""
    name, variant, _ = REAL_CLOUD
    case = fusion_cases.case(name)
    pts = {dev: fused(gpu_pkg, ob, case, variant, dev) for dev in (False, True)}
    before = arrays_of(pts[False])
    radius = real_cloud_radius(radius_checker, before)
    smoothed = {dev: pts[dev].with_smoothed_positions(radius, REAL_MIN, 2)[0] for dev in (False, True)}
    after = host(smoothed[False].xyz)
    assert np.array_equal(bits32(after), bits32(host(smoothed[True].xyz))) and not np.array_equal(bits32(after), bits32(before.xyz))
    tau = float(np.float32(radius / 8.0))
    want = (PX.nearest(checker, after, before.xyz, tau), PX.nearest(checker, before.xyz, after, tau), PX.score(checker, after, before.xyz, tau))
    assert 0 < want[2].p_within <= len(after) and want[2].mean_p > 0.0
    for p_dev, q_dev in RESIDENCIES:
        check_objects(smoothed[p_dev], pts[q_dev], after, before.xyz, want, tau, None, (name, p_dev, q_dev))


# --------------------------------------------------------------------------------------------------------------------
# the pipeline and the binary
# --------------------------------------------------------------------------------------------------------------------

def truth_of(pkg, xyz, tau, path):
    """A ground truth for the cloud at xyz, written to `path`: two of every three of its points, moved by a Gaussian of tau per
    axis.  Returns its positions."""
    rng = np.random.default_rng(16)
    keep = np.arange(len(xyz)) % 3 != 0
    truth = (xyz[keep].astype(np.float64) + rng.normal(size=(int(keep.sum()), 3)) * tau).astype(np.float32)
    points_at(pkg, truth, False).write_ply(path)
    return truth


def test_through_the_pipeline(gpu_pkg, ob, radius_checker, checker, tmp_path):
    """fuse(score=...) scores the points every other option has produced and changes none of them: the returned score against
    Points.score on the returned points against the checker; the files have the bytes they have without the option."""
    from apd_mvs_amd import pipeline
    case = fusion_cases.case("mixed_sizes")
    scene, results = _scene(gpu_pkg, pipeline, case)
    for kw in (dict(), dict(average=True, voxel=0.05, component_filter=(0.2, 2))):
        n, whole = pipeline.fuse(scene, results, tmp_path / "plain.ply", return_points=True, vis_path=tmp_path / "plain.vis", **kw)
        w = arrays_of(whole)
        tau = real_cloud_radius(radius_checker, w)
        truth_xyz = truth_of(gpu_pkg, w.xyz, tau, tmp_path / "truth.ply")
        want = PX.score(checker, w.xyz, truth_xyz, tau)
        assert 0 < want.p_within < n and 0 < want.q_within <= len(truth_xyz)
        for on_device in (False, True):
            truth = gpu_pkg.Points.read_ply(tmp_path / "truth.ply", on_device=on_device)
            assert truth.on_device == on_device and np.array_equal(bits32(host(truth.xyz)), bits32(truth_xyz))
            assert_score(whole.score(truth, tau), want, kw)
            m, pts, s = pipeline.fuse(scene, results, tmp_path / "m.ply", return_points=True, vis_path=tmp_path / "m.vis", score=(truth, tau), **kw)
            assert m == n == pts.count and np.array_equal(bits32(host(pts.xyz)), bits32(w.xyz))
            assert_score(s, want, kw)
            assert (tmp_path / "m.ply").read_bytes() == (tmp_path / "plain.ply").read_bytes()
            assert (tmp_path / "m.vis").read_bytes() == (tmp_path / "plain.vis").read_bytes()
            m, s = pipeline.fuse(scene, results, tmp_path / "file_only.ply", score=(truth, tau), **kw)
            assert m == n and (tmp_path / "file_only.ply").read_bytes() == (tmp_path / "plain.ply").read_bytes()
            assert_score(s, want, kw)


FLAGS_BEFORE = {"score": [], "score_all": ["--ply-mean", "--ply-voxel", "0.25", "--ply-vis", "--ply-normals", "--ply-radius-filter", "2,1"]}


def run_binary(folder, *extra):
    r = subprocess.run([APD_BIN, str(folder), "0", "--seed", "21", "--iters", "1", "--keep-maps"] + [str(e) for e in extra], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "All done" in r.stdout, r.stdout[-2000:]
    return r.stdout


@pytest.fixture(scope="module")
def folders(gpu_pkg, synth, radius_checker, tmp_path_factory):
    """One small synthetic dense folder (the size of the drop-in tests): per set of flags a run without --ply-score, a ground truth
    made from that run's APD.ply, and a run with the flag after the others.  name -> (plain folder, scored folder, the truth file,
    tau, the scored run's output)."""
    root = tmp_path_factory.mktemp("dense")
    a = root / "a"
    a.mkdir()
    _write_dense_folder(a, synth, 96, 72, 4)
    out = {}
    for name, flags in FLAGS_BEFORE.items():
        plain, scored = root / (name + "_plain"), root / name
        shutil.copytree(a, plain)
        _run(plain, *flags)
        made = gpu_pkg.Points.read_ply(plain / "APD" / "APD.ply")
        tau = real_cloud_radius(radius_checker, arrays_of(made))
        truth = root / (name + ",truth.ply")       # a comma in the path: the value is split at its last one
        truth_of(gpu_pkg, np.asarray(made.xyz), tau, truth)
        shutil.copytree(a, scored)
        out[name] = (plain, scored, truth, tau, run_binary(scored, *flags, "--ply-score", "%s,%.9g" % (truth, tau)))
    return out


def test_binary_prints_and_writes_the_score(gpu_pkg, checker, folders):
    """The printed line, APD.ply.score, Points.score on the files and the checker agree in every bit; APD.ply and APD.ply.vis are
    byte-identical to the run without the flag."""
    for name, (plain, scored, truth, tau, output) in folders.items():
        for file in ("APD.ply", "APD.ply.vis"):
            assert (plain / "APD" / file).exists() == (scored / "APD" / file).exists(), (name, file)
            if (plain / "APD" / file).exists():
                assert (plain / "APD" / file).read_bytes() == (scored / "APD" / file).read_bytes(), (name, file)
        assert not (plain / "APD" / "APD.ply.score").exists()
        made, truth_points = gpu_pkg.Points.read_ply(scored / "APD" / "APD.ply"), gpu_pkg.Points.read_ply(truth)
        want = PX.score(checker, np.asarray(made.xyz), np.asarray(truth_points.xyz), tau)
        assert 0 < want.p_within < made.count and 0 < want.q_within
        assert_score(made.score(truth_points, tau), want, name)
        lines = [ln for ln in output.splitlines() if ln.startswith("Score against ")]
        assert len(lines) == 1 and lines[0].startswith("Score against %s at " % truth), (name, lines)
        words = lines[0].split(":")[-1].split()
        printed = dict(zip(words[0::2], words[1::2]))
        written = dict(ln.split(" ") for ln in (scored / "APD" / "APD.ply.score").read_text().splitlines())
        assert list(written) == list(PX.FIELDS) and printed == written, (name, printed, written)
        got = PX.Score(*[int(written[f]) for f in PX.FIELDS[:4]], *[float(written[f]) for f in PX.FIELDS[4:]])
        assert PX.score_bits(got) == PX.score_bits(want), (name, got, want)


def test_binary_refuses_a_bad_value_before_anything_is_read(tmp_path):
    for bad in ("", "truth.ply", "truth.ply,", ",1", "truth.ply,0", "truth.ply,-1", "truth.ply,nan", "truth.ply,inf", "truth.ply,1e30", "truth.ply,1e-30",
                "truth.ply,1x"):
        r = subprocess.run([APD_BIN, str(tmp_path / "no_such_folder"), "0", "--ply-score", bad], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=60)
        assert r.returncode != 0 and "bad value '%s' of --ply-score" % bad in r.stdout and "USAGE" in r.stdout, (bad, r.stdout[-500:])
    for good in ("truth.ply,1", "a,b.ply,0.5"):
        r = subprocess.run([APD_BIN, str(tmp_path / "no_such_folder"), "0", "--ply-score", good], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=60)
        assert r.returncode != 0 and "bad value" not in r.stdout and "USAGE" not in r.stdout, (good, r.stdout[-500:])
