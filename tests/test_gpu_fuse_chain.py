"""Every reworking option at once: one pipeline.fuse call with all eleven, and one run of the drop-in binary with every --ply-* flag,
bitwise against the same Points methods called by hand in the documented order (average, voxel, stat_filter, radius_filter,
component_filter, smooth, estimate_normals, render_visibility, register, align, then score).  What each step computes is checked
where it was added (test_gpu_points_*.py); the order of all of them, the hand-over from each to the next, the files and the
returned tuple are checked here.  tests/test_fuse_chain.py runs every subset against a recording stand-in without a GPU."""
import shutil

import numpy as np
import pytest

import fusion_cases
import points_align_checker as PA
import points_radius_checker as PR
import points_register_checker as RC
import points_voxel_checker as PV
from test_gpu_dropin_binary import _write_dense_folder
from test_gpu_fusion_options import _fuse_saved_maps, _read_dmb, _scene
from test_gpu_points_nearest import run_binary
from test_points_align import rotation
from test_points_radius import real_cloud_radius
from test_points_voxel import arrays_of

pytestmark = pytest.mark.gpu

MIN, SMOOTH_ITERATIONS, SPLAT, TOLERANCE, TRIALS, SEED, ICP_STEPS = 3, 2, 1, 0.01, 512, 3, 4


def steps_at(voxel, radius):
    """The options of pipeline.fuse but the three with a truth, at one radius that keeps most of a cloud of cells of size `voxel`."""
    return dict(average=True, voxel=voxel, stat_filter=(radius, 2, 3.0), radius_filter=(radius, 2), component_filter=(radius, 3),
                smooth=(radius, MIN, SMOOTH_ITERATIONS), estimate_normals=(radius, MIN), render_visibility=(SPLAT, TOLERANCE))


def before_the_truth(pipeline, scene, results, fused, kw):
    """The documented order, one method after the other, up to the steps that take a truth."""
    p = pipeline.average_points(scene, results, fused)
    p, _ = p.merge_voxels(kw["voxel"])
    p, _, _ = p.remove_statistical(*kw["stat_filter"])
    p, _ = p.remove_sparse(*kw["radius_filter"])
    p, _, _ = p.remove_small_components(*kw["component_filter"])
    p, _ = p.with_smoothed_positions(*kw["smooth"])
    p, _ = p.with_estimated_normals(*kw["estimate_normals"])
    return p.with_rendered_visibility([scene.cameras[v] for v in range(scene.num_views)], *kw["render_visibility"])[0]


def nearby(pkg, pts, path, radius):
    """`pts` turned by 2 degrees about (1, 2, 3) through its centre and shifted by a tenth of the radius along every axis, written to
    `path` and read back as the truth.  Smoothed positions and re-estimated normals leave these clouds too few distinct descriptors
    for a registration from far away (that one is held against its checker in test_gpu_points_register.py, through the pipeline and
    the binary, with --ply-align and --ply-score after it); from here the ICP has work to do and the score something to count."""
    xyz = np.asarray(pts.xyz, np.float64)
    R, centre = rotation(2.0), xyz[np.isfinite(xyz).all(axis=1)].mean(axis=0)
    pts.transformed(1.0, R, centre - R @ centre + 0.1 * radius).write_ply(path, normals=True)
    return pkg.Points.read_ply(path)


def by_hand(p, truth, radius):
    """... and the rest of it: (points, Registration, Alignment, Score); the alignment moves the points and the score counts some."""
    registration = p.register(truth, radius, radius / 2, trials=TRIALS, seed=SEED)
    p = p.transformed(registration)
    alignment = p.align(truth, radius, iterations=ICP_STEPS)
    p = p.transformed(alignment)
    score = p.score(truth, radius / 4)
    assert alignment.matched_after > 0 and alignment.steps > 0 and not np.array_equal(alignment.rotation, np.eye(3)) and score.p_within > 0, (alignment, score)
    return p, registration, alignment, score


def score_bits(s):
    return tuple(int(np.float64(v).view(np.uint64)) for v in s)


def radius_for(checker_dir, points):
    """Four times the radius of the real clouds, on averaged and merged points."""
    return float(np.float32(4.0 * real_cloud_radius(PR.build(checker_dir), arrays_of(points))))


def saved_maps(pkg, pipeline, folder):
    """The scene of a dense folder and the maps a run with --keep-maps has left in it, as _fuse_saved_maps reads them."""
    scene = pipeline.load_dense_folder(str(folder), pkg.Camera)
    names = ("depths.dmb", "normals.dmb", "weak.bin", "selected_views.bin")
    return scene, {v: pipeline.ViewState(*[_read_dmb(folder / "APD" / ("%08d" % v) / name) for name in names]) for v in range(scene.num_views)}


def test_all_eleven_options_through_the_pipeline(gpu_pkg, tmp_path):
    from apd_mvs_amd import pipeline
    scene, results = _scene(gpu_pkg, pipeline, fusion_cases.case("mixed_sizes"))
    options = gpu_pkg.default_fusion_options(ply_normals=1)
    _, start = pipeline.fuse(scene, results, None, return_points=True, options=options, average=True, voxel=0.05)
    radius = radius_for(tmp_path, start)
    kw = steps_at(0.05, radius)
    _, fused = pipeline.fuse(scene, results, None, return_points=True, options=options)
    reworked = before_the_truth(pipeline, scene, results, fused, kw)
    truth = nearby(gpu_pkg, reworked, tmp_path / "truth.ply", radius)   # the cloud the last three steps are given, moved a little
    want, registration, alignment, score = by_hand(reworked, truth, radius)
    want.write_ply(tmp_path / "hand.ply", normals=True)
    want.write_vis(tmp_path / "hand.vis")
    w = arrays_of(want)
    print(fused.count, "fused,", w.count, "left, radius", radius, registration, alignment, score)
    assert 0 < w.count <= start.count

    asked = dict(kw, register=(truth, radius, radius / 2, TRIALS, SEED), align=(truth, radius, ICP_STEPS), score=(truth, radius / 4), options=options)
    n, got, r, a, s = pipeline.fuse(scene, results, tmp_path / "all.ply", return_points=True, vis_path=tmp_path / "all.vis", **asked)
    assert n == got.count == w.count
    PV.assert_equal(arrays_of(got), w, "all eleven")
    assert RC.bits(r) == RC.bits(registration) and PA.bits(a) == PA.bits(alignment) and score_bits(s) == score_bits(score)
    assert (tmp_path / "all.ply").read_bytes() == (tmp_path / "hand.ply").read_bytes()
    assert (tmp_path / "all.vis").read_bytes() == (tmp_path / "hand.vis").read_bytes()
    # the files alone: the same bytes and the same values without the points
    m, r, a, s = pipeline.fuse(scene, results, tmp_path / "files.ply", vis_path=tmp_path / "files.vis", **asked)
    assert m == n and RC.bits(r) == RC.bits(registration) and PA.bits(a) == PA.bits(alignment) and score_bits(s) == score_bits(score)
    assert (tmp_path / "files.ply").read_bytes() == (tmp_path / "hand.ply").read_bytes()
    assert (tmp_path / "files.vis").read_bytes() == (tmp_path / "hand.vis").read_bytes()


def test_binary_with_every_ply_flag(gpu_pkg, synth, tmp_path):
    """APD.ply, APD.ply.vis and the figures of APD.ply.register, .align and .score of one run with every --ply-* flag against the
    methods by hand on the points the pipeline makes from the binary's maps."""
    from apd_mvs_amd import pipeline
    a, plain, folder = tmp_path / "a", tmp_path / "plain", tmp_path / "all"
    a.mkdir()
    _write_dense_folder(a, synth, 96, 72, 4)
    shutil.copytree(a, plain)
    run_binary(plain)
    options = gpu_pkg.default_fusion_options(ply_normals=1)
    _, start = _fuse_saved_maps(gpu_pkg, plain, None, return_points=True, options=options, average=True, voxel=0.25)
    truth_file = tmp_path / "truth,1.ply"          # a comma in the path: the values are read from their ends
    radius = radius_for(tmp_path, start)
    kw = steps_at(0.25, radius)
    # the truth: what the maps of the plain run, which are those of every run, give up to --ply-render-vis, moved a little
    scene, results = saved_maps(gpu_pkg, pipeline, plain)
    truth = nearby(gpu_pkg, before_the_truth(pipeline, scene, results, pipeline.fuse(scene, results, None, return_points=True, options=options)[1], kw),
                   truth_file, radius)
    shutil.copytree(a, folder)
    number = lambda *values: ",".join("%.9g" % v if isinstance(v, float) else str(v) for v in values)
    output = run_binary(folder, "--ply-normals", "--ply-vis", "--ply-mean", "--ply-voxel", number(kw["voxel"]), "--ply-stat-filter", number(*kw["stat_filter"]),
                        "--ply-radius-filter", number(*kw["radius_filter"]), "--ply-component-filter", number(*kw["component_filter"]),
                        "--ply-smooth", number(*kw["smooth"]), "--ply-estimate-normals", number(*kw["estimate_normals"]),
                        "--ply-render-vis", number(*kw["render_visibility"]),
                        "--ply-register", number(truth_file, radius, float(np.float32(radius / 2)), TRIALS, SEED),
                        "--ply-align", number(truth_file, radius, ICP_STEPS), "--ply-score", number(truth_file, float(np.float32(radius / 4))))
    said = [ln.split(" ")[0] for ln in output.splitlines()]
    order = ["Merged", "Removed", "Removed", "Removed", "Smoothed", "Estimated", "Rendered", "Registered", "Aligned", "Score", "Fused", "Visibility"]
    assert [word for word in said if word in order] == order, output[-3000:]

    scene, results = saved_maps(gpu_pkg, pipeline, folder)
    _, fused = pipeline.fuse(scene, results, None, return_points=True, options=options)
    want, registration, alignment, score = by_hand(before_the_truth(pipeline, scene, results, fused, kw), truth, radius)
    want.write_ply(tmp_path / "hand.ply", normals=True)
    want.write_vis(tmp_path / "hand.vis")
    print(fused.count, "fused,", want.count, "left, radius", radius, registration, alignment, score)
    assert 0 < want.count <= start.count
    assert (folder / "APD" / "APD.ply").read_bytes() == (tmp_path / "hand.ply").read_bytes()
    assert (folder / "APD" / "APD.ply.vis").read_bytes() == (tmp_path / "hand.vis").read_bytes()
    written = {kind: dict(ln.split(" ") for ln in (folder / "APD" / ("APD.ply." + kind)).read_text().splitlines()) for kind in ("register", "align", "score")}
    transform = lambda d: (float(d["scale"]), tuple(float(d["rotation%d" % e]) for e in range(9)), tuple(float(d["translation%d" % e]) for e in range(3)))
    r, al, s = written["register"], written["align"], written["score"]
    assert RC.bits(RC.Registration(*transform(r), *[int(r[f]) for f in RC.FIELDS[3:10]], float(r["rms_after"]), int(r["stopped"]))) == RC.bits(registration)
    assert PA.bits(PA.Alignment(*transform(al), int(al["matched_before"]), int(al["matched_after"]), float(al["rms_before"]), float(al["rms_after"]),
                                int(al["steps"]), int(al["stopped"]))) == PA.bits(alignment)
    assert list(s) == list(score._fields) and score_bits([int(s[f]) if f in score._fields[:4] else float(s[f]) for f in score._fields]) == score_bits(score)
