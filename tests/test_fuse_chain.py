"""pipeline.fuse strings the reworking options together after one fusion: which Points methods it calls, in which order and with
which defaults, what it closes, what it writes and what it returns.  The fusion itself (pipeline._fuse_views) is replaced by a
stand-in that hands out a recording Points, so every subset of the ten reworking options, with and without `score`, runs here in
a few calls each.  No GPU needed."""
import itertools
import types

import pytest

ORDER = ["average", "voxel", "stat_filter", "radius_filter", "component_filter", "smooth", "estimate_normals", "render_visibility",
         "register", "align"]
TRUTH = object()
FUSED = 100   # the count the stand-in fusion returns; every Points made afterwards counts 1000 + its number


class Recorder:
    def __init__(self, fail_at=None):
        self.calls = []      # (number of the object, method, args, kwargs), and ("fusion", ...) for the fusion
        self.made = []
        self.fail_at = fail_at   # (method, occurrence): that call raises

    def called(self, who, method, args, kw):
        self.calls.append((who, method, args, kw))
        if self.fail_at is not None and self.fail_at[0] == method:
            if self.fail_at[1] == 0:
                self.fail_at = None
                raise RuntimeError("planted in " + method)
            self.fail_at = (method, self.fail_at[1] - 1)


class FakePoints:
    device = 0

    def __init__(self, rec):
        self.rec, self.number, self.closed = rec, len(rec.made), 0
        self.count = FUSED if self.number == 0 else 1000 + self.number
        rec.made.append(self)

    def _new(self, method, args, kw, extra):
        assert not self.closed, "%s of a closed Points" % method
        self.rec.called(self.number, method, args, kw)
        return (FakePoints(self.rec),) + extra

    def average(self, *a, **k): return self._new("average", a, k, ())[0]
    def merge_voxels(self, *a, **k): return self._new("merge_voxels", a, k, (0,))
    def remove_statistical(self, *a, **k): return self._new("remove_statistical", a, k, (0, 0.0))
    def remove_sparse(self, *a, **k): return self._new("remove_sparse", a, k, (0,))
    def remove_small_components(self, *a, **k): return self._new("remove_small_components", a, k, (0, 0))
    def with_smoothed_positions(self, *a, **k): return self._new("with_smoothed_positions", a, k, (0,))
    def with_estimated_normals(self, *a, **k): return self._new("with_estimated_normals", a, k, (0,))
    def with_rendered_visibility(self, *a, **k): return self._new("with_rendered_visibility", a, k, (0,))
    def transformed(self, *a, **k): return self._new("transformed", a, k, ())[0]

    def _value(self, method, args, kw):
        assert not self.closed, "%s of a closed Points" % method
        self.rec.called(self.number, method, args, kw)
        return (method, self.number)   # stands for the Registration, the Alignment, the Score

    def register(self, *a, **k): return self._value("register", a, k)
    def align(self, *a, **k): return self._value("align", a, k)
    def score(self, *a, **k): return self._value("score", a, k)
    def write_ply(self, *a, **k): self._value("write_ply", a, k)
    def write_vis(self, *a, **k): self._value("write_vis", a, k)

    def close(self):
        self.closed += 1


GIVEN = dict(average=True, voxel=0.5, stat_filter=(0.3, 8, 1.5), radius_filter=(0.25, 3), component_filter=(0.2, 50), smooth=(0.15, 6, 2),
             estimate_normals=(0.12, 7), render_visibility=(1, 0.01), register=(TRUTH, 0.4, 0.05), align=(TRUTH, 0.1))
ORIGIN = (1.0, 2.0, 3.0)
SCENE = types.SimpleNamespace(num_views=3, cameras=["cam0", "cam1", "cam2", "source only"])


def expected_calls(name, on):
    """The Points calls of one step on object number `on`, as (object, method, args, kwargs); the step's last call makes the next."""
    simple = {"average": ("average", ("cams", "deps", "nors")), "voxel": ("merge_voxels", (0.5, ORIGIN)),
              "stat_filter": ("remove_statistical", (0.3, 8, 1.5)), "radius_filter": ("remove_sparse", (0.25, 3)),
              "component_filter": ("remove_small_components", (0.2, 50)), "smooth": ("with_smoothed_positions", (0.15, 6, 2)),
              "estimate_normals": ("with_estimated_normals", (0.12, 7)),
              "render_visibility": ("with_rendered_visibility", (["cam0", "cam1", "cam2"], 1, 0.01))}
    if name in simple:
        return [(on, simple[name][0], simple[name][1], {})]
    if name == "register":
        return [(on, "register", (TRUTH, 0.4, 0.05), {"trials": 4096, "seed": 0}), (on, "transformed", (("register", on),), {})]
    return [(on, "align", (TRUTH, 0.1), {"iterations": 16, "with_scale": False}), (on, "transformed", (("align", on),), {})]


@pytest.fixture
def chain(pkg, monkeypatch):
    from apd_mvs_amd import pipeline
    monkeypatch.setattr(pipeline, "_fusion_views", lambda scene, results: ("cams", "deps", "nors"))

    def run(rec, ply_path, vis_path, return_points, options=None, **kw):
        def fusion(scene, results, ply, device, colour_images, block_masks, variant, opts, wrap, vis):
            rec.called(None, "fusion", (ply, wrap, vis), {})
            return FUSED, (FakePoints(rec) if wrap else None)
        monkeypatch.setattr(pipeline, "_fuse_views", fusion)
        return pipeline.fuse(SCENE, "results", ply_path, options=options, return_points=return_points, vis_path=vis_path, **kw)
    return run


OUTPUTS = [("a.ply", None, False, None), ("a.ply", "a.vis", False, types.SimpleNamespace(ply_normals=1)), (None, "a.vis", False, None),
           (None, None, True, None), ("a.ply", "a.vis", True, types.SimpleNamespace(ply_normals=0)),
           ("a.ply", None, True, types.SimpleNamespace(ply_normals=1))]


@pytest.mark.parametrize("ply_path,vis_path,return_points,options", OUTPUTS)
def test_every_subset_of_the_options(chain, ply_path, vis_path, return_points, options):
    normals = bool(options is not None and options.ply_normals)
    for picked in itertools.product((False, True), repeat=len(ORDER)):
        names = [name for name, on in zip(ORDER, picked) if on]
        for scored in (False, True):
            kw = {name: GIVEN[name] for name in names}
            if "voxel" in names:
                kw["voxel_origin"] = ORIGIN
            if scored:
                kw["score"] = (TRUTH, 0.02)
            rec = Recorder()
            out = chain(rec, ply_path, vis_path, return_points, options, **kw)
            case = (names, scored)

            wrap = bool(return_points or names or scored)
            want = [(None, "fusion", (None if names else ply_path, wrap, None if wrap else vis_path), {})]
            on = 0
            for name in names:
                want += expected_calls(name, on)
                on += 1
            if names and ply_path is not None:
                want.append((on, "write_ply", (ply_path,), {"normals": normals}))
            if wrap and vis_path is not None:
                want.append((on, "write_vis", (vis_path,), {}))
            if scored:
                want.append((on, "score", (TRUTH, 0.02), {}))
            assert rec.calls == want, case

            assert len(rec.made) == (on + 1 if wrap else 0), case
            for p in rec.made[:-1]:
                assert p.closed == 1, (case, p.number)
            if wrap:
                assert rec.made[-1].closed == (0 if return_points else 1), case

            count = FUSED if names in ([], ["average"]) else 1000 + on
            values = [(name, at) for at, name in enumerate(names) if name in ("register", "align")]
            if scored:
                values.append(("score", on))
            whole = (count,) + ((rec.made[-1],) if return_points else ()) + tuple(values)
            if len(whole) == 1:
                assert type(out) is int and out == count, case
            else:
                assert type(out) is tuple and out == whole, case


def full_chain_methods():
    methods = [c[1] for name in ORDER for c in expected_calls(name, 0)]
    return [(m, k) for m in sorted(set(methods)) for k in range(methods.count(m))] + [("write_ply", 0), ("write_vis", 0), ("score", 0)]


@pytest.mark.parametrize("return_points", [False, True])
@pytest.mark.parametrize("method,occurrence", full_chain_methods())
def test_a_step_that_raises_leaves_nothing_open(chain, method, occurrence, return_points):
    rec = Recorder(fail_at=(method, occurrence))
    with pytest.raises(RuntimeError, match="planted in " + method):
        chain(rec, "a.ply", "a.vis", return_points, None, voxel_origin=ORIGIN, score=(TRUTH, 0.02), **GIVEN)
    assert rec.made and [p.closed for p in rec.made] == [1] * len(rec.made)
    assert rec.calls[-1][1] == method   # nothing ran after the call that raised


@pytest.mark.parametrize("others", [{}, {k: v for k, v in GIVEN.items() if k not in ("align", "register")}])
@pytest.mark.parametrize("bad,message", [
    (dict(align=(TRUTH,)), "not enough values to unpack"),
    (dict(align=(TRUTH, 0.1, 16, False, 5)), r"fuse: align=\(truth, radius\[, iterations\[, with_scale\]\]\), not 5 values"),
    (dict(register=(TRUTH, 0.4)), "not enough values to unpack"),
    (dict(register=(TRUTH, 0.4, 0.05, 4096, 0, 1)),
     r"fuse: register=\(truth, radius, inlier_distance\[, trials\[, seed\]\]\), not 6 values"),
    (dict(score=(TRUTH,)), "not enough values to unpack"),
    (dict(smooth=(0.1, 5)), "not enough values to unpack"),
    (dict(radius_filter=(0.1, 5, 6)), "too many values to unpack")])
def test_a_malformed_option_is_refused_before_the_fusion(chain, bad, message, others):
    rec = Recorder()
    with pytest.raises(ValueError, match=message):
        chain(rec, "a.ply", None, True, None, **{**others, **bad})
    assert rec.calls == [] and rec.made == []


def test_the_optional_tails_of_align_and_register_are_passed_on(chain):
    rec = Recorder()
    n, registration, alignment = chain(rec, "a.ply", None, False, None, register=(TRUTH, 0.4, 0.05, 77, 9), align=(TRUTH, 0.1, 3, True))
    assert (n, registration, alignment) == (1002, ("register", 0), ("align", 1))
    assert [c for c in rec.calls if c[1] in ("register", "align")] == [
        (0, "register", (TRUTH, 0.4, 0.05), {"trials": 77, "seed": 9}), (1, "align", (TRUTH, 0.1), {"iterations": 3, "with_scale": True})]
    rec = Recorder()
    chain(rec, "a.ply", None, False, None, register=(TRUTH, 0.4, 0.05, 77), align=(TRUTH, 0.1, 3))
    assert [c[3] for c in rec.calls if c[1] in ("register", "align")] == [{"trials": 77, "seed": 0}, {"iterations": 3, "with_scale": False}]


def test_neither_file_nor_points_is_refused(chain):
    rec = Recorder()
    with pytest.raises(ValueError, match="neither a PLY file nor the points nor the visibility file"):
        chain(rec, None, None, False, None, **GIVEN)
    assert rec.calls == []
