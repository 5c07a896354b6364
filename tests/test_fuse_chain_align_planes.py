"""pipeline.fuse with align_planes: the step after `align` and before `score`, with the recording stand-ins of test_fuse_chain.py
-- which Points methods it calls, in which order and with which defaults, what it closes and what it returns.  No GPU needed."""
import pytest

import test_fuse_chain as T
from test_fuse_chain import FUSED, GIVEN, ORIGIN, SCENE, TRUTH, Recorder

ORDER = T.ORDER + ["align_planes"]
PLANES = (TRUTH, 0.07)


class FakePoints(T.FakePoints):
    def _new(self, method, args, kw, extra):
        assert not self.closed, "%s of a closed Points" % method
        self.rec.called(self.number, method, args, kw)
        return (FakePoints(self.rec),) + extra

    def align_planes(self, *a, **k): return self._value("align_planes", a, k)


def expected_calls(name, on):
    if name == "align_planes":
        return [(on, "align_planes", PLANES, {"iterations": 16}), (on, "transformed", (("align_planes", on),), {})]
    return T.expected_calls(name, on)


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


@pytest.mark.parametrize("return_points", [False, True])
@pytest.mark.parametrize("names", [[], ["align"], ["register", "align"], ["voxel", "register"], T.ORDER])
def test_the_step_comes_after_align_and_before_score(chain, names, return_points):
    for scored in (False, True):
        kw = {name: GIVEN[name] for name in names}
        if "voxel" in names:
            kw["voxel_origin"] = ORIGIN
        if scored:
            kw["score"] = (TRUTH, 0.02)
        rec = Recorder()
        out = chain(rec, "a.ply", "a.vis", return_points, None, align_planes=PLANES, **kw)
        steps = names + ["align_planes"]
        want = [(None, "fusion", (None, True, None), {})]
        for on, name in enumerate(steps):
            want += expected_calls(name, on)
        on = len(steps)
        want += [(on, "write_ply", ("a.ply",), {"normals": False}), (on, "write_vis", ("a.vis",), {})]
        if scored:
            want.append((on, "score", (TRUTH, 0.02), {}))
        assert rec.calls == want, (names, scored)
        assert [p.closed for p in rec.made] == [1] * on + [0 if return_points else 1]
        values = [(name, at) for at, name in enumerate(steps) if name in ("register", "align", "align_planes")] + ([("score", on)] if scored else [])
        assert out == (1000 + on,) + ((rec.made[-1],) if return_points else ()) + tuple(values), (names, scored)


def test_the_iterations_are_passed_on_and_four_values_are_refused(chain):
    rec = Recorder()
    n, alignment, planes, score = chain(rec, None, "a.vis", False, None, align=(TRUTH, 0.1), align_planes=(TRUTH, 0.07, 3), score=(TRUTH, 0.02))
    assert (n, alignment, planes, score) == (1002, ("align", 0), ("align_planes", 1), ("score", 2))
    assert [c for c in rec.calls if c[1] == "align_planes"] == [(1, "align_planes", (TRUTH, 0.07), {"iterations": 3})]
    for others in ({}, {k: v for k, v in GIVEN.items()}):
        for bad, message in (((TRUTH, 0.07, 16, False), r"fuse: align_planes=\(truth, radius\[, iterations\]\), not 4 values"),
                             ((TRUTH, 0.07, 16, 1e-6, 5), r"fuse: align_planes=\(truth, radius\[, iterations\]\), not 5 values"),
                             ((TRUTH,), "not enough values to unpack")):
            rec = Recorder()
            with pytest.raises(ValueError, match=message):
                chain(rec, "a.ply", None, True, None, align_planes=bad, **others)
            assert rec.calls == [] and rec.made == []


def test_without_the_option_nothing_changes(chain):
    rec, again = Recorder(), Recorder()
    out = chain(rec, "a.ply", "a.vis", False, None, voxel_origin=ORIGIN, score=(TRUTH, 0.02), **GIVEN)
    assert chain(again, "a.ply", "a.vis", False, None, voxel_origin=ORIGIN, score=(TRUTH, 0.02), align_planes=None, **GIVEN) == out
    assert rec.calls == again.calls and not [c for c in rec.calls if c[1] == "align_planes"]


@pytest.mark.parametrize("return_points", [False, True])
@pytest.mark.parametrize("method,occurrence", [("align_planes", 0), ("transformed", 2), ("write_ply", 0), ("score", 0)])
def test_the_step_that_raises_leaves_nothing_open(chain, method, occurrence, return_points):
    rec = Recorder(fail_at=(method, occurrence))
    with pytest.raises(RuntimeError, match="planted in " + method):
        chain(rec, "a.ply", "a.vis", return_points, None, voxel_origin=ORIGIN, score=(TRUTH, 0.02), align_planes=PLANES, **GIVEN)
    assert rec.made and [p.closed for p in rec.made] == [1] * len(rec.made)
    assert rec.calls[-1][1] == method
    if method in ("align_planes", "transformed"):    # the third transformed is the new step's
        assert [c[1] for c in rec.calls].count("align_planes") == 1 and rec.calls[-1][0] == len(T.ORDER)
