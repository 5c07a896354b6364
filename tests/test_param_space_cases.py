"""The ORACLE ALONE on every case of tests/param_space_cases.py: bit equality of the HIP path with the oracle
(tests/test_gpu_param_space.py) shows that a kernel honours a parameter only where the parameter changes what the oracle computes,
so each case is held to that here, on the host.

  * 19 to 31 source views: the upper views are selected and weighted in the APD and the geometric pass, and the scene drives
    pixels through the weak path (K3 finds reliable WEAK pixels);
  * every variation: some state array of the oracle differs from the same case with the field at its default.

Lines starting with PARAM_SPACE carry the counts (profiles/param_space/README.md)."""
import numpy as np
import pytest

import common
import param_space_cases as pc

_PRIORS = {}


def _key(case, plist):
    return (case.W, case.H, case.N, case.scene_seed, case.textureless, case.floats, repr([sorted(p.items()) for p in plist]))


def run_oracle(ob, synth, case, default=False, observe=None):
    """The oracle through every pass of `case`; observe(pi, kid, it, oracle) after every kernel.  Returns the state arrays after the
    last kernel.  The prior a sequence of passes leaves is kept: variations of one scene share their first passes."""
    sc, imgs, deps = pc.scene(synth, case)
    plist, prior, last = [], None, len(case.passes) - 1
    for pi in range(len(case.passes)):
        p = pc.pass_params(case, sc, pi, default)
        plist.append(p)
        if pi < last and observe is None and _key(case, plist) in _PRIORS:
            prior = _PRIORS[_key(case, plist)]
            continue
        o = common.make_oracle(ob, sc, imgs, case.N, p, depths=deps if p.get("geom_consistency") else None, prior=prior)
        for kid, it in pc.steps(case, pi, p, o.weak_count):
            o.run_kernel(kid, it)
            if observe is not None:
                observe(pi, kid, it, o)
        out = {name: getattr(o, oa).copy() for name, _, oa in common.ORACLE_STATES if name != "neighbours" or o.weak_count > 0}
        prior = common.postprocess(o.planes.copy(), o.weak_info.copy(), o.selected_views.copy(), np.float32(p["depth_min"]), np.float32(p["depth_max"]))
        _PRIORS[_key(case, plist)] = prior
        o.close()
    return out


def _differing(a, b):
    """{state: pixels (rows) whose bytes differ}; NaNs of both sides compare equal."""
    out = {}
    for name in a:
        if name not in b or a[name].shape != b[name].shape:
            out[name] = -1   # the neighbour table exists on one side only, or has another length
            continue
        rows = a[name].shape[0] * (1 if name == "neighbours" else a[name].shape[1])   # pixels; WEAK pixels of the neighbour table
        n = int((common.canon_nan(a[name]).reshape(rows, -1) != common.canon_nan(b[name]).reshape(rows, -1)).any(axis=1).sum())
        if n:
            out[name] = n
    return out


@pytest.mark.parametrize("case", pc.VIEW_CASES, ids=repr)
def test_upper_views_are_selected_weighted_and_the_weak_path_runs(ob, synth, case):
    """What a kernel that drops the views past 16 (or past 24: the fourth word of ViewWeights<32>) would get wrong must be there to
    get wrong: after the APD pass and after the geometric pass some pixel selects, and some pixel weights, a view of the upper range.
    The upper range is 24..30 at N = 31 and 16..N-1 below (N = 19 and 24 have no view 24)."""
    lo = 24 if case.N > 24 else 16
    upper = np.uint32(sum(1 << b for b in range(lo, case.N)))
    seen = {}

    def observe(pi, kid, it, o):
        if kid == 3:
            seen[(pi, "weak")] = o.weak_count
            seen[(pi, "reliable")] = int(((o.weak_reliable != 0) & (o.weak_info == pc.fl.WEAK)).sum())
        if kid == 15:
            seen[(pi, "selected")] = int(((o.selected_views & upper) != 0).sum())
            seen[(pi, "weighted")] = int((o.view_weight[..., lo:case.N] != 0).any(axis=-1).sum())
        if kid in (9, 10) and it == 1:
            seen[(pi, "weak selected")] = int((((o.selected_views & upper) != 0) & (o.weak_info == pc.fl.WEAK)).sum())

    run_oracle(ob, synth, case, observe=observe)
    for pi, kind in ((1, "APD"), (2, "geometric")):
        print("PARAM_SPACE %s, %s pass: weak_count %d, reliable WEAK pixels after K3 %d; pixels with a bit %d..%d of selected_views %d "
              "(WEAK pixels after K10: %d), with a non-zero view_weight byte %d..%d %d"
              % (case, kind, seen[(pi, "weak")], seen[(pi, "reliable")], lo, case.N - 1, seen[(pi, "selected")], seen[(pi, "weak selected")],
                 lo, case.N - 1, seen[(pi, "weighted")]))
        assert seen[(pi, "selected")] > 0 and seen[(pi, "weighted")] > 0, (kind, seen)
        assert seen[(pi, "weak selected")] > 0, (kind, seen)      # K9/K10 wrote such a bit too, not K6/K7 alone
        assert seen[(pi, "weak")] > 50 and seen[(pi, "reliable")] > 0, (kind, seen)


@pytest.mark.parametrize("case", pc.VARIATION_CASES, ids=repr)
def test_a_variation_changes_what_the_oracle_computes(ob, synth, case):
    after_k5 = {}

    def observe(pi, kid, it, o):
        if kid == 5 and pi == len(case.passes) - 1:
            after_k5["costs"], after_k5["views"] = o.costs.copy(), o.selected_views.copy()

    varied = run_oracle(ob, synth, case, observe=observe if case.vary == "top_k" else None)
    default = run_oracle(ob, synth, case, default=True)
    diff = _differing(varied, default)
    print("PARAM_SPACE %s against %s at its default: pixels that differ %s" % (case, case.vary, diff or "NONE"))
    assert diff, "the oracle computes the same with and without the variation: the case can catch nothing"
    if case.vary == "top_k" and case.passes[-1]["top_k"] <= 0:
        # no view is summed: APD.cu:616-662 returns 2.0 and leaves selected_views empty
        assert (after_k5["costs"] == np.float32(2.0)).all() and not after_k5["views"].any()
    has_nan = any(a.dtype == np.float32 and bool(np.isnan(a).any()) for a in varied.values())
    assert has_nan == case.nans, "tests/test_gpu_param_space.py compares NaN words as one pattern exactly where the oracle leaves some"
    if case.vary in ("rotate_time", "depth_range"):
        assert "neighbours" in diff or "reliable" in diff, diff   # K3's own outputs moved, not only what follows them
    if case.vary == "depth_range":
        sc = pc.scene(synth, case)[0]
        lo, hi = pc.depth_range(case, sc)
        assert hi <= lo
