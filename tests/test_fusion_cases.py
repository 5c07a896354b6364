"""The committed fusion cases (tests/fusion_cases.py) on the sequential loops alone: the ETH oracle (oracle/fusion_oracle.cpp,
RunFusion) and the Tanks and Temples checker (tests/helpers/tat_fusion_ref.cpp).  These tests keep the inputs of
test_gpu_fusion_scale.py honest: every edge they are meant to cover occurs, every case that can emit points does, the long carry
is long and the non-finite case does emit non-finite points.  No GPU needed."""
import copy

import numpy as np
import pytest

import fusion_cases
import tat_checker

VARIANTS = ("eth", "tat_intermediate", "tat_advanced")


@pytest.fixture(scope="module")
def checker(ob, tmp_path_factory):
    return tat_checker.build(ob, tmp_path_factory.mktemp("tat_checker"))


def reference(ob, checker, case, variant, ply_path, stats=None):
    """The sequential loop of `variant` on `case`; writes ply_path, returns the point count."""
    cams = case.cameras(ob.make_camera)
    if variant == "eth":
        return ob.fuse(cams, case.images, case.depths, case.normals, case.weaks, case.pairs, ply_path, blocks=case.block_arrays())
    n, _ = tat_checker.fuse(checker, variant, cams, case.images, case.depths, case.normals, case.pairs, ply_path, blocks=case.blocks,
                            stats=stats)
    return n


def test_every_tag_class_occurs_in_a_committed_case():
    """Every committed case runs through all three loops (here and in test_gpu_fusion_scale.py), so an edge of any case is an
    edge of each loop."""
    seen = set().union(*[fusion_cases.case(name).tags for name in fusion_cases.names()])
    missing = {cls: [t for t in tags if t not in seen] for cls, tags in fusion_cases.TAG_CLASSES.items()}
    assert not any(missing.values()), missing
    assert {"long_carry", "empty"} <= seen
    assert set(fusion_cases.names()) == set(fusion_cases.names("full_frame") + fusion_cases.names("boundary") +
                                            fusion_cases.names("generated") + fusion_cases.names("non_finite"))


@pytest.mark.parametrize("name", fusion_cases.names())
def test_committed_case_on_the_sequential_loops(ob, checker, tmp_path, name):
    """Points > 0 wherever some view has >= 2 sources (ETH: >= 1), exactly 0 in a case empty by construction; the long carry
    spans more than 1024 blocks of 256 pixels; the non-finite case makes each T&T loop emit points with non-finite
    coordinates."""
    case = fusion_cases.case(name)
    most = max(len(p) for p in case.pairs)
    for variant in VARIANTS:
        stats = {}
        n = reference(ob, checker, case, variant, tmp_path / (variant + ".ply"), stats)
        xyz, _ = tat_checker.read_ply(tmp_path / (variant + ".ply"))
        print("%s %s: %d points, %d non-finite, largest gap %s" % (name, variant, n, (~np.isfinite(xyz)).any(1).sum(), stats.get("max_gap")))
        assert n == len(xyz)
        if "empty" in case.tags:
            assert n == 0, variant
        elif most >= (1 if variant == "eth" else 2):
            assert n > 0, variant
        if variant != "eth" and "long_carry" in case.tags:
            assert stats["max_gap"] > 1024 * 256, stats
        if variant != "eth" and name in fusion_cases.names("non_finite"):
            assert (~np.isfinite(xyz)).any(1).sum() >= 1, variant


def test_source_behind_has_points_behind_its_sources():
    """What `vote_target` and the loops' projections meet in this case: z <= 0 for part of the other views' points in one source, for
    every point in the other, which has no depth of its own."""
    case = fusion_cases.case("source_behind")
    assert "source_behind" in case.tags and not case.depths[fusion_cases.BEHIND_ALL].any()
    for i in (0, 1):
        z_part, z_all = fusion_cases.projected_z(case, i, fusion_cases.BEHIND_PART), fusion_cases.projected_z(case, i, fusion_cases.BEHIND_ALL)
        print("source_behind: view %d, %d points, %.1f %% with z <= 0 in view %d, all z < 0 in view %d: %s"
              % (i, len(z_part), 100 * (z_part <= 0).mean(), fusion_cases.BEHIND_PART, fusion_cases.BEHIND_ALL, bool((z_all < 0).all())))
        assert len(z_part) > 1000 and 0.05 <= (z_part <= 0).mean() <= 0.95 and (z_all < 0).all()
        assert fusion_cases.BEHIND_PART in case.pairs[i] and fusion_cases.BEHIND_ALL in case.pairs[i]


def test_rolled_aniso_emits_points_from_the_rolled_views(ob, checker, tmp_path):
    """Every loop emits points whose reference is a rolled view: the case with the source lists of all other views emptied."""
    case = fusion_cases.case("rolled_aniso")
    assert {"rolled", "aniso", "offcentre"} <= case.tags
    for v in fusion_cases.ROLLED_VIEWS:
        assert abs(float(case.views[v]["R"][1])) > 0.5
        only = copy.copy(case)
        only.pairs = [list(p) if i == v else [] for i, p in enumerate(case.pairs)]
        for variant in VARIANTS:
            n = reference(ob, checker, only, variant, tmp_path / ("%s_%d.ply" % (variant, v)))
            print("rolled_aniso: view %d alone, %s: %d points" % (v, variant, n))
            assert n > 100, (v, variant)
