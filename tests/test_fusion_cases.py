"""The committed fusion cases (tests/fusion_cases.py) on the sequential loops alone: the ETH oracle (oracle/fusion_oracle.cpp,
RunFusion) and the Tanks and Temples checker (tests/helpers/tat_fusion_ref.cpp).  These tests keep the inputs of
test_gpu_fusion_scale.py honest: every edge they are meant to cover occurs, every case that can emit points does, the long carry
is long and the non-finite case does emit non-finite points.  No GPU needed."""
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
