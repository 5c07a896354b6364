"""The geometric filter without a device: known answers of the sequential checker (tests/helpers/filter_ref.cpp), the argument
refusals of apd_filter_views (include/apd_mi355x.h), which answer before any device is touched, and its declaration and export."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import filter_checker as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 8, 6


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return F.build(tmp_path_factory.mktemp("filter_checker"))


def _twin_views(make_camera):
    """Two views with one camera (f = 8, R = I, t = 0) looking at the fronto-parallel plane z = 8 with normal (0, 0, -1): pixel
    (x, y) lifts to (x - cx, y - cy, 8) and drops on itself in both views, in exact binary32 arithmetic."""
    K = np.array([8, 0, 3, 0, 8, 2, 0, 0, 1], np.float32)
    cam = make_camera(K, np.eye(3, dtype=np.float32), np.zeros(3, np.float32), W, H, 1.0, 100.0)
    cams = (type(cam) * 2)(cam, cam)
    depths = [np.full((H, W), 8.0, np.float32) for _ in range(2)]
    normal = np.zeros((H, W, 3), np.float32)
    normal[..., 2] = -1.0
    weaks = [(np.arange(H * W).reshape(H, W) % 2).astype(np.uint8) for _ in range(2)]   # WEAK (0) and STRONG (1) pixels
    return cams, depths, [normal, normal.copy()], weaks, [[1], [0]]


def test_identical_views_vote_once_with_weight_one(ob, checker):
    cams, depths, normals, weaks, pairs = _twin_views(ob.make_camera)
    for depth, votes, consistency in F.filter_views(checker, cams, depths, normals, weaks, pairs):
        # reprojection error 0, depth difference 0, angle acos(1) = 0: exp_c9(-0.0f) == 1, above 0.3 and above 0.45
        assert (votes == 1).all() and np.array_equal(consistency.view(np.uint32), np.full((H, W), 0x3F800000, np.uint32))
        assert np.array_equal(depth.view(np.uint32), depths[0].view(np.uint32))
        assert (weaks[0] == 0).any() and (weaks[0] == 1).any()


def test_a_source_depth_two_percent_off_takes_the_vote(ob, checker):
    cams, depths, normals, weaks, pairs = _twin_views(ob.make_camera)
    depths[1][4, 5] = np.float32(8.0 * 1.02)
    (depth, votes, consistency), _ = F.filter_views(checker, cams, depths, normals, weaks, pairs)
    assert votes[4, 5] == 0 and consistency[4, 5] == 0.0 and depth[4, 5] == 0.0
    others = np.ones((H, W), bool)
    others[4, 5] = False
    assert (votes[others] == 1).all() and (depth[others] == 8.0).all() and (consistency[others] == 1.0).all()


def test_two_votes_asked_of_one_source_accepts_nothing_and_keeps_the_counts(ob, checker):
    cams, depths, normals, weaks, pairs = _twin_views(ob.make_camera)
    plain = F.filter_views(checker, cams, depths, normals, weaks, pairs)
    strict = F.filter_views(checker, cams, depths, normals, weaks, pairs, min_consistent=2)
    for (_, votes, consistency), (depth2, votes2, consistency2) in zip(plain, strict):
        assert (depth2 == 0.0).all()
        assert np.array_equal(votes, votes2) and np.array_equal(consistency.view(np.uint32), consistency2.view(np.uint32))
        assert (votes2 == 1).all()


def test_blocked_and_empty_pixels_are_zero_in_all_three(ob, checker):
    cams, depths, normals, weaks, pairs = _twin_views(ob.make_camera)
    depths[0][1, 1] = 0.0
    depths[0][1, 2] = -3.0
    block = np.full((H, W), 128, np.uint8)
    block[2, 3] = 127
    (depth, votes, consistency), (depth1, votes1, _) = F.filter_views(checker, cams, depths, normals, weaks, pairs, blocks=[block, None])
    for r, c in ((1, 1), (1, 2), (2, 3)):
        assert votes[r, c] == 0 and consistency[r, c] == 0.0 and depth[r, c] == 0.0
    assert votes.sum() == H * W - 3
    # the block mask of view 0 hides nothing from view 1: only the two pixels without a depth cannot vote for it
    assert votes1[2, 3] == 1 and votes1[1, 1] == 0 and votes1[1, 2] == 0 and depth1[2, 3] == 8.0


# --------------------------------------------------------------------------------------------------------------------
# apd_filter_views: declared, exported, and its refusals
# --------------------------------------------------------------------------------------------------------------------

def test_the_entry_point_is_declared_and_exported(pkg):
    text = open(os.path.join(ROOT, "include", "apd_mi355x.h")).read()
    assert re.search(r"\bint apd_filter_views\(const apd_fusion_options \*options, int device, int num_views,", text)
    assert hasattr(C.CDLL(pkg.library_path()), "apd_filter_views")
    assert hasattr(pkg.lib().apd_filter_views, "argtypes")


class _Call:
    """A well-formed apd_filter_views call on the twin views, whose parts a test replaces before it is made."""

    def __init__(self, pkg):
        self.pkg = pkg
        self.cams, self.depths, self.normals, self.weaks, pairs = _twin_views(pkg.make_camera)
        self.options = pkg.default_fusion_options()
        self.rows, self.cols = [H, H], [W, W]
        self.pairs = pairs
        self.out = [[np.full((H, W), -7.0, np.float32) for _ in range(2)], [np.full((H, W), 77, np.uint8) for _ in range(2)],
                    [np.full((H, W), -7.0, np.float32) for _ in range(2)]]
        self.tables = [self.table(t) for t in self.out]
        self.maps = [self.table(m) for m in (self.depths, self.normals, self.weaks)]

    @staticmethod
    def table(arrays):
        return (C.c_void_p * len(arrays))(*[None if a is None else a.ctypes.data for a in arrays])

    def __call__(self):
        L = self.pkg.lib()
        flat = [s for p in self.pairs for s in p]
        offs = (C.c_int * 3)(*np.cumsum([0] + [len(p) for p in self.pairs]).tolist())
        rc = L.apd_filter_views(C.byref(self.options), 0, 2, C.byref(self.cams), self.maps[0], self.maps[1], self.maps[2], None,
                                (C.c_int * 2)(*self.rows), (C.c_int * 2)(*self.cols), offs, (C.c_int * max(len(flat), 1))(*flat), 0,
                                self.tables[0], self.tables[1], self.tables[2], 0)
        return rc, L.apd_fusion_last_error().decode()

    def untouched(self):
        return all((a == (77 if a.dtype == np.uint8 else -7.0)).all() for t in self.out for a in t)


def _set(**fields):
    def change(call):
        for k, v in fields.items():
            setattr(call.options, k, v)
    return change


def _no_tables(call):
    call.tables = [None, None, None]


def _empty_tables(call):
    call.tables = [call.table([None, None]), None, call.table([None, None])]


def _output_is_an_input(call):
    call.tables[0] = call.table([call.out[0][0], call.depths[0]])


def _output_is_a_weak_map(call):
    call.tables[1] = call.table([call.weaks[1], None])


def _no_weak_maps(call):
    call.maps[2] = None


def _own_source(call):
    call.pairs = [[1], [1]]


def _oversized(call):
    call.rows, call.cols = [H, 65536], [W, 65536]


REFUSALS = {
    "struct_size": _set(struct_size=8), "tat_variant": _set(variant=1), "unknown_variant": _set(variant=9),
    "negative": _set(max_reproj_error=-1.0), "nan": _set(depth_weight=float("nan")), "infinite": _set(factor_weak=float("inf")),
    "min_consistent_0": _set(min_consistent=0), "min_consistent_33": _set(min_consistent=33), "no_tables": _no_tables,
    "empty_tables": _empty_tables, "output_is_an_input": _output_is_an_input, "output_is_a_weak_map": _output_is_a_weak_map,
    "no_weak_maps": _no_weak_maps, "own_source": _own_source, "oversized": _oversized,
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_bad_arguments_are_refused_before_any_device_call(pkg, name):
    """APD_ERR_INVALID (-1) with the entry point's name in front, on a machine with or without a device (without one, a call
    that got as far as the device would answer APD_ERR_HIP), and no output buffer is written."""
    call = _Call(pkg)
    REFUSALS[name](call)
    rc, message = call()
    assert rc == -1 and message.startswith("apd_filter_views: ") and len(message) > len("apd_filter_views: "), (rc, message)
    assert call.untouched()
    assert np.array_equal(call.depths[0], np.full((H, W), 8.0, np.float32)) and (call.weaks[1] == call.weaks[0]).all()


def test_without_a_device_a_good_call_fails_loudly(pkg):
    """No host fall-back: the well-formed call needs the device."""
    if pkg.device_count() > 0:
        pytest.skip("a GPU is visible")
    call = _Call(pkg)
    rc, message = call()
    assert rc == -2 and message.startswith("apd_filter_views: ") and call.untouched()
