"""Fusion options (apd_fusion_options, apd_fuse_views_opt) where they need no device: the sequential checker of the ETH loop with
options (tests/helpers/eth_fusion_opt_ref.cpp) is pinned to the fixed fusion oracle at the default values, every option set the
device tests use changes some committed case, min_consistent = 2 exercises the consumption order, and the C ABI refuses bad
options before it touches a device.  The fusion itself has no host form (host/fusion.cpp hands the maps to the device): the
fusion with options is compared with this checker in test_gpu_fusion_options.py, through the C ABI, libapd_host.so and the
binary."""
import ctypes as C

import numpy as np
import pytest

import eth_fusion_checker as E
import fusion_cases
from test_tat_fusion_checker import _abi_args

PINNED = [n for n in fusion_cases.names() if n not in fusion_cases.names("non_finite")]
# the committed cases each option set is compared on (here and on the device); chosen by running the checker on every case
CASES_OF_SET = {"a": ["mixed_sizes", "blocks_641x409"], "b": ["mixed_sizes"], "c": ["mixed_sizes", "source_lists"]}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return E.build(tmp_path_factory.mktemp("eth_checker"))


@pytest.mark.parametrize("name", PINNED)
def test_checker_with_default_values_writes_the_oracles_bytes(ob, checker, tmp_path, name):
    case = fusion_cases.case(name)
    n_ref = ob.fuse(case.cameras(ob.make_camera), case.images, case.depths, case.normals, case.weaks, case.pairs, tmp_path / "oracle.ply",
                    blocks=case.block_arrays())
    res = E.fuse_case(checker, ob, case, tmp_path / "checker.ply")
    assert res.count == n_ref
    assert (tmp_path / "checker.ply").read_bytes() == (tmp_path / "oracle.ply").read_bytes()


@pytest.mark.parametrize("key", sorted(E.OPTION_SETS))
def test_every_option_set_changes_the_point_count_of_its_cases(ob, checker, key):
    for name in CASES_OF_SET[key]:
        case = fusion_cases.case(name)
        default, with_options = E.fuse_case(checker, ob, case).count, E.fuse_case(checker, ob, case, **E.OPTION_SETS[key]).count
        print(key, name, default, with_options)
        assert default != with_options and with_options > 0, (key, name, default, with_options)


def test_many_sources_with_three_votes_changes_the_point_count(ob, checker):
    case = fusion_cases.case("sources_32")
    assert 0 < E.fuse_case(checker, ob, case, min_consistent=3).count < E.fuse_case(checker, ob, case).count


def test_points_carry_the_reference_pixels_normal_support_view_and_pixel(ob, checker, tmp_path):
    """The per-point arrays agree with the file and with the inputs: the normal is the normal map's at (view, pixel), the support
    is at least min_consistent and at most the view's sources, pixels rise within a view and views do not fall."""
    case = fusion_cases.case("mixed_sizes")
    res = E.fuse_case(checker, ob, case, tmp_path / "n.ply", ply_normals=True, points=True, min_consistent=2)
    lines, rec = E.read_ply(tmp_path / "n.ply")
    at = lines.index("property float x")
    assert lines[at:at + 9] == ["property float " + k for k in ("x", "y", "z", "nx", "ny", "nz")] + \
        ["property uchar diffuse_" + k for k in ("blue", "green", "red")]
    assert np.array_equal(rec["xyz"], res.xyz) and np.array_equal(rec["normal"], res.normal) and np.array_equal(rec["bgr"], res.bgr)
    for k in range(res.count):
        v, p = res.view[k], res.pixel[k]
        assert np.array_equal(res.normal[k], case.normals[v].reshape(-1, 3)[p])
        assert 2 <= res.support[k] <= len(case.pairs[v])
    assert (np.diff(res.view) >= 0).all()
    assert (np.diff(res.pixel)[np.diff(res.view) == 0] > 0).all()
    _, plain = E.read_ply(_write(checker, ob, case, tmp_path / "p.ply", min_consistent=2))
    assert np.array_equal(plain["xyz"], rec["xyz"]) and np.array_equal(plain["bgr"], rec["bgr"])


def _write(checker, ob, case, path, **kw):
    E.fuse_case(checker, ob, case, path, **kw)
    return path


@pytest.mark.parametrize("name", CASES_OF_SET["a"])
def test_two_votes_exercise_the_consumption_order(ob, checker, name):
    """With min_consistent = 2 a pixel with exactly one vote (which the default rule accepts) is rejected and consumes nothing,
    and a later pixel of the same view then uses the source pixel it would have consumed: the rejected pixel is not in the
    view's pixel list, the later one is, and the default rule -- which accepts the first and lets it consume -- differs."""
    case = fusion_cases.case(name)
    res = E.fuse_case(checker, ob, case, points=True, min_consistent=2)
    base = E.fuse_case(checker, ob, case, points=True)
    assert len(res.reuse) > 0
    for view, rejected, later in res.reuse:
        pixels = res.pixel[res.view == view]
        assert rejected < later and later in pixels and rejected not in pixels
        assert rejected in base.pixel[base.view == view]   # one vote is enough there, and it consumes


# --------------------------------------------------------------------------------------------------------------------
# the C ABI without a device
# --------------------------------------------------------------------------------------------------------------------

def _call(pkg, options, ply, points=True, args=None):
    """apd_fuse_views_opt on two 4 x 4 views that list each other; returns (status, message, count left, points handle left)."""
    L = pkg.lib()
    L.apd_fusion_last_error.restype = C.c_char_p
    keep, a = _abi_args(pkg, [[1], [0]])
    a = list(a if args is None else args)
    weak = np.zeros((4, 4), np.uint8)
    a[5] = (C.c_void_p * 2)(weak.ctypes.data, weak.ctypes.data)
    n, handle = C.c_longlong(-7), C.c_void_p(0x5a5a)
    rc = L.apd_fuse_views_opt(None if options is None else C.byref(options), 0, 2, *a, None if ply is None else str(ply).encode(), C.byref(n),
                              C.byref(handle) if points else None)
    del keep
    return rc, L.apd_fusion_last_error(), n.value, handle.value


def test_default_options_are_the_reference_literals_bit_for_bit(pkg):
    o = pkg.default_fusion_options()
    assert o.struct_size == C.sizeof(pkg.FusionOptions) == 56
    want = dict(E.DEFAULTS)
    for name, value in want.items():
        got = getattr(o, name)
        if isinstance(value, int):
            assert got == value, name
        else:
            assert np.float32(got).tobytes() == np.float32(value).tobytes(), (name, got, value)
    assert (o.variant, o.ply_normals, o.result_on_device) == (0, 0, 0)
    # the literals of csrc/apd_fusion_math.h, as the compiler reads them
    assert np.float32(o.max_angle) == np.float32(0.174533) and np.float32(o.factor_weak) == np.float32(0.45)
    assert pkg.default_fusion_options(min_consistent=2, ply_normals=1).min_consistent == 2
    with pytest.raises(TypeError):
        pkg.default_fusion_options(min_votes=2)


def _bad_options(pkg):
    d = pkg.default_fusion_options
    cases = {"struct_size 0": d(struct_size=0), "struct_size + 8": d(struct_size=64), "struct_size - 4": d(struct_size=52),
             "variant 3": d(variant=3), "variant -1": d(variant=-1), "min_consistent 0": d(min_consistent=0),
             "min_consistent 33": d(min_consistent=33), "min_consistent -2": d(min_consistent=-2)}
    for field in ("max_reproj_error", "max_relative_depth", "max_angle", "depth_weight", "angle_weight", "factor_strong", "factor_weak"):
        for what, value in (("nan", float("nan")), ("inf", float("inf")), ("-inf", float("-inf")), ("negative", -0.5)):
            cases["%s %s" % (field, what)] = d(**{field: value})
    return cases


def test_bad_options_are_refused_before_a_device_is_touched(pkg, tmp_path):
    """struct_size, variant, a threshold that is negative or not finite, min_consistent outside 1 .. 32, neither file nor points:
    APD_ERR_INVALID, a message that starts with the entry point's name, no file, count and points handle untouched -- with or
    without a device (nothing here reaches hipSetDevice: on a machine without one that call would answer APD_ERR_HIP)."""
    out = tmp_path / "x.ply"
    for what, options in _bad_options(pkg).items():
        rc, msg, n, handle = _call(pkg, options, out)
        assert rc == -1, what
        assert msg.startswith(b"apd_fuse_views_opt: ") and not out.exists() and (n, handle) == (-7, 0x5a5a), (what, msg)
    rc, msg, n, handle = _call(pkg, None, out)
    assert rc == -1 and msg == b"apd_fuse_views_opt: null options" and not out.exists() and (n, handle) == (-7, 0x5a5a)
    rc, msg, n, handle = _call(pkg, pkg.default_fusion_options(), None, points=False)
    assert rc == -1 and msg == b"apd_fuse_views_opt: ply_path and points are both NULL" and n == -7
    assert b"struct_size" in _call(pkg, pkg.default_fusion_options(struct_size=8), out)[1]
    assert b"min_consistent" in _call(pkg, pkg.default_fusion_options(min_consistent=40), out)[1]
    assert b"max_angle" in _call(pkg, pkg.default_fusion_options(max_angle=float("nan")), out)[1]


@pytest.mark.parametrize("variant", [1, 2])
def test_tat_variants_refuse_eth_thresholds_and_take_output_options(pkg, tmp_path, variant):
    """Any of the eight values off its default with a T&T variant: APD_ERR_UNSUPPORTED, nothing written.  The output options
    pass the check (the call then goes on to the device)."""
    out = tmp_path / "x.ply"
    for field, value in (("max_reproj_error", 1.0), ("max_relative_depth", 0.02), ("max_angle", 0.2), ("depth_weight", 100.0),
                         ("angle_weight", 5.0), ("min_consistent", 2), ("factor_strong", 0.2), ("factor_weak", 0.5)):
        rc, msg, n, handle = _call(pkg, pkg.default_fusion_options(variant=variant, **{field: value}), out)
        assert rc == -5 and msg.startswith(b"apd_fuse_views_opt: ") and not out.exists() and (n, handle) == (-7, 0x5a5a), (field, msg)
    rc, msg, n, handle = _call(pkg, pkg.default_fusion_options(variant=variant, ply_normals=1, result_on_device=1), out)
    if pkg.device_count() > 0:
        assert rc == 0 and n == 0 and out.exists() and handle not in (None, 0x5a5a)
        assert pkg.lib().apd_points_count(handle) == 0 and pkg.lib().apd_points_xyz(handle) is None
        pkg.lib().apd_points_destroy(handle)
    else:
        assert rc == -2 and msg.startswith(b"apd_fuse_views_opt: hipSetDevice(") and not out.exists() and (n, handle) == (-7, 0x5a5a)


def test_the_shared_argument_checks_answer_under_the_new_name(pkg, tmp_path):
    """What apd_fuse_views refuses, apd_fuse_views_opt refuses with its own prefix; a null ply_path is no longer one of them when
    the points are asked for."""
    out = tmp_path / "x.ply"
    keep, args = _abi_args(pkg, [[1, 0], [0]])
    rc, msg, n, handle = _call(pkg, pkg.default_fusion_options(), out, args=args)
    assert rc == -1 and msg == b"apd_fuse_views_opt: a view lists itself as a source (use the host fusion)" and not out.exists()
    keep, args = _abi_args(pkg, [[1], [0]])
    args = list(args)
    args[2] = 2
    rc, msg, n, handle = _call(pkg, pkg.default_fusion_options(), None, args=args)
    assert rc == -1 and msg.startswith(b"apd_fuse_views_opt: images have") and (n, handle) == (-7, 0x5a5a)
    del keep


def test_points_accessors_take_a_null_object(pkg):
    L = pkg.lib()
    assert L.apd_points_count(None) == 0 and L.apd_points_xyz(None) is None and L.apd_points_pixel(None) is None
    assert L.apd_points_destroy(None) == 0


def test_version_went_up(pkg):
    assert pkg.lib().apd_version() >= 107
