"""The Tanks and Temples fusion checker (tests/helpers/tat_fusion_ref.cpp: RunFusion_TAT_Intermediate / RunFusion_TAT_advanced,
APD.cpp:979-1296, as the sequential loops they are) against answers derived by hand on tiny scenes, and the C ABI of the device
fusion (apd_fuse_views_variant) where it needs no device.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import tat_checker

W, H, F, Z = 8, 6, 10.0, 10.0


@pytest.fixture(scope="module")
def checker(ob, tmp_path_factory):
    return tat_checker.build(ob, tmp_path_factory.mktemp("tat_checker"))


def _scene(pkg, shifts, tilt_deg=None):
    """Fronto-parallel plane at depth Z seen by cameras R = I, t = (-s, 0, 0): pixel (r, c) of view 0 is pixel (r, c - s) of
    a view with shift s, exactly (f = Z).  Normals face the cameras; tilt_deg[v] tilts view v's normals about the y axis."""
    K = [F, 0, 3.5, 0, F, 2.5, 0, 0, 1]
    cams = [pkg.make_camera(K, np.eye(3), [-s, 0.0, 0.0], W, H, 1.0, 100.0) for s in shifts]
    depths, normals, images = [], [], []
    for v in range(len(shifts)):
        depths.append(np.full((H, W), Z, np.float32))
        a = np.deg2rad((tilt_deg or {}).get(v, 0.0))
        n = np.zeros((H, W, 3), np.float32)
        n[..., 0], n[..., 2] = np.sin(a), -np.cos(a)
        normals.append(n)
        images.append((np.arange(H * W, dtype=np.float32).reshape(H, W) * 3 + 40 * v) % 256)
    return (type(cams[0]) * len(cams))(*cams), images, depths, normals


def _pixels(xyz):
    """(row, col) of view 0's pixels the points were lifted from: world x = c - 3.5, y = r - 2.5."""
    return [(int(round(p[1] + 2.5)), int(round(p[0] + 3.5))) for p in xyz]


@pytest.mark.parametrize("variant", ["tat_intermediate", "tat_advanced"])
def test_stale_entries_emit_and_never_valid_sources_do_not(pkg, checker, tmp_path, variant):
    """Pixel (r, c) of view 0 is (r, c + 1) of source 1 and (r, c + 2) of source 2; source 2 has no depth in row 0.  Row 0: source 2
    is never valid -> no point, even at (0, 7) where both sources are out of bounds.  Rows >= 1: (r, 6) has source 2 out of bounds
    and its entry stale from (r, 5), (r, 7) has both out of bounds and both entries stale -> points all the same."""
    cams, images, depths, normals = _scene(pkg, [0, -1, -2])
    depths[2][0] = 0.0
    n, stale = tat_checker.fuse(checker, variant, cams, images, depths, normals, [[1, 2], [], []], tmp_path / "a.ply")
    xyz, bgr = tat_checker.read_ply(tmp_path / "a.ply")
    assert n == len(xyz) == W * (H - 1)
    assert _pixels(xyz) == [(r, c) for r in range(1, H) for c in range(W)]
    assert stale == 2 * (H - 1)
    assert np.array_equal(xyz[:, 2], np.full(n, Z, np.float32))
    ref = images[0].reshape(-1)[W:]
    if variant == "tat_advanced":  # the reference pixel's colour alone
        assert np.array_equal(bgr, np.repeat(ref.astype(np.uint8)[:, None], 3, 1))
    else:  # (ref + the colours at the entries' source pixels) / (count + 1)
        for (r, c), (r1, c1), (r2, c2) in (((1, 7), (1, 7), (1, 7)),   # stale: source 1 from (1, 6), source 2 from (1, 5)
                                           ((2, 4), (2, 5), (2, 6))):  # fresh
            want = np.uint8(np.float32(np.float32(images[0][r, c] + images[1][r1, c1]) + images[2][r2, c2]) / np.float32(3.0))
            assert (bgr[_pixels(xyz).index((r, c))] == want).all()
        assert not np.array_equal(bgr[:, 0], ref.astype(np.uint8))


@pytest.mark.parametrize("variant", ["tat_intermediate", "tat_advanced"])
def test_gap_statistic_of_the_stale_entries(pkg, checker, tmp_path, variant):
    """The scene above: (r, 6) uses source 2's entry from (r, 5) (gap 1), (r, 7) uses source 1's from (r, 6) (gap 1) and
    source 2's from (r, 5) (gap 2); every other point uses fresh entries (gap 0) -> the largest gap is 2."""
    cams, images, depths, normals = _scene(pkg, [0, -1, -2])
    depths[2][0] = 0.0
    stats = {}
    n, stale = tat_checker.fuse(checker, variant, cams, images, depths, normals, [[1, 2], [], []], tmp_path / "a.ply", stats=stats)
    assert (n, stale) == (W * (H - 1), 2 * (H - 1))
    assert stats == {"max_gap": 2}
    # source 2 keeps depth in rows 0 (zeroed above) and 1 only: every pixel of rows >= 2 carries its entry from (1, 5)
    depths[2][2:] = 0.0
    n, _ = tat_checker.fuse(checker, variant, cams, images, depths, normals, [[1, 2], [], []], tmp_path / "b.ply", stats=stats)
    assert n == W * (H - 1) and stats["max_gap"] == (H - 1) * W + 7 - (W + 5)


def test_one_source_emits_nothing(pkg, checker, tmp_path):
    cams, images, depths, normals = _scene(pkg, [0, 1, 2])
    for variant in ("tat_intermediate", "tat_advanced"):
        n, stale = tat_checker.fuse(checker, variant, cams, images, depths, normals, [[1], [0], [0]], tmp_path / "a.ply")
        assert (n, stale) == (0, 0)
        assert tat_checker.read_ply(tmp_path / "a.ply")[0].shape == (0, 3)


@pytest.mark.parametrize("tilt,kept", [(9.0, True), (11.0, False)])
def test_intermediate_rejects_normals_tilted_past_k_times_3_plus_4_degrees_and_advanced_ignores_them(pkg, checker, tmp_path, tilt, kept):
    """Two sources: only k = 2, angle threshold 2 * 3 + 4 = 10 degrees.  Source 1's normals tilted by 9 degrees still count, by
    11 they do not and no pixel has two sources; the advanced loop has no angle test."""
    cams, images, depths, normals = _scene(pkg, [0, -1, 1], tilt_deg={1: tilt})
    pairs = [[1, 2], [], []]
    n_int, _ = tat_checker.fuse(checker, "tat_intermediate", cams, images, depths, normals, pairs, tmp_path / "i.ply")
    n_adv, _ = tat_checker.fuse(checker, "tat_advanced", cams, images, depths, normals, pairs, tmp_path / "a.ply")
    flat = _scene(pkg, [0, -1, 1])
    n_flat, _ = tat_checker.fuse(checker, "tat_advanced", flat[0], flat[1], flat[2], flat[3], pairs, tmp_path / "f.ply")
    assert n_flat > 0 and n_adv == n_flat
    assert n_int == (n_flat if kept else 0)


def test_masks_of_emitted_reference_pixels_invalidate_them_as_sources(pkg, checker, tmp_path):
    """View 0 emits every pixel it can and marks it; view 1 then finds every source pixel in view 0 masked (never valid: no
    entry, no point) but those view 0 could not emit."""
    cams, images, depths, normals = _scene(pkg, [0, 0, 0])
    n0, _ = tat_checker.fuse(checker, "tat_advanced", cams, images, depths, normals, [[1, 2], [], []], tmp_path / "a.ply")
    assert n0 == W * H
    n, _ = tat_checker.fuse(checker, "tat_advanced", cams, images, depths, normals, [[1, 2], [0, 2], []], tmp_path / "b.ply")
    assert n == W * H  # view 1: source 0 is masked everywhere, so one source at most
    n, _ = tat_checker.fuse(checker, "tat_advanced", cams, images, depths, normals, [[1, 2], [2, 0], [0, 1]], tmp_path / "c.ply")
    assert n == W * H  # view 2 has source 1 unmasked (view 1 emitted nothing) and source 0 masked


def _abi_args(pkg, pairs):
    cams = (pkg.Camera * 2)()
    img = np.zeros((4, 4), np.float32)
    nrm = np.zeros((4, 4, 3), np.float32)
    keep = (img, nrm)
    fptr = (C.c_void_p * 2)(img.ctypes.data, img.ctypes.data)
    nptr = (C.c_void_p * 2)(nrm.ctypes.data, nrm.ctypes.data)
    rows, cols = (C.c_int * 2)(4, 4), (C.c_int * 2)(4, 4)
    flat = pairs[0] + pairs[1]
    offs, idx = (C.c_int * 3)(0, len(pairs[0]), len(flat)), (C.c_int * len(flat))(*flat)
    return keep, (cams, fptr, 1, fptr, nptr, None, None, rows, cols, offs, idx, 0)


def test_variant_entry_is_exported_and_refuses_bad_arguments_before_touching_a_device(pkg, tmp_path):
    """An unknown variant and a view that is its own source are refused (APD_ERR_INVALID) and nothing is written, with or without
    a device."""
    L = pkg.lib()
    assert hasattr(L, "apd_fuse_views_variant")
    L.apd_fusion_last_error.restype = C.c_char_p
    n = C.c_longlong(0)
    out = tmp_path / "x.ply"
    keep, args = _abi_args(pkg, [[1, 1], [0, 0]])
    for variant in (3, -1, 99):
        assert L.apd_fuse_views_variant(variant, 0, 2, *args, str(out).encode(), C.byref(n)) == -1
        assert not out.exists() and b"unknown variant" in L.apd_fusion_last_error()
    keep, args = _abi_args(pkg, [[1, 0], [0]])
    for variant in (1, 2):
        assert L.apd_fuse_views_variant(variant, 0, 2, *args, str(out).encode(), C.byref(n)) == -1
        assert not out.exists() and b"itself" in L.apd_fusion_last_error()
    del keep


def _entry_points(L):
    """(name, call) of apd_fuse_views and of the three variants of apd_fuse_views_variant: call(device, num_views, *args, path, n)."""
    L.apd_fusion_last_error.restype = C.c_char_p
    entries = [(b"apd_fuse_views", L.apd_fuse_views), (b"apd_fuse_views", lambda *a: L.apd_fuse_views_variant(0, *a))]
    for variant in (1, 2):
        entries.append((b"apd_fuse_views_variant", lambda *a, v=variant: L.apd_fuse_views_variant(v, *a)))
    return entries


def _refusal_cases(pkg):
    """name -> the twelve arguments between num_views and ply_path of a two-view call that one shared check refuses."""
    weak = np.zeros((4, 4), np.uint8)
    wptr = (C.c_void_p * 2)(weak.ctypes.data, weak.ctypes.data)
    keep = [weak, wptr]

    def args(pairs=([1], [0]), channels=1, size=(4, 4), **null):
        k, a = _abi_args(pkg, [list(pairs[0]), list(pairs[1])])
        keep.append((k, a))
        a = list(a)
        a[2], a[5] = channels, wptr
        a[7], a[8] = (C.c_int * 2)(size[0], 4), (C.c_int * 2)(size[1], 4)
        for name in null:
            a[("cameras", "images", "channels", "depths", "normals", "weaks", "blocks", "rows", "cols", "offsets", "indices").index(name)] = None
        return a

    cases = {"null cameras": args(cameras=None), "null depths": args(depths=None), "null rows": args(rows=None),
             "null pair indices": args(indices=None), "two channels": args(channels=2), "33 sources": args(pairs=([1] * 33, [])),
             "source index == num_views": args(pairs=([2], [0])), "negative source index": args(pairs=([1], [-1])),
             "self-source": args(pairs=([1, 0], [0])), "65536 x 65536": args(size=(65536, 65536)),
             "negative rows": args(size=(-4, 4))}
    return keep, cases, args


def test_every_fusion_entry_point_refuses_bad_arguments_before_touching_a_device(pkg, tmp_path):
    """apd_fuse_views and the three variants of apd_fuse_views_variant share one argument check: a null required pointer, two image
    channels, a view with 33 sources, a source index outside the views, a view that is its own source and a view of 65536 x 65536
    pixels (rows * cols does not fit the kernels' int pixel index) each give APD_ERR_INVALID, no file, and a message that starts
    with the entry point's name -- with or without a device.  The ETH loop needs the weak maps, the T&T loops do not."""
    L = pkg.lib()
    n = C.c_longlong(-7)
    out = tmp_path / "x.ply"
    keep, cases, args = _refusal_cases(pkg)
    for name, call in _entry_points(L):
        for what, a in cases.items():
            assert call(0, 2, *a, str(out).encode(), C.byref(n)) == -1, (name, what)
            assert L.apd_fusion_last_error().startswith(name + b": "), (name, what, L.apd_fusion_last_error())
            assert not out.exists() and n.value == -7, (name, what)
        for bad in ((2, *args(), None, C.byref(n)), (2, *args(), str(out).encode(), None), (0, *args(), str(out).encode(), C.byref(n))):
            assert call(0, *bad) == -1, (name, bad)
            assert L.apd_fusion_last_error() == name + b": null argument" and not out.exists() and n.value == -7, (name, bad)
        written, m = tmp_path / (name.decode() + "_no_weaks.ply"), C.c_longlong(-7)
        written.unlink(missing_ok=True)
        st = call(0, 2, *args(weaks=None), str(written).encode(), C.byref(m))
        if name == b"apd_fuse_views":
            assert st == -1 and L.apd_fusion_last_error() == b"apd_fuse_views: null argument" and not written.exists() and m.value == -7
        elif pkg.device_count() > 0:  # past the checks: two views of one source each fuse to a file without points
            assert st == 0 and written.exists() and m.value == 0 and L.apd_fusion_last_error() == b""
        else:  # past the checks: the first HIP call fails, APD_ERR_HIP
            assert st == -2 and not written.exists() and m.value == -7
            assert L.apd_fusion_last_error().startswith(name + b": hipSetDevice(")
    # the messages other tests and callers match on
    assert L.apd_fuse_views(0, 2, *cases["self-source"], str(out).encode(), C.byref(n)) == -1
    assert L.apd_fusion_last_error() == b"apd_fuse_views: a view lists itself as a source (use the host fusion)"
    assert L.apd_fuse_views_variant(2, 0, 2, *cases["self-source"], str(out).encode(), C.byref(n)) == -1
    assert L.apd_fusion_last_error() == b"apd_fuse_views_variant: a view lists itself as a source"
    assert L.apd_fuse_views_variant(1, 0, 2, *cases["65536 x 65536"], str(out).encode(), C.byref(n)) == -1
    assert L.apd_fusion_last_error() == b"apd_fuse_views_variant: view size out of range"
    del keep


def test_no_gpu_means_the_tat_fusions_fail_loudly(pkg, tmp_path):
    """No host fallback: without a device the T&T variants return an error and write nothing."""
    if pkg.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = pkg.lib()
    L.apd_fusion_last_error.restype = C.c_char_p
    n = C.c_longlong(0)
    out = tmp_path / "x.ply"
    keep, args = _abi_args(pkg, [[1, 1], [0, 0]])
    for variant in (1, 2):
        st = L.apd_fuse_views_variant(variant, 0, 2, *args, str(out).encode(), C.byref(n))
        assert st != 0 and not out.exists() and L.apd_fusion_last_error()
    del keep
