"""The sequential checker of the fusions' visibility (tests/helpers/fusion_vis_ref.cpp): the three loops with the agreeing sources
of every point kept.  Built with the host compiler into a directory of the caller's choice and called through ctypes.  Shared
by test_fusion_visibility.py (CPU) and test_gpu_fusion_visibility.py."""
import ctypes as C
import os
import subprocess

import numpy as np

import fusion_cases as fc
from eth_fusion_checker import DEFAULTS, MATH_DIR, Rule

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "helpers", "fusion_vis_ref.cpp")
VARIANTS = {"eth": 0, "tat_intermediate": 1, "tat_advanced": 2}


class Result:
    """count; xyz / normal / bgr / support / view / pixel / sources of every point; offsets int64 [count + 1] and views int32: point
    k is seen by views[offsets[k]:offsets[k + 1]]."""


def build(out_dir):
    out = os.path.join(str(out_dir), "libfusion_vis_ref.so")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wextra", "-I" + MATH_DIR,
           SOURCE, "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(out)
    L.vis_fuse.restype = C.c_longlong
    L.vis_entries.restype = C.c_longlong
    L.vis_points.restype = None
    L.vis_lists.restype = None
    return L


def fuse(L, variant, cameras, images, depths, normals, weaks, pairs, ply_path=None, blocks=None, ply_normals=False, vis_path=None, **rule):
    """variant "eth" / "tat_intermediate" / "tat_advanced"; the other arguments as eth_fusion_checker.fuse (**rule: the values of
    its DEFAULTS to replace, ETH only).  Writes ply_path and vis_path if given.  Returns a Result."""
    V = len(images)
    keep = []

    def ptrs(arrs, dt):
        out = (C.c_void_p * V)()
        for i, a in enumerate(arrs):
            if a is None:
                continue
            a = np.ascontiguousarray(a, dt)
            keep.append(a)
            out[i] = a.ctypes.data
        return out

    unknown = set(rule) - set(DEFAULTS)
    assert not unknown, unknown
    assert variant == "eth" or not rule, "the T&T loops keep their own thresholds"
    values = Rule(**dict(DEFAULTS, **rule))
    rows = (C.c_int * V)(*[d.shape[0] for d in depths])
    cols = (C.c_int * V)(*[d.shape[1] for d in depths])
    flat = [s for p in pairs for s in p]
    offs = (C.c_int * (V + 1))(*np.cumsum([0] + [len(p) for p in pairs]).tolist())
    idx = (C.c_int * max(len(flat), 1))(*flat)
    channels = 3 if np.asarray(images[0]).ndim == 3 else 1
    n = L.vis_fuse(VARIANTS[variant], C.byref(values), V, C.byref(cameras), ptrs(images, np.float32), channels, ptrs(depths, np.float32),
                   ptrs(normals, np.float32), ptrs(weaks, np.uint8), None if blocks is None else ptrs(blocks, np.uint8), rows, cols, offs,
                   idx, None if ply_path is None else str(ply_path).encode(), int(bool(ply_normals)))
    if n < 0:
        raise IOError("cannot write " + str(ply_path))
    res = Result()
    res.count = int(n)
    res.xyz, res.normal = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
    res.bgr, res.support = np.empty((n, 3), np.uint8), np.empty(n, np.uint8)
    res.view, res.pixel, res.sources = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.uint32)
    L.vis_points(*[C.c_void_p(a.ctypes.data) for a in (res.xyz, res.normal, res.bgr, res.support, res.view, res.pixel, res.sources)])
    res.offsets, res.views = np.empty(n + 1, np.int64), np.empty(L.vis_entries(), np.int32)
    L.vis_lists(C.c_void_p(res.offsets.ctypes.data), C.c_void_p(res.views.ctypes.data))
    if vis_path is not None and L.vis_write(str(vis_path).encode()) != 0:
        raise IOError("cannot write " + str(vis_path))
    return res


def fuse_case(L, ob, variant, case, ply_path=None, **kw):
    """fuse() on a case of tests/fusion_cases.py."""
    return fuse(L, variant, case.cameras(ob.make_camera), case.images, case.depths, case.normals, case.weaks, case.pairs, ply_path,
                blocks=case.blocks, **kw)


def vis_bytes(offsets, views):
    """The bytes of a fused.ply.vis with these lists, written with numpy alone."""
    n = len(offsets) - 1
    words = np.empty(n + len(views), "<u4")
    heads = np.asarray(offsets[:-1], np.int64) + np.arange(n)
    body = np.ones(len(words), bool)
    body[heads] = False
    words[heads] = np.diff(offsets)
    words[body] = views
    return np.array([n], "<u8").tobytes() + words.tobytes()


# --------------------------------------------------------------------------------------------------------------------
# cases of this feature, derived from tests/fusion_cases.py (which stays as it is)
# --------------------------------------------------------------------------------------------------------------------

def _copy(case, name):
    c = fc.Case(name, case.views, [a.copy() for a in case.images], [a.copy() for a in case.depths], [a.copy() for a in case.normals],
                [a.copy() for a in case.weaks], case.pairs, blocks=None if case.blocks is None else [None if b is None else b.copy() for b in case.blocks],
                tags=case.declared)
    return c


def first_pixels(case, name, pixels_of_view):
    """`case` with block masks that leave view v only its first pixels_of_view[v] pixels in raster order as reference pixels (None:
    the view as it is).  The blocked pixels still serve as sources, and no loop lets a pixel depend on a later one of its view, so
    the points of the kept pixels are the ones they were."""
    c = _copy(case, name)
    c.blocks = []
    for d, keep in zip(c.depths, pixels_of_view):
        if keep is None:
            c.blocks.append(None)
            continue
        b = np.zeros(d.shape, np.uint8)
        b.reshape(-1)[:keep] = 255
        c.blocks.append(b)
    c.retag()
    return c


def last_source_case():
    """The many-sources case with the most sources a mask has room for short of APD_MAX_IMAGES: sources_31 (view 0 lists 31 sources;
    only those at positions 30 and 5 agree with it), so every point of view 0 has bit 30 set."""
    return fc.case("sources_31")


# Scan edges.  The device builds the offsets with one workgroup of 1024 lanes over the sums of blocks of 256 points: up to
# SCAN_SPAN points every lane has at most one block, above it a lane runs over several.
SCAN_SPAN = 1024 * 256


# counts below a wave, on both sides of a wave (64) and of a block (256), and on both sides of SCAN_SPAN
SCAN_EDGES = {"below_wave": 40, "wave_minus": 63, "wave": 64, "wave_plus": 65, "block_minus": 255, "block": 256, "block_plus": 257,
              "span": SCAN_SPAN, "span_plus": SCAN_SPAN + 1}


def scan_edge_case(label):
    """(case, points): the plane scene of fusion_cases.tiny(), where every pixel of view 0 is a point of the ETH loop, with view 0
    cut to its first `points` pixels and the other views blocked entirely, so the fusion has exactly that many points (the tests
    assert it against the checker).  40 x 30 for the small counts, 600 x 450 for those around SCAN_SPAN."""
    points = SCAN_EDGES[label]
    W, H = (40, 30) if points <= 1200 else (600, 450)
    return first_pixels(fc.tiny(24, W, H), "scan_" + label, [points, 0, 0, 0]), points
