"""The sequential checker of the voxel-grid merge (tests/helpers/points_voxel_ref.cpp): built with the host compiler into a directory
of the caller's choice and called through ctypes.  Shared by test_points_voxel.py (CPU) and test_gpu_points_voxel.py."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "helpers", "points_voxel_ref.cpp")
FIELDS = ("xyz", "normal", "bgr", "support", "view", "pixel", "sources")
DTYPES = (np.float32, np.float32, np.uint8, np.uint8, np.int32, np.int32, np.uint32)
WIDTHS = (3, 3, 3, 1, 1, 1, 1)


class Cloud:
    """The seven arrays of a cloud and its visibility lists (offsets int64 [count + 1], views int32); `dropped` on a merge's result."""

    def __init__(self, xyz, normal, bgr, support, view, pixel, sources, offsets, views):
        given = (xyz, normal, bgr, support, view, pixel, sources)
        self.count = len(np.asarray(view))
        for f, a, t, w in zip(FIELDS, given, DTYPES, WIDTHS):
            a = np.asarray(a)
            a = a.view(np.uint32) if f == "sources" and a.dtype == np.int32 else a
            setattr(self, f, np.ascontiguousarray(a, t).reshape((self.count, w) if w > 1 else (self.count,)))
        self.offsets = np.ascontiguousarray(offsets, np.int64)
        self.views = np.ascontiguousarray(views, np.int32)
        assert len(self.offsets) == self.count + 1 and self.offsets[-1] == len(self.views)


def source_lists(view, sources, pairs):
    """The lists of apd_points_visibility for points of a fusion: the point's own view, then its agreeing sources in bit order."""
    offsets, views = [0], []
    for v, m in zip(np.asarray(view).tolist(), (np.asarray(sources).astype(np.int64) & 0xFFFFFFFF).tolist()):
        views.append(v)
        views += [pairs[v][j] for j in range(32) if (m >> j) & 1]
        offsets.append(len(views))
    return np.array(offsets, np.int64), np.array(views, np.int32)


def build(out_dir):
    out = os.path.join(str(out_dir), "libpoints_voxel_ref.so")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wextra", SOURCE, "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(out)
    L.points_voxel.restype = C.c_longlong
    return L


def merge(L, cloud, size, origin=None):
    """The merge of `cloud` (a Cloud) on the grid of cell size `size` at `origin`: a Cloud with `dropped`."""
    n = cloud.count
    org = np.zeros(3, np.float32) if origin is None else np.ascontiguousarray(origin, np.float32)
    out = [np.zeros((n, w) if w > 1 else (n,), t) for t, w in zip(DTYPES, WIDTHS)]
    offsets, views = np.zeros(n + 1, np.int64), np.zeros(max(len(cloud.views), 1), np.int32)
    dropped = C.c_longlong(-1)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    cells = L.points_voxel(C.c_longlong(n), ptr(cloud.xyz), ptr(cloud.normal), ptr(cloud.bgr), ptr(cloud.view), ptr(cloud.pixel), ptr(cloud.sources),
                           ptr(cloud.offsets), ptr(cloud.views), C.c_float(size), ptr(org), *[ptr(a) for a in out], ptr(offsets), ptr(views),
                           C.byref(dropped))
    res = Cloud(*[a[:cells] for a in out], offsets[:cells + 1], views[:offsets[cells]])
    res.dropped = int(dropped.value)
    return res


def assert_equal(got, want, what=""):
    """Every array and the lists, bit for bit."""
    assert got.count == want.count, (what, "count", got.count, want.count)
    for f in FIELDS + ("offsets", "views"):
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, f, a.dtype, b.dtype, a.shape, b.shape)
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        assert np.array_equal(a, b), (what, f)
