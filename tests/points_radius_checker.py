"""The sequential checker of the neighbour counts and the removal of sparse points (tests/helpers/points_radius_ref.cpp): built with
the host compiler into a directory of the caller's choice and called through ctypes.  Shared by test_points_radius.py (CPU) and
test_gpu_points_radius.py.  Clouds are points_voxel_checker.Cloud objects."""
import ctypes as C
import os
import subprocess

import numpy as np

from points_voxel_checker import DTYPES, WIDTHS, Cloud

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "helpers", "points_radius_ref.cpp")
BRUTE, GRID = 0, 1


def build(out_dir):
    out = os.path.join(str(out_dir), "libpoints_radius_ref.so")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wextra", SOURCE, "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(out)
    L.points_radius.restype = C.c_longlong
    return L


def run(L, cloud, radius, cap=0, min_neighbours=0, origin=None, mode=GRID):
    """(counts uint32 [n] with `cap`, kept: a Cloud of the points with at least `min_neighbours` neighbours, with `removed` and
    `index`, the input indices of its points)."""
    n = cloud.count
    org = np.zeros(3, np.float32) if origin is None else np.ascontiguousarray(origin, np.float32)
    out = [np.zeros((n, w) if w > 1 else (n,), t) for t, w in zip(DTYPES, WIDTHS)]
    counts, index = np.zeros(n, np.uint32), np.zeros(n, np.int64)
    offsets, views = np.zeros(n + 1, np.int64), np.zeros(max(len(cloud.views), 1), np.int32)
    removed = C.c_longlong(-1)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    kept = L.points_radius(C.c_int(mode), C.c_longlong(n), ptr(cloud.xyz), ptr(cloud.normal), ptr(cloud.bgr), ptr(cloud.support), ptr(cloud.view),
                           ptr(cloud.pixel), ptr(cloud.sources), ptr(cloud.offsets), ptr(cloud.views), C.c_float(radius), ptr(org), C.c_uint32(cap),
                           C.c_uint32(min_neighbours), ptr(counts), ptr(index), *[ptr(a) for a in out], ptr(offsets), ptr(views), C.byref(removed))
    res = Cloud(*[a[:kept] for a in out], offsets[:kept + 1], views[:offsets[kept]])
    res.removed = int(removed.value)
    res.index = index[:kept]
    return counts, res


def counts(L, cloud, radius, cap=0, origin=None, mode=GRID):
    return run(L, cloud, radius, cap, 0, origin, mode)[0]


def remove(L, cloud, radius, min_neighbours, origin=None, mode=GRID):
    return run(L, cloud, radius, 0, min_neighbours, origin, mode)[1]
