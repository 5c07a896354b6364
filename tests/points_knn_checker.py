"""The sequential checker of the k-nearest mean distances and the statistical removal (tests/helpers/points_knn_ref.cpp): built with
the host compiler into a directory of the caller's choice and called through ctypes.  Shared by test_points_knn.py (CPU) and
test_gpu_points_knn.py.  Clouds are points_voxel_checker.Cloud objects."""
import ctypes as C
import os
import subprocess

import numpy as np

from points_voxel_checker import DTYPES, WIDTHS, Cloud

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "helpers", "points_knn_ref.cpp")
BRUTE, GRID = 0, 1


def build(out_dir):
    out = os.path.join(str(out_dir), "libpoints_knn_ref.so")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-pthread", "-Wall", "-Wextra", SOURCE, "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(out)
    L.points_knn.restype = C.c_longlong
    L.knn_threshold_of.restype = C.c_double
    return L


def run(L, cloud, radius, k, std_ratio=0.0, origin=None, mode=GRID):
    """(scores float32 [n], kept: a Cloud of the points kept at `std_ratio`, with `removed`, `threshold` and `index`, the input
    indices of its points)."""
    n = cloud.count
    org = np.zeros(3, np.float32) if origin is None else np.ascontiguousarray(origin, np.float32)
    out = [np.zeros((n, w) if w > 1 else (n,), t) for t, w in zip(DTYPES, WIDTHS)]
    scores, index = np.zeros(n, np.float32), np.zeros(n, np.int64)
    offsets, views = np.zeros(n + 1, np.int64), np.zeros(max(len(cloud.views), 1), np.int32)
    removed, threshold = C.c_longlong(-1), C.c_double(-1.0)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    kept = L.points_knn(C.c_int(mode), C.c_longlong(n), ptr(cloud.xyz), ptr(cloud.normal), ptr(cloud.bgr), ptr(cloud.support), ptr(cloud.view),
                        ptr(cloud.pixel), ptr(cloud.sources), ptr(cloud.offsets), ptr(cloud.views), C.c_float(radius), ptr(org), C.c_uint32(k),
                        C.c_float(std_ratio), ptr(scores), C.byref(threshold), ptr(index), *[ptr(a) for a in out], ptr(offsets), ptr(views),
                        C.byref(removed))
    res = Cloud(*[a[:kept] for a in out], offsets[:kept + 1], views[:offsets[kept]])
    res.removed = int(removed.value)
    res.threshold = float(threshold.value)
    res.index = index[:kept]
    return scores, res


def scores(L, cloud, radius, k, origin=None, mode=GRID):
    return run(L, cloud, radius, k, 0.0, origin, mode)[0]


def remove(L, cloud, radius, k, std_ratio, origin=None, mode=GRID):
    return run(L, cloud, radius, k, std_ratio, origin, mode)[1]


def threshold(L, values, std_ratio):
    """(T, n_f, S1, S2) of contract C12 for the scores `values` in input order."""
    v = np.ascontiguousarray(values, np.float32)
    full, s1, s2 = C.c_longlong(-1), C.c_double(-1.0), C.c_double(-1.0)
    T = L.knn_threshold_of(C.c_longlong(len(v)), C.c_void_p(v.ctypes.data), C.c_float(std_ratio), C.byref(full), C.byref(s1), C.byref(s2))
    return float(T), int(full.value), float(s1.value), float(s2.value)
