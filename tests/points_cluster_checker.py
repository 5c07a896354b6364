"""The sequential checker of the connected components within a radius and the removal of small ones
(tests/helpers/points_cluster_ref.cpp): built with the host compiler into a directory of the caller's choice and called through
ctypes.  Shared by test_points_clusters.py (CPU) and test_gpu_points_clusters.py.  Clouds are points_voxel_checker.Cloud objects."""
import ctypes as C
import os
import subprocess

import numpy as np

from points_voxel_checker import DTYPES, WIDTHS, Cloud

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "helpers", "points_cluster_ref.cpp")
BRUTE, GRID = 0, 1


def build(out_dir):
    out = os.path.join(str(out_dir), "libpoints_cluster_ref.so")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wextra", SOURCE, "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(out)
    L.points_clusters.restype = C.c_longlong
    return L


def run(L, cloud, radius, min_size=0, origin=None, mode=GRID):
    """(label uint32 [n], size uint32 [n], the number of components, kept: a Cloud of the points whose component has at least
    `min_size` points, with `removed` and `index`, the input indices of its points)."""
    n = cloud.count
    org = np.zeros(3, np.float32) if origin is None else np.ascontiguousarray(origin, np.float32)
    out = [np.zeros((n, w) if w > 1 else (n,), t) for t, w in zip(DTYPES, WIDTHS)]
    label, size, index = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.int64)
    offsets, views = np.zeros(n + 1, np.int64), np.zeros(max(len(cloud.views), 1), np.int32)
    removed, components = C.c_longlong(-1), C.c_longlong(-1)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    kept = L.points_clusters(C.c_int(mode), C.c_longlong(n), ptr(cloud.xyz), ptr(cloud.normal), ptr(cloud.bgr), ptr(cloud.support), ptr(cloud.view),
                             ptr(cloud.pixel), ptr(cloud.sources), ptr(cloud.offsets), ptr(cloud.views), C.c_float(radius), ptr(org),
                             C.c_uint32(min_size), ptr(label), ptr(size), C.byref(components), ptr(index), *[ptr(a) for a in out], ptr(offsets),
                             ptr(views), C.byref(removed))
    res = Cloud(*[a[:kept] for a in out], offsets[:kept + 1], views[:offsets[kept]])
    res.removed = int(removed.value)
    res.index = index[:kept]
    return label, size, int(components.value), res


def components(L, cloud, radius, origin=None, mode=GRID):
    """(label, size, the number of components)"""
    return run(L, cloud, radius, 0, origin, mode)[:3]


def remove(L, cloud, radius, min_size, origin=None, mode=GRID):
    return run(L, cloud, radius, min_size, origin, mode)[3]
