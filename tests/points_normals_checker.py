"""The sequential checker of the estimated normals (tests/helpers/points_normals_ref.cpp): built with the host compiler into a
directory of the caller's choice and called through ctypes.  Shared by test_points_normals.py (CPU) and test_gpu_points_normals.py.
Clouds are points_voxel_checker.Cloud objects."""
import ctypes as C
import os
import subprocess

import numpy as np

from points_voxel_checker import FIELDS, Cloud

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "helpers", "points_normals_ref.cpp")
BRUTE, GRID = 0, 1


def build(out_dir):
    out = os.path.join(str(out_dir), "libpoints_normals_ref.so")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-pthread", "-Wall", "-Wextra", SOURCE, "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(out)
    L.points_normals.restype = C.c_longlong
    L.points_normals_sweep_cap.restype = C.c_uint
    return L


class Result:
    """normal float32 [n, 3], variation float32 [n], sweeps uint32 [n], estimated and capped bool [n], count: the points with an
    estimate."""


def run(L, cloud, radius, min_neighbours, origin=None, mode=GRID):
    n = cloud.count
    org = np.zeros(3, np.float32) if origin is None else np.ascontiguousarray(origin, np.float32)
    res = Result()
    res.normal, res.variation = np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
    res.sweeps, estimated, capped = np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    res.count = int(L.points_normals(C.c_int(mode), C.c_longlong(n), ptr(cloud.xyz), ptr(cloud.normal), C.c_float(radius), ptr(org),
                                     C.c_uint32(min_neighbours), ptr(res.normal), ptr(res.variation), ptr(res.sweeps), ptr(estimated), ptr(capped)))
    res.estimated, res.capped = estimated.astype(bool), capped.astype(bool)
    return res


def with_normals(cloud, res):
    """`cloud` with the checker's normals in place of its own: what apd_points_with_estimated_normals gives."""
    return Cloud(*[res.normal if f == "normal" else getattr(cloud, f) for f in FIELDS], cloud.offsets, cloud.views)


def sweep_cap(L):
    return int(L.points_normals_sweep_cap())
