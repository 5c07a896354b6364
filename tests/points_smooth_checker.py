"""The sequential checker of the smoothed positions (tests/helpers/points_smooth_ref.cpp): built with the host compiler into a
directory of the caller's choice and called through ctypes.  Shared by test_points_smooth.py (CPU) and test_gpu_points_smooth.py.
Clouds are points_voxel_checker.Cloud objects."""
import ctypes as C
import os
import subprocess

import numpy as np

from points_voxel_checker import FIELDS, Cloud

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "helpers", "points_smooth_ref.cpp")
BRUTE, GRID = 0, 1


def build(out_dir):
    out = os.path.join(str(out_dir), "libpoints_smooth_ref.so")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-pthread", "-Wall", "-Wextra", SOURCE, "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(out)
    L.points_smooth.restype = C.c_longlong
    L.points_smooth_max_iterations.restype = C.c_uint
    return L


class Result:
    """xyz float32 [n, 3]: the positions after the last iteration; offset float32 [n], normal float32 [n, 3] (the weighted plane's; the
    stored one where there is no estimate), sweeps uint32 [n], estimated and capped bool [n]: those of the last iteration; ever bool [n]: estimated in at least one iteration; moved: their number."""


def run(L, cloud, radius, min_neighbours, iterations=1, origin=None, mode=GRID):
    n = cloud.count
    org = np.zeros(3, np.float32) if origin is None else np.ascontiguousarray(origin, np.float32)
    res = Result()
    res.xyz, res.offset, res.normal = np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros((n, 3), np.float32)
    res.sweeps, estimated, capped, ever = np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    res.moved = int(L.points_smooth(C.c_int(mode), C.c_longlong(n), ptr(cloud.xyz), ptr(cloud.normal), C.c_float(radius), ptr(org),
                                    C.c_uint32(min_neighbours), C.c_uint32(iterations), ptr(res.xyz), ptr(res.offset), ptr(res.normal), ptr(res.sweeps),
                                    ptr(estimated), ptr(capped), ptr(ever)))
    res.estimated, res.capped, res.ever = estimated.astype(bool), capped.astype(bool), ever.astype(bool)
    return res


def with_positions(cloud, res):
    """`cloud` with the checker's positions in place of its own: what apd_points_with_smoothed_positions gives."""
    return Cloud(*[res.xyz if f == "xyz" else getattr(cloud, f) for f in FIELDS], cloud.offsets, cloud.views)


def max_iterations(L):
    return int(L.points_smooth_max_iterations())
