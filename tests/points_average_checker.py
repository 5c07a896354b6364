"""The sequential checker of the mean geometry (tests/helpers/points_average_ref.cpp): built with the host compiler into a directory
of the caller's choice and called through ctypes.  Shared by test_points_average.py (CPU) and test_gpu_points_average.py.
build_header() builds the product's own arithmetic (apd_fusion::mean_point, tests/helpers/points_average_header.cpp) the same way,
for the CPU comparison of the two."""
import ctypes as C
import os
import subprocess

import numpy as np

from eth_fusion_checker import MATH_DIR

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "helpers", "points_average_ref.cpp")
HEADER_SOURCE = os.path.join(HERE, "helpers", "points_average_header.cpp")
FIELDS = ("xyz", "normal", "bgr", "support", "view", "pixel", "sources")


class Result:
    """xyz / normal / bgr / support / view / pixel / sources of every averaged point; with contributions=True also `contributions` and
    `normal_contributions`, float32 [count, 32, 3]: the lifted point and the normal of source j of point k (zeros where bit j of
    sources[k] is clear)."""


def _compile(source, out):
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wextra", "-I" + MATH_DIR,
           source, "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return C.CDLL(out)


def build(out_dir):
    L = _compile(SOURCE, os.path.join(str(out_dir), "libpoints_average_ref.so"))
    L.points_average.restype = None
    return L


def build_header(out_dir):
    L = _compile(HEADER_SOURCE, os.path.join(str(out_dir), "libpoints_average_header.so"))
    L.points_average_header.restype = None
    return L


def average(L, cameras, depths, normals, pairs, points, contributions=False, header=False):
    """The means of `points` (anything with the arrays FIELDS: a vis_checker.Result, a Points of host memory) over the maps.
    header: L is build_header()'s and the product's own function runs.  Returns a Result."""
    V = len(depths)
    keep = [np.ascontiguousarray(a, np.float32) for a in list(depths) + list(normals)]
    dptr = (C.c_void_p * V)(*[a.ctypes.data for a in keep[:V]])
    nptr = (C.c_void_p * V)(*[a.ctypes.data for a in keep[V:]])
    rows = (C.c_int * V)(*[d.shape[0] for d in depths])
    cols = (C.c_int * V)(*[d.shape[1] for d in depths])
    flat = [s for p in pairs for s in p]
    offs = (C.c_int * (V + 1))(*np.cumsum([0] + [len(p) for p in pairs]).tolist())
    idx = (C.c_int * max(len(flat), 1))(*flat)
    n = len(points.view)
    src = [np.ascontiguousarray(points.xyz, np.float32), np.ascontiguousarray(points.normal, np.float32),
           np.ascontiguousarray(points.view, np.int32), np.ascontiguousarray(np.asarray(points.sources).view(np.uint32))]
    res = Result()
    res.count = n
    res.xyz, res.normal = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
    res.sources, res.support = np.empty(n, np.uint32), np.empty(n, np.uint8)
    res.bgr, res.view, res.pixel = np.array(points.bgr, np.uint8), np.array(points.view, np.int32), np.array(points.pixel, np.int32)
    args = [V, C.byref(cameras), dptr, nptr, rows, cols, offs, idx, C.c_longlong(n)] + \
        [C.c_void_p(a.ctypes.data) for a in src + [res.xyz, res.normal, res.sources, res.support]]
    if header:
        assert not contributions
        L.points_average_header(*args)
        return res
    res.contributions = np.zeros((n, 32, 3), np.float32) if contributions else None
    res.normal_contributions = np.zeros((n, 32, 3), np.float32) if contributions else None
    L.points_average(*(args + [C.c_void_p(a.ctypes.data) if contributions else None for a in (res.contributions, res.normal_contributions)]))
    return res


def average_case(L, ob, case, points, depths=None, **kw):
    """average() on a case of tests/fusion_cases.py; depths: other depth maps than the case's."""
    return average(L, case.cameras(ob.make_camera), case.depths if depths is None else depths, case.normals, case.pairs, points, **kw)
