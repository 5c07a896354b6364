"""The sequential checker of the rendered maps and the rendered visibility (tests/helpers/points_render_ref.cpp): built with the host
compiler into a directory of the caller's choice and called through ctypes.  Shared by test_points_render.py (CPU) and
test_gpu_points_render.py.  Clouds are points_voxel_checker.Cloud objects or plain xyz arrays; cameras are the package's Camera
structures (K, R, t, width, height are read)."""
import ctypes as C
import os
import subprocess

import numpy as np

from points_voxel_checker import FIELDS, Cloud

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "helpers", "points_render_ref.cpp")
NO_INDEX = 0xFFFFFFFF


def build(out_dir):
    out = os.path.join(str(out_dir), "libpoints_render_ref.so")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wextra", SOURCE, "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(out)
    L.points_render.restype = None
    L.points_rendered_visibility.restype = C.c_longlong
    return L


def camera_floats(cam):
    """K, R, t of a Camera as the 21 floats the checker reads."""
    return np.array(list(cam.K) + list(cam.R) + list(cam.t), np.float32)


def _xyz(cloud):
    return np.ascontiguousarray(cloud.xyz if hasattr(cloud, "xyz") else cloud, np.float32).reshape(-1, 3)


def render(L, cloud, cam, splat):
    """(depth float32 [height, width], index uint32 [height, width]) of the cloud drawn into `cam`."""
    xyz = _xyz(cloud)
    W, H = int(cam.width), int(cam.height)
    depth, index = np.zeros((H, W), np.float32), np.zeros((H, W), np.uint32)
    k = camera_floats(cam)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    L.points_render(C.c_longlong(len(xyz)), ptr(xyz), ptr(k), C.c_int(W), C.c_int(H), C.c_int(splat), ptr(depth), ptr(index))
    return depth, index


class Lists:
    """offsets int64 [n + 1], views int32, support uint8 [n], unseen: the points with an empty list."""


def visibility(L, cloud, cams, splat, rel_tolerance):
    xyz = _xyz(cloud)
    n, V = len(xyz), len(cams)
    ks = np.concatenate([camera_floats(c) for c in cams])
    sizes = np.array([[int(c.width), int(c.height)] for c in cams], np.int32)
    res = Lists()
    res.offsets, views, res.support = np.zeros(n + 1, np.int64), np.zeros(max(n * V, 1), np.int32), np.zeros(n, np.uint8)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    res.unseen = int(L.points_rendered_visibility(C.c_longlong(n), ptr(xyz), C.c_int(V), ptr(ks), ptr(sizes), C.c_int(splat), C.c_float(rel_tolerance),
                                                  ptr(res.offsets), ptr(views), ptr(res.support)))
    res.views = views[:res.offsets[n]].copy()
    return res


def with_lists(cloud, res):
    """`cloud` with the checker's lists and support in place of its own: what apd_points_rendered_visibility gives."""
    return Cloud(*[res.support if f == "support" else getattr(cloud, f) for f in FIELDS], res.offsets, res.views)
