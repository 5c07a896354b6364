"""The sequential checker of the FPFH descriptors, their matches and the registration to another cloud
(tests/helpers/points_register_ref.cpp): built with the host compiler into a directory of the caller's choice and called through
ctypes.  Shared by test_points_register.py (CPU) and test_gpu_points_register.py.  Clouds are float32 [n, 3] arrays of positions
and of normals."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "helpers", "points_register_ref.cpp")
BRUTE, GRID = 0, 1
OK, TOO_FEW_MATCHES, NO_TRIAL = 0, 1, 2
WIDTH = 33
FIELDS = ("scale", "rotation", "translation", "features_p", "features_q", "matches", "trials_admitted", "best_trial", "inliers", "inliers_after",
          "rms_after", "stopped")
Registration = collections.namedtuple("Registration", FIELDS)
DEFAULTS = dict(trials=4096, seed=0, edge_ratio=0.9, min_neighbours=5, mutual=True, with_scale=False)     # inlier_distance: radius / 2


class _Options(C.Structure):
    _fields_ = [("trials", C.c_uint), ("seed", C.c_ulonglong), ("inlier_distance", C.c_float), ("edge_ratio", C.c_float), ("min_neighbours", C.c_uint),
                ("mutual", C.c_int), ("with_scale", C.c_int)]


class _Registration(C.Structure):
    _fields_ = [("scale", C.c_double), ("rotation", C.c_double * 9), ("translation", C.c_double * 3)] + \
               [(n, C.c_longlong) for n in FIELDS[3:10]] + [("rms_after", C.c_double), ("stopped", C.c_int)]


def build(out_dir):
    out = os.path.join(str(out_dir), "libpoints_register_ref.so")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wextra", SOURCE, "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(out)
    for name in ("points_features", "points_match_features", "points_register", "points_register_matches", "points_register_three"):
        getattr(L, name).restype = None
    L.points_register_theta_bin.restype = C.c_int
    L.points_register_theta_bin.argtypes = [C.c_double, C.c_double]
    L.points_register_linear_bin.restype = C.c_int
    L.points_register_linear_bin.argtypes = [C.c_double]
    L.points_register_draw.restype = C.c_uint
    L.points_register_draw.argtypes = [C.c_ulonglong, C.c_uint, C.c_uint, C.c_uint]
    L.points_register_pair.restype = C.c_int
    return L


def _cloud(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1, 3)


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def _origin(origin):
    return np.zeros(3, np.float32) if origin is None else np.ascontiguousarray(origin, np.float32)


def options(radius, inlier_distance=None, **kw):
    o = dict(DEFAULTS, **kw)
    distance = float(np.float32(radius) * np.float32(0.5)) if inlier_distance is None else inlier_distance
    return _Options(int(o["trials"]), int(o["seed"]), float(distance), float(o["edge_ratio"]), int(o["min_neighbours"]), int(bool(o["mutual"])),
                    int(bool(o["with_scale"])))


def features(L, xyz, normal, radius, origin=None, min_neighbours=5, mode=GRID):
    """(features float32 [n, 33], has uint8 [n])."""
    xyz, normal = _cloud(xyz), _cloud(normal)
    out, has = np.zeros((len(xyz), WIDTH), np.float32), np.zeros(len(xyz), np.uint8)
    L.points_features(C.c_int(mode), C.c_longlong(len(xyz)), _ptr(xyz), _ptr(normal), C.c_float(radius), _ptr(_origin(origin)), C.c_uint(min_neighbours),
                      _ptr(out), _ptr(has))
    return out, has


def match_features(L, p, p_normal, q, q_normal, radius, origin=None, min_neighbours=5, mutual=True, mode=GRID):
    """(index int32 [n_p], distance float32 [n_p])."""
    p, p_normal, q, q_normal = _cloud(p), _cloud(p_normal), _cloud(q), _cloud(q_normal)
    index, distance = np.zeros(len(p), np.int32), np.zeros(len(p), np.float32)
    L.points_match_features(C.c_int(mode), C.c_longlong(len(p)), _ptr(p), _ptr(p_normal), C.c_longlong(len(q)), _ptr(q), _ptr(q_normal), C.c_float(radius),
                            _ptr(_origin(origin)), C.c_uint(min_neighbours), C.c_int(int(bool(mutual))), _ptr(index), _ptr(distance))
    return index, distance


def _registration(out):
    return Registration(out.scale, tuple(out.rotation), tuple(out.translation), *[getattr(out, n) for n in FIELDS[3:]])


def register(L, p, p_normal, q, q_normal, radius, origin=None, inlier_distance=None, mode=GRID, **kw):
    p, p_normal, q, q_normal = _cloud(p), _cloud(p_normal), _cloud(q), _cloud(q_normal)
    o, out = options(radius, inlier_distance, **kw), _Registration()
    L.points_register(C.c_int(mode), C.c_longlong(len(p)), _ptr(p), _ptr(p_normal), C.c_longlong(len(q)), _ptr(q), _ptr(q_normal), C.c_float(radius),
                      _ptr(_origin(origin)), C.byref(o), C.byref(out))
    return _registration(out)


def register_matches(L, p, q, pairs, inlier_distance, **kw):
    """The trials, the best one and the refit over given matches: pairs int [M, 2] of (index in p ascending, index in q)."""
    p, q = _cloud(p), _cloud(q)
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    start, to = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
    o, out = options(1.0, inlier_distance, **kw), _Registration()
    L.points_register_matches(C.c_longlong(len(p)), _ptr(p), _ptr(q), C.c_longlong(len(pairs)), _ptr(start), _ptr(to), C.byref(o), C.byref(out))
    return _registration(out)


def three(L, seed, t, M):
    at = (C.c_uint * 3)()
    L.points_register_three(C.c_ulonglong(seed), C.c_uint(t), C.c_uint(M), at)
    return tuple(at)


def pair(L, c, nc, q, nq):
    """(admitted: 1, 0, or -1 without a frame; d2; [alpha bin, phi bin, theta bin])."""
    a = [np.ascontiguousarray(v, np.float32) for v in (c, nc, q, nq)]
    d2, bins = C.c_double(0.0), (C.c_int * 3)()
    rc = L.points_register_pair(_ptr(a[0]), _ptr(a[1]), _ptr(a[2]), _ptr(a[3]), C.byref(d2), bins)
    return rc, d2.value, list(bins)


def bits(r):
    """The fields of a Registration (the checker's or Points.register's) as integers: the doubles by their bits."""
    def d(v):
        return int(np.float64(v).view(np.uint64))
    return ((d(r.scale),) + tuple(d(v) for v in np.asarray(r.rotation, np.float64).reshape(9)) + tuple(d(v) for v in np.asarray(r.translation, np.float64).reshape(3))
            + tuple(int(getattr(r, n)) for n in FIELDS[3:10]) + (d(r.rms_after), int(r.stopped)))
