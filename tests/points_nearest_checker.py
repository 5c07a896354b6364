"""The sequential checker of the nearest point of another cloud and of the score (tests/helpers/points_nearest_ref.cpp): built with
the host compiler into a directory of the caller's choice and called through ctypes.  Shared by test_points_nearest.py (CPU) and
test_gpu_points_nearest.py.  Clouds are float32 [n, 3] arrays of positions."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "helpers", "points_nearest_ref.cpp")
BRUTE, GRID = 0, 1
FIELDS = ("n_p", "n_q", "p_within", "q_within", "precision", "recall", "fscore", "mean_p", "mean_q")
Score = collections.namedtuple("Score", FIELDS)


def build(out_dir):
    out = os.path.join(str(out_dir), "libpoints_nearest_ref.so")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-pthread", "-Wall", "-Wextra", SOURCE, "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(out)
    L.points_nearest.restype = None
    L.points_score.restype = None
    return L


def _args(p, q, origin):
    p, q = np.ascontiguousarray(p, np.float32).reshape(-1, 3), np.ascontiguousarray(q, np.float32).reshape(-1, 3)
    org = np.zeros(3, np.float32) if origin is None else np.ascontiguousarray(origin, np.float32)
    return p, q, org


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def nearest(L, p, q, radius, origin=None, mode=GRID):
    """(distance float32 [n_p], index int32 [n_p]) of the positions p among the positions q."""
    p, q, org = _args(p, q, origin)
    distance, index = np.zeros(len(p), np.float32), np.zeros(len(p), np.int32)
    L.points_nearest(C.c_int(mode), C.c_longlong(len(p)), _ptr(p), C.c_longlong(len(q)), _ptr(q), C.c_float(radius), _ptr(org), _ptr(distance), _ptr(index))
    return distance, index


def score(L, p, truth, threshold, origin=None, mode=GRID):
    """Score of the positions p against the positions `truth`."""
    p, q, org = _args(p, truth, origin)
    integers, reals = np.zeros(4, np.int64), np.zeros(5, np.float64)
    L.points_score(C.c_int(mode), C.c_longlong(len(p)), _ptr(p), C.c_longlong(len(q)), _ptr(q), C.c_float(threshold), _ptr(org), _ptr(integers), _ptr(reals))
    return Score(*[int(v) for v in integers], *[float(v) for v in reals])


def score_bits(s):
    """The nine fields as integers: the doubles by their bits."""
    return tuple(int(v) for v in s[:4]) + tuple(int(np.float64(v).view(np.uint64)) for v in s[4:])
