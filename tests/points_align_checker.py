"""The sequential checker of the alignment to another cloud and of the move by a transform (tests/helpers/points_align_ref.cpp):
built with the host compiler into a directory of the caller's choice and called through ctypes.  Shared by test_points_align.py
(CPU) and test_gpu_points_align.py.  Clouds are float32 [n, 3] arrays of positions."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "helpers", "points_align_ref.cpp")
BRUTE, GRID = 0, 1
ITERATIONS, CONVERGED, TOO_FEW = 0, 1, 2
FIELDS = ("scale", "rotation", "translation", "matched_before", "matched_after", "rms_before", "rms_after", "steps", "stopped")
Alignment = collections.namedtuple("Alignment", FIELDS)


class _Alignment(C.Structure):
    _fields_ = [("scale", C.c_double), ("rotation", C.c_double * 9), ("translation", C.c_double * 3), ("matched_before", C.c_longlong),
                ("matched_after", C.c_longlong), ("rms_before", C.c_double), ("rms_after", C.c_double), ("steps", C.c_int), ("stopped", C.c_int)]


def build(out_dir):
    out = os.path.join(str(out_dir), "libpoints_align_ref.so")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-pthread", "-Wall", "-Wextra", SOURCE, "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(out)
    L.points_align.restype = C.c_int
    L.points_align_solve_pairs.restype = None
    L.points_transformed.restype = None
    return L


def _cloud(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1, 3)


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def align(L, p, q, radius, origin=None, iterations=16, tolerance=1e-6, with_scale=False, mode=GRID, trace=False):
    """Alignment of the positions p onto the positions q; trace: (Alignment, [rms_k of every search])."""
    p, q = _cloud(p), _cloud(q)
    org = np.zeros(3, np.float32) if origin is None else np.ascontiguousarray(origin, np.float32)
    out, rms, searches = _Alignment(), np.zeros(65, np.float64), C.c_int(0)
    rc = L.points_align(C.c_int(mode), C.c_longlong(len(p)), _ptr(p), C.c_longlong(len(q)), _ptr(q), C.c_float(radius), _ptr(org), C.c_uint(iterations),
                        C.c_double(tolerance), C.c_int(int(bool(with_scale))), C.byref(out), _ptr(rms), C.byref(searches))
    assert rc == 0
    a = Alignment(out.scale, tuple(out.rotation), tuple(out.translation), out.matched_before, out.matched_after, out.rms_before, out.rms_after, out.steps,
                  out.stopped)
    return (a, [float(v) for v in rms[:searches.value]]) if trace else a


def solve_pairs(L, p, q, with_scale=False):
    """(scale, R float64 [3, 3], t float64 [3], quaternion float64 [4] as w x y z, sweeps) of one step on the pairs (p_i, q_i)."""
    p, q = _cloud(p), _cloud(q)
    assert len(p) == len(q)
    scale, sweeps = C.c_double(0.0), C.c_uint(0)
    R, t, quaternion = np.zeros(9, np.float64), np.zeros(3, np.float64), np.zeros(4, np.float64)
    L.points_align_solve_pairs(C.c_longlong(len(p)), _ptr(p), _ptr(q), C.c_int(int(bool(with_scale))), C.byref(scale), _ptr(R), _ptr(t), _ptr(quaternion),
                               C.byref(sweeps))
    return scale.value, R.reshape(3, 3), t, quaternion, sweeps.value


def transformed(L, xyz, normal, scale, rotation, translation):
    """(xyz, normal) float32 [n, 3] moved by x' = scale R x + t and n' = R n."""
    xyz, normal = _cloud(xyz), _cloud(normal)
    R, t = np.ascontiguousarray(rotation, np.float64).reshape(9), np.ascontiguousarray(translation, np.float64).reshape(3)
    out_xyz, out_normal = np.zeros_like(xyz), np.zeros_like(normal)
    L.points_transformed(C.c_longlong(len(xyz)), _ptr(xyz), _ptr(normal), C.c_double(scale), _ptr(R), _ptr(t), _ptr(out_xyz), _ptr(out_normal))
    return out_xyz, out_normal


def bits(a):
    """The fields of an Alignment (the checker's or Points.align's) as integers: the doubles by their bits."""
    def d(v):
        return int(np.float64(v).view(np.uint64))
    return ((d(a.scale),) + tuple(d(v) for v in np.asarray(a.rotation, np.float64).reshape(9)) + tuple(d(v) for v in np.asarray(a.translation, np.float64).reshape(3))
            + (int(a.matched_before), int(a.matched_after), d(a.rms_before), d(a.rms_after), int(a.steps), int(a.stopped)))
