"""The sequential checker of the alignment to another cloud's tangent planes (tests/helpers/points_align_planes_ref.cpp): built
with the host compiler into a directory of the caller's choice and called through ctypes.  Shared by test_points_align_planes.py
(CPU) and test_gpu_points_align_planes.py.  Clouds are float32 [n, 3] arrays of positions, normals float32 [n, 3] arrays."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "helpers", "points_align_planes_ref.cpp")
BRUTE, GRID = 0, 1
ITERATIONS, CONVERGED, TOO_FEW, DEGENERATE = 0, 1, 2, 3
POINT_FIELDS = ("scale", "rotation", "translation", "matched_before", "matched_after", "rms_before", "rms_after", "steps", "stopped")
FIELDS = POINT_FIELDS + ("planes_before", "planes_after", "plane_rms_before", "plane_rms_after")
PlaneAlignment = collections.namedtuple("PlaneAlignment", FIELDS)
Solve = collections.namedtuple("Solve", ("degenerate", "z", "d", "rotation", "translation"))


class _PlaneAlignment(C.Structure):
    _fields_ = [("scale", C.c_double), ("rotation", C.c_double * 9), ("translation", C.c_double * 3), ("matched_before", C.c_longlong),
                ("matched_after", C.c_longlong), ("rms_before", C.c_double), ("rms_after", C.c_double), ("steps", C.c_int), ("stopped", C.c_int),
                ("planes_before", C.c_longlong), ("planes_after", C.c_longlong), ("plane_rms_before", C.c_double), ("plane_rms_after", C.c_double)]


def build(out_dir):
    out = os.path.join(str(out_dir), "libpoints_align_planes_ref.so")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-pthread", "-Wall", "-Wextra", SOURCE, "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(out)
    L.points_align_planes.restype = C.c_int
    L.points_align_planes_sums.restype = None
    L.points_align_planes_solve.restype = C.c_int
    return L


def _cloud(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1, 3)


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def align_planes(L, p, q, normal, radius, origin=None, iterations=16, tolerance=1e-6, mode=GRID):
    """PlaneAlignment of the positions p onto the planes at the positions q with the normals `normal`."""
    p, q, normal = _cloud(p), _cloud(q), _cloud(normal)
    assert len(q) == len(normal)
    org = np.zeros(3, np.float32) if origin is None else np.ascontiguousarray(origin, np.float32)
    out = _PlaneAlignment()
    rc = L.points_align_planes(C.c_int(mode), C.c_longlong(len(p)), _ptr(p), C.c_longlong(len(q)), _ptr(q), _ptr(normal), C.c_float(radius), _ptr(org),
                               C.c_uint(iterations), C.c_double(tolerance), C.byref(out))
    assert rc == 0
    return PlaneAlignment(out.scale, tuple(out.rotation), tuple(out.translation), out.matched_before, out.matched_after, out.rms_before, out.rms_after,
                          out.steps, out.stopped, out.planes_before, out.planes_after, out.plane_rms_before, out.plane_rms_after)


def sums_of_pairs(L, p, q, normal):
    """(centre float64 [3], the thirty sums float64 [30]) of pass 2 over the pairs (p_i, q_i) with the normals n_i."""
    p, q, normal = _cloud(p), _cloud(q), _cloud(normal)
    assert len(p) == len(q) == len(normal)
    centre, sums = np.zeros(3, np.float64), np.zeros(30, np.float64)
    L.points_align_planes_sums(C.c_longlong(len(p)), _ptr(p), _ptr(q), _ptr(normal), _ptr(centre), _ptr(sums))
    return centre, sums


def solve(L, centre, sums):
    """Solve(degenerate, z float64 [6] as omega then tau, the pivots d float64 [6], R float64 [3, 3], t float64 [3]) of one step."""
    centre, sums = np.ascontiguousarray(centre, np.float64).reshape(3), np.ascontiguousarray(sums, np.float64).reshape(30)
    z, d, R, t = np.zeros(6, np.float64), np.zeros(6, np.float64), np.zeros(9, np.float64), np.zeros(3, np.float64)
    degenerate = L.points_align_planes_solve(_ptr(centre), _ptr(sums), _ptr(z), _ptr(d), _ptr(R), _ptr(t))
    return Solve(bool(degenerate), z, d, R.reshape(3, 3), t)


def bits(a):
    """The fields of a PlaneAlignment (the checker's or Points.align_planes's) as integers: the doubles by their bits."""
    def d(v):
        return int(np.float64(v).view(np.uint64))
    return ((d(a.scale),) + tuple(d(v) for v in np.asarray(a.rotation, np.float64).reshape(9)) + tuple(d(v) for v in np.asarray(a.translation, np.float64).reshape(3))
            + (int(a.matched_before), int(a.matched_after), d(a.rms_before), d(a.rms_after), int(a.steps), int(a.stopped), int(a.planes_before),
               int(a.planes_after), d(a.plane_rms_before), d(a.plane_rms_after)))
