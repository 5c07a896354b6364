"""The sequential checker of apd_mesh_nearest, apd_mesh_sample_points and apd_mesh_score (tests/helpers/mesh_nearest_ref.cpp, contract
C27): built with the host compiler into a directory of the caller's choice, as mesh_colour_checker.py builds its own, and called
through ctypes.  Shared by test_mesh_nearest.py (CPU) and test_gpu_mesh_nearest.py.  A mesh is vertices float32 [n, 3] and faces
int32 [m, 3] (colours uint8 [n, 3] or None); points are float32 [k, 3]."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "helpers", "mesh_nearest_ref.cpp")
F = np.float32
Score = collections.namedtuple("Score", "n_p n_q p_within q_within precision recall fscore mean_p mean_q")


def build(out_dir):
    out = os.path.join(str(out_dir), "libmesh_nearest_ref.so")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wextra", SOURCE, "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(out)
    L.mesh_nearest.restype = None
    L.mesh_score.restype = None
    L.mesh_nearest_pairs.restype = C.c_longlong
    L.mesh_sample_points.restype = C.c_longlong
    L.mesh_sample_number.restype = C.c_double
    L.mesh_sample_number.argtypes = [C.c_ulonglong] * 4
    return L


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _mesh(vertices, faces):
    return np.ascontiguousarray(vertices, F).reshape(-1, 3), np.ascontiguousarray(faces, np.int32).reshape(-1, 3)


def _origin(origin):
    return np.zeros(3, F) if origin is None else np.ascontiguousarray(origin, F).reshape(3)


def nearest(L, vertices, faces, points, radius, origin=None):
    """(distance float32 [k], face int32 [k], closest float32 [k, 3], d2 float64 [k])."""
    v, f = _mesh(vertices, faces)
    p = np.ascontiguousarray(points, F).reshape(-1, 3)
    n = len(p)
    distance, face, closest, d2 = np.zeros(n, F), np.zeros(n, np.int32), np.zeros((n, 3), F), np.zeros(n, np.float64)
    org = _origin(origin)
    L.mesh_nearest(_ptr(v), C.c_longlong(len(f)), _ptr(f), C.c_longlong(n), _ptr(p), C.c_float(F(radius)), _ptr(org), _ptr(distance), _ptr(face),
                   _ptr(closest), _ptr(d2))
    return distance, face, closest, d2


def pairs(L, vertices, faces, radius, origin=None):
    v, f = _mesh(vertices, faces)
    org = _origin(origin)
    return int(L.mesh_nearest_pairs(_ptr(v), C.c_longlong(len(f)), _ptr(f), C.c_float(F(radius)), _ptr(org)))


def reached(L, triangle, point, radius, origin=None):
    """Whether the 27 cells around `point` hold a cell that the face of corners `triangle` [3, 3] is binned into."""
    v = np.ascontiguousarray(triangle, F).reshape(3, 3)
    f = np.array([[0, 1, 2]], np.int32)
    p = np.ascontiguousarray(point, F).reshape(3)
    box, cell = np.zeros(6, np.int32), np.zeros(3, np.int32)
    org = _origin(origin)
    if not L.mesh_nearest_cells(_ptr(v), _ptr(f), _ptr(p), C.c_float(F(radius)), _ptr(org), _ptr(box), _ptr(cell)):
        return False
    return bool(((cell + 1 >= box[:3]) & (cell - 1 <= box[3:])).all())


# Faces and queries less than a radius apart whose binary32 cells are two apart: (origin, radius, triangle, query)
ROUNDING_CASES = [
    ((0.3, 0.0, 0.0), 0.4, [[16.699999, 0.0, 0.0], [16.699999, 1.0, 0.0], [16.699999, 0.0, 1.0]], [16.3, 0.25, 0.25]),
    ((3 * 2.0 ** -25, 0.0, 0.0), 1.0, [[3.0, 0.25, 0.25], [3.5, 0.25, 0.25], [3.0, 0.75, 0.5]], [2.0, 0.25, 0.25]),
    ((0.0, 0.0, 0.0), 1.0, [[-1e-45, 0.25, 0.25], [-1e-45, 0.75, 0.25], [-1e-45, 0.25, 0.75]], [1.0, 0.25, 0.25]),
    ((0.0, 0.0, 3 * 2.0 ** -25), 1.0, [[0.25, 0.25, 2.0], [0.75, 0.25, 1.5], [0.25, 0.75, 2.0]], [0.25, 0.25, 3.0]),   # the upper side
]


def sample_points(L, vertices, faces, density, seed=0, colours=None):
    """(xyz float32 [s, 3], normal float32 [s, 3], bgr uint8 [s, 3], face int32 [s])."""
    v, f = _mesh(vertices, faces)
    c = None if colours is None else np.ascontiguousarray(colours, np.uint8).reshape(-1, 3)
    args = [_ptr(v), _ptr(c), C.c_longlong(len(f)), _ptr(f), C.c_double(density), C.c_ulonglong(seed)]
    n = int(L.mesh_sample_points(*args, None, None, None, None))
    xyz, normal, bgr, face = np.zeros((n, 3), F), np.zeros((n, 3), F), np.zeros((n, 3), np.uint8), np.zeros(n, np.int32)
    if n:
        assert int(L.mesh_sample_points(*args, _ptr(xyz), _ptr(normal), _ptr(bgr), _ptr(face))) == n
    return xyz, normal, bgr, face


def score(L, vertices, faces, truth, threshold, density=None, seed=0, origin=None):
    v, f = _mesh(vertices, faces)
    t = np.ascontiguousarray(truth, F).reshape(-1, 3)
    if density is None or not density > 0:
        density = 4.0 / (float(F(threshold)) * float(F(threshold)))
    out = np.zeros(9, np.float64)
    org = _origin(origin)
    L.mesh_score(_ptr(v), C.c_longlong(len(f)), _ptr(f), C.c_longlong(len(t)), _ptr(t), C.c_float(F(threshold)), _ptr(org), C.c_double(density),
                 C.c_ulonglong(seed), _ptr(out))
    return Score(*[int(x) for x in out[:4]], *[float(x) for x in out[4:]])


def number(L, seed, f, k, c):
    return float(L.mesh_sample_number(seed, f, k, c))


# ---- meshes the tests share ----

def sheet(nx, ny, step=1.0, z=0.0, origin=(0.0, 0.0)):
    """nx x ny squares of side `step` in the plane z, two faces each: (vertices, faces)."""
    xs, ys = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="xy")
    v = np.stack([origin[0] + xs.ravel() * step, origin[1] + ys.ravel() * step, np.full(xs.size, z)], 1).astype(F)
    f = []
    for j in range(ny):
        for i in range(nx):
            a = j * (nx + 1) + i
            f += [[a, a + 1, a + nx + 2], [a, a + nx + 2, a + nx + 1]]
    return v, np.array(f, np.int32)


def strip(faces, step=1.0):
    """A strip of `faces` triangles along x between y = 0 and y = step."""
    n = faces + 2
    v = np.array([[(k // 2) * step + (0.5 * step if k % 2 else 0.0), step if k % 2 else 0.0, 0.0] for k in range(n)], F)
    f = np.array([[k, k + 1, k + 2] if k % 2 == 0 else [k + 1, k, k + 2] for k in range(faces)], np.int32)
    return v, f
