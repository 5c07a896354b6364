"""The sequential checker of apd_mesh_adjacency and apd_mesh_smooth (tests/helpers/mesh_smooth_ref.cpp, contract C24): built with the
host compiler into a directory of the caller's choice, as mesh_checker.py builds its own, and called through ctypes.  Shared by
test_mesh_smooth.py (CPU) and test_gpu_mesh_smooth.py.  A mesh is mesh_checker.Mesh."""
import ctypes as C
import os
import subprocess

import numpy as np

import mesh_checker as MC

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "helpers", "mesh_smooth_ref.cpp")
F = np.float32
MODES = {"fixed": 0, "along": 1, "free": 2}


def build(out_dir):
    out = os.path.join(str(out_dir), "libmesh_smooth_ref.so")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wextra", SOURCE, "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(out)
    L.mesh_adjacency.restype = None
    L.mesh_smooth.restype = C.c_longlong
    return L


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def adjacency(L, mesh):
    """(valence uint32 [n], boundary bool [n], edges, boundary_edges, nonmanifold_edges)."""
    nv, nf = len(mesh.vertices), len(mesh.faces)
    valence, boundary, counts = np.zeros(nv, np.uint32), np.zeros(nv, np.uint8), np.zeros(3, np.int64)
    L.mesh_adjacency(C.c_longlong(nv), C.c_longlong(nf), _ptr(mesh.faces), _ptr(valence), _ptr(boundary), _ptr(counts))
    return valence, boundary.astype(bool), int(counts[0]), int(counts[1]), int(counts[2])


def smooth(L, mesh, iterations, lam=0.5, mu=-0.53, boundary="along"):
    """(the checker's result, a mesh_checker.Mesh without normals; the vertices that move in the first step)."""
    nv, nf = len(mesh.vertices), len(mesh.faces)
    xyz = np.zeros((nv, 3), F)
    moved = L.mesh_smooth(C.c_longlong(nv), _ptr(mesh.vertices), C.c_longlong(nf), _ptr(mesh.faces), C.c_int(iterations), C.c_float(F(lam)), C.c_float(F(mu)),
                          C.c_int(MODES[boundary]), _ptr(xyz))
    return MC.Mesh(xyz, mesh.faces.copy(), None if mesh.colours is None else mesh.colours.copy()), moved
