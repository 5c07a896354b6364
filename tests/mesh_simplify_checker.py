"""The sequential checker of apd_mesh_simplify (tests/helpers/mesh_simplify_ref.cpp, contract C23): built with the host compiler
into a directory of the caller's choice, as mesh_checker.py builds its own, and called through ctypes.  Shared by
test_mesh_simplify.py (CPU) and test_gpu_mesh_simplify.py.  A mesh is mesh_checker.Mesh."""
import ctypes as C
import os
import subprocess

import numpy as np

import mesh_checker as MC

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "helpers", "mesh_simplify_ref.cpp")
F = np.float32
PLACEMENTS = {"mean": 0, "quadric": 1}


def build(out_dir):
    out = os.path.join(str(out_dir), "libmesh_simplify_ref.so")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wextra", SOURCE, "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(out)
    L.mesh_simplify.restype = None
    L.mesh_simplify_place.restype = None
    L.mesh_simplify_rank_cut.restype = C.c_double
    return L


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def simplify(L, mesh, cell, origin=None, placement="quadric"):
    """The checker's result: a mesh_checker.Mesh without normals."""
    nv, nf = len(mesh.vertices), len(mesh.faces)
    org = np.zeros(3, F) if origin is None else np.ascontiguousarray(origin, F)
    xyz, idx = np.zeros((nv, 3), F), np.zeros((nf, 3), np.int32)
    bgr = None if mesh.colours is None else np.zeros((nv, 3), np.uint8)
    onv, onf = C.c_longlong(0), C.c_longlong(0)
    L.mesh_simplify(C.c_longlong(nv), _ptr(mesh.vertices), _ptr(mesh.colours), C.c_longlong(nf), _ptr(mesh.faces), C.c_float(F(cell)), _ptr(org),
                    C.c_int(PLACEMENTS[placement]), C.byref(onv), C.byref(onf), _ptr(xyz), _ptr(bgr), _ptr(idx))
    return MC.Mesh(xyz[:onv.value].copy(), idx[:onf.value].copy(), None if bgr is None else bgr[:onv.value].copy())


def place(L, sums9, mu, cell):
    """Steps 4 to 7 of the QUADRIC placement: the offset from the centre for the nine sums and the mean offset."""
    s, m, x = np.ascontiguousarray(sums9, np.float64), np.ascontiguousarray(mu, np.float64), np.zeros(3, np.float64)
    L.mesh_simplify_place(_ptr(s), _ptr(m), C.c_float(F(cell)), _ptr(x))
    return x
