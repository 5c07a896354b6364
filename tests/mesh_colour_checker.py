"""The sequential checker of apd_mesh_colour_from_views (tests/helpers/mesh_colour_ref.cpp, contract C26): built with the host compiler
into a directory of the caller's choice, as mesh_render_checker.py builds its own, and called through ctypes.  Shared by
test_mesh_colour.py (CPU) and test_gpu_mesh_colour.py.  A mesh is mesh_checker.Mesh; cameras are the package's Camera structures (K, R,
t, width, height are read); images are float32 [height, width] or [height, width, 3] (blue, green, red), all alike."""
import ctypes as C
import os
import subprocess

import numpy as np

import mesh_checker as MC
from mesh_render_checker import camera_floats

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "helpers", "mesh_colour_ref.cpp")
F = np.float32


def build(out_dir):
    out = os.path.join(str(out_dir), "libmesh_colour_ref.so")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wextra", SOURCE, "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(out)
    L.mesh_colour_from_views.restype = C.c_longlong
    L.mesh_colour_geometry.restype = None
    return L


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def colour_from_views(L, mesh, cams, images, rel_tolerance=0.01, min_cos=0.1):
    """(the mesh with its new colours, views uint32 [n], uncoloured)."""
    nv = len(mesh.vertices)
    imgs = [np.ascontiguousarray(a, F) for a in images]
    assert len(imgs) == len(cams) and len({a.ndim for a in imgs}) == 1
    channels = 3 if imgs[0].ndim == 3 else 1
    for a, c in zip(imgs, cams):
        assert a.shape == (int(c.height), int(c.width)) + ((3,) if channels == 3 else ()), (a.shape, c.width, c.height)
    ks = np.concatenate([camera_floats(c) for c in cams])
    sizes = np.array([[int(c.width), int(c.height)] for c in cams], np.int32)
    table = (C.c_void_p * len(imgs))(*[a.ctypes.data for a in imgs])
    bgr, views = np.zeros((nv, 3), np.uint8), np.zeros(nv, np.uint32)
    uncoloured = L.mesh_colour_from_views(C.c_longlong(nv), _ptr(mesh.vertices), _ptr(mesh.normals), _ptr(mesh.colours), C.c_longlong(len(mesh.faces)),
                                          _ptr(mesh.faces), C.c_int(len(cams)), _ptr(ks), _ptr(sizes), table, C.c_int(channels), C.c_float(F(rel_tolerance)),
                                          C.c_float(F(min_cos)), _ptr(bgr), _ptr(views))
    out = MC.Mesh(mesh.vertices.copy(), mesh.faces.copy(), bgr, None if mesh.normals is None else mesh.normals.copy())
    return out, views, int(uncoloured)


def geometry(L, mesh, cam):
    """(u, w, d, c) float64 [n] each: every vertex's binary32 projection into `cam` and the cosine of rule 5 with the mesh's normals."""
    out = np.zeros((len(mesh.vertices), 4), np.float64)
    k = camera_floats(cam)
    L.mesh_colour_geometry(C.c_longlong(len(mesh.vertices)), _ptr(mesh.vertices), _ptr(mesh.normals), _ptr(k), C.c_int(int(cam.width)), C.c_int(int(cam.height)),
                           _ptr(out))
    return out[:, 0].copy(), out[:, 1].copy(), out[:, 2].copy(), out[:, 3].copy()
