"""The sequential checker of apd_mesh_render, apd_mesh_face_visibility and apd_mesh_remove_unseen (tests/helpers/mesh_render_ref.cpp,
contract C25): built with the host compiler into a directory of the caller's choice, as mesh_smooth_checker.py builds its own, and
called through ctypes.  Shared by test_mesh_render.py (CPU) and test_gpu_mesh_render.py.  A mesh is mesh_checker.Mesh; cameras are
the package's Camera structures (K, R, t, width, height are read)."""
import ctypes as C
import os
import subprocess

import numpy as np

import mesh_checker as MC

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "helpers", "mesh_render_ref.cpp")
F = np.float32
NO_FACE = 0xFFFFFFFF
CULL = {"none": 0, "back": 1}


def build(out_dir):
    out = os.path.join(str(out_dir), "libmesh_render_ref.so")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wextra", SOURCE, "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(out)
    L.mesh_render.restype = None
    L.mesh_render_vertices.restype = None
    L.mesh_face_visibility.restype = C.c_longlong
    return L


def camera_floats(cam):
    """K, R, t of a Camera as the 21 floats the checker reads."""
    return np.array(list(cam.K) + list(cam.R) + list(cam.t), F)


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def render(L, mesh, cam, cull="none"):
    """(depth float32 [height, width], face uint32 [height, width]) of the mesh drawn into `cam`."""
    W, H = int(cam.width), int(cam.height)
    depth, face = np.zeros((H, W), F), np.full((H, W), NO_FACE, np.uint32)
    k = camera_floats(cam)
    L.mesh_render(C.c_longlong(len(mesh.vertices)), _ptr(mesh.vertices), C.c_longlong(len(mesh.faces)), _ptr(mesh.faces), _ptr(k), C.c_int(W), C.c_int(H),
                  C.c_int(CULL[cull]), _ptr(depth), _ptr(face))
    return depth, face


def vertices(L, mesh, cam):
    """(X int32 [n], Y int32 [n], d float32 [n], usable bool [n]): the projection of every vertex."""
    out = np.zeros((len(mesh.vertices), 4), np.int32)
    k = camera_floats(cam)
    L.mesh_render_vertices(C.c_longlong(len(mesh.vertices)), _ptr(mesh.vertices), _ptr(k), C.c_int(int(cam.width)), C.c_int(int(cam.height)), _ptr(out))
    return out[:, 0].copy(), out[:, 1].copy(), out[:, 2].copy().view(F), out[:, 3] != 0


def face_visibility(L, mesh, cams, cull="back", min_pixels=1, rel_tolerance=0.01):
    """(views uint32 [m], pixels uint64 [m], unseen)."""
    nf = len(mesh.faces)
    ks = np.concatenate([camera_floats(c) for c in cams])
    sizes = np.array([[int(c.width), int(c.height)] for c in cams], np.int32)
    views, pixels = np.zeros(nf, np.uint32), np.zeros(nf, np.uint64)
    unseen = L.mesh_face_visibility(C.c_longlong(len(mesh.vertices)), _ptr(mesh.vertices), C.c_longlong(nf), _ptr(mesh.faces), C.c_int(len(cams)), _ptr(ks),
                                    _ptr(sizes), C.c_int(CULL[cull]), C.c_uint(min_pixels), C.c_float(F(rel_tolerance)), _ptr(views), _ptr(pixels))
    return views, pixels, int(unseen)


def kept(mesh, keep):
    """The faces with keep[f], in their order, and the vertices they name, renumbered in their order: a direct numpy filter."""
    faces = mesh.faces[np.asarray(keep, bool)]
    used = np.zeros(len(mesh.vertices), bool)
    used[faces.reshape(-1)] = True
    new = np.cumsum(used) - 1
    cut = lambda a: None if a is None else a[used].copy()
    return MC.Mesh(mesh.vertices[used].copy(), new[faces].astype(np.int32).reshape(-1, 3), cut(mesh.colours), cut(mesh.normals))


def remove_unseen(L, mesh, cams, min_views=1, cull="back", min_pixels=1, rel_tolerance=0.01):
    """(the mesh of the faces at least min_views cameras see, the number of faces that went)."""
    views = face_visibility(L, mesh, cams, cull, min_pixels, rel_tolerance)[0]
    out = kept(mesh, views >= min_views)
    return out, len(mesh.faces) - len(out.faces)
