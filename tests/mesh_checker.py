"""The sequential checker of the mesh cleaning calls (tests/helpers/mesh_ref.cpp, contract C22): built with the host compiler into a
directory of the caller's choice and called through ctypes.  Shared by test_mesh.py (CPU) and test_gpu_mesh.py.  A mesh is a Mesh
below: vertices float32 [n, 3], colours uint8 [n, 3] or None, normals float32 [n, 3] or None, faces int32 [m, 3]."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "helpers", "mesh_ref.cpp")
F = np.float32


def build(out_dir):
    out = os.path.join(str(out_dir), "libmesh_ref.so")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wextra", SOURCE, "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(out)
    L.mesh_weld.restype = None
    L.mesh_remove_small.restype = None
    L.mesh_normals.restype = None
    L.mesh_components.restype = C.c_longlong
    return L


class Mesh:
    def __init__(self, vertices, faces, colours=None, normals=None):
        self.vertices = np.ascontiguousarray(vertices, F).reshape(-1, 3)
        self.faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
        self.colours = None if colours is None else np.ascontiguousarray(colours, np.uint8).reshape(-1, 3)
        self.normals = None if normals is None else np.ascontiguousarray(normals, F).reshape(-1, 3)


def of(mesh):
    """The arrays of the package's Mesh object."""
    return Mesh(mesh.vertices, mesh.faces, mesh.colours, mesh.normals)


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _compacted(call, mesh, *middle):
    nv, nf = len(mesh.vertices), len(mesh.faces)
    xyz, idx = np.zeros((nv, 3), F), np.zeros((nf, 3), np.int32)
    bgr = None if mesh.colours is None else np.zeros((nv, 3), np.uint8)
    nor = None if mesh.normals is None else np.zeros((nv, 3), F)
    onv, onf = C.c_longlong(0), C.c_longlong(0)
    call(C.c_longlong(nv), _ptr(mesh.vertices), _ptr(mesh.colours), _ptr(mesh.normals), C.c_longlong(nf), _ptr(mesh.faces), *middle, C.byref(onv),
         C.byref(onf), _ptr(xyz), _ptr(bgr), _ptr(nor), _ptr(idx))
    cut = lambda a, n: None if a is None else a[:n].copy()
    return Mesh(cut(xyz, onv.value), cut(idx, onf.value), cut(bgr, onv.value), cut(nor, onv.value))


def weld(L, mesh, tolerance, origin=None):
    org = np.zeros(3, F) if origin is None else np.ascontiguousarray(origin, F)
    return _compacted(L.mesh_weld, mesh, C.c_float(F(tolerance)), _ptr(org))


def components(L, mesh):
    """(label uint32 [m], size uint32 [m], count)."""
    nf = len(mesh.faces)
    label, size = np.zeros(nf, np.uint32), np.zeros(nf, np.uint32)
    count = L.mesh_components(C.c_longlong(len(mesh.vertices)), C.c_longlong(nf), _ptr(mesh.faces), _ptr(label), _ptr(size))
    return label, size, count


def remove_small(L, mesh, min_faces):
    return _compacted(L.mesh_remove_small, mesh, C.c_uint32(min_faces))


def with_normals(L, mesh):
    normals = np.zeros((len(mesh.vertices), 3), F)
    L.mesh_normals(C.c_longlong(len(mesh.vertices)), _ptr(mesh.vertices), C.c_longlong(len(mesh.faces)), _ptr(mesh.faces), _ptr(normals))
    return Mesh(mesh.vertices.copy(), mesh.faces.copy(), None if mesh.colours is None else mesh.colours.copy(), normals)


def ply_bytes(mesh):
    """The file apd_mesh_write_ply writes of these arrays."""
    n, m = len(mesh.vertices), len(mesh.faces)
    head = "ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % n
    fields = [("xyz", "<f4", 3)]
    if mesh.normals is not None:
        head += "property float nx\nproperty float ny\nproperty float nz\n"
        fields.append(("n", "<f4", 3))
    if mesh.colours is not None:
        head += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
        fields.append(("rgb", "u1", 3))
    head += "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % m
    rec = np.zeros(n, np.dtype(fields))
    rec["xyz"] = mesh.vertices
    if mesh.normals is not None:
        rec["n"] = mesh.normals
    if mesh.colours is not None:
        rec["rgb"] = mesh.colours[:, ::-1]
    faces = np.zeros(m, np.dtype([("n", "u1"), ("v", "<i4", 3)]))
    faces["n"], faces["v"] = 3, mesh.faces
    return head.encode() + rec.tobytes() + faces.tobytes()


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_mesh_equal(got, want, what=""):
    """Bitwise: floats as uint32."""
    assert got.vertices.shape == want.vertices.shape and got.faces.shape == want.faces.shape, (what, got.vertices.shape, want.vertices.shape,
                                                                                                got.faces.shape, want.faces.shape)
    assert np.array_equal(bits(got.vertices), bits(want.vertices)), (what, "vertices", np.argwhere(bits(got.vertices) != bits(want.vertices))[:5])
    assert np.array_equal(got.faces, want.faces), (what, "faces", np.argwhere(got.faces != want.faces)[:5])
    assert (got.colours is None) == (want.colours is None), (what, "colours")
    if want.colours is not None:
        assert np.array_equal(got.colours, want.colours), (what, "colours", np.argwhere(got.colours != want.colours)[:5])
    assert (got.normals is None) == (want.normals is None), (what, "normals")
    if want.normals is not None:
        assert np.array_equal(bits(got.normals), bits(want.normals)), (what, "normals", np.argwhere(bits(got.normals) != bits(want.normals))[:5])
