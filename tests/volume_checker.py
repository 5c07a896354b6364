"""The sequential checker of the signed distance volume and its mesh (tests/helpers/volume_ref.cpp): built with the host compiler
into a directory of the caller's choice and called through ctypes.  Shared by test_volume.py (CPU) and test_gpu_volume.py.  A grid is
a Grid below; cameras are the package's Camera structures (K, R, t, width, height are read); depth maps are float32 [height, width],
images float32 [height, width] or [height, width, 3]."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "helpers", "volume_ref.cpp")
F = np.float32


def build(out_dir):
    out = os.path.join(str(out_dir), "libvolume_ref.so")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wextra", SOURCE, "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(out)
    L.volume_integrate.restype = None
    L.volume_extract.restype = None
    L.volume_cases.restype = None
    return L


class Grid:
    """dims (nx, ny, nz), origin float32 [3], voxel, trunc, max_weight as binary32 values."""

    def __init__(self, dims, origin, voxel, trunc, max_weight=64.0):
        self.dims = tuple(int(d) for d in dims)
        self.origin = np.array(origin, F)
        self.voxel, self.trunc, self.max_weight = F(voxel), F(trunc), F(max_weight)

    @property
    def samples(self):
        return self.dims[0] * self.dims[1] * self.dims[2]

    def positions(self):
        """float32 [samples, 3] in linear order: origin + (float)index * voxel."""
        nx, ny, nz = self.dims
        k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        return np.stack([self.origin[a] + idx.ravel().astype(F) * self.voxel for a, idx in enumerate((i, j, k))], 1).astype(F)


class State:
    """tsdf, weight float32 [samples]; colour float32 [samples, 4] (blue, green, red, colour weight) or None."""

    def __init__(self, grid, colour=False):
        self.tsdf, self.weight = np.ones(grid.samples, F), np.zeros(grid.samples, F)
        self.colour = np.zeros((grid.samples, 4), F) if colour else None

    def copy(self):
        new = State.__new__(State)
        new.tsdf, new.weight, new.colour = self.tsdf.copy(), self.weight.copy(), None if self.colour is None else self.colour.copy()
        return new


def camera_floats(cam):
    return np.array(list(cam.K) + list(cam.R) + list(cam.t), F)


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def integrate(L, grid, state, cams, depths, images=None, weights=None):
    """Applies the views to `state` in place."""
    V = len(cams)
    ks = np.concatenate([camera_floats(c) for c in cams])
    sizes = np.array([[int(c.width), int(c.height)] for c in cams], np.int32)
    deps = [np.ascontiguousarray(d, F) for d in depths]
    imgs = None if images is None else [np.ascontiguousarray(m, F) for m in images]
    channels = 1 if imgs is None or imgs[0].ndim == 2 else 3
    for c, d in zip(cams, deps):
        assert d.shape == (c.height, c.width)
    w = None if weights is None else np.ascontiguousarray(weights, F)
    table = lambda arrs: None if arrs is None else (C.c_void_p * V)(*[a.ctypes.data for a in arrs])
    dims, origin = np.array(grid.dims, np.int32), np.ascontiguousarray(grid.origin, F)
    L.volume_integrate(_ptr(dims), _ptr(origin), C.c_float(grid.voxel), C.c_float(grid.trunc), C.c_float(grid.max_weight), C.c_int(V), _ptr(ks),
                       _ptr(sizes), table(deps), table(imgs), C.c_int(channels), _ptr(w), _ptr(state.tsdf), _ptr(state.weight), _ptr(state.colour))
    return state


class MeshArrays:
    """vertices float32 [n, 3], colours uint8 [n, 3] (blue, green, red) or None, faces int32 [m, 3]."""

    def __init__(self, vertices, colours, faces):
        self.vertices, self.colours, self.faces = vertices, colours, faces


def extract(L, grid, tsdf, weight, colour=None):
    dims, origin = np.array(grid.dims, np.int32), np.ascontiguousarray(grid.origin, F)
    D, W = np.ascontiguousarray(tsdf, F).ravel(), np.ascontiguousarray(weight, F).ravel()
    Cc = None if colour is None else np.ascontiguousarray(colour, F).reshape(-1, 4)
    assert len(D) == len(W) == grid.samples
    nv, nf = C.c_longlong(0), C.c_longlong(0)
    args = [_ptr(dims), _ptr(origin), C.c_float(grid.voxel), _ptr(D), _ptr(W), _ptr(Cc), C.byref(nv), C.byref(nf)]
    L.volume_extract(*args, None, None, None)
    xyz, bgr, faces = np.zeros((nv.value, 3), F), np.zeros((nv.value, 3), np.uint8), np.zeros((nf.value, 3), np.int32)
    if nv.value or nf.value:
        L.volume_extract(*args, C.c_void_p(xyz.ctypes.data), C.c_void_p(bgr.ctypes.data), C.c_void_p(faces.ctypes.data))
    return MeshArrays(xyz, None if colour is None else bgr, faces)


def cases(L):
    """The table of the header: uint8 [6, 16, 7] -- the number of triangles, then six edges as (lower corner << 2) | upper corner."""
    out = np.zeros((6, 16, 7), np.uint8)
    L.volume_cases(_ptr(out))
    return out


def ply_bytes(mesh):
    """The file apd_mesh_write_ply writes of these arrays."""
    n, m = len(mesh.vertices), len(mesh.faces)
    head = "ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % n
    if mesh.colours is not None:
        head += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    head += "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % m
    if mesh.colours is None:
        body = np.ascontiguousarray(mesh.vertices, "<f4").tobytes()
    else:
        rec = np.zeros(n, np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)]))
        rec["xyz"], rec["rgb"] = mesh.vertices, mesh.colours[:, ::-1]
        body = rec.tobytes()
    faces = np.zeros(m, np.dtype([("n", "u1"), ("v", "<i4", 3)]))
    faces["n"], faces["v"] = 3, mesh.faces
    return head.encode() + body + faces.tobytes()


def assert_mesh_equal(got, want, what=""):
    """Bitwise: floats as uint32."""
    assert got.vertices.shape == want.vertices.shape and got.faces.shape == want.faces.shape, (what, got.vertices.shape, want.vertices.shape,
                                                                                                got.faces.shape, want.faces.shape)
    a, b = np.ascontiguousarray(got.vertices, F).view(np.uint32), np.ascontiguousarray(want.vertices, F).view(np.uint32)
    assert np.array_equal(a, b), (what, "vertices", np.argwhere(a != b)[:5])
    assert np.array_equal(got.faces, want.faces), (what, "faces", np.argwhere(got.faces != want.faces)[:5])
    assert (got.colours is None) == (want.colours is None), (what, "colours")
    if want.colours is not None:
        assert np.array_equal(got.colours, want.colours), (what, "colours", np.argwhere(got.colours != want.colours)[:5])


def assert_state_equal(got, want, what=""):
    for name in ("tsdf", "weight", "colour"):
        a, b = getattr(got, name), getattr(want, name)
        assert (a is None) == (b is None), (what, name)
        if b is not None:
            a, b = np.ascontiguousarray(a, F).view(np.uint32), np.ascontiguousarray(b, F).view(np.uint32)
            assert a.shape == b.shape, (what, name, a.shape, b.shape)
            assert np.array_equal(a, b), (what, name, np.argwhere(a != b)[:5])
