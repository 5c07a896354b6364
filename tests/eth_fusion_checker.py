"""The sequential checker of the ETH fusion with options (tests/helpers/eth_fusion_opt_ref.cpp): built with the host compiler into
a directory of the caller's choice and called through ctypes.  Shared by test_fusion_options.py (CPU) and
test_gpu_fusion_options.py."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "helpers", "eth_fusion_opt_ref.cpp")
MATH_DIR = os.path.join(os.path.dirname(HERE), "apd-mvs_amd", "csrc")   # apd_fusion_math.h: acos_c9, exp_c9, lift, drop

# apd_fusion_options' eight values of the ETH loop and the reference's literals (APD.cpp:941-951)
DEFAULTS = dict(max_reproj_error=2.0, max_relative_depth=0.01, max_angle=0.174533, depth_weight=200.0, angle_weight=10.0,
                min_consistent=1, factor_strong=0.3, factor_weak=0.45)

# the three option sets the host and device fusions are checked with
OPTION_SETS = {
    "a": dict(min_consistent=2),
    "b": dict(max_reproj_error=0.75, max_relative_depth=0.004),
    "c": dict(factor_strong=0.6, factor_weak=0.2, depth_weight=50.0),
}


class Rule(C.Structure):
    _fields_ = [("max_reproj_error", C.c_float), ("max_relative_depth", C.c_float), ("max_angle", C.c_float), ("depth_weight", C.c_float),
                ("angle_weight", C.c_float), ("min_consistent", C.c_int), ("factor_strong", C.c_float), ("factor_weak", C.c_float)]


class Result:
    """count and, with points=True, xyz / normal / bgr / support / view / pixel of every point and `reuse`: int32 [K, 3] rows
    (view, rejected pixel, later pixel) -- a pixel rejected for having exactly one vote whose source pixel a later pixel of
    the same view then used."""


def build(out_dir):
    out = os.path.join(str(out_dir), "libeth_fusion_opt_ref.so")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wextra", "-I" + MATH_DIR,
           SOURCE, "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(out)
    L.eth_fuse_opt.restype = C.c_longlong
    L.eth_fuse_reuse_count.restype = C.c_longlong
    L.eth_fuse_points.restype = None
    L.eth_fuse_reuse.restype = None
    return L


def fuse(L, cameras, images, depths, normals, weaks, pairs, ply_path=None, blocks=None, ply_normals=False, points=False, **rule):
    """Arguments as oracle.binding.fuse (blocks: a list of uint8 arrays, None for a view without a block mask); **rule: the
    values of DEFAULTS to replace.  Writes ply_path if given.  Returns a Result."""
    V = len(images)
    keep = []

    def ptrs(arrs, dt):
        out = (C.c_void_p * V)()
        for i, a in enumerate(arrs):
            if a is None:
                continue
            a = np.ascontiguousarray(a, dt)
            keep.append(a)
            out[i] = a.ctypes.data
        return out

    unknown = set(rule) - set(DEFAULTS)
    assert not unknown, unknown
    values = Rule(**dict(DEFAULTS, **rule))
    rows = (C.c_int * V)(*[d.shape[0] for d in depths])
    cols = (C.c_int * V)(*[d.shape[1] for d in depths])
    flat = [s for p in pairs for s in p]
    offs = (C.c_int * (V + 1))(*np.cumsum([0] + [len(p) for p in pairs]).tolist())
    idx = (C.c_int * max(len(flat), 1))(*flat)
    channels = 3 if np.asarray(images[0]).ndim == 3 else 1
    n = L.eth_fuse_opt(C.byref(values), V, C.byref(cameras), ptrs(images, np.float32), channels, ptrs(depths, np.float32),
                       ptrs(normals, np.float32), ptrs(weaks, np.uint8), None if blocks is None else ptrs(blocks, np.uint8), rows, cols,
                       offs, idx, None if ply_path is None else str(ply_path).encode(), int(bool(ply_normals)))
    if n < 0:
        raise IOError("cannot write " + str(ply_path))
    res = Result()
    res.count = int(n)
    if points:
        res.xyz, res.normal = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
        res.bgr, res.support = np.empty((n, 3), np.uint8), np.empty(n, np.uint8)
        res.view, res.pixel = np.empty(n, np.int32), np.empty(n, np.int32)
        L.eth_fuse_points(*[C.c_void_p(a.ctypes.data) for a in (res.xyz, res.normal, res.bgr, res.support, res.view, res.pixel)])
        res.reuse = np.empty((L.eth_fuse_reuse_count(), 3), np.int32)
        L.eth_fuse_reuse(C.c_void_p(res.reuse.ctypes.data))
    return res


def fuse_case(L, ob, case, ply_path=None, **kw):
    """fuse() on a case of tests/fusion_cases.py."""
    return fuse(L, case.cameras(ob.make_camera), case.images, case.depths, case.normals, case.weaks, case.pairs, ply_path,
                blocks=case.blocks, **kw)


def read_ply(path):
    """(header lines, records) of a fusion's PLY: records have xyz, bgr and, with normals in the file, normal."""
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode().split("\n")
    n = int([l for l in lines if l.startswith("element vertex")][0].split()[2])
    fields = [("xyz", "<f4", 3)] + ([("normal", "<f4", 3)] if "property float nx" in lines else []) + [("bgr", "u1", 3)]
    rec = np.frombuffer(body, np.dtype(fields))
    assert len(rec) == n, (len(body), n)
    return lines, rec
