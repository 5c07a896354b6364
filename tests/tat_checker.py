"""The sequential checker of the Tanks and Temples fusions (tests/helpers/tat_fusion_ref.cpp): built with the host compiler into a
directory of the caller's choice and called through ctypes.  Shared by test_tat_fusion_checker.py (CPU) and
test_gpu_fusion_tat.py."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "helpers", "tat_fusion_ref.cpp")
VARIANTS = {"tat_intermediate": 1, "tat_advanced": 2}


def build(ob, out_dir):
    """Compiles the checker against the fusion oracle's libapd_fusion_oracle.so (orc_fusion_acos); returns the loaded library."""
    ob.build()
    oracle_dir = os.path.dirname(ob._FUSION_LIB_PATH)
    out = os.path.join(str(out_dir), "libtat_fusion_ref.so")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wextra", SOURCE,
           "-o", out, "-L" + oracle_dir, "-l:libapd_fusion_oracle.so", "-Wl,-rpath," + oracle_dir]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(out)
    L.tat_fuse.restype = C.c_longlong
    return L


def fuse(L, variant, cameras, images, depths, normals, pairs, ply_path, blocks=None, stats=None):
    """variant "tat_intermediate" / "tat_advanced"; arguments as oracle.binding.fuse without the weak maps (blocks: a list of
    uint8 arrays, None for a view without a block mask).  Returns (points, points that used a stale diff entry).  stats: a
    dict that receives "max_gap", the largest (pixel - pixel that wrote the entry) in raster pixels over the diff entries the
    points used."""
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

    rows = (C.c_int * V)(*[d.shape[0] for d in depths])
    cols = (C.c_int * V)(*[d.shape[1] for d in depths])
    offs = (C.c_int * (V + 1))()
    flat = []
    for v in range(V):
        offs[v] = len(flat)
        flat += list(pairs[v])
    offs[V] = len(flat)
    idx = (C.c_int * max(len(flat), 1))(*flat)
    channels = 3 if np.asarray(images[0]).ndim == 3 else 1
    stale, gap = C.c_longlong(0), C.c_longlong(0)
    n = L.tat_fuse(VARIANTS[variant], V, C.byref(cameras), ptrs(images, np.float32), channels, ptrs(depths, np.float32),
                   ptrs(normals, np.float32), None if blocks is None else ptrs(blocks, np.uint8), rows, cols, offs, idx,
                   str(ply_path).encode(), C.byref(stale), C.byref(gap))
    if n < 0:
        raise IOError("cannot write " + str(ply_path))
    if stats is not None:
        stats["max_gap"] = int(gap.value)
    return int(n), int(stale.value)


def read_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    n = int([l for l in head.decode().split("\n") if l.startswith("element vertex")][0].split()[2])
    assert len(body) == 15 * n
    rec = np.frombuffer(body, np.dtype([("xyz", "<f4", 3), ("bgr", "u1", 3)]))
    return rec["xyz"].copy(), rec["bgr"].copy()
