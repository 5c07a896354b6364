"""The sequential checker of the geometric filter (tests/helpers/filter_ref.cpp): built with the host compiler into a directory
of the caller's choice and called through ctypes.  Shared by test_filter_maps.py (CPU) and test_gpu_filter_maps.py."""
import ctypes as C
import os
import subprocess

import numpy as np

from eth_fusion_checker import DEFAULTS, MATH_DIR, Rule

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "helpers", "filter_ref.cpp")


def build(out_dir):
    out = os.path.join(str(out_dir), "libfilter_ref.so")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wextra", "-I" + MATH_DIR,
           SOURCE, "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(out)
    L.filter_views_ref.restype = None
    return L


def filter_views(L, cameras, depths, normals, weaks, pairs, blocks=None, **rule):
    """cameras: a ctypes array of the reference's Camera; blocks: a list of uint8 arrays, None for a view without a block mask;
    **rule: the values of eth_fusion_checker.DEFAULTS to replace.  Returns per view (depth float32, votes uint8, consistency
    float32), each [H, W]."""
    V = len(depths)
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
    shapes = [d.shape for d in depths]
    rows = (C.c_int * V)(*[s[0] for s in shapes])
    cols = (C.c_int * V)(*[s[1] for s in shapes])
    flat = [s for p in pairs for s in p]
    offs = (C.c_int * (V + 1))(*np.cumsum([0] + [len(p) for p in pairs]).tolist())
    idx = (C.c_int * max(len(flat), 1))(*flat)
    # filled with a value no output can hold everywhere, so that an unwritten pixel shows
    out = [(np.full(s, -1.0, np.float32), np.full(s, 255, np.uint8), np.full(s, -1.0, np.float32)) for s in shapes]
    L.filter_views_ref(C.byref(values), V, C.byref(cameras), ptrs(depths, np.float32), ptrs(normals, np.float32), ptrs(weaks, np.uint8),
                       None if blocks is None else ptrs(blocks, np.uint8), rows, cols, offs, idx,
                       (C.c_void_p * V)(*[o[0].ctypes.data for o in out]), (C.c_void_p * V)(*[o[1].ctypes.data for o in out]),
                       (C.c_void_p * V)(*[o[2].ctypes.data for o in out]))
    return out


def filter_case(L, ob, case, **rule):
    """filter_views() on a case of tests/fusion_cases.py."""
    return filter_views(L, case.cameras(ob.make_camera), case.depths, case.normals, case.weaks, case.pairs, blocks=case.blocks, **rule)
