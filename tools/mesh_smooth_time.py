#!/usr/bin/env python3
"""What smoothing a mesh costs, call by call, on a device-resident mesh of about a million faces (a jittered sheet of tests/test_mesh.py),
for both layouts of the positions between the steps (apd_mesh_smooth_layout: 16 bytes a vertex, one 128-bit load a neighbour; 12
bytes, three 32-bit loads), beside apd_mesh_with_vertex_normals on the same mesh, the existing call of the same sort-then-gather
shape.  Not part of bench.py; needs a GPU.

  tools/mesh_smooth_time.py            1 warm-up round, then 7 rounds that alternate the calls; the median, the minimum and the maximum of
                                       the host clock around each call (the library call, which ends in a device synchronise; the
                                       result is closed outside the clock): adjacency() with its three counts, smooth(1, mu = 0) = the
                                       adjacency build and one step, smooth(10) = the build and 20 steps; one step alone is the
                                       difference of the two over 19
  --side N                             the sheet has N x (N - 4) vertices (default 710: 999,690 faces)"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def option(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def measure(side):
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    assert pkg.device_count() >= 1, "no HIP device visible"
    L = pkg.lib()
    print("library: %s" % pkg.LIB_PATH, flush=True)
    from test_mesh import sheet
    host = sheet(side, side - 4, 0.2)
    mesh = pkg.Mesh.from_arrays(host.vertices, host.faces)
    print("sheet of %d x %d = %d vertices, %d faces; a single run" % (side, side - 4, len(host.vertices), len(host.faces)))
    out, moved = C.c_void_p(), C.c_longlong(0)
    counts = [C.c_longlong(0) for _ in range(3)]

    def smooth(iterations, mu):
        assert L.apd_mesh_smooth(mesh._m, iterations, 0.5, mu, 1, C.byref(out), C.byref(moved)) == 0

    def normals():
        assert L.apd_mesh_with_vertex_normals(mesh._m, C.byref(out)) == 0

    def adjacency():
        assert L.apd_mesh_adjacency(mesh._m, None, None, *[C.byref(c) for c in counts]) == 0
        out.value = None

    todo = [("with_vertex_normals()", normals), ("adjacency(), counts only", adjacency), ("smooth(1, mu = 0)", lambda: smooth(1, 0.0)),
            ("smooth(10, 0.5, -0.53)", lambda: smooth(10, -0.53))]
    before = L.apd_mesh_smooth_layout(1)
    medians = {}
    try:
        for wide in (1, 0):
            L.apd_mesh_smooth_layout(wide)
            times = {what: [] for what, _ in todo}
            for round_ in range(8):   # the first is the warm-up
                for what, f in todo:
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    f()
                    took = 1e3 * (time.perf_counter() - t)
                    if out.value:
                        L.apd_mesh_destroy(out)
                    if round_ > 0:
                        times[what].append(took)
            print("positions between the steps: %s" % ("16 bytes a vertex, one 128-bit load" if wide else "12 bytes a vertex, three 32-bit loads"))
            for what, _ in todo:
                medians[(wide, what)] = statistics.median(times[what])
                print("    %-28s call ms: median %9.3f  min %9.3f  max %9.3f" % (what, medians[(wide, what)], min(times[what]), max(times[what])))
            step = (medians[(wide, todo[3][0])] - medians[(wide, todo[2][0])]) / 19.0
            print("    one step alone (the difference of the two smooth calls / 19): %.4f ms; smooth(10) / with_vertex_normals() = %.2f" % (
                step, medians[(wide, todo[3][0])] / medians[(wide, todo[0][0])]))
    finally:
        L.apd_mesh_smooth_layout(before)
    print("edges %d, boundary edges %d, non-manifold edges %d; %d vertices moved in the first step" % (counts[0].value, counts[1].value, counts[2].value, moved.value))
    sys.stdout.flush()
    mesh.close()


if __name__ == "__main__":
    measure(int(option("--side", "710")))
