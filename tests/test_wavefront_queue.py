"""The task queue of the one-rank in-memory scheduler (apd-mvs_amd/host/wavefront.h): which (pass, view) a free lane may take
while the passes of a pyramid level run without a barrier between them.  The class holds no device call, thread or lock, so it
is driven here from Python (host_capi.cpp: apdhost_wavefront_*) the way the scheduler's lanes drive it, with seeded random
completion orders, and what the scheduler relies on is asserted at every hand-out.  No GPU needed."""
import ctypes as C
import os
import random

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "apd-mvs_amd", "_build", "libapd_host.so")
TASK, WAIT, FINISHED = 0, 1, 2


@pytest.fixture(scope="module")
def host(pkg):
    assert os.path.exists(HOST_LIB), "run __graft_entry__.build() first"
    pkg.lib()  # libapd_host.so depends on libapd_mi355x.so
    L = C.CDLL(HOST_LIB)
    ip = C.POINTER(C.c_int)
    L.apdhost_wavefront_create.restype = C.c_void_p
    L.apdhost_wavefront_create.argtypes = [C.c_int, ip, ip, C.c_int, ip, ip, C.c_int, C.c_int]
    L.apdhost_wavefront_take.argtypes = [C.c_void_p, ip, ip]
    L.apdhost_wavefront_publish.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.apdhost_wavefront_finish.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.apdhost_wavefront_published.argtypes = [C.c_void_p, C.c_int]
    L.apdhost_wavefront_source_iteration.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.apdhost_wavefront_destroy.argtypes = [C.c_void_p]
    return L


def _ints(values):
    return (C.c_int * max(1, len(values)))(*values)


# Source lists as pair.txt gives them, per reference view; an index >= the number of views is a source-only image.
def _chain(n):
    return [[j for j in (v - 1, v + 1) if 0 <= j < n] for v in range(n)]


def _ring(n):
    return [[(v + 1) % n, (v - 1) % n] for v in range(n)]


# tests/test_gpu_dropin_binary.py::test_reference_order_in_memory_with_asymmetric_source_lists: u lists v but v does not list u,
# a view nobody lists, a view that lists only later views
ASYMMETRIC = [[3, 5], [0], [6, 0, 1], [2], [5, 6], [1, 4, 0, 2], [0]]
# the same with source-only images 7, 8 and 9 among the sources, and a view that has nothing else
WITH_SOURCE_ONLY = [[7, 3, 5], [0, 8], [6, 0, 9, 1], [2], [8, 9], [1, 4, 7, 0, 2], [0]]


def _random_lists(n, rng):
    return [rng.sample([j for j in range(n + 2) if j != v], rng.randint(0, min(4, n))) for v in range(n)]


TOPOLOGIES = {
    "chain": lambda rng: _chain(9),
    "ring": lambda rng: _ring(8),
    "asymmetric": lambda rng: ASYMMETRIC,
    "source_only": lambda rng: WITH_SOURCE_ONLY,
    "random": lambda rng: _random_lists(rng.randint(1, 10), rng),
}


def _level(num_passes, first_iteration):
    """The passes of one pyramid level as BuildSchedule lays them out: one photometric pass, then geometric ones."""
    return [(first_iteration + k, k > 0) for k in range(num_passes)]


def _drive(host, passes, lists, gauss_seidel, lanes, rng, cap):
    """Runs one level to its end with `lanes` lanes and a random completion order; asserts the scheduler's conditions on the way.
    The state the assertions read (`published`, `running`, `handed`) is this function's own record of what it told the queue."""
    V, P = len(lists), len(passes)
    first_iteration = passes[0][0]
    sources = [[j for j in lst if j < V] for lst in lists]     # the reconstructed views among them: the others have no depth map
    begin = [0]
    for s in sources:
        begin.append(begin[-1] + len(s))
    q = host.apdhost_wavefront_create(P, _ints([it for it, _ in passes]), _ints([1 if g else 0 for _, g in passes]), V, _ints(begin),
                                      _ints([j for s in sources for j in s]), 1 if gauss_seidel else 0, cap)
    assert q

    def reads(pi, v, j):   # the iteration of view j's depth map that task (pi, v) reads: the reference's order, or Jacobi
        it = passes[pi][0]
        return it if (gauss_seidel and j < v) else it - 1

    published = [first_iteration - 1] * V     # newest iteration whose map view v has published
    handed = [0] * P                          # views of pass pi handed out so far (they must go out in order)
    running = []                              # tasks a lane holds: [pi, v, has_published]
    try:
        while True:
            rc = WAIT
            while len(running) < lanes:
                pi_c, v_c = C.c_int(-1), C.c_int(-1)
                rc = host.apdhost_wavefront_take(q, C.byref(pi_c), C.byref(v_c))
                if rc != TASK:
                    break
                pi, v = pi_c.value, v_c.value
                it, geom = passes[pi]
                assert 0 <= pi < P and v == handed[pi], "a pass hands its views out in order, each once"
                handed[pi] += 1
                assert pi == 0 or published[v] >= it - 1, "the view's own previous pass is not finished"
                for j in ([v] + sources[v]) if geom else []:
                    need = reads(pi, v, j)
                    assert host.apdhost_wavefront_source_iteration(q, pi, v, j) == need
                    if published[j] < need:
                        # ... then the task will wait for it: only for its own pass, and only for a view handed out before it
                        assert need == it and j < handed[pi] and j != v, "a task may only wait for earlier views of its own pass"
                    assert need == it or published[j] >= it - 1, "a previous-pass map the task reads is not published"
                # the export overwrites the view's map of iteration it - 2 (two versions by parity): every task that reads that
                # version must have finished
                for pw in range(P):
                    for w in range(V):
                        if passes[pw][1] and v in sources[w] and reads(pw, w, v) == it - 2:
                            assert published[w] >= passes[pw][0], "view %d of pass %d still reads the map that (%d, %d) overwrites" % (w, pw, pi, v)
                running.append([pi, v, False])
                if geom and gauss_seidel:
                    assert sum(1 for t in running if t[0] == pi) <= cap, "more lanes on one geometric pass than the cap"
            if not running:
                assert rc == FINISHED, "no task is running and none is eligible: the level would hang"
                break
            # a lane makes progress: a task whose maps are all there publishes, a published one finishes
            ready = [t for t in running if t[2] or not passes[t[0]][1] or all(published[j] >= reads(t[0], t[1], j) for j in [t[1]] + sources[t[1]])]
            assert ready, "every running task waits for another one"
            t = rng.choice(ready)
            if not t[2]:
                host.apdhost_wavefront_publish(q, t[0], t[1])
                published[t[1]] = passes[t[0]][0]
                assert host.apdhost_wavefront_published(q, t[1]) == published[t[1]]
                t[2] = True
                if rng.random() < 0.5:
                    continue       # another lane gets a turn between this task's export and its lane coming free
            last_of_pass = host.apdhost_wavefront_finish(q, t[0], t[1])
            running.remove(t)
            assert bool(last_of_pass) == (handed[t[0]] == V and not any(u[0] == t[0] for u in running))
        assert handed == [V] * P, "every (pass, view) is handed out exactly once"
        assert published == [passes[-1][0]] * V
    finally:
        host.apdhost_wavefront_destroy(q)


@pytest.mark.parametrize("gauss_seidel", [True, False], ids=["reference_order", "jacobi"])
@pytest.mark.parametrize("num_passes", [1, 2, 4])
@pytest.mark.parametrize("topology", sorted(TOPOLOGIES))
def test_every_task_goes_out_once_when_ready_and_the_level_drains(host, topology, num_passes, gauss_seidel):
    cap = host.apdhost_wavefront_lanes_per_pass()
    assert cap >= 1
    for lanes in range(1, 9):
        for seed in range(6):
            rng = random.Random(1000 * lanes + seed)
            lists = TOPOLOGIES[topology](rng)
            _drive(host, _level(num_passes, 4 * (seed % 2)), lists, gauss_seidel, lanes, rng, cap)


@pytest.mark.parametrize("cap", [1, 3, 8])
def test_the_cap_on_lanes_per_geometric_pass_is_an_input(host, cap):
    for lanes in (1, 4, 8):
        rng = random.Random(cap * 10 + lanes)
        _drive(host, _level(4, 4), _ring(8), True, lanes, rng, cap)
