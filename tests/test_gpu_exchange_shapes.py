"""The exchange and the stream / host-memory helpers of the C ABI (csrc/apd_exchange.hip, apd_set_stream / apd_get_stream and
apd_image_pixels of csrc/apd_capi.hip) called directly at the sizes and alignments host/multi_device.cpp gives them, and held to
byte-exact host references: every reference is numpy on the bytes that were uploaded, every comparison is of raw bytes (uint32
words for floats), there is no tolerance.  Every buffer a helper writes or reads lies inside ONE device allocation per case, with
64 guard bytes (0xA5) or more on either side; the allocation is uploaded and read back whole (one apd_device_memcpy each way) and
compared whole, so a changed guard, a changed send buffer and a wrong result all show in one comparison.

Which arm of exchange_allgather a case reaches cannot be seen from outside, so `arms()` restates its selection predicates and
test_every_arm_of_the_all_gather_is_reached (no GPU) asserts that the case lists below reach every one.  By the code as it stands,
all ranks on device 0, t = bytes % 16, "aligned" = send[src] and recv[0] + src * bytes on 16-byte boundaries:

  backend   ranks  bytes              offsets                      rank 0 gathers by                  ranks 1.. copy by
  copy      1      t == 0, > 0        aligned                      k_gather_blocks, no tail           --
  copy      1      t != 0             aligned                      k_gather_blocks with the tail      --
  copy      1      any                recv+1 / send+8              plain hipMemcpyAsync               --
  copy      2..64  t == 0, > 0        aligned                      k_gather_blocks, no tail           twin copy by kernel
  copy      2..64  t == 0, > 0        odd ranks' send +4           mixed: kernel + hipMemcpyAsync     twin copy by kernel
  copy      2..64  t == 0, > 0        send+8                       plain hipMemcpyAsync               twin copy by kernel
  copy      2..64  t == 0, > 0        recv+1                       plain hipMemcpyAsync               twin copy by hipMemcpyAsync
  copy      2..64  t != 0             any                          plain hipMemcpyAsync               by kernel if ranks * bytes % 16 == 0 and
                                                                                                      recv aligned (8 x 6, 8 x 4082 ...), else
                                                                                                      hipMemcpyAsync (2 x 6887, 3 x 17 ...)
  copy      any    0                  any                          hipMemcpyAsync of 0 bytes          hipMemcpyAsync of 0 bytes
  copy      65     any                any                          the fallback: 65 hipMemcpyAsync    as above
  rccl      n      any                any                          n one-rank ncclAllGather of the leader, then n - 1 follower copies

"recv base aligned with an odd bytes_per_rank" of the final gather is the `aligned` offsets at 1, 15, 17 and 6887 bytes (and the
GatherFinalMaps test itself): with more than one rank an odd size switches the kernel off altogether, so the alternating block
alignment only ever decides between copies.

The grid of k_gather_blocks is capped at 2048 / min(direct, 8) + 1 workgroups per block and at 2048 for a twin copy.
(2048 * 256 + 1) * 16 + 5 bytes is therefore NOT past the cap of a single rank (2049 workgroups hold its 524289 words) and with
more ranks its tail switches the kernel off; it stays in the list for its copies and its tail, and two sizes are added that do make
the grid-stride loop take a second trip: (2049 * 256 + 1) * 16 + 5 for one rank (with a tail) and (257 * 256 + 1) * 16 for eight
(257 workgroups per block; its twin copy has 8 * 65793 = 526344 words against 2048 * 256).  `arms()` reports both trips and the
self-check requires them.

Pruning: the nine sizes up to 27548 bytes run the full product (four offset patterns x three entry points x {1, 2, 3, 8} ranks x
both backends; 65 ranks at 4080 and 6887 bytes on the copy backend).  The three sizes of 1 MB and more run with
apd_exchange_allgather alone and aligned offsets (the arms they add depend on neither), at {1, 2, 3, 8} ranks on both backends
for the issue's size, and where they make the second trip for the other two -- plus the mixed gather at eight ranks.

Measured on the MI355X: profiles/exchange_shapes/test_times.txt."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_exchange import _host_ptr, _lib, _malloc, _rescale_reference

gpu = pytest.mark.gpu

GUARD = 64            # bytes before and after every carved buffer, at least
GUARD_BYTE = 0xA5     # payload bytes are drawn from 1 .. 0x7F, fresh result areas hold 0xEE
RECV_FILL = 0xEE
MAX_RANKS = 64        # kGatherMaxRanks

SMALL_SIZES = [0, 1, 15, 16, 17, 4080, 4112, 97 * 71, 97 * 71 * 4]
ISSUE_BIG = (2048 * 256 + 1) * 16 + 5
TRIP_ONE_RANK = (2049 * 256 + 1) * 16 + 5
TRIP_EIGHT_RANKS = (257 * 256 + 1) * 16
# (send offset, recv offset) of rank r from a 16-byte boundary
OFFSETS = {"aligned": (lambda r: 0, lambda r: 0), "recv+1": (lambda r: 0, lambda r: 1), "send+8": (lambda r: 8, lambda r: 0),
           "odd_send+4": (lambda r: 4 * (r % 2), lambda r: 0)}
ENTRIES = ["allgather", "after_no_events", "after_done_event"]
RANKS_AND_BACKENDS = [(n, rccl) for n in (1, 2, 3, 8) for rccl in (0, 1)]
BIG_CASES = ([(n, rccl, ISSUE_BIG, "aligned") for n in (1, 2, 3, 8) for rccl in (0, 1)] +
             [(1, 0, TRIP_ONE_RANK, "aligned"), (8, 0, TRIP_EIGHT_RANKS, "aligned"), (8, 0, TRIP_EIGHT_RANKS, "odd_send+4")])
ALL_ARMS = {"blocks", "blocks+tail", "mixed", "copy", "twin-kernel", "twin-copy", "rccl", "rccl-followers", "fallback65",
            "second-trip-blocks", "second-trip-tail", "second-trip-twin", "zero-bytes"}


def small_cases(n):
    sizes = [4080, 97 * 71] if n > MAX_RANKS else SMALL_SIZES
    return [(b, o, e) for b in sizes for o in OFFSETS for e in ENTRIES]


def arms(n, nbytes, offsets, rccl):
    """The selection predicates of exchange_allgather (csrc/apd_exchange.hip) for n ranks on one device: the arms one exchange runs."""
    send_off, recv_off = OFFSETS[offsets]
    out = set()
    if nbytes == 0:
        out.add("zero-bytes")
    if rccl:
        out.add("rccl")
        if n > 1:
            out.add("rccl-followers")
        return out
    words, tail = divmod(nbytes, 16)
    kernel_ok = n <= MAX_RANKS and (tail == 0 or n == 1)
    if n > MAX_RANKS:
        out.add("fallback65")
    direct = 0
    for src in range(n):   # rank 0 has no twin: it gathers block by block
        aligned = send_off(src) % 16 == 0 and (recv_off(0) + src * nbytes) % 16 == 0
        direct += 1 if kernel_ok and aligned and nbytes > 0 else 0
    if direct == n:
        out.add("blocks+tail" if tail else "blocks")
    elif direct > 0:
        out.add("mixed")
    elif n <= MAX_RANKS:
        out.add("copy")
    if direct > 0:
        gx = min((words + 255) // 256 + 1, 2048 // max(1, min(direct, 8)) + 1)
        if words > gx * 256:
            out.add("second-trip-tail" if tail else "second-trip-blocks")
    for dst in range(1, n):   # every later rank has rank 0 as its twin
        total = n * nbytes
        if total % 16 == 0 and total > 0 and recv_off(dst) % 16 == 0 and recv_off(0) % 16 == 0:
            out.add("twin-kernel")
            if total // 16 > min((total // 16 + 255) // 256, 2048) * 256:
                out.add("second-trip-twin")
        else:
            out.add("twin-copy")
    return out


def test_every_arm_of_the_all_gather_is_reached():
    """No GPU: the case lists of the tests below, through the restated predicates, reach every arm of the table in the module's
    docstring -- and the rows of that table are what the predicates say."""
    reached = set()
    for n, rccl in RANKS_AND_BACKENDS + [(65, 0)]:
        for nbytes, offsets, _ in small_cases(n):
            reached |= arms(n, nbytes, offsets, rccl)
    small = set(reached)
    for n, rccl, nbytes, offsets in BIG_CASES:
        reached |= arms(n, nbytes, offsets, rccl)
    assert reached == ALL_ARMS, (ALL_ARMS - reached, reached - ALL_ARMS)
    assert small == ALL_ARMS - {"second-trip-blocks", "second-trip-tail", "second-trip-twin"}   # only the large sizes add the second trips
    # the rows of the table
    assert arms(1, 4080, "aligned", 0) == {"blocks"} and arms(1, 6887, "aligned", 0) == {"blocks+tail"} and arms(1, 1, "aligned", 0) == {"blocks+tail"}
    assert arms(1, 4080, "recv+1", 0) == {"copy"} and arms(1, 6887, "send+8", 0) == {"copy"}
    assert arms(3, 4112, "aligned", 0) == {"blocks", "twin-kernel"} and arms(3, 4112, "odd_send+4", 0) == {"mixed", "twin-kernel"}
    assert arms(2, 4080, "send+8", 0) == {"copy", "twin-kernel"} and arms(8, 4080, "recv+1", 0) == {"copy", "twin-copy"}
    assert arms(2, 6887, "aligned", 0) == {"copy", "twin-copy"} and arms(3, 17, "aligned", 0) == {"copy", "twin-copy"}
    assert arms(8, 97 * 71 * 4 + 2, "aligned", 0) == {"copy", "twin-kernel"}    # 8 x 27550 is a multiple of 16
    assert arms(3, 0, "aligned", 0) == {"zero-bytes", "copy", "twin-copy"}
    assert arms(65, 4080, "aligned", 0) == {"fallback65", "twin-kernel"} and arms(65, 6887, "aligned", 0) == {"fallback65", "twin-copy"}
    assert arms(8, 6887, "recv+1", 1) == {"rccl", "rccl-followers"} and arms(1, 16, "aligned", 1) == {"rccl"}
    # the issue's large size makes no second trip (see the docstring); the two added sizes do
    assert arms(1, ISSUE_BIG, "aligned", 0) == {"blocks+tail"} and arms(8, ISSUE_BIG, "aligned", 0) == {"copy", "twin-copy"}
    assert arms(1, TRIP_ONE_RANK, "aligned", 0) == {"blocks+tail", "second-trip-tail"}
    assert arms(8, TRIP_EIGHT_RANKS, "aligned", 0) == {"blocks", "second-trip-blocks", "twin-kernel", "second-trip-twin"}
    assert arms(8, TRIP_EIGHT_RANKS, "odd_send+4", 0) == {"mixed", "twin-kernel", "second-trip-twin"}
    # every GatherFinalMaps exchange of 97 x 71 pixels: planes through the kernels, weak maps (6887 bytes) through the copies
    assert arms(3, 97 * 71 * 16, "aligned", 0) == {"blocks", "twin-kernel"} and arms(3, 97 * 71, "aligned", 0) == {"copy", "twin-copy"}


# ---- one device allocation per case, buffers carved out of it ---------------------------------------------------------------------

class Arena:
    """Offsets of buffers inside one allocation: every buffer starts `off` bytes past a 16-byte boundary and has GUARD bytes or more
    of GUARD_BYTE on either side."""

    def __init__(self):
        self.size = 0

    def carve(self, nbytes, off=0):
        start = self.size + GUARD + off
        self.size = -(-(start + nbytes + GUARD) // 16) * 16
        return start

    def host(self):
        return np.full(self.size, GUARD_BYTE, np.uint8)


def _lib2(pkg):
    L = _lib(pkg)
    vp, pvp = C.c_void_p, C.POINTER(C.c_void_p)
    L.apd_exchange_allgather_after.argtypes = [vp, pvp, pvp, C.c_size_t, C.c_int, pvp]
    L.apd_split_planes_async.argtypes = [C.c_int, vp, vp, C.c_size_t, vp, vp]
    L.apd_rescale_nearest_async.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int]
    L.apd_device_memcpy_async.argtypes = [C.c_int, vp, vp, vp, C.c_size_t]
    L.apd_stream_create.argtypes = [C.c_int, pvp]
    L.apd_stream_destroy.argtypes = [C.c_int, vp]
    L.apd_stream_synchronize.argtypes = [C.c_int, vp]
    L.apd_host_alloc.argtypes = [C.c_size_t, pvp]
    L.apd_host_free.argtypes = [vp]
    L.apd_host_register.argtypes = [vp, C.c_size_t]
    L.apd_host_unregister.argtypes = [vp]
    L.apd_device_memory.argtypes = [C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.apd_image_pixels.argtypes = [vp]
    L.apd_image_pixels.restype = vp
    L.apd_get_stream.argtypes = [vp, pvp]
    L.apd_set_stream.argtypes = [vp, vp]
    return L


def _upload(L, dev, host):
    assert dev.value % 256 == 0   # what the offsets inside the arena count from
    assert L.apd_device_memcpy(0, dev, _host_ptr(host), host.size) == 0, L.apd_exchange_last_error()


def _download(L, dev, nbytes):
    got = np.empty(nbytes, np.uint8)
    assert L.apd_device_memcpy(0, _host_ptr(got), dev, nbytes) == 0, L.apd_exchange_last_error()
    return got


def _assert_same(got, want, regions, where):
    """Whole-allocation comparison; on a difference, names the first differing byte's region."""
    if np.array_equal(got, want):
        return
    bad = np.flatnonzero(got != want)
    first = int(bad[0])
    name = "guard"
    for label, start, length in regions:
        if start <= first < start + length:
            name = "%s+%d" % (label, first - start)
    raise AssertionError("%s: %d bytes differ, the first at %d (%s): got 0x%02x, want 0x%02x" % (where, bad.size, first, name, got[first], want[first]))


def _new_stream(L):
    st = C.c_void_p()
    assert L.apd_stream_create(0, C.byref(st)) == 0 and st.value, L.apd_exchange_last_error()
    return st


@pytest.fixture(scope="module")
def exchanges(gpu_pkg):
    """One exchange per (ranks, backend) for the whole file: RCCL's set-up takes most of a second per communicator."""
    L = _lib2(gpu_pkg)
    made = {}

    def get(n, rccl):
        if (n, rccl) not in made:
            x = C.c_void_p()
            devs = (C.c_int * n)(*([0] * n))
            assert L.apd_exchange_create(C.byref(x), n, devs, rccl) == 0, L.apd_exchange_last_error()
            assert L.apd_exchange_backend(x) == (b"rccl" if rccl else b"peer-copy")
            made[(n, rccl)] = x
        return made[(n, rccl)]

    def release():
        while made:
            assert L.apd_exchange_destroy(made.popitem()[1]) == 0

    get.release = release
    yield get
    release()


def _counts(L, x):
    a, b = C.c_int(), C.c_int()
    assert L.apd_exchange_counts(x, C.byref(a), C.byref(b)) == 0
    return a.value, b.value


def _exchange(L, x, entry, send, recv, nbytes, done_event):
    n = len(send)
    sp, rp = (C.c_void_p * n)(*send), (C.c_void_p * n)(*recv)
    if entry == "allgather":
        return L.apd_exchange_allgather(x, sp, rp, nbytes)
    if entry == "after_no_events":
        return L.apd_exchange_allgather_after(x, sp, rp, nbytes, 0, None)
    evs = (C.c_void_p * 2)(done_event, None)   # one event that has completed, one NULL entry (skipped)
    return L.apd_exchange_allgather_after(x, sp, rp, nbytes, 2, evs)


def _layout(n, nbytes, offsets):
    send_off, recv_off = OFFSETS[offsets]
    a = Arena()
    send_at = [a.carve(nbytes, send_off(r)) for r in range(n)]
    recv_at = [a.carve(n * nbytes, recv_off(r)) for r in range(n)]
    return a, send_at, recv_at


def _gather_case(L, x, rccl, dev, n, nbytes, offsets, entry, rng, done_event):
    a, send_at, recv_at = _layout(n, nbytes, offsets)
    host = a.host()
    blocks = [rng.integers(1, 0x80, nbytes, dtype=np.uint8) for _ in range(n)]
    regions = []
    for r in range(n):
        host[send_at[r]:send_at[r] + nbytes] = blocks[r]
        host[recv_at[r]:recv_at[r] + n * nbytes] = RECV_FILL
        regions += [("send[%d]" % r, send_at[r], nbytes), ("recv[%d]" % r, recv_at[r], n * nbytes)]
    _upload(L, dev, host)
    before = _counts(L, x)
    rc = _exchange(L, x, entry, [dev.value + s for s in send_at], [dev.value + r for r in recv_at], nbytes, done_event)
    where = "%d ranks, %s, %d bytes, %s, %s" % (n, "rccl" if rccl else "copies", nbytes, offsets, entry)
    assert rc == 0, (where, L.apd_exchange_last_error())
    after = _counts(L, x)
    assert (after[0] - before[0], after[1] - before[1]) == ((1, 0) if rccl else (0, 1)), (where, before, after)
    got = _download(L, dev, a.size)
    if nbytes > 0:
        want_blocks = np.concatenate(blocks)
        for r in range(n):
            host[recv_at[r]:recv_at[r] + n * nbytes] = want_blocks   # `host` becomes the expectation: guards and send buffers as uploaded
    _assert_same(got, host, regions, where)


def _done_event():
    import torch
    ev = torch.cuda.Event()
    ev.record()
    ev.synchronize()
    return ev


@gpu
@pytest.mark.parametrize("n,rccl", [(65, 0)] + RANKS_AND_BACKENDS)
def test_allgather_over_sizes_offsets_and_entry_points(gpu_pkg, exchanges, n, rccl):
    """apd_exchange_allgather and apd_exchange_allgather_after at every small size x offset pattern x entry point (small_cases): the
    result of every rank, every guard byte and every send buffer, byte for byte, and the backend's counter.  A zero-byte exchange
    returns APD_OK and changes nothing.  65 ranks (one past kGatherMaxRanks) have an exchange of their own, created after the shared
    ones are released and destroyed here: at most 65 streams of this file exist at a time."""
    L = _lib2(gpu_pkg)
    own = n > MAX_RANKS
    if own:
        exchanges.release()
        x = C.c_void_p()
        assert L.apd_exchange_create(C.byref(x), n, (C.c_int * n)(*([0] * n)), rccl) == 0, L.apd_exchange_last_error()
    else:
        x = exchanges(n, rccl)
    cases = small_cases(n)
    dev = _malloc(L, max(_layout(n, b, o)[0].size for b, o, _ in cases))
    ev = _done_event()
    rng = np.random.default_rng(100 * n + rccl)
    try:
        for nbytes, offsets, entry in cases:
            _gather_case(L, x, rccl, dev, n, nbytes, offsets, entry, rng, ev.cuda_event)
    finally:
        L.apd_device_free(0, dev)
        if own:
            assert L.apd_exchange_destroy(x) == 0
    print("EXCHANGE_SHAPES %d ranks, %s: %d exchanges" % (n, "rccl" if rccl else "copies", len(cases)))


@gpu
@pytest.mark.parametrize("n,rccl,nbytes,offsets", BIG_CASES)
def test_allgather_at_the_grid_cap(gpu_pkg, exchanges, n, rccl, nbytes, offsets):
    """The sizes around the capped grid of k_gather_blocks (BIG_CASES; which of them makes a second trip of the grid-stride loop:
    the module's docstring and the self-check)."""
    L = _lib2(gpu_pkg)
    dev = _malloc(L, _layout(n, nbytes, offsets)[0].size)
    try:
        _gather_case(L, exchanges(n, rccl), rccl, dev, n, nbytes, offsets, "allgather", np.random.default_rng(n + nbytes % 1000), None)
    finally:
        L.apd_device_free(0, dev)


@gpu
@pytest.mark.parametrize("rccl", [0, 1])
def test_allgather_in_the_pattern_of_the_final_gather(gpu_pkg, exchanges, rccl):
    """GatherFinalMaps of host/multi_device.cpp: 3 ranks, 2 slots, 5 views of 97 x 71 pixels (view v = slot * 3 + rank), per slot one
    exchange of the planes (16 bytes per pixel) and one of the weak maps (1 byte per pixel) out of the views' own buffers into block
    FinalBlock(slot) = slot * 3 of one result per rank and kind; rank 2 has no view in slot 1 and sends its first view's buffer.
    The weak maps' 6887 bytes put slot 1 of every result on an odd address.  Expected: the views in order, then the padding."""
    L = _lib2(gpu_pkg)
    G, slots, V, pix = 3, 2, 5, 97 * 71
    x = exchanges(G, rccl)
    a = Arena()
    rng = np.random.default_rng(41 + rccl)
    elems = (16, 1)
    view_at = [[a.carve(pix * e) for e in elems] for _ in range(V)]
    all_at = [[a.carve(slots * G * pix * e) for e in elems] for _ in range(G)]
    host = a.host()
    views = [[rng.integers(1, 0x80, pix * e, dtype=np.uint8) for e in elems] for _ in range(V)]
    regions = []
    for v in range(V):
        for k, e in enumerate(elems):
            host[view_at[v][k]:view_at[v][k] + pix * e] = views[v][k]
            regions.append(("view %d kind %d" % (v, k), view_at[v][k], pix * e))
    for r in range(G):
        for k, e in enumerate(elems):
            host[all_at[r][k]:all_at[r][k] + slots * G * pix * e] = RECV_FILL
            regions.append(("result of rank %d kind %d" % (r, k), all_at[r][k], slots * G * pix * e))
    dev = _malloc(L, a.size)
    try:
        _upload(L, dev, host)
        for sl in range(slots):
            for k, e in enumerate(elems):
                sent = [sl * G + r if sl * G + r < V else r for r in range(G)]   # own[sl] of rank r, or its first view as padding
                send = [dev.value + view_at[v][k] for v in sent]
                recv = [dev.value + all_at[r][k] + sl * G * pix * e for r in range(G)]
                assert (recv[0] % 16 == 0) == (k == 0 or sl == 0)
                before = _counts(L, x)
                assert _exchange(L, x, "allgather", send, recv, pix * e, None) == 0, L.apd_exchange_last_error()
                after = _counts(L, x)
                assert (after[0] - before[0], after[1] - before[1]) == ((1, 0) if rccl else (0, 1))
                for r in range(G):
                    at = all_at[r][k] + sl * G * pix * e
                    host[at:at + G * pix * e] = np.concatenate([views[v][k] for v in sent])
                _assert_same(_download(L, dev, a.size), host, regions, "slot %d kind %d" % (sl, k))
        for k, e in enumerate(elems):   # what the fusion reads: view v at block v
            want = np.concatenate([views[v][k] for v in range(V)])
            assert np.array_equal(host[all_at[0][k]:all_at[0][k] + V * pix * e], want)
    finally:
        L.apd_device_free(0, dev)


@gpu
def test_exchange_refusals(gpu_pkg, exchanges):
    L = _lib2(gpu_pkg)
    x = exchanges(2, 0)
    dev = _malloc(L, 256)
    two = (C.c_void_p * 2)(dev.value, dev.value + 64)
    before = _counts(L, x)
    try:
        for args in ((None, two, two, 16), (x, None, two, 16), (x, two, None, 16)):
            assert L.apd_exchange_allgather(*args) != 0 and b"apd_exchange_allgather" in L.apd_exchange_last_error()
            assert L.apd_exchange_allgather_after(*args, 0, None) != 0 and b"apd_exchange_allgather" in L.apd_exchange_last_error()
        assert _counts(L, x) == before   # a refused call is no exchange
        y = C.c_void_p()
        zero = (C.c_int * 1)(0)
        assert L.apd_exchange_create(C.byref(y), 0, zero, 0) != 0 and b"apd_exchange_create" in L.apd_exchange_last_error()
        assert L.apd_exchange_create(C.byref(y), 1, None, 0) != 0 and b"apd_exchange_create" in L.apd_exchange_last_error()
        assert L.apd_exchange_create(C.byref(y), 1, (C.c_int * 1)(-1), 0) != 0 and b"-1" in L.apd_exchange_last_error()
        assert L.apd_exchange_create(None, 1, zero, 0) != 0 and b"apd_exchange_create" in L.apd_exchange_last_error()
        assert not y.value
        assert L.apd_exchange_destroy(None) == 0
    finally:
        L.apd_device_free(0, dev)


# ---- apd_split_planes_async ---------------------------------------------------------------------------------------------------------

# NaNs with payloads (quiet, signalling, negative), both zeros, denormals, infinities: a copy through arithmetic would change some
SPECIAL_WORDS = np.array([0x7FC12345, 0xFFA00001, 0x7F800001, 0xFFFFFFFF, 0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x007FFFFF,
                          0x7F800000, 0xFF800000, 0x3F800000], np.uint32)


def _planes_words(rng, pixels):
    w = rng.integers(0, 1 << 32, (pixels, 4), dtype=np.uint64).astype(np.uint32)
    flat = w.reshape(-1)
    flat[::3] = SPECIAL_WORDS[np.arange(flat[::3].size) % SPECIAL_WORDS.size]   # every third word, so all four components meet every special
    return w


@gpu
@pytest.mark.parametrize("own_stream", [False, True])
def test_split_planes_async_moves_raw_words(gpu_pkg, own_stream):
    """apd_split_planes_async against planes[:, 3] and planes[:, :3] as uint32 words, on the null stream (GatherFinalMaps) and on a
    stream of apd_stream_create; 0 pixels write nothing; guards around both results; NULL pointers are refused."""
    L = _lib2(gpu_pkg)
    st = _new_stream(L) if own_stream else C.c_void_p(None)
    rng = np.random.default_rng(5)
    try:
        for pixels in (0, 1, 255, 256, 257, 97 * 71):
            a = Arena()
            p_at, d_at, n_at = a.carve(pixels * 16), a.carve(pixels * 4), a.carve(pixels * 12)
            host = a.host()
            words = _planes_words(rng, pixels)
            host[p_at:p_at + pixels * 16] = words.reshape(-1).view(np.uint8)
            host[d_at:d_at + pixels * 4] = RECV_FILL
            host[n_at:n_at + pixels * 12] = RECV_FILL
            dev = _malloc(L, a.size)
            try:
                _upload(L, dev, host)
                assert L.apd_split_planes_async(0, st, dev.value + p_at, pixels, dev.value + d_at, dev.value + n_at) == 0, L.apd_exchange_last_error()
                assert L.apd_stream_synchronize(0, st) == 0
                got = _download(L, dev, a.size)
                host[d_at:d_at + pixels * 4] = np.ascontiguousarray(words[:, 3]).view(np.uint8)
                host[n_at:n_at + pixels * 12] = np.ascontiguousarray(words[:, :3]).reshape(-1).view(np.uint8)
                _assert_same(got, host, [("planes", p_at, pixels * 16), ("depth", d_at, pixels * 4), ("normal", n_at, pixels * 12)], "%d pixels" % pixels)
            finally:
                L.apd_device_free(0, dev)
        dev = _malloc(L, 256)
        for args in ((None, dev, dev), (dev, None, dev), (dev, dev, None)):
            assert L.apd_split_planes_async(0, st, args[0], 1, args[1], args[2]) != 0
            assert b"apd_split_planes_async" in L.apd_exchange_last_error()
        L.apd_device_free(0, dev)
    finally:
        assert L.apd_stream_destroy(0, st) == 0


# ---- apd_rescale_nearest_async ------------------------------------------------------------------------------------------------------

RESCALE_SHAPES = [((155, 103), (310, 207)), ((388, 258), (775, 516)), ((64, 48), (64, 48)), ((775, 516), (1550, 1033)),
                  ((97, 71), (146, 107)), ((146, 107), (97, 71)), ((64, 48), (48, 64)), ((100, 40), (50, 80))]
ZERO_FILLED = {((64, 48), (48, 64)): 1344, ((100, 40), (50, 80)): 3000}   # pixels whose swapped-factor source index leaves the frame


@gpu
@pytest.mark.parametrize("elem,dtype,ch", [(1, np.uint8, 1), (4, np.uint32, 1), (16, np.float32, 4)])
def test_rescale_nearest_async_equals_the_host_restatement(gpu_pkg, elem, dtype, ch):
    """apd_rescale_nearest_async on a stream of its own against the host restatement and against apd_rescale_nearest_device on the
    same input; the two shapes that change the aspect ratio make the swapped factors of RescaleMatToTargetSize leave the frame
    (1344 of 3072 and 3000 of 4000 pixels become 0: asserted, with an input that holds no zero and results pre-filled with 0xEE)."""
    L = _lib2(gpu_pkg)
    st = _new_stream(L)
    rng = np.random.default_rng(9 + elem)
    try:
        for (sw, sh), (dw, dh) in RESCALE_SHAPES:
            src = rng.integers(1, 250, (sh, sw, ch) if ch > 1 else (sh, sw)).astype(dtype)
            want = np.ascontiguousarray(_rescale_reference(src, dw, dh))
            assert want.shape[:2] == (dh, dw) and want.dtype == dtype
            zero_pixels = int((want.reshape(dh * dw, ch) == 0).all(axis=1).sum())
            if ((sw, sh), (dw, dh)) in ZERO_FILLED:   # (the other shapes lose a last row or column at the most)
                assert zero_pixels == ZERO_FILLED[((sw, sh), (dw, dh))], ((sw, sh), (dw, dh), zero_pixels)
            a = Arena()
            s_at, async_at, sync_at = a.carve(src.nbytes), a.carve(want.nbytes), a.carve(want.nbytes)
            host = a.host()
            host[s_at:s_at + src.nbytes] = src.reshape(-1).view(np.uint8)
            host[async_at:async_at + want.nbytes] = RECV_FILL
            host[sync_at:sync_at + want.nbytes] = RECV_FILL
            dev = _malloc(L, a.size)
            try:
                _upload(L, dev, host)
                assert L.apd_rescale_nearest_async(0, st, dev.value + s_at, sw, sh, dev.value + async_at, dw, dh, elem) == 0, L.apd_exchange_last_error()
                assert L.apd_stream_synchronize(0, st) == 0
                assert L.apd_rescale_nearest_device(0, dev.value + s_at, sw, sh, dev.value + sync_at, dw, dh, elem) == 0
                got = _download(L, dev, a.size)
                host[async_at:async_at + want.nbytes] = want.reshape(-1).view(np.uint8)
                host[sync_at:sync_at + want.nbytes] = want.reshape(-1).view(np.uint8)
                _assert_same(got, host, [("source", s_at, src.nbytes), ("async", async_at, want.nbytes), ("device-wide", sync_at, want.nbytes)],
                             "%s -> %s, %d bytes" % ((sw, sh), (dw, dh), elem))
            finally:
                L.apd_device_free(0, dev)
        p, q = _malloc(L, 1024), _malloc(L, 1024)
        bad = [(None, 2, 2, q, 4, 4, elem), (p, 2, 2, None, 4, 4, elem), (p, 0, 2, q, 4, 4, elem), (p, 2, 0, q, 4, 4, elem),
               (p, 2, 2, q, 0, 4, elem), (p, 2, 2, q, 4, 0, elem), (p, -2, 2, q, 4, 4, elem), (p, 2, 2, q, 4, -4, elem), (p, 2, 2, q, 4, 4, 3)]
        for args in bad:
            assert L.apd_rescale_nearest_async(0, st, *args) != 0, args
            assert b"apd_rescale_nearest_async" in L.apd_exchange_last_error()
        assert L.apd_stream_synchronize(0, st) == 0
        L.apd_device_free(0, p)
        L.apd_device_free(0, q)
    finally:
        assert L.apd_stream_destroy(0, st) == 0


# ---- ordered with the caller's stream -----------------------------------------------------------------------------------------------

@gpu
def test_stream_forms_run_behind_the_work_queued_on_their_stream(gpu_pkg):
    """apd_split_planes_async, apd_rescale_nearest_async and apd_device_memcpy_async (device to device) on a torch stream whose queue
    holds a long burn and then the copy that writes their input: called while that copy's event is still pending, followed by
    apd_stream_synchronize of that stream, each must give the function of the late-written input, not of what the buffer held
    before (the shape of test_allgather_after_waits_for_pending_writer_events)."""
    import torch
    L = _lib2(gpu_pkg)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(23)
    pixels, (sw, sh), (dw, dh) = 1 << 18, (775, 516), (1550, 1033)
    burn = torch.randn(4096, 4096, device=dev)
    (burn @ burn).sum().item()   # the library's one-time set-up of the first matrix product, paid before anything is timed against it
    side = torch.cuda.Stream(device=dev)
    seen_pending = 0

    def late_write(target, late):
        with torch.cuda.stream(side):
            acc = burn
            for _ in range(150):         # hundreds of milliseconds of queued work ahead of the write
                acc = acc @ burn
                acc = acc / acc.abs().max()
            target.copy_(late)
            ev = torch.cuda.Event()
            ev.record(side)
        return ev

    def randint(shape):
        return torch.randint(1, 1 << 30, shape, dtype=torch.int32, generator=g).to(dev)

    # apd_split_planes_async
    early, late = randint((pixels, 4)), randint((pixels, 4))
    inp = early.clone()
    depth, normal = torch.zeros(pixels, dtype=torch.int32, device=dev), torch.zeros((pixels, 3), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ev = late_write(inp, late)
    pending = not ev.query()
    assert L.apd_split_planes_async(0, side.cuda_stream, inp.data_ptr(), pixels, depth.data_ptr(), normal.data_ptr()) == 0, L.apd_exchange_last_error()
    assert L.apd_stream_synchronize(0, side.cuda_stream) == 0
    seen_pending += 1 if pending else 0
    assert ev.query()
    assert torch.equal(depth, late[:, 3]) and torch.equal(normal, late[:, :3]), "apd_split_planes_async read its input before the stream wrote it"

    # apd_rescale_nearest_async, 4-byte elements
    early, late = randint((sh, sw)), randint((sh, sw))
    want = torch.from_numpy(np.ascontiguousarray(_rescale_reference(late.cpu().numpy(), dw, dh))).to(dev)
    inp = early.clone()
    out = torch.zeros((dh, dw), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ev = late_write(inp, late)
    pending = not ev.query()
    assert L.apd_rescale_nearest_async(0, side.cuda_stream, inp.data_ptr(), sw, sh, out.data_ptr(), dw, dh, 4) == 0, L.apd_exchange_last_error()
    assert L.apd_stream_synchronize(0, side.cuda_stream) == 0
    seen_pending += 1 if pending else 0
    assert torch.equal(out, want), "apd_rescale_nearest_async read its input before the stream wrote it"

    # apd_device_memcpy_async, device to device
    nbytes = (4 << 20) + 7
    early = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, generator=g).to(dev)
    late = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, generator=g).to(dev)
    inp = early.clone()
    out = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ev = late_write(inp, late)
    pending = not ev.query()
    assert L.apd_device_memcpy_async(0, side.cuda_stream, out.data_ptr(), inp.data_ptr(), nbytes) == 0, L.apd_exchange_last_error()
    assert L.apd_stream_synchronize(0, side.cuda_stream) == 0
    seen_pending += 1 if pending else 0
    assert torch.equal(out, late), "apd_device_memcpy_async read its input before the stream wrote it"
    torch.cuda.synchronize()
    # the wait must have been exercised: the writer's event was still pending when the helper was called
    assert seen_pending >= 2, seen_pending


# ---- apd_device_memcpy_async, streams, host memory, apd_device_memory, apd_image_pixels -------------------------------------------

@gpu
@pytest.mark.parametrize("host_memory", ["apd_host_alloc", "apd_host_register"])
def test_memcpy_async_in_all_three_directions(gpu_pkg, host_memory):
    """apd_device_memcpy_async on a stream of apd_stream_create, host to device, device to device and device to host, 0, 1, 4097 and
    6887 bytes, out of and into page-locked memory of apd_host_alloc or a numpy array under apd_host_register; apd_stream_synchronize
    before every read; guards on the host and on the device."""
    L = _lib2(gpu_pkg)
    st = _new_stream(L)
    cap = 2 * GUARD + 6887
    if host_memory == "apd_host_alloc":
        pinned = C.c_void_p()
        assert L.apd_host_alloc(2 * cap, C.byref(pinned)) == 0 and pinned.value, L.apd_exchange_last_error()
        both = np.ctypeslib.as_array(C.cast(pinned, C.POINTER(C.c_uint8)), (2 * cap,))
    else:
        both = np.empty(2 * cap, np.uint8)   # one registration: the two halves share pages
        assert L.apd_host_register(_host_ptr(both), 2 * cap) == 0, L.apd_exchange_last_error()
    up, down = both[:cap], both[cap:]
    rng = np.random.default_rng(77)
    try:
        for nbytes in (0, 1, 4097, 6887):
            a = Arena()
            first_at, second_at = a.carve(nbytes, 1), a.carve(nbytes, 3)   # odd addresses on the device
            dev = _malloc(L, a.size)
            try:
                host = a.host()
                host[first_at:first_at + nbytes] = RECV_FILL
                host[second_at:second_at + nbytes] = RECV_FILL
                _upload(L, dev, host)
                payload = rng.integers(1, 0x80, nbytes, dtype=np.uint8)
                up[:] = GUARD_BYTE
                up[GUARD:GUARD + nbytes] = payload
                down[:] = GUARD_BYTE
                assert L.apd_device_memcpy_async(0, st, dev.value + first_at, up.ctypes.data + GUARD, nbytes) == 0, L.apd_exchange_last_error()
                assert L.apd_device_memcpy_async(0, st, dev.value + second_at, dev.value + first_at, nbytes) == 0, L.apd_exchange_last_error()
                assert L.apd_device_memcpy_async(0, st, down.ctypes.data + GUARD, dev.value + second_at, nbytes) == 0, L.apd_exchange_last_error()
                assert L.apd_stream_synchronize(0, st) == 0
                want_down = np.full(cap, GUARD_BYTE, np.uint8)
                want_down[GUARD:GUARD + nbytes] = payload
                assert np.array_equal(down, want_down), nbytes
                host[first_at:first_at + nbytes] = payload
                host[second_at:second_at + nbytes] = payload
                _assert_same(_download(L, dev, a.size), host, [("first", first_at, nbytes), ("second", second_at, nbytes)], "%d bytes" % nbytes)
            finally:
                L.apd_device_free(0, dev)
    finally:
        assert L.apd_stream_synchronize(0, st) == 0
        if host_memory == "apd_host_alloc":
            del up, down, both
            assert L.apd_host_free(pinned) == 0
        else:
            assert L.apd_host_unregister(_host_ptr(both)) == 0
        assert L.apd_stream_destroy(0, st) == 0


@gpu
def test_stream_and_host_memory_refusals_device_memory_and_image_pixels(gpu_pkg):
    L = _lib2(gpu_pkg)
    p = C.c_void_p()
    assert L.apd_host_alloc(0, C.byref(p)) != 0 and b"apd_host_alloc" in L.apd_exchange_last_error()
    assert L.apd_host_alloc(16, None) != 0 and b"apd_host_alloc" in L.apd_exchange_last_error()
    assert L.apd_host_register(None, 16) != 0 and b"apd_host_register" in L.apd_exchange_last_error()
    assert L.apd_host_free(None) == 0 and L.apd_host_unregister(None) == 0
    assert L.apd_stream_create(0, None) != 0 and b"apd_stream_create" in L.apd_exchange_last_error()
    assert L.apd_stream_destroy(0, None) == 0
    # apd_device_memory
    free, total = C.c_size_t(), C.c_size_t()
    assert L.apd_device_memory(0, C.byref(free), C.byref(total)) == 0 and 0 < free.value <= total.value
    only_free, only_total = C.c_size_t(), C.c_size_t()
    assert L.apd_device_memory(0, C.byref(only_free), None) == 0 and 0 < only_free.value <= total.value
    assert L.apd_device_memory(0, None, C.byref(only_total)) == 0 and only_total.value == total.value
    assert L.apd_device_memory(0, None, None) == 0
    assert L.apd_device_memory(99, C.byref(free), C.byref(total)) != 0 and L.apd_exchange_last_error()
    # apd_image_pixels: the float plane of an image on the device.  Created right behind the refused device 99: the runtime used to keep
    # that call's error for the thread's next hipGetLastError(), and apd_image_create's first launch failed with "invalid device ordinal"
    W, H = 97, 71
    pixels = (np.random.default_rng(2).random((H, W), dtype=np.float32) * np.float32(255.0)).astype(np.float32)
    im = gpu_pkg.SharedImage(W, H, pixels)
    try:
        plane = L.apd_image_pixels(im.ptr)
        assert plane
        got = np.empty((H, W), np.float32)
        assert L.apd_device_memcpy(0, _host_ptr(got), plane, got.nbytes) == 0
        assert np.array_equal(got.view(np.uint32), pixels.view(np.uint32))
    finally:
        im.close()
    assert L.apd_image_pixels(None) is None


# ---- apd_set_stream / apd_get_stream ------------------------------------------------------------------------------------------------

@gpu
def test_set_stream_runs_the_same_pass_on_the_callers_stream(gpu_pkg, ob, synth):
    """A FIRST_INIT pass of two iterations on the handle's own stream and on a stream of apd_stream_create given to apd_set_stream:
    every state array bit-identical between the two, and equal to the oracle's; apd_get_stream names the stream in use; an export
    of the handle on the set stream and a torch clone queued on that stream (torch.cuda.ExternalStream) agree after one final
    synchronisation; the stream is destroyed after the handle."""
    import torch
    import common
    L = _lib2(gpu_pkg)
    W, H, N = 64, 48, 2
    sc, imgs = common.scene_inputs(synth, W, H, N)
    p = common.base_params(sc, N, state=gpu_pkg.FIRST_INIT, max_iterations=2)
    cams = [gpu_pkg.make_camera(sc.K[i], sc.R[i], sc.t[i], W, H, sc.depth_min, sc.depth_max) for i in range(N + 1)]
    st = _new_stream(L)
    own = gpu_pkg.Handle(W, H, gpu_pkg.default_params(**p), device=0)
    other = gpu_pkg.Handle(W, H, gpu_pkg.default_params(**p), device=0)
    o = common.make_oracle(ob, sc, imgs, N, p)
    try:
        got = C.c_void_p()
        assert L.apd_get_stream(own._h, C.byref(got)) == 0 and got.value
        own_stream = got.value
        assert L.apd_get_stream(other._h, C.byref(got)) == 0 and got.value and got.value not in (own_stream, st.value)
        assert L.apd_set_stream(other._h, st) == 0, L.apd_last_error()
        assert L.apd_get_stream(other._h, C.byref(got)) == 0 and got.value == st.value
        assert L.apd_get_stream(own._h, C.byref(got)) == 0 and got.value == own_stream
        assert L.apd_set_stream(None, st) != 0 and b"apd_set_stream" in L.apd_last_error()
        assert L.apd_get_stream(None, C.byref(got)) != 0 and b"apd_get_stream" in L.apd_last_error()
        assert L.apd_get_stream(own._h, None) != 0 and b"apd_get_stream" in L.apd_last_error()
        for h in (own, other):
            h.upload_views(cams, imgs)
            h.run()
        o.run()
        for name, hs, _ in common.ORACLE_STATES:
            if name == "neighbours" and own.weak_count == 0:
                continue
            a, b = own.state(getattr(gpu_pkg, hs)), other.state(getattr(gpu_pkg, hs))
            assert np.array_equal(common.bits(a), common.bits(b)), name
        assert own.weak_count == other.weak_count
        common.assert_state_equal(gpu_pkg, other, o, "on the set stream")
        depth = torch.empty((H, W), device="cuda", dtype=torch.float32)
        normal = torch.empty((H, W, 3), device="cuda", dtype=torch.float32)
        other.export_depth_normal(depth, normal)
        with torch.cuda.stream(torch.cuda.ExternalStream(st.value)):   # queued behind the export, no host synchronisation in between
            depth_clone, normal_clone = depth.clone(), normal.clone()
        assert L.apd_stream_synchronize(0, st) == 0
        assert torch.equal(depth_clone.view(torch.int32), depth.view(torch.int32))
        assert torch.equal(normal_clone.view(torch.int32), normal.view(torch.int32))
        planes = other.state(gpu_pkg.STATE_PLANES)
        assert np.isfinite(depth_clone.cpu().numpy()).all() and planes.shape == (H, W, 4)
    finally:
        own.close()
        other.close()
        o.close()
        assert L.apd_stream_destroy(0, st) == 0   # after the handle that used it
