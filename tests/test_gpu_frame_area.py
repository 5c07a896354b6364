"""HIP path vs CPU oracle on frames with BOTH axes large: 8192 x 8200 (2^26 px) ... 16384 x 16382, the largest apd_create accepts.

tests/frame_area_cases.py lists which 32-bit products of which device array reach 2^31 and 2^32 on these frames and at which
pixel; the oracle windows sit on those pixels' rows, on the first rows and on the last rows of the frame.  The mechanism is the
one of tests/test_gpu_fullsize_parity.py: the HIP kernel runs the whole frame, the oracle (orc_set_roi) the same kernel on the
windows from the HIP path's own pre-kernel state, and every array of common.ORACLE_STATES is compared inside the windows as raw
bits after EVERY kernel (a float word that is NaN on both sides compares equal, as in tests/test_gpu_frame_limits.py).

Whole-array downloads of a 268-Mpix frame (27 GB of state per kernel) do not fit a test: the state moves in BANDS, each window
grown by BAND px on all sides.  apd_download_state copies an array into a device scratch buffer, the band is cut out on the
device and only that goes to the host and into the oracle.  BAND covers what a window's kernels read around it: K2 looks 100 px
around a WEAK pixel, the propagation of K6 / K7 25 px, K3 walks to the nearest STRONG pixels (a few px on the crafted WEAK
stripes; the accepted neighbours are checked to lie inside the band).

Images: a tiled texture with the rows around the windows rendered from the camera ring of the 16384-px frames of
tests/frame_limits_cases.py (frame_area_cases.images); N = 2 sources, which runs the full path of every kernel.

Lines starting with FRAME_AREA carry the figures the tests measured, from the oracle's windows alone: the share of costs below 2
after K6, the WEAK pixels after K14, the bytes every kernel changed (profiles/frame_limits/test_times.txt)."""
import time

import numpy as np
import pytest

import common
import frame_area_cases as fa
import frame_limits_cases as fl
from test_gpu_frame_limits import OTHER_ARM, TILED_EVERYWHERE

pytestmark = pytest.mark.gpu

N = 2
BAND = 128
ARMS = {"default": {}, "other-arm": OTHER_ARM, "tiled-everywhere": TILED_EVERYWHERE}
_WEAK_KERNELS = (3, 4, 9, 10)


# ---- inputs, one frame at a time -----------------------------------------------------------------------------------------------

_CASE = {}


def _case(synth, frame, floats):
    key = (frame, floats)
    if key not in _CASE:
        _CASE.clear()   # the images of C are 3.2 GB
        W, H = fa.FRAMES[frame]
        sc = fa.cameras(synth, W, H, N)
        wins = fa.windows(W, H)
        _CASE[key] = dict(sc=sc, wins=wins, imgs=fa.images(sc, N, wins, floats), priors={})
    return _CASE[key]


def _require_memory(W, H, floats, options, geom):
    """Fails (never skips) when the card cannot hold the frame: the state arrays (107 bytes per pixel), N + 1 images with their
    copies, the depth maps, the 32-byte-per-pixel scratch of the band downloads and the prior of the next pass."""
    import torch
    free, _ = torch.cuda.mem_get_info(0)
    fquads = floats or options.get("source_quads", 1) == 0
    per_px = 107 + (N + 1) * (4 + (16 if fquads else 5)) + (4 * (N + 1) if geom else 0) + 32 + 21
    need = per_px * W * H + (1 << 30)
    assert free >= need, "the device has %.1f GB free, a %d x %d frame needs about %.1f GB" % (free / 2**30, W, H, need / 2**30)
    return free


def _handle(pkg, case, p, options, prior=None, depths=None, floats=False, label=""):
    import torch
    W, H = case["sc"].width, case["sc"].height
    before = _require_memory(W, H, floats, options, depths is not None)
    h = common.make_handle(pkg, case["sc"], case["imgs"], N, p, depths=depths, prior=prior, options=options)
    h.synchronize()
    after, _ = torch.cuda.mem_get_info(0)
    print("FRAME_AREA %s: device footprint of the handle %.2f GB (%.1f bytes per pixel)" % (label, (before - after) / 2**30, (before - after) / (W * H)))
    return h


def _first_pass_prior(pkg, case, floats, options):
    """Planes, selected views and the crafted WEAK map (5 columns of 48) for the APD passes: one FIRST_INIT pass of one iteration
    on the HIP path over the whole frame, common.postprocess in place."""
    key = tuple(sorted(options.items()))
    if key not in case["priors"]:
        case["priors"].clear()
        sc = case["sc"]
        p = common.base_params(sc, N, seed=41, max_iterations=1, **fl.PASSES[0])
        h = _handle(pkg, case, p, options, floats=floats, label="%dx%d prior" % (sc.width, sc.height))
        h.run()
        planes, weak, views = h.download()
        h.close()
        d = planes[..., 3]
        bad = (d < p["depth_min"]) | (d > p["depth_max"])
        d[bad] = 0
        weak[:] = fl.STRONG
        weak[:, fa.weak_stripes(sc.width, sc.height)] = fl.WEAK
        weak[bad] = fl.UNKNOWN
        case["priors"][key] = (planes, views, weak)
    return case["priors"][key]


# ---- lock-step on bands ----------------------------------------------------------------------------------------------------------

class _Bands:
    """Moves the bands of a handle's state arrays to the host: a device-to-device apd_download_state into one scratch buffer,
    the bands cut out on the device."""

    def __init__(self, pkg, h, bands):
        import torch
        self.pkg, self.h, self.bands, self.L = pkg, h, bands, pkg.lib()
        self.scratch = torch.empty(32 * h.W * h.H, dtype=torch.uint8, device="cuda:0")

    def _fill(self, which):
        nbytes = self.L.apd_state_bytes(self.h._h, which)
        assert 0 < nbytes <= self.scratch.numel()
        rc = self.L.apd_download_state(self.h._h, which, self.scratch.data_ptr(), nbytes)
        assert rc == 0, self.L.apd_last_error()
        return nbytes

    def pixel_state(self, which, like):
        """The bands of one per-pixel array, each shaped and typed as `like[y0:y1, x0:x1]`."""
        nbytes = self._fill(which)
        H, W = self.h.H, self.h.W
        bpp = nbytes // (W * H)
        assert bpp * W * H == nbytes and bpp == like.dtype.itemsize * int(np.prod(like.shape[2:]))
        rows = self.scratch[:nbytes].view(H, W * bpp)
        out = []
        for (x0, y0, x1, y1) in self.bands:
            a = rows[y0:y1, x0 * bpp:x1 * bpp].contiguous().cpu().numpy()
            out.append(a.view(like.dtype).reshape((y1 - y0, x1 - x0) + like.shape[2:]))
        return out

    def neighbour_rows(self, index):
        """Rows `index` (a device tensor) of the neighbour table."""
        nbytes = self._fill(self.pkg.STATE_NEIGHBOURS)
        table = self.scratch[:nbytes].view(-1, 36)
        return table[index].cpu().numpy().view(np.int16).reshape(-1, 9, 2)


def _lockstep(pkg, h, o, schedule, wins, label, apd, prior_weak=None):
    """common.fullsize_lockstep on bands.  Returns (kernels compared, figures): per kernel and window the bytes the ORACLE changed
    inside the window, the share of costs below 2 after K6, the WEAK pixels after K14."""
    import torch
    W, H = h.W, h.H
    bands = fa.bands(wins, W, H, BAND)
    mover = _Bands(pkg, h, bands)
    inner = [(x0 - bx0, y0 - by0, x1 - bx0, y1 - by0) for (x0, y0, x1, y1), (bx0, by0, _, _) in zip(wins, bands)]
    weak = h.weak_count > 0
    states = [s for s in common.ORACLE_STATES if s[0] != "neighbours"]
    if weak:
        nmap = o.neighbours_map
        got = mover.pixel_state(pkg.STATE_NEIGHBOURS_MAP, nmap)
        for b, a in zip(bands, got):
            assert np.array_equal(a, nmap[b[1]:b[3], b[0]:b[2]]), "%s: neighbours_map differs in band %s" % (label, b)
        band_rows = np.unique(np.concatenate([nmap[b[1]:b[3], b[0]:b[2]][prior_weak[b[1]:b[3], b[0]:b[2]] == fl.WEAK] for b in bands]))
        win_rows = [nmap[w[1]:w[3], w[0]:w[2]][prior_weak[w[1]:w[3], w[0]:w[2]] == fl.WEAK] for w in wins]
        win_pos = [np.searchsorted(band_rows, r) for r in win_rows]
        band_rows_dev = torch.from_numpy(band_rows.astype(np.int64)).to("cuda:0")

    def sync():
        """HIP bands -> host; returns them and writes them into the oracle after the comparison (load)."""
        snap = {name: mover.pixel_state(getattr(pkg, hs), getattr(o, oa)) for name, hs, oa in states}
        if weak:
            snap["neighbours"] = mover.neighbour_rows(band_rows_dev)
        return snap

    def load(snap):
        for name, _, oa in states:
            arr = getattr(o, oa)
            for b, a in zip(bands, snap[name]):
                arr[b[1]:b[3], b[0]:b[2]] = a
        if weak:
            o.neighbours[band_rows] = snap["neighbours"]

    def oracle_windows():
        out = {name: [getattr(o, oa)[w[1]:w[3], w[0]:w[2]].copy() for w in wins] for name, _, oa in states}
        if weak:
            nb = o.neighbours
            out["neighbours"] = [nb[r].copy() for r in win_rows]
        return out

    load(sync())
    figures = dict(changed={}, cost_share=[], weak_after_k14=None, weak_before={}, times={})
    compared = 0
    for kid, it in schedule:
        where = "%s after K%d(iter %d)" % (label, kid, it)
        before = oracle_windows()
        t0 = time.perf_counter()
        h.run_kernel(kid, it)
        t1 = time.perf_counter()
        for (x0, y0, x1, y1) in wins:
            o.set_roi(x0, y0, x1, y1)
            o.run_kernel(kid, it)
        o.set_roi()
        t2 = time.perf_counter()
        after = oracle_windows()
        figures["changed"][(kid, it)] = [sum(int((common.canon_nan(before[n][i]) != common.canon_nan(after[n][i])).sum()) for n in after)
                                         for i in range(len(wins))]
        figures["weak_before"][(kid, it)] = [int((b == fl.WEAK).sum()) for b in before["weak"]]
        if kid == 6:
            figures["cost_share"].append([float((c < 2.0).mean()) for c in after["costs"]])
        if kid == 14:
            figures["weak_after_k14"] = [int((x == fl.WEAK).sum()) for x in after["weak"]]
        snap = sync()
        for name in after:
            for i, w in enumerate(wins):
                if name == "neighbours":
                    a = snap[name][win_pos[i]]
                else:
                    ix0, iy0, ix1, iy1 = inner[i]
                    a = snap[name][i][iy0:iy1, ix0:ix1]
                b = after[name][i]
                if not np.array_equal(common.canon_nan(a), common.canon_nan(b)):
                    neq = common.canon_nan(a).reshape(a.shape[0], -1) != common.canon_nan(b).reshape(a.shape[0], -1)
                    first = np.argwhere(neq.reshape(a.shape[0], -1))[0]
                    raise AssertionError("%s: HIP and oracle differ in `%s` on window %s (%d bytes), first at row %d, byte %d of the window"
                                         % (where, name, w, int(neq.sum()), int(first[0]), int(first[1])))
        if kid == 3:
            # what K4, K8, K9 and K10 read through the table must lie inside the band
            for i, w in enumerate(wins):
                nb = after["neighbours"][i].astype(np.int32)
                reach = np.abs(nb[:, 1:, :] - nb[:, :1, :])[nb[:, 1:, 0] >= 0]
                assert reach.size == 0 or int(reach.max()) <= BAND, (where, w, int(reach.max()))
        load(snap)
        compared += 1
        figures["times"][(kid, it)] = (t1 - t0, t2 - t1, time.perf_counter() - t2)
    del mover
    torch.cuda.empty_cache()
    return compared, figures


def _assert_not_vacuous(figures, wins, label, apd):
    """Every window, from the oracle alone: a majority of costs below 2 after K6, more than 50 WEAK pixels after K14 of an APD pass,
    and every kernel at work: it changed bytes inside the window (K4 only demotes WEAK pixels K3 found no neighbours for; it is at
    work on a window that holds WEAK pixels)."""
    for share in figures["cost_share"]:
        assert min(share) > 0.5, (label, share)
    print("FRAME_AREA %s: share of costs below 2 after K6 per window, first iteration: %s" % (label, " ".join("%.3f" % s for s in figures["cost_share"][0])))
    if apd:
        assert min(figures["weak_after_k14"]) > 50, (label, figures["weak_after_k14"])
    print("FRAME_AREA %s: WEAK pixels after K14 per window: %s" % (label, figures["weak_after_k14"]))
    for (kid, it), changed in figures["changed"].items():
        if kid == 4:
            assert min(figures["weak_before"][(kid, it)]) > 0, (label, kid, figures["weak_before"][(kid, it)])
        else:
            assert min(changed) > 0, (label, "K%d(iter %d) changed nothing in window %s" % (kid, it, wins[int(np.argmin(changed))]))
    print("FRAME_AREA %s: fewest bytes a kernel changed in a window: %s" % (label, " ".join("K%d.%d:%d" % (k, i, min(c)) for (k, i), c in figures["changed"].items())))
    hip = sum(t[0] for t in figures["times"].values())
    orc = sum(t[1] for t in figures["times"].values())
    mv = sum(t[2] for t in figures["times"].values())
    print("FRAME_AREA %s: %d kernels, %d windows; HIP %.2f s, oracle windows %.2f s, band moves and comparison %.2f s" % (label, len(figures["times"]), len(wins), hip, orc, mv))


PASS_KINDS = {"first": 0, "apd": 1, "geom": 2}

# (frame, pass kind, arm, float images): A runs the three pass kinds; B, C and C' FIRST_INIT and one APD pass (K14 / K15, the weak
# kernels); A and C the other arm of every bit-preserving option; A float images
CASES = ([("A", k, "default", False) for k in ("first", "apd", "geom")]
         + [(f, k, "default", False) for f in ("B", "C", "Ct") for k in ("first", "apd")]
         + [(f, k, arm, False) for f in ("A", "C") for arm in ("other-arm", "tiled-everywhere") for k in ("first", "apd")]
         + [("A", k, "default", True) for k in ("first", "apd")])
CASES.sort(key=lambda c: (c[0], c[3]))   # one frame's images at a time


@pytest.mark.parametrize("frame,kind,arm,floats", CASES, ids=["%s-%s-%s-%s" % (f, k, a, "float" if fl_ else "u8") for f, k, a, fl_ in CASES])
def test_frame_area_lockstep(gpu_pkg, ob, synth, frame, kind, arm, floats):
    """One pass kind on one frame on one arm: FIRST_INIT (K1, K2, K5, K6..K8, K11..K15), REFINE_INIT + APD or REFINE_ITER + APD +
    geometric term (K1..K5, K6..K10, K11..K15), one iteration, every kernel compared on every window."""
    t_start = time.perf_counter()
    case = _case(synth, frame, floats)
    sc, wins = case["sc"], case["wins"]
    W, H = sc.width, sc.height
    options = ARMS[arm]
    pi = PASS_KINDS[kind]
    label = "%s %dx%d %s %s %s" % (frame, W, H, kind, arm, "float" if floats else "8-bit")
    p = common.base_params(sc, N, seed=41 + pi, max_iterations=1, **fl.PASSES[pi])
    prior = _first_pass_prior(gpu_pkg, case, floats, options) if pi else None
    deps = None
    if pi == 2:
        deps = [np.ascontiguousarray(prior[0][..., 3])] + fa.depth_maps(W, H, N)
    h = _handle(gpu_pkg, case, p, options, prior=prior, depths=deps, floats=floats, label=label)
    o = common.make_oracle(ob, sc, case["imgs"], N, p, depths=deps, prior=prior)
    try:
        assert h.weak_count == o.weak_count
        assert (h.weak_count > 0) == bool(pi)
        sched = fl.schedule(1, h.weak_count > 0)
        n, figures = _lockstep(gpu_pkg, h, o, sched, wins, label, bool(pi), prior[2] if pi else None)
        assert n == len(sched) == (15 if pi else 11)
        _assert_not_vacuous(figures, wins, label, bool(pi))
    finally:
        h.close()
        o.close()
    print("FRAME_AREA %s: test time %.1f s" % (label, time.perf_counter() - t_start))
