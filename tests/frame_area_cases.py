"""What can wrap on a frame with both axes large, and where: shared by tests/test_frame_area_cases.py (CPU) and
tests/test_gpu_frame_area.py (HIP path vs oracle windows on 2^26 px ... the largest frame apd_create accepts).

ARRAYS lists every per-pixel or per-texel device array of a handle with its element size, its bytes per entry and the grid it
is laid out on, read from csrc/ (each entry cites the line).  For a frame W x H, crossings() gives for each array the first
entry at which the byte offset, the element index and the row-pitch product reach 2^31 and 2^32, and the frame row that entry
belongs to; windows() places one oracle window (two where the crossing sits at a row end) on every such row, plus the first
and the last rows of the frame.  Nothing here touches the device."""
import numpy as np

import frame_limits_cases as fl

PATCH_RADIUS = 5          # kPatchRadius, csrc/apd_device.h:662: an 11 x 11 px patch reads 5 rows on both sides of its pixel
# rows on both sides of a crossing row inside its window: the larger of "two rows" and the patch radius + the second bilinear tap
ROW_MARGIN = max(2, PATCH_RADIUS + 1)
WINDOW_W = 128
THRESHOLDS = (1 << 31, 1 << 32)

# grid: "pixel" = W x H entries, row pitch W; "quad" = (W + 1) x (H + 1) entries, entry (qx + 1, qy + 1) for qx, qy >= -1;
# "pairs" = (W + 2) x (H + 1) 2-byte column pairs; "tiled" = 128-byte tiles of 7 x 8 pairs, ceil((W + 2) / 7) tiles per tile row;
# "weak" = one entry per WEAK pixel of the prior, in raster order.
# (name, element bytes, bytes per entry, grid, where it is declared / sized / indexed)
ARRAYS = [
    # common.ORACLE_STATES (kPixelState)
    ("costs", 4, 4, "pixel", "apd_capi.hip:199"),
    ("rng", 4, 24, "pixel", "apd_capi.hip:200"),
    ("selected_views", 4, 4, "pixel", "apd_capi.hip:201"),
    ("view_weight", 1, 32, "pixel", "apd_capi.hip:202, apd_sweep.h:135 (center * APD_MAX_IMAGES, as uint4)"),
    ("planes", 16, 16, "pixel", "apd_capi.hip:203"),
    ("fit_planes", 16, 16, "pixel", "apd_capi.hip:204"),
    ("weak_info", 1, 1, "pixel", "apd_capi.hip:205"),
    ("weak_reliable", 1, 1, "pixel", "apd_capi.hip:206"),
    ("nearest_strong", 4, 4, "pixel", "apd_capi.hip:207"),
    ("column_nearest", 1, 1, "pixel", "apd_capi.hip:208"),
    ("neighbours_map", 4, 4, "pixel", "apd_capi.hip:209"),
    ("neighbours", 4, 36, "weak", "apd_capi.hip:144, :215; apd_kernels_weak.hip:158 (neighbours_map[center] * APD_NEIGHBOUR_NUM)"),
    ("weak_list", 4, 4, "weak", "apd_capi.hip:147, :934"),
    ("mask", 1, 1, "pixel", "apd_capi.hip:165, :872"),
    # the image copies of the reference and of every source
    ("img (float)", 4, 4, "pixel", "apd_capi.hip:79, :620; apd_device.h:530 (__mul24(y, W)); apd_window.h:174"),
    ("pairs (byte)", 2, 2, "pairs", "apd_capi.hip:80; apd_device.h:37-39 (pitch 2 (W + 2)), :649 entry_byte_offset<1>"),
    ("tiled (byte)", 2, 2, "tiled", "apd_capi.hip:80; apd_device.h:610-619 quad_tiled_offset_tu"),
    ("fquads (float quad)", 16, 16, "quad", "apd_capi.hip:81; apd_device.h:71, :856 (pitch (W + 1) << 4), :649 entry_byte_offset<4>"),
    # the geometric pass
    ("depths", 4, 4, "pixel", "apd_capi.hip:131, :623"),
]

A = (8192, 8200)      # just past 2^26 px
B = (16384, 8200)     # just past 2^27 px
C = (16384, 16382)    # the largest frame apd_create accepts
CT = (16382, 16384)   # its transpose: the row pitch and the tiled copy's division see the other axis long
FRAMES = {"A": A, "B": B, "C": C, "Ct": CT}


def grid_shape(grid, W, H):
    """(entries per row, rows) of a row-major grid."""
    if grid == "pixel":
        return W, H
    if grid == "quad":
        return W + 1, H + 1
    if grid == "pairs":
        return W + 2, H + 1
    raise ValueError(grid)


def _ceil_div(a, b):
    return -(-a // b)


def crossings(W, H, weak_entries=0):
    """Every (array, quantity, threshold) that is reached on a W x H frame: a list of dicts with the first entry index at which
    the quantity reaches the threshold and the frame pixel (x, y) the entry belongs to.  Quantities: "byte offset" =
    entry * bytes per entry, "element index" = entry * (bytes per entry / element bytes), "row pitch" = row * bytes per row (the
    product the kernels form before the column is added)."""
    out = []
    for name, elem, bpe, grid, cite in ARRAYS:
        if grid == "weak":
            # indexed by WEAK pixel: which frame row a crossing lies in depends on the WEAK map; reported by entry only
            for thr in THRESHOLDS:
                first = _ceil_div(thr, bpe)
                if first < weak_entries:
                    out.append(dict(array=name, quantity="byte offset", threshold=thr, entry=first, x=None, y=None, cite=cite))
            continue
        if grid == "tiled":
            tiles_x, tiles_y = _ceil_div(W + 2, 7), _ceil_div(H + 1, 8)
            for thr in THRESHOLDS:
                tile = _ceil_div(thr, 128)
                if tile < tiles_x * tiles_y:
                    u, t = 8 * (tile // tiles_x), 7 * (tile % tiles_x)
                    out.append(dict(array=name, quantity="byte offset", threshold=thr, entry=tile, x=min(max(t - 1, 0), W - 1),
                                    y=min(max(u - 1, 0), H - 1), cite=cite))
            continue
        pitch, rows = grid_shape(grid, W, H)
        n = pitch * rows
        shift = 0 if grid == "pixel" else 1   # entry (t, u) = (qx + 1, qy + 1)
        firsts = [("byte offset", thr, _ceil_div(thr, bpe)) for thr in THRESHOLDS]
        if bpe != elem:
            firsts += [("element index", thr, _ceil_div(thr, bpe // elem)) for thr in THRESHOLDS]
        firsts += [("row pitch", thr, _ceil_div(thr, pitch * bpe) * pitch) for thr in THRESHOLDS]
        for quantity, thr, first in firsts:
            if first < n:
                x, y = first % pitch - shift, first // pitch - shift
                out.append(dict(array=name, quantity=quantity, threshold=thr, entry=first, x=min(max(x, 0), W - 1),
                                y=min(max(y, 0), H - 1), cite=cite))
    return out


def crossing_pixels(W, H):
    """The distinct frame pixels (x, y) of crossings(W, H), in raster order."""
    return sorted({(c["x"], c["y"]) for c in crossings(W, H) if c["y"] is not None}, key=lambda p: (p[1], p[0]))


def crossing_rows(W, H):
    return sorted({y for _, y in crossing_pixels(W, H)})


def _rows_around(y, H):
    return max(y - ROW_MARGIN, 0), min(y + ROW_MARGIN + 1, H)


def windows(W, H):
    """Oracle windows (x0, y0, x1, y1) of a frame, disjoint: the first rows at the left end and the last rows at the right end
    (the last window holds the last pixel of the frame), and for every crossing pixel ROW_MARGIN rows on both sides of its row,
    WINDOW_W px around its column.  The entry before a crossing at a row's first columns is the END of the row above: such a
    crossing gets a second window at the right end of the same rows (and one at a row's last columns one at the left end)."""
    mid = []
    for x, y in crossing_pixels(W, H):
        y0, y1 = _rows_around(y, H)
        x0 = min(max(x - WINDOW_W // 2, 0), W - WINDOW_W)
        cand = [(x0, y0, x0 + WINDOW_W, y1)]
        if x < ROW_MARGIN + 1:
            cand.append((W - WINDOW_W, y0, W, y1))
        if x >= W - ROW_MARGIN - 1:
            cand.append((0, y0, WINDOW_W, y1))
        mid += cand
    wins = [(0, 0, WINDOW_W, 2 * ROW_MARGIN + 1)]
    for w in mid + [(W - WINDOW_W, H - 2 * ROW_MARGIN - 1, W, H)]:
        hit = [i for i, d in enumerate(wins) if not (w[2] <= d[0] or d[2] <= w[0] or w[3] <= d[1] or d[3] <= w[1])]
        if not hit:
            wins.append(w)
        elif len(hit) == 1 and wins[hit[0]][0] == w[0] and wins[hit[0]][2] == w[2]:
            # two crossings in the same columns and overlapping rows (or a crossing in the frame's last rows): one window over both
            d = wins[hit[0]]
            wins[hit[0]] = (d[0], min(d[1], w[1]), d[2], max(d[3], w[3]))
        # any other overlap: the window placed first stays (tests/test_frame_area_cases.py checks that every crossing still has
        # its rows and columns inside one window)
    return wins


def bands(wins, W, H, margin):
    """Every window grown by `margin` px on all sides, clipped to the frame: what the oracle needs of the frame's state to run
    the window (K2 looks 100 px around a WEAK pixel, the propagation 25 px, K3 as far as the nearest STRONG pixel)."""
    return [(max(x0 - margin, 0), max(y0 - margin, 0), min(x1 + margin, W), min(y1 + margin, H)) for (x0, y0, x1, y1) in wins]


# ---- cheap images ------------------------------------------------------------------------------------------------------------

BASELINE = 7.5e-4   # the camera ring of frame_limits' 16384-px frames: at f = 0.9 W the default puts projections rows away
RENDER_ROWS = 48    # rendered rows on both sides of a window: its patches and their projections in the sources (< 20 px parallax)


def cameras(synth, W, H, N):
    """K, R, t of synth.make_scene(W, H, N, seed=3, baseline=BASELINE) without its W x H rendering: the poses do not depend on
    the frame size, the intrinsics are f = 0.9 W, cx = W / 2, cy = H / 2.  One change: make_scene puts its sources up to 0.02
    scene units in FRONT of the reference whatever the baseline, a 1 % zoom, which at 8000 rows from the principal point moves
    every sample of the frame's first and last rows 40 px and more out of both sources (every cost there is 2).  The sources
    keep their place on the ring and their rotation and stand in the reference's plane z = 0."""
    sc = synth.make_scene(16, 16, N, seed=3, baseline=BASELINE)
    for k in range(1, N + 1):
        R = sc.R[k].astype(np.float64).reshape(3, 3)
        c = -R.T @ sc.t[k].astype(np.float64)
        c[2] = 0.0
        sc.t[k] = (-R @ c).astype(np.float32)
    K = np.array([0.9 * W, 0, 0.5 * W, 0, 0.9 * W, 0.5 * H, 0, 0, 1], np.float32)
    sc.K = [K.copy() for _ in range(N + 1)]
    sc.width, sc.height = W, H
    sc.images, sc.gt_depth = [], None
    return sc


def _render_rows(sc, k, y0, y1):
    """Rows [y0, y1) of view k of a textured plane n.P + d = 0 seen by the scene's cameras, float64 on the host: the sources of a
    window are images of the surface its reference pixels show (make_scene's first plane, four sine products, low-texture
    stripes)."""
    W = sc.width
    K = sc.K[k].astype(np.float64)
    R = sc.R[k].astype(np.float64).reshape(3, 3)
    c = -R.T @ sc.t[k].astype(np.float64)
    xs = (np.arange(W, dtype=np.float64) - K[2]) / K[0]
    ys = (np.arange(y0, y1, dtype=np.float64) - K[5]) / K[4]
    dw = [R[0, i] * xs[None, :] + R[1, i] * ys[:, None] + R[2, i] for i in range(3)]
    n, d = np.array([-0.15, -0.10, 1.0]), -2.0
    s = -(n @ c + d) / (n[0] * dw[0] + n[1] * dw[1] + n[2] * dw[2])
    X, Y = c[0] + s * dw[0], c[1] + s * dw[1]
    pix = 2.0 / K[0]
    tex = np.zeros_like(X)
    for lam, phi, amp in ((5.0, 0.4, 38.0), (9.0, 1.3, 30.0), (17.0, 2.1, 24.0), (31.0, 2.9, 18.0)):
        w = 2 * np.pi / (lam * pix)
        u, v = X * np.cos(phi) + Y * np.sin(phi), -X * np.sin(phi) + Y * np.cos(phi)
        tex += amp * np.sin(w * u + phi) * np.sin(w * v + 2 * phi)
    # stripes of the surface with 2 % of the texture, 32 of every 64 px at depth 2: K14 finds WEAK pixels in every window
    tex = np.where(np.mod(X / pix, 64.0) >= 32.0, 0.02 * tex, tex)
    # make_scene's sensor noise, another draw in every view: what makes the low-texture stripes ambiguous
    tex += np.random.RandomState(1000 + 17 * k + y0).uniform(-1.5, 1.5, tex.shape)
    return np.clip(np.round(128.0 + tex), 0, 255).astype(np.float32)


def images(sc, N, wins, floats=False):
    """N + 1 float32 [H, W] images with integer grey values: a 256 x 256 texture tile repeated over the frame with another grey
    offset on every tile (no 268-Mpix rendering), and the rows within RENDER_ROWS of a window rendered from the scene."""
    W, H = sc.width, sc.height
    rng = np.random.RandomState(5)
    t = 256
    yy, xx = np.mgrid[0:t, 0:t].astype(np.float32)
    out = []
    for k in range(N + 1):
        tile = 128 + 40 * np.sin(0.7 * xx + k) * np.sin(0.45 * yy) + 30 * np.sin(0.23 * (xx + yy)) + rng.uniform(-8, 8, (t, t))
        strip = np.tile(np.round(tile).astype(np.float32), (1, _ceil_div(W, t)))[:, :W]
        strip = strip + np.repeat((np.arange(_ceil_div(W, t)) * 7 % 24).astype(np.float32), t)[:W]
        img = np.empty((H, W), np.float32)
        for r in range(_ceil_div(H, t)):
            rows = min(t, H - r * t)
            img[r * t:r * t + rows] = strip[:rows] + np.float32(r * 5 % 16)
        for (_, y0, _, y1) in wins:
            a, b = max(y0 - RENDER_ROWS, 0), min(y1 + RENDER_ROWS, H)
            img[a:b] = _render_rows(sc, k, a, b)
        out.append(img)
    return fl.float_images(out) if floats else out


def weak_stripes(W, H):
    """The crafted WEAK map of the APD passes: 5 columns of every 48 (two stripes or more in every window)."""
    return (np.arange(W) % 48) >= 43


def depth_maps(W, H, n):
    """common.fake_depth_maps without its two W x H index arrays."""
    xs, ys = np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32)
    out = []
    for k in range(n):
        d = (np.float32(2.2) + np.float32(0.1) * np.sin(np.float32(0.05) * xs + k)[None, :] + np.float32(0.05) * np.cos(np.float32(0.07) * ys)[:, None])
        d = d.astype(np.float32)
        d[::13, ::17] = 0.0
        out.append(d)
    return out
