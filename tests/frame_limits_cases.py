"""Shapes, pass parameters and crafted WEAK maps shared by tests/test_gpu_frame_limits.py (HIP path vs oracle at the ends
of the size range apd_create accepts) and tests/test_oracle_frame_limits.py (the oracle alone at the same tiny shapes)."""
import numpy as np

WEAK, STRONG, UNKNOWN = 0, 1, 2

# (W, H): fewer pixels than a wave, an empty checkerboard colour, a single row / column; one tile and just over one tile of the
# tiled copy (W + 2, H + 1 entries against 7 x 8); the frame is one 11-px strong patch; below the 32 x 4 checkerboard footprint
# and the 8 x 8 full-frame block, one column past a 64-entry window; below the suite's former minimum with interior pixels that
# survive K14's 6-px margin
TINY_SHAPES = [(1, 1), (2, 2), (1, 40), (40, 1), (3, 5), (5, 7), (7, 8), (8, 9), (11, 11), (12, 10), (16, 4), (64, 5), (5, 64),
               (65, 9), (24, 20), (31, 32), (33, 17)]

# the three pass kinds of tools/parity_fuzz.py (main.cpp:168-215)
PASSES = [dict(state=0, use_APD=0, weak_peak_radius=6),
          dict(state=1, use_APD=1, weak_peak_radius=6, rotate_time=2, ransac_threshold=0.01 - 0.00125),
          dict(state=2, use_APD=1, weak_peak_radius=4, rotate_time=4, ransac_threshold=0.01 - 0.0025, geom_consistency=1)]


def weak_block(W, H):
    """(x0, y0, x1, y1) of the central half-by-half block; empty when an axis is a single pixel."""
    return W // 4, H // 4, W // 4 + W // 2, H // 4 + H // 2


def crafted_weak_map(W, H):
    """The central half-by-half block WEAK, the rest STRONG, and one UNKNOWN pixel (the last one) where the frame has room.  The
    natural map of a frame below 13 x 13 is all UNKNOWN (K14's 6-px margin, APD.cu:1990-2143): without a crafted one K3, K4,
    K9 and K10 would never see a pixel."""
    weak = np.full((H, W), STRONG, np.uint8)
    x0, y0, x1, y1 = weak_block(W, H)
    weak[y0:y1, x0:x1] = WEAK
    if W >= 3 and H >= 3:
        weak[H - 1, W - 1] = UNKNOWN
    return weak


def float_images(imgs):
    """Non-integer grey values (what a resampled pyramid level holds): the float texel-quad path."""
    return [(im * np.float32(0.731) + np.float32(1.5)).astype(np.float32) for im in imgs]


def schedule(iters, weak):
    """The kernels of one pass in launch order, (kernel id, iteration); K3, K4, K9 and K10 only with a WEAK pixel."""
    s = [(1, 0), (2, 0)] + ([(3, 0), (4, 0)] if weak else []) + [(5, 0)]
    for i in range(iters):
        s += [(6, i), (7, i), (8, i)] + ([(9, i), (10, i)] if weak else [])
    return s + [(11, 0), (12, 0), (13, 0), (14, 0), (15, 0)]
