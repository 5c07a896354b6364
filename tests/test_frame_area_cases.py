"""The oracle windows of tests/test_gpu_frame_area.py sit on the rows where a 32-bit product can wrap (tests/frame_area_cases.py).
Host arithmetic only."""
import pytest

import common
import frame_area_cases as fa


def _inside(win, x, y):
    return win[0] <= x < win[2] and win[1] <= y < win[3]


def test_the_table_lists_every_oracle_state_and_image_copy():
    names = [a[0] for a in fa.ARRAYS]
    assert len(set(names)) == len(names)
    for _, hs, oa in common.ORACLE_STATES:
        assert oa in names, oa
    for name in ("neighbours_map", "column_nearest", "weak_list", "mask", "img (float)", "pairs (byte)", "tiled (byte)", "fquads (float quad)", "depths"):
        assert name in names
    for name, elem, bpe, grid, cite in fa.ARRAYS:
        assert bpe % elem == 0 and grid in ("pixel", "quad", "pairs", "tiled", "weak") and ".h" in cite, name


def test_the_thresholds_the_frames_reach():
    """A: the 32-byte array passes 2^31 bytes; B: ... and 2^32, the 16- and 24-byte arrays 2^31; C and C': ... and the 24-byte
    array 2^32.  No frame apd_create accepts reaches more: 2^28 px (a 16-byte offset at 2^32, pixel * 8 at 2^31) is 32,768 px
    past the largest frame, and the arrays of 4 bytes per pixel and less stay below 2^31 bytes."""
    def reached(frame):
        return {(c["array"], c["quantity"], c["threshold"].bit_length() - 1) for c in fa.crossings(*frame)}
    a, b, c, ct = (reached(f) for f in (fa.A, fa.B, fa.C, fa.CT))
    assert a == {("view_weight", q, 31) for q in ("byte offset", "element index", "row pitch")}
    assert a < b < c and c == ct
    assert ("view_weight", "byte offset", 32) in b and ("planes", "byte offset", 31) in b and ("rng", "byte offset", 31) in b
    assert ("fquads (float quad)", "byte offset", 31) in b and ("fquads (float quad)", "row pitch", 31) in b
    assert c - b == {("rng", "byte offset", 32), ("rng", "row pitch", 32)}
    assert {n for n, _, _ in c} == {"view_weight", "rng", "planes", "fit_planes", "fquads (float quad)"}
    # the same table on the frame one row past the limit: nothing but the float-quad image at 2^32, which apd_create refuses
    assert reached((16384, 16383)) - c == {("fquads (float quad)", "byte offset", 32)}
    # the neighbour table (36 bytes per WEAK pixel) passes 2^31 bytes only with 59.7 M WEAK pixels, 22 % of C: the crafted map
    # of the GPU tests (5 columns of 48) holds 28 M
    stripes = int(fa.weak_stripes(*fa.C).sum()) * fa.C[1]
    assert not [c for c in fa.crossings(*fa.C, weak_entries=stripes) if c["y"] is None]
    assert [c["array"] for c in fa.crossings(*fa.C, weak_entries=60_000_000) if c["y"] is None] == ["neighbours"]


@pytest.mark.parametrize("frame", sorted(fa.FRAMES))
def test_windows_hold_every_crossing_row(frame):
    W, H = fa.FRAMES[frame]
    assert W > 6200 and H > 6200
    wins = fa.windows(W, H)
    for i, a in enumerate(wins):
        assert 0 <= a[0] < a[2] <= W and 0 <= a[1] < a[3] <= H
        for b in wins[:i]:
            assert a[2] <= b[0] or b[2] <= a[0] or a[3] <= b[1] or b[3] <= a[1], (a, b)
    cross = fa.crossings(W, H)
    assert cross
    for c in cross:
        x, y = c["x"], c["y"]
        rows = range(max(y - fa.ROW_MARGIN, 0), min(y + fa.ROW_MARGIN + 1, H))
        assert fa.ROW_MARGIN >= 2 and fa.ROW_MARGIN >= fa.PATCH_RADIUS
        home = [w for w in wins if all(_inside(w, x, r) for r in rows)]
        assert home, (frame, c)
        # the entries on both sides of the crossing: in the same window, or at the other end of the rows in another one
        for dx in (-fa.ROW_MARGIN, fa.ROW_MARGIN):
            xn = (x + dx) % W
            assert any(all(_inside(w, xn, r) for r in rows) for w in wins), (frame, c, dx)
    assert any(w[1] == 0 for w in wins) and any(w[3] == H for w in wins)
    if (W, H) == fa.C:
        assert _inside(wins[-1], W - 1, H - 1)
    assert _inside(max(wins, key=lambda w: (w[3], w[2])), W - 1, H - 1)
    assert set(fa.crossing_rows(W, H)) <= {y for w in wins for y in range(w[1], w[3])}


def test_bands_and_stripes():
    W, H = fa.C
    wins = fa.windows(W, H)
    for w, b in zip(wins, fa.bands(wins, W, H, 128)):
        assert b[0] <= w[0] and b[1] <= w[1] and b[2] >= w[2] and b[3] >= w[3] and 0 <= b[0] and b[2] <= W and 0 <= b[1] and b[3] <= H
    stripes = fa.weak_stripes(W, H)
    for (x0, y0, x1, y1) in wins:
        assert int(stripes[x0:x1].sum()) * (y1 - y0) > 50
