"""Plain numpy / Python restatement of the rectangle rule and plan of DESIGN.md section 16, written from the rule and not
from the library: the three windows of a (frame range x rectangle), the cut of a symbol volume down to the virtual chunk, the
blocks of a channel that hold a kept symbol, the symbols stored, the classes of such a plan, and the case table of
tests/test_gpu_rect.py (so that the host test can hold it to the classes it claims)."""
from __future__ import annotations

import numpy as np

import frames_ref as FR

CDF53, CDF97, HAAR = FR.CDF53, FR.CDF97, FR.HAAR
WAVELETS = FR.WAVELETS
LIFT_STEPS = FR.LIFT_STEPS


def padded(w: int, h: int, f: int):
    """(pw, ph, pf)"""
    return w + (w & 1), h + (h & 1), FR.padded_frames(f)


# ---- the rule ----
def axis_window(ns: int, pn: int, c0: int, c1: int):
    """(a, b): the real positions [c0, c1) of an axis of padded length pn depend on the pairs inside [a, b) only"""
    assert 0 <= c0 < c1 <= pn
    a = 0 if c0 - ns <= 0 else (c0 - ns) & ~1
    b = min(pn, (c1 + ns + 1) & ~1)
    return a, b


def windows(kind: int, w: int, h: int, f: int, t0: int, t1: int, rect, halo=None):
    """((ta, tb), (ya, yb), (xa, xb)) of frames [t0, t1) and rect = (x, y, rw, rh); halo = (on t, on y, on x) replaces the
    rule's NS per axis"""
    x, y, rw, rh = rect
    assert 0 <= t0 < t1 <= f and rw >= 1 and rh >= 1 and 0 <= x and x + rw <= w and 0 <= y and y + rh <= h
    pw, ph, pf = padded(w, h, f)
    ns = (LIFT_STEPS[kind],) * 3 if halo is None else halo
    return axis_window(ns[0], pf, t0, t1), axis_window(ns[1], ph, y, y + rh), axis_window(ns[2], pw, x, x + rw)


def axis_indices(pn: int, a: int, b: int):
    """the kept coordinates of an axis, low run then high run: the virtual chunk's order"""
    half = pn // 2
    return list(range(a // 2, b // 2)) + list(range(half + a // 2, half + b // 2))


def cut(vol, dims, win) -> np.ndarray:
    """The (tb - ta, yb - ya, xb - xa) volume of the virtual chunk cut from one channel's (pf, ph, pw) volume (symbols or
    coefficients alike); dims = (pw, ph, pf), win = windows(...)"""
    pw, ph, pf = dims
    v = np.asarray(vol).reshape(pf, ph, pw)
    (ta, tb), (ya, yb), (xa, xb) = win
    return v[np.ix_(axis_indices(pf, ta, tb), axis_indices(ph, ya, yb), axis_indices(pw, xa, xb))]


# ---- the plan ----
def rect_plan(kind: int, w: int, h: int, f: int, L: int, t0: int, t1: int, rect, classes: bool = True) -> dict:
    """The plan of one channel (all three are alike): the windows, the ascending list of the blocks that intersect an x
    run of a kept row of a planned plane, the symbols stored over the three channels, and (classes = True: needs a mask of
    the whole channel, so small shapes only) the classes of the plan."""
    x, y, rw, rh = rect
    pw, ph, pf = padded(w, h, f)
    P, B = pw * ph, 64 * L
    n = P * pf
    n_blocks = -(-n // B)
    win = windows(kind, w, h, f, t0, t1, rect)
    (ta, tb), (ya, yb), (xa, xb) = win
    for a, b in win:
        assert a % 2 == 0 and b % 2 == 0 and a < b
    if xa == 0 and xb == pw:
        runs = [(0, pw)]
    else:
        runs = [(xa // 2, xb // 2), (pw // 2 + xa // 2, pw // 2 + xb // 2)]
    planned = set()
    per_plane = []          # (blocks of the plane's low rows, blocks of its high rows)
    for tp in axis_indices(pf, ta, tb):
        halves = []
        for rows in (range(ya // 2, yb // 2), range(ph // 2 + ya // 2, ph // 2 + yb // 2)):
            mine = set()
            for r in rows:
                for lo, hi in runs:
                    p0 = (tp * ph + r) * pw
                    mine |= set(range((p0 + lo) // B, (p0 + hi - 1) // B + 1))
            halves.append(mine)
            planned |= mine
        per_plane.append(tuple(halves))
    assert max(planned) < n_blocks
    vw, vh, vf = xb - xa, yb - ya, tb - ta
    out = dict(ta=ta, tb=tb, ya=ya, yb=yb, xa=xa, xb=xb, planned=sorted(planned), n_planned=len(planned), n_blocks=n_blocks,
               dims=(pw, ph, pf), vdims=(vw, vh, vf), stored=3 * vw * vh * vf, per_channel=vw * vh * vf)
    if not classes:
        return out
    cls = set()
    for name, a, b, pn in (("x", xa, xb, pw), ("y", ya, yb, ph)):
        cls.add(name + ("_full" if a == 0 and b == pn else "_left" if a == 0 else "_right" if b == pn else "_interior"))
    if w & 1 and xb == pw:
        cls.add("pad_column")
    if h & 1 and yb == ph:
        cls.add("pad_row")
    # the tile kernels cover a chunk whose padded width and height are at least 6; a tile is 96 x 32 with a halo, so a chunk
    # of 193 x 65 or more has a tile with neighbours on every side
    cls.add("virtual_tiles" if min(vw, vh) >= 6 else "virtual_generic")
    if vw >= 193 and vh >= 65:
        cls.add("virtual_interior_tile")
    if n_blocks == 1:
        cls.add("one_block_channel")
    if P < 64:
        cls.add("plane_below_64")
    for low, high in per_plane:
        if low and high and set(range(max(low) + 1, min(high))) - planned:
            cls.add("gap_inside_plane")
    kept = np.zeros((pf, ph, pw), bool)
    kept[np.ix_(axis_indices(pf, ta, tb), axis_indices(ph, ya, yb), axis_indices(pw, xa, xb))] = True
    assert int(kept.sum()) == vw * vh * vf
    flat = kept.reshape(-1)
    per_block = np.add.reduceat(flat.astype(np.int64), np.arange(0, n, B))
    assert set(np.flatnonzero(per_block).tolist()) == planned, "the planned blocks are the blocks that hold a kept symbol"
    sizes = np.minimum(B, n - np.arange(0, n, B))
    if np.any(per_block == sizes):
        cls.add("block_whole")
    if np.any((per_block > 0) & (per_block < sizes)):
        cls.add("block_partial")
    if n % B and (n_blocks - 1) in planned:
        cls.add("short_last_block")
    if len(planned) < n_blocks:
        cls.add("blocks_skipped")
    out["classes"] = cls
    return out


REQUIRED_CLASSES = {"x_full", "x_left", "x_right", "x_interior", "y_full", "y_left", "y_right", "y_interior", "pad_column", "pad_row",
                    "virtual_tiles", "virtual_generic", "virtual_interior_tile", "one_block_channel", "plane_below_64",
                    "gap_inside_plane", "block_whole", "block_partial", "short_last_block", "blocks_skipped"}

# ---- the case table of tests/test_gpu_rect.py ----
LANE = 64          # a block is 4096 symbols
# 64x64x16: a plane is exactly one block; 50x38x13: planes of 1900 symbols, a pad frame, a short last block; 33x17x5: one
# block, a pad column and a pad row; 160x104x6: a plane is 4.06 blocks, so a small rectangle skips the blocks between a
# plane's low and high rows; 224x104x4: the whole frame's virtual chunk has a tile with neighbours on every side; 5x3x7: planes
# of 24 symbols, the generic path; 40x24x1: pf = 2
SHAPES = [(64, 64, 16), (50, 38, 13), (33, 17, 5), (160, 104, 6), (224, 104, 4), (5, 3, 7), (40, 24, 1)]


def rects_for(shape, kind: int):
    """(x, y, w, h): the whole frame; 1 x 1 at the first, the last and the middle pixel; with m = NS + 2 the frame without a
    margin of m and a 3 x 2 at (m + 1, m), where they fit; a left strip 3 wide; a bottom strip 3 high; a top-right 5 x 4"""
    w, h, _ = shape
    m = LIFT_STEPS[kind] + 2
    out = [(0, 0, w, h), (0, 0, 1, 1), (w - 1, h - 1, 1, 1), (w // 2, h // 2, 1, 1)]
    if w - 2 * m >= 1 and h - 2 * m >= 1:
        out.append((m, m, w - 2 * m, h - 2 * m))
    if m + 1 + 3 <= w and m + 2 <= h:
        out.append((m + 1, m, 3, 2))
    out.append((0, 0, min(3, w), h))
    out.append((0, h - min(3, h), w, min(3, h)))
    out.append((w - min(5, w), 0, min(5, w), min(4, h)))
    return list(dict.fromkeys(out))


def ranges_for(shape):
    """[0, 1), [f - 1, f), [0, f) and one middle frame"""
    f = shape[2]
    return list(dict.fromkeys([(0, 1), (f - 1, f), (0, f), (f // 2, f // 2 + 1)]))


def cases_for(shape, kind: int):
    return [(r, rect) for rect in rects_for(shape, kind) for r in ranges_for(shape)]


def all_cases():
    return [(shape, kind, r, rect) for shape in SHAPES for kind in WAVELETS for r, rect in cases_for(shape, kind)]


def named_rects(shape, kind: int):
    """the rectangles that go through the host call too: the whole frame, the middle pixel, the margin-free interior or the
    left strip"""
    rs = rects_for(shape, kind)
    return {rs[0], rs[3], rs[4]}
