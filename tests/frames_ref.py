"""Plain-Python restatement of the frame-range rule and plan of DESIGN.md section 14, written from the rule and not from
the library: the window of coefficient planes a frame range depends on, the symbol ranges and blocks of a channel that
hold them, and the cut of a symbol volume down to the window's virtual chunk.  The case table of the GPU tests lives here
too, so that the host test can hold it to the plan classes it claims to reach."""
from __future__ import annotations

import numpy as np

CDF53, CDF97, HAAR = 0, 1, 2
WAVELETS = (CDF53, CDF97, HAAR)
# lifting steps: an error at an interior window end travels one position per step.  Haar's predict step averages both even
# neighbours like CDF 5/3's, so it is not pair-local and needs the halo too.
LIFT_STEPS = {CDF53: 2, CDF97: 4, HAAR: 2}


def padded_frames(f: int) -> int:
    return 2 if f == 1 else f + (f & 1)


def frame_window(kind: int, f: int, t0: int, t1: int, halo: int | None = None):
    """(a, b): frames [t0, t1) of f depend on the frame pairs inside [a, b) only.  halo: the rule's NS unless given."""
    assert 0 <= t0 < t1 <= f
    ns = LIFT_STEPS[kind] if halo is None else halo
    pf = padded_frames(f)
    a = max(0, (t0 - ns) & ~1) if t0 - ns > 0 else 0
    b = min(pf, (t1 + ns + 1) & ~1)
    return a, b


def window_planes(f: int, a: int, b: int):
    """Indices t' of the needed coefficient planes, low band then high band: the virtual chunk's plane order."""
    half = padded_frames(f) // 2
    return list(range(a // 2, b // 2)) + list(range(half + a // 2, half + b // 2))


def window_volume(sym, dims, a: int, b: int) -> np.ndarray:
    """The (b - a, ph, pw) symbol volume of the virtual chunk cut from one channel's symbols; dims = (pw, ph, pf)."""
    pw, ph, pf = dims
    v = np.asarray(sym).reshape(pf, ph, pw)
    half = pf // 2
    return np.concatenate([v[a // 2:b // 2], v[half + a // 2:half + b // 2]], axis=0)


def frame_plan(kind: int, w: int, h: int, f: int, L: int, t0: int, t1: int) -> dict:
    """The plan of one channel (all three are alike): window, symbol ranges, (first block, count) per range with a block
    that both ranges touch given to the first, the block count, and the classes of the plan."""
    pw, ph, pf = w + (w & 1), h + (h & 1), padded_frames(f)
    P, half, B = pw * ph, pf // 2, 64 * L
    n = P * pf
    n_blocks = -(-n // B)
    a, b = frame_window(kind, f, t0, t1)
    ranges = [(a // 2 * P, b // 2 * P), ((half + a // 2) * P, (half + b // 2) * P)]
    if ranges[0][1] == ranges[1][0]:
        ranges = [(ranges[0][0], ranges[1][1])]
    assert (len(ranges) == 1) == (a == 0 and b == pf)
    blocks, nxt, touched = [], 0, []
    for lo, hi in ranges:
        first, end = lo // B, -(-hi // B)
        touched.append(set(range(first, end)))
        first = max(first, nxt)
        blocks.append((first, max(end - first, 0)))
        nxt = max(nxt, end)
    planned = set()
    for first, count in blocks:
        assert not planned & set(range(first, first + count))
        planned |= set(range(first, first + count))
    assert planned == set().union(*touched) and max(planned) < n_blocks
    cls = set()
    cls.add("merged" if len(ranges) == 1 else "two_ranges")
    edges = [e for r in ranges for e in r]
    cls.add("start_aligned" if ranges[0][0] % B == 0 else "start_clipped")
    cls.add("end_aligned" if (ranges[-1][1] % B == 0 or ranges[-1][1] == n) else "end_clipped")
    if any(e % B for e in edges if e != n):
        cls.add("edge_inside_block")
    if len(ranges) == 2:
        cls.add("shared_block" if touched[0] & touched[1] else "separate_blocks")
        if blocks[1][0] > blocks[0][0] + blocks[0][1]:
            cls.add("gap_between_ranges")
    if len(planned) < n_blocks:
        cls.add("blocks_skipped")
    if n_blocks == 1:
        cls.add("one_block_channel")
    if n % B and (n_blocks - 1) in planned:
        cls.add("short_last_block")
    if f & 1 or f == 1:
        cls.add("pad_frame")
    if a > 0 and b < pf:
        cls.add("halo_touches_neither_end")
    if a == 0 and b == pf and (t0 > 0 or t1 < f):
        cls.add("halo_touches_both_ends")
    return dict(a=a, b=b, ranges=ranges, blocks=blocks, n_planned=len(planned), planned=sorted(planned), n_blocks=n_blocks,
                dims=(pw, ph, pf), classes=cls)


# ---- the case table of tests/test_gpu_frames.py ----
LANE = 64          # a block is 4096 symbols
# 64x64x16: a plane is exactly one block (aligned ends, gaps between the ranges, skipped blocks); 50x38x13: planes of 1900
# symbols (ends clipped inside a block, low and high range inside one shared block, a short last block, an odd f with a pad
# frame); 33x17x5: the whole channel is one block; 96x70x24 and 130x66x40: a plane spans 1.6 and 2.1 blocks, several tiles
# with interior ones; 5x3x7: not tile-eligible (the generic path); 40x24x1 and 40x24x2: pf = 2, the ranges merge.
SHAPES = [(64, 64, 16), (50, 38, 13), (33, 17, 5), (96, 70, 24), (130, 66, 40), (5, 3, 7), (40, 24, 1), (40, 24, 2)]
ALL_RANGES_CASE = ((50, 38, 13), CDF97)
REQUIRED_CLASSES = {"merged", "two_ranges", "start_aligned", "start_clipped", "end_aligned", "end_clipped", "edge_inside_block",
                    "shared_block", "separate_blocks", "gap_between_ranges", "blocks_skipped", "one_block_channel",
                    "short_last_block", "pad_frame", "halo_touches_neither_end", "halo_touches_both_ends"}


def named_ranges(kind: int, f: int):
    """[0, 1), [f-1, f), [0, f), a window whose halo touches neither end (where f allows one) and one that touches both."""
    ns, pf = LIFT_STEPS[kind], padded_frames(f)
    out = [(0, 1), (f - 1, f), (0, f)]
    t0, t1 = ns + 2, pf - ns - 2          # a = (t0 - ns) & ~1 >= 2 and b = (t1 + ns + 1) & ~1 <= pf - 2
    if t0 < t1 <= f:
        out.append((t0, t1))
        out.append((t0, t0 + 1))
    out.append((1, f - 1) if f >= 3 and frame_window(kind, f, 1, f - 1) == (0, pf) else (0, f))
    return list(dict.fromkeys(out))


def ranges_for(shape, kind: int):
    f = shape[2]
    out = named_ranges(kind, f) + [(t, t + 1) for t in range(f)]
    if (tuple(shape), kind) == ALL_RANGES_CASE:
        out += [(t0, t1) for t0 in range(f) for t1 in range(t0 + 1, f + 1)]
    return list(dict.fromkeys(out))


def all_cases():
    return [(shape, kind, r) for shape in SHAPES for kind in WAVELETS for r in ranges_for(shape, kind)]
