"""Plain numpy / Python restatement of the half-resolution preview of DESIGN.md section 15, written from the contract and
not from the library: the gain constant from the lifting steps in exact rationals, the preview of a frame range from the
low-low quadrants of the window's coefficient planes, the blocks of a channel that hold those quadrants, the classes of such
a plan, and the case table of tests/test_gpu_preview.py (so that the host test can hold it to the classes it claims)."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

import frames_ref as FR
import oracle.alice_oracle_np as o
import reversible_ref as RR
import wide_ref as R3

CDF53, CDF97, HAAR = FR.CDF53, FR.CDF97, FR.HAAR
WAVELETS = FR.WAVELETS


# ---- the gain constant ----
def dc_gain(kind: int) -> Fraction:
    """The per-axis DC gain of the low band: a constant signal (even = odd = 1) pushed through the forward lifting steps
    (coefficient c over 8192, a predict step adds c / 8192 * (left + right) of the even samples to the odd ones, an update
    step the other way round) in exact rationals; the low band is the even samples."""
    even, odd = Fraction(1), Fraction(1)
    for coeff, predict in o.STEPS[kind]:
        if predict:
            odd += Fraction(coeff, 8192) * 2 * even
        else:
            even += Fraction(coeff, 8192) * 2 * odd
    return even


def gain_constant(kind: int) -> int:
    """K = round(65536 / g^2): two spatial axes"""
    g = dc_gain(kind)
    return int(round(Fraction(65536) / (g * g)))


K = {CDF53: 65536, CDF97: 47484, HAAR: 65536}


def preview_dims(w: int, h: int):
    return (w + 1) // 2, (h + 1) // 2


# ---- the contract ----
def inverse_axis0(v, kind: int, mirrored: bool) -> np.ndarray:
    return RR.mirror_axis(v, 0, o.STEPS[kind]) if mirrored else o._lift_axis(v, 0, o.STEPS[kind], True)


def from_symbols(V, version: int) -> np.ndarray:
    return o.from_symbols(np.asarray(V, np.uint8)) if version == 2 else R3.from_wide_symbols(V)


def preview(syms, dims, f: int, kind: int, steps, version: int, t0: int, t1: int, normalise: bool = True) -> np.ndarray:
    """Packed RGB bytes, (t1 - t0) * qh * qw * 3, of the preview of frames [t0, t1): syms are the three channels' symbol
    volumes of the padded chunk (dims = (pw, ph, pf)).  normalise = False leaves step 4 out."""
    pw, ph, pf = dims
    qw, qh = pw // 2, ph // 2
    a, b = FR.frame_window(kind, f, t0, t1)
    chans = []
    for c in range(3):
        V = FR.window_volume(syms[c], dims, a, b)[:, :qh, :qw]
        q = np.asarray(from_symbols(V, version), np.int64)
        v = o._wrap32(q * int(steps[c]))
        v = np.asarray(inverse_axis0(v, kind, version == 4), np.int64)[t0 - a:t1 - a]
        n = (v * K[kind] + 32768) >> 16 if normalise else v
        chans.append(o._wrap16(n).reshape(-1))
    return o.ycocg_r_to_rgb(*chans)


def box_average(rgb, w: int, h: int, f: int) -> np.ndarray:
    """(sum + 2) // 4 over 2x2 blocks of the edge-padded frames: (f, qh, qw, 3) u8"""
    v = np.asarray(rgb, np.int64).reshape(f, h, w, 3)
    v = np.pad(v, ((0, 0), (0, h & 1), (0, w & 1), (0, 0)), mode="edge")
    s = v[:, 0::2, 0::2] + v[:, 1::2, 0::2] + v[:, 0::2, 1::2] + v[:, 1::2, 1::2]
    return ((s + 2) // 4).astype(np.uint8)


# ---- the plan ----
def preview_plan(kind: int, w: int, h: int, f: int, L: int, t0: int, t1: int) -> dict:
    """The plan of one channel (all three are alike): window, the ascending list of planned blocks -- the union, over the
    window's planes t', of the blocks that intersect [t' P, t' P + (qh - 1) pw + qw) --, and the classes of the plan."""
    pw, ph, pf = w + (w & 1), h + (h & 1), FR.padded_frames(f)
    qw, qh = pw // 2, ph // 2
    assert (qw, qh) == preview_dims(w, h)
    P, B = pw * ph, 64 * L
    n = P * pf
    n_blocks = -(-n // B)
    a, b = FR.frame_window(kind, f, t0, t1)
    run = (qh - 1) * pw + qw
    planned, per_plane = set(), []
    for tp in FR.window_planes(f, a, b):
        lo, hi = tp * P, tp * P + run
        mine = set(range(lo // B, (hi - 1) // B + 1))
        per_plane.append((lo, hi, mine))
        planned |= mine
    assert max(planned) < n_blocks
    cls = set()
    for lo, hi, mine in per_plane:
        nxt = (lo + P) // B                      # the block in which the next plane starts
        full = set(range(lo // B, (lo + P - 1) // B + 1))
        if full - mine - {nxt}:
            cls.add("blocks_skipped_inside_a_plane")
        # aligned: the top half of the plane, [lo, lo + qh pw), ends with a block, so the last planned block holds no row
        # of the bottom half; clipped: it holds symbols that are decoded and dropped
        cls.add("plane_end_aligned" if (lo + qh * pw) % B == 0 else "plane_end_clipped")
    for i, (_, _, x) in enumerate(per_plane):
        for _, _, y in per_plane[i + 1:]:
            if x & y:
                cls.add("block_shared_by_two_planes")
    if n_blocks == 1:
        cls.add("one_block_channel")
    if n % B and (n_blocks - 1) in planned:
        cls.add("short_last_block")
    cls.add("qw_odd" if qw & 1 else "qw_even")
    if qw == 1:
        cls.add("qw_one")
    cls.add(f"q_mod4_{(qw * qh) % 4}")
    if f & 1 or f == 1:
        cls.add("pad_frame")
    if a > 0 and b < pf:
        cls.add("window_touches_neither_end")
    if a == 0 and b == pf:
        cls.add("window_touches_both_ends")
    if f == 1:
        cls.add("one_frame_chunk")
    return dict(a=a, b=b, planned=sorted(planned), n_planned=len(planned), n_blocks=n_blocks, dims=(pw, ph, pf), qw=qw, qh=qh,
                stored=3 * (b - a) * qw * qh, classes=cls)


def plan_classes(kind: int, w: int, h: int, f: int, L: int, t0: int, t1: int) -> set:
    return preview_plan(kind, w, h, f, L, t0, t1)["classes"]


REQUIRED_CLASSES = {"blocks_skipped_inside_a_plane", "block_shared_by_two_planes", "plane_end_clipped", "plane_end_aligned",
                    "one_block_channel", "short_last_block", "qw_odd", "qw_one", "q_mod4_0", "q_mod4_1", "q_mod4_2", "q_mod4_3",
                    "pad_frame", "window_touches_neither_end", "window_touches_both_ends", "one_frame_chunk"}

# ---- the case table of tests/test_gpu_preview.py ----
LANE = 64          # a block is 4096 symbols
# 128x128x8: a plane is 4 blocks, its top half exactly 2 (aligned end, half of the blocks skipped); 200x120x6: a plane is 5.9
# blocks (clipped ends); 50x38x13: planes of 1900 symbols (blocks shared between planes, qw = 25, a pad frame, a short last
# block, qw * qh = 475 = 3 mod 4); 33x17x5: one block (qw * qh = 153 = 1 mod 4); 5x3x7: qw = 3, qw * qh = 6; 2x2x1: qw = qh = 1;
# 40x24x1: pf = 2
SHAPES = [(128, 128, 8), (200, 120, 6), (50, 38, 13), (33, 17, 5), (5, 3, 7), (2, 2, 1), (40, 24, 1)]
ALL_RANGES_SHAPE = (50, 38, 13)


def ranges_for(shape, kind: int):
    """[0, 1), [f - 1, f), [0, f), one interior window and every single frame; every range on one shape"""
    f = shape[2]
    out = [r for r in FR.named_ranges(kind, f)] + [(t, t + 1) for t in range(f)]
    if tuple(shape) == ALL_RANGES_SHAPE:
        out += [(t0, t1) for t0 in range(f) for t1 in range(t0 + 1, f + 1)]
    return list(dict.fromkeys(out))


def class_ranges(kind: int, f: int):
    """The ranges of the frame-count-class cases: the whole chunk (its window is the chunk: half = pf / 2), the first, a
    middle and the last frame (short windows clipped at the start, at neither end, at the end)"""
    return list(dict.fromkeys([(0, f), (0, 1), (f // 2, f // 2 + 1), (f - 1, f)]))


def all_cases():
    return [(shape, kind, r) for shape in SHAPES for kind in WAVELETS for r in ranges_for(shape, kind)]
