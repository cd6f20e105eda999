"""Plain Python / numpy restatement of the rule of DESIGN.md section 22 (frame ranges and half-size previews of a banded
chunk), written from the rule and not from the library: the kept band-order indices and the planned blocks of every kept
band, where a kept symbol goes in the two compact volumes, the classes of such a plan, and the case table of
tests/test_gpu_banded_partial.py (so that the host test can hold it to the classes it claims)."""
from __future__ import annotations

import numpy as np

import banded_ref as B
import frames_ref as FR
import temporal_cases as TC

CDF53, CDF97, HAAR = FR.CDF53, FR.CDF97, FR.HAAR
WAVELETS = FR.WAVELETS
FRAMES, PREVIEW = "frames", "preview"
KEPT = {FRAMES: tuple(range(8)), PREVIEW: (0, 4)}


def padded(w: int, h: int, f: int):
    return w + (w & 1), h + (h & 1), FR.padded_frames(f)


# ---- the plan ----
def plan(mode: str, kind: int, w: int, h: int, f: int, L: int, t0: int, t1: int) -> dict:
    """The plan of every kept band of every channel (all alike): the window, the kept band-order indices [idx_lo, idx_hi),
    the planned blocks [blk_first, blk_first + blk_count), the totals the test hooks report, and the classes of the plan."""
    pw, ph, pf = padded(w, h, f)
    hw, hh, ht = pw // 2, ph // 2, pf // 2
    Q, blk = hw * hh, 64 * L
    n_band = Q * ht
    n_blocks = -(-n_band // blk)
    a, b = FR.frame_window(kind, f, t0, t1)
    idx_lo, idx_hi = a // 2 * Q, b // 2 * Q
    first, end = idx_lo // blk, -(-idx_hi // blk)
    assert 0 <= idx_lo < idx_hi <= n_band and first < end <= n_blocks
    bands = KEPT[mode]
    stored = 3 * (b - a) * (pw * ph if mode == FRAMES else Q)
    assert stored == 3 * len(bands) * (idx_hi - idx_lo)
    cls = set()
    if idx_lo % blk == 0 and idx_hi % blk == 0:
        cls.add("edges_on_block_edges")
    if idx_lo % blk:
        cls.add("first_block_clipped")
    if idx_hi < min(end * blk, n_band):
        cls.add("last_block_clipped")          # the last planned block holds symbols that are decoded and dropped
    if n_blocks > 1 and end - first == 1 and idx_hi - idx_lo < min(blk, n_band - first * blk):
        cls.add("range_inside_one_block")
    if n_blocks == 1:
        cls.add("one_block_band")
    if n_band % blk and end == n_blocks and n_blocks > 1:
        cls.add("short_last_block_planned")
    if Q > blk:
        cls.add("plane_longer_than_block")
    if Q < 64:
        cls.add("q_below_64")
        if end - first >= 2:
            cls.add("q_below_64_two_blocks")
    cls.add(f"q_mod4_{Q % 4}")
    if a == 0 and b == pf:
        cls.add("window_touches_both_ends")
    if a > 0 and b < pf:
        cls.add("window_touches_neither_end")
    if f & 1 or f == 1:
        cls.add("pad_frame")
    if f == 1:
        cls.add("one_frame_chunk")
    if n_band == 1:
        cls.add("n_band_one")
    return dict(a=a, b=b, idx_lo=idx_lo, idx_hi=idx_hi, blk_first=first, blk_count=end - first, bands=bands,
                blocks_total=3 * len(bands) * (end - first), stored=stored, n_blocks=n_blocks, n_band=n_band, Q=Q,
                dims=(pw, ph, pf), classes=cls)


REQUIRED_CLASSES = {"edges_on_block_edges", "first_block_clipped", "last_block_clipped", "range_inside_one_block", "one_block_band",
                    "short_last_block_planned", "plane_longer_than_block", "q_below_64", "q_below_64_two_blocks", "q_mod4_0",
                    "q_mod4_1", "q_mod4_2", "q_mod4_3", "window_touches_both_ends", "window_touches_neither_end", "pad_frame",
                    "one_frame_chunk", "n_band_one"}


# ---- where the kept symbols go ----
def _place(vol, band, p, origin: int, row_pitch: int, plane_pitch: int, hw: int, hh: int):
    """The rule, literally: band index idx in [idx_lo, idx_hi) goes to origin + (t'' - idx_lo / Q) plane_pitch + y'' row_pitch + x''."""
    idx = np.arange(p["idx_lo"], p["idx_hi"])
    Q = hw * hh
    t, y, x = idx // Q, idx % Q // hw, idx % hw
    at = origin + (t - p["idx_lo"] // Q) * plane_pitch + y * row_pitch + x
    assert np.unique(at).size == at.size and at.max() < vol.size
    assert not vol[at].any(), "two kept symbols at one place"
    vol[at] = np.asarray(band)[idx] + 1          # (+ 1: so that a place written twice or never shows)


def frames_volume(sym, dims, p) -> np.ndarray:
    """One channel's kept symbols as the virtual chunk's volume [b - a planes, low then high][ph][pw]"""
    pw, ph, pf = dims
    hw, hh = pw // 2, ph // 2
    n = p["b"] - p["a"]
    vol = np.zeros(n * ph * pw, np.int64)
    bands = B.gather_bands(sym, pw, ph, pf)
    for k in p["bands"]:
        bt, by, bx = k >> 2 & 1, k >> 1 & 1, k & 1
        _place(vol, bands[k], p, (bt * (n // 2) * ph + by * hh) * pw + bx * hw, pw, pw * ph, hw, hh)
    assert vol.all(), "a place of the virtual chunk was not written"
    return (vol - 1).reshape(n, ph, pw)


def preview_volume(sym, dims, p) -> np.ndarray:
    """One channel's kept symbols as the compact volume [b - a][pitch] of the preview's finish, pitch = round_up(Q, 4);
    returned without the pad symbols: (b - a, hh, hw)"""
    pw, ph, pf = dims
    hw, hh = pw // 2, ph // 2
    Q = hw * hh
    pitch = -(-Q // 4) * 4
    n = p["b"] - p["a"]
    vol = np.zeros(n * pitch, np.int64)
    bands = B.gather_bands(sym, pw, ph, pf)
    for k in p["bands"]:
        _place(vol, bands[k], p, (k >> 2) * (n // 2) * pitch, hw, pitch, hw, hh)
    v = vol.reshape(n, pitch)
    assert v[:, :Q].all() and not v[:, Q:].any()
    return (v[:, :Q] - 1).reshape(n, hh, hw)


def planned_payload_bytes(blob, p) -> int:
    """The lengths of the planned blocks of the kept bands, summed from the container's block-length tables"""
    info = B.parse_container(blob)
    total = 0
    for c in range(3):
        for k in p["bands"]:
            j = 8 * c + k
            table = np.frombuffer(info["payload"][j], "<u4", info["n_blocks"][j]).astype(np.int64)
            total += int(table[p["blk_first"]:p["blk_first"] + p["blk_count"]].sum())
    return total


# ---- the case table of tests/test_gpu_banded_partial.py ----
LANE = 64          # a block is 4096 band symbols
# (the shapes and what each is for: DESIGN.md section 22)
SHAPES = [(128, 128, 16), (160, 96, 16), (200, 120, 6), (50, 38, 13), (33, 17, 5), (5, 3, 7), (6, 4, 64), (18, 10, 200), (2, 2, 1),
          (40, 24, 1)]
ALL_RANGES_SHAPE = (50, 38, 13)
CLASS_SHAPE = (6, 4, 64)      # also gets windows of every half up to 16: the frame-count classes of the finish kernels
HAAR_SHAPES = [(50, 38, 13), (6, 4, 64)]


def ranges_for(shape, kind: int):
    """FR.named_ranges plus every single frame, as preview_ref.ranges_for; every range on one shape"""
    f = shape[2]
    out = list(FR.named_ranges(kind, f)) + [(t, t + 1) for t in range(f)]
    if tuple(shape) == ALL_RANGES_SHAPE:
        out += [(t0, t1) for t0 in range(f) for t1 in range(t0 + 1, f + 1)]
    if tuple(shape) == CLASS_SHAPE:
        out += [(8, t1) for t1 in range(9, 36, 2)]
    return list(dict.fromkeys(out))


def kinds_for(shape):
    return (CDF53, CDF97, HAAR) if tuple(shape) in HAAR_SHAPES else (CDF53, CDF97)


def all_cases():
    return [(shape, kind, r) for shape in SHAPES for kind in kinds_for(shape) for r in ranges_for(shape, kind)]


def window_class(kind: int, f: int, t0: int, t1: int):
    a, b = FR.frame_window(kind, f, t0, t1)
    return TC.inverse_class((b - a) // 2)

