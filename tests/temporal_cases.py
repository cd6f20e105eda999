"""The plan of the temporal stream tests ("Frame-count classes"), CPU only: which frame counts, shapes,
contents, quantiser steps and frame ranges tests/test_gpu_temporal_streams.py runs through every instance of the two
streaming temporal kernels' bodies (FwdT::run and InvT::run of csrc/transform.hip), with the numpy and oracle references,
and what tests/test_temporal_cases_host.py holds that plan to without a device.

Both bodies peel their loop over the frame pairs k = 0 .. half - 1 (half = padded frames / 2) by hand: a first block of four
pairs with the left mirrors static, a steady loop of whole 4-pair blocks, a tail, and the right mirror on the last pair.
Which pieces run depends on half alone, and the forward keeps the last pair out of its steady loop while the inverse does
not:

                short (first block only)   tail only   steady loop entered   tail after steady
    forward     half 1..4                  half 5..8   half >= 9             1..4 pairs
    inverse     half 1..4                  half 5..7   half >= 8             0..3 pairs

forward_class / inverse_class restate that table as a rule; nothing here is read from the library but
alice_codec_test_inverse_variant, which names the quantiser steps of the inverse's instance classes.  Everything is built
once per key and never written again."""
from __future__ import annotations

import numpy as np

import frames_ref as FR
import reversible_extreme_cases as P
import reversible_ref as RR
import split_ref as R2
import transform_extremes as X
import wide_ref as R3

CDF53, CDF97, HAAR = 0, 1, 2
KINDS = (CDF53, CDF97, HAAR)
NAMES = {CDF53: "CDF 5/3", CDF97: "CDF 9/7", HAAR: "Haar"}
VERSIONS = (2, 3, 4)
LANE_SYMBOLS = 64

FRAMES = list(range(1, 27)) + [33, 34, 39, 40]     # half 1 .. 13, 17 and 20, each from an even and from an odd f
FRAMES_WIDE = [17, 18, 25, 26]                     # half 9 and 13: one and two steady blocks of both bodies
# 12x10: tile-eligible, 120 pixels per frame = 30 four-pixel groups in one partly filled wavefront.  70x34: 2380 pixels =
# three workgroups per channel with the last one partial, rows of both halves of band_plane_index, and the seam between
# the two inverse tiles of a row (tiles are 96 x 32: rows 32 and 33 belong to the second tile row).
SHAPE, SHAPE_WIDE = (12, 10), (70, 34)


def shapes():
    """[(w, h, f)]: every frame count on the main shape, then the steady-loop counts on the second"""
    return [SHAPE + (f,) for f in FRAMES] + [SHAPE_WIDE + (f,) for f in FRAMES_WIDE]


def half_of(f: int) -> int:
    return FR.padded_frames(f) // 2


# ---- the class rule ----
def _class(half: int, blocks: int):
    if half <= 4:
        return ("short", half)
    return (min(blocks, 2), half - 4 - 4 * blocks)


def forward_class(half: int):
    """("short", half) or (steady blocks capped at 2, tail pairs 1..4): the steady loop runs blocks [kb, kb + 4) from kb = 4
    while kb + 4 <= half - 1"""
    return _class(half, max(0, (half - 1) // 4 - 1))


def inverse_class(half: int):
    """("short", half) or (steady blocks capped at 2, tail pairs 0..3): the steady loop runs while kb + 4 <= half"""
    return _class(half, max(0, half // 4 - 1))


FORWARD_CLASSES = ([("short", n) for n in (1, 2, 3, 4)] + [(0, t) for t in (1, 2, 3, 4)] + [(1, t) for t in (1, 2, 3, 4)]
                   + [(2, 1), (2, 4)])
INVERSE_CLASSES = ([("short", n) for n in (1, 2, 3, 4)] + [(0, t) for t in (1, 2, 3)] + [(1, t) for t in (0, 1, 2, 3)]
                   + [(2, 0), (2, 1)])
STEADY_FRAMES = [f for f in FRAMES if half_of(f) >= 9]      # both bodies enter their steady loop


# ---- steps ----
def class_steps(lib, kind: int, wide: int):
    """[(step, class)]: one step from the middle of every instance class of the inverse (the open exact class: a few steps
    past its first)"""
    cl = X.classes(lib, kind, wide)
    out = []
    for i, (v, first, last) in enumerate(cl):
        out.append(((first + last) // 2 if i + 1 < len(cl) else first + 3, v))
    return out


def step_cases(lib, kind: int, wide: int):
    """[((s0, s1, s2), class the launcher picks)]: every class step in all three channels, then one call with a step of a
    different class in each channel"""
    steps = class_steps(lib, kind, wide)
    cases = [((s, s, s), v) for s, v in steps]
    mixed = tuple(steps[i % len(steps)][0] for i in range(3))
    cases.append((mixed, X.variant(lib, kind, mixed, wide)))
    for c, v in cases:
        assert X.variant(lib, kind, c, wide) == v
    return cases


def expected_classes(kind: int, wide: int) -> set:
    """the instance classes of the inverse the launcher can pick: u8 symbols, or the wide ones"""
    return (P.EXPECTED_CLASSES if wide else X.EXPECTED_VARIANTS)[kind]


# ---- contents and symbol volumes ----
_cache = {}


def _once(key, make):
    if key not in _cache:
        v = make()
        for a in (v if isinstance(v, (list, tuple)) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = v
    return _cache[key]


def dims(w, h, f):
    """(pw, ph, pf)"""
    return R3.padded_dims(w, h, f)


def random_rgb(w, h, f) -> np.ndarray:
    return _once(("rgb", w, h, f), lambda: np.random.default_rng(7000 + 100 * w + f).integers(0, 256, w * h * f * 3, dtype=np.uint8))


def byte_symbols(kind, w, h, f) -> np.ndarray:
    """(3, pf, ph, pw) u8: transform_extremes.loud_random_bytes per channel"""
    pw, ph, pf = dims(w, h, f)
    return _once(("u8", kind, w, h, f), lambda: np.stack([X.loud_random_bytes((pf, ph, pw), 900 + 37 * f + 3 * kind + c) for c in range(3)]))


def wide_symbols(kind, w, h, f):
    """[Y, Co, Cg] flat u16: transform_extremes.loud_random_wide per channel"""
    pw, ph, pf = dims(w, h, f)
    return _once(("u16", kind, w, h, f), lambda: [X.loud_random_wide((pf, ph, pw), 1900 + 37 * f + 3 * kind + c).reshape(-1) for c in range(3)])


# ---- references of the inverse ----
def byte_reference(kind, w, h, f, steps) -> np.ndarray:
    """interleaved RGB of byte_symbols through the CPU oracle's decoder"""
    from slab_oracle_stages import OracleStages
    import torch

    def make():
        sym = torch.from_numpy(np.array(byte_symbols(kind, w, h, f)))
        return OracleStages().inverse_symbols(sym, w, h, f, kind, list(steps)).numpy().reshape(-1)
    return _once(("ref8", kind, w, h, f, tuple(steps)), make)


def wide_reference(kind, w, h, f, steps, mirrored: bool) -> np.ndarray:
    """interleaved RGB of wide_symbols: transform_extremes.inverse_quantised_steps, or reversible_ref.inverse_quantised"""
    def make():
        qs = [R3.from_wide_symbols(z) for z in wide_symbols(kind, w, h, f)]
        inverse = RR.inverse_quantised if mirrored else X.inverse_quantised_steps
        return inverse(qs, steps, dims(w, h, f), w, h, f, kind)
    return _once(("ref16", kind, w, h, f, tuple(steps), bool(mirrored)), make)


def reference(kind, w, h, f, version, steps) -> np.ndarray:
    if version == 2:
        return byte_reference(kind, w, h, f, steps)
    return wide_reference(kind, w, h, f, steps, version == 4)


# ---- containers ----
def container(kind, w, h, f, version, steps) -> bytes:
    """split_ref / wide_ref write_container of the volume, coded once per (wavelet, shape, symbol width) -- the payloads do
    not depend on the steps --, with the header's steps (and byte 4 for version 4) patched"""
    ref = R2 if version == 2 else R3

    def make():
        sym = byte_symbols(kind, w, h, f).reshape(3, -1) if version == 2 else wide_symbols(kind, w, h, f)
        return ref.write_container(kind, w, h, f, LANE_SYMBOLS, (1, 1, 1), sym)
    blob = bytearray(_once(("blob", kind, w, h, f, version != 2), make))
    for c in range(3):
        at = ref.FIXED + c * ref.CHANNEL
        blob[at:at + 8] = int(steps[c]).to_bytes(4, "little", signed=True) * 2       # step and dead zone
    assert ref.parse_container(bytes(blob))["step"] == list(steps)
    return bytes(blob) if version != 4 else RR.with_version(bytes(blob), 4)


# ---- windows ----
# The window instances lift the virtual chunk of the window [a, b): their half is (b - a) / 2.  A
# window holds a kept frame and its halo, so no range of a chunk of 26 frames or more has a virtual chunk shorter than
# 2 pairs (3 for CDF 9/7): chunks of 2 and 4 frames give the one- and the two-pair window.
WINDOW_FRAMES = (2, 4, 26, 33, 40)
WINDOW_KINDS = {"neither_end", "start_only", "end_only", "whole"}


def window_ranges(kind: int, f: int):
    """The nine ranges every long chunk gets; on the 26-frame chunk also, for every half a window of this wavelet can have
    up to 11, the range whose window is [2, 2 + 2 half) (clipped at neither end) and, for the small ones, the range [0, t1)
    whose window is [0, 2 half)."""
    if f <= 4:
        return list(dict.fromkeys([(0, 1), (f - 1, f), (0, f)]))
    out = [(0, 1), (f // 2, f // 2 + 1), (3, 9), (5, 17), (4, 20), (2, f - 3), (f - 20, f), (f - 1, f), (0, f)]
    if f == 26:
        ns = FR.LIFT_STEPS[kind]
        for half in range(1, 12):
            t0, t1 = ns + 2, 2 * half + 1 - ns
            if t0 < t1 and FR.frame_window(kind, f, t0, t1) == (2, 2 + 2 * half):
                out.append((t0, t1))
            t1 = 2 * half - ns - 1
            if half <= 5 and t1 >= 1 and FR.frame_window(kind, f, 0, t1) == (0, 2 * half):
                out.append((0, t1))
    return list(dict.fromkeys(out))


def window_class(kind: int, f: int, t0: int, t1: int):
    a, b = FR.frame_window(kind, f, t0, t1)
    return inverse_class((b - a) // 2)


def window_kind(kind: int, f: int, t0: int, t1: int) -> str:
    a, b = FR.frame_window(kind, f, t0, t1)
    pf = FR.padded_frames(f)
    if a > 0:
        return "neither_end" if b < pf else "end_only"
    return "start_only" if b < pf else "whole"
