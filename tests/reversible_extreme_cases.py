"""The plan of the mirrored inverse's worst-case tests (.alc version 4), CPU only: which volumes,
shapes and quantiser steps tests/test_gpu_reversible_extremes.py decodes on the device, with the numpy references and the
containers, and what tests/test_reversible_extremes_host.py holds that plan to without one.

Volumes are those of tests/transform_extremes.py: the worst-sign volume of the shape (|q| = 2175 in every sample, the signs
that drive one output sample highest; the second channel with the signs flipped) and loud random ones (magnitudes from
{2175, 2174, 1087, 1, 0}, random signs).  Steps are the first and the last of every instance class, read from the library,
and the last fast step in each channel in turn.  Everything is built once per key and never written again."""
from __future__ import annotations

import ctypes as C

import numpy as np

import oracle.alice_oracle_np as o
import reversible_ref as RR
import transform_extremes as X
import wide_ref as R3

CDF53, CDF97, HAAR = 0, 1, 2
KINDS = (CDF53, CDF97, HAAR)
NAMES = {CDF53: "CDF 5/3", CDF97: "CDF 9/7", HAAR: "Haar"}
LANE_SYMBOLS = 64
# the class table of DESIGN.md 11.4 / 12.3: the first and last step of the packed i16 tile (3), the i16 band slot (2), the
# fast i32 class (1) and the first exact step (0); CDF 9/7 has neither a packed nor a fast i32 class at |q| <= 2175
EDGE_STEPS = {CDF53: [1, 2, 3, 6, 7, 19, 20], CDF97: [1, 2, 3], HAAR: [1, 2, 3, 6, 7, 12, 13]}
EXPECTED_CLASSES = {CDF53: {0, 1, 2, 3}, CDF97: {0, 2}, HAAR: {0, 1, 2, 3}}

# (w, h, f) -> (band target in KiB or None, centre (t, y, x) of the worst volume, seeds of the loud volumes).  Inverse tiles
# are 96 x 32 with a halo of 4.
SHAPES = {
    (200, 70, 4): (None, (1, 47, 143), (400,)),       # interior tile
    (199, 69, 3): (None, (1, 67, 197), (410,)),       # border: the tile with the pad row and column
    (104, 40, 1): (None, (1, 31, 95), (420,)),        # a single frame (pf = 2); the tile seam
    (3, 40, 4): (None, (1, 21, 3), (430, 452)),       # generic path: the mirrored axis_lift_kernel instances; with seed 430
                                                      # alone no CDF 9/7 case at step 3 tells the two inverses apart
    (256, 250, 6): (96, (3, 63, 143), (440,)),        # one tile row per band: row 63 reads the next band's rows
}
DEVICE_SHAPE = (200, 70, 4)                           # the device, region and lossless tests


def tile_eligible(shape) -> bool:
    pw, ph, _ = R3.padded_dims(*shape)
    return min(pw, ph) >= 6


# ---- steps ----
def variant(lib, kind, steps) -> int:
    """the instance class the launcher picks for a wide (u16) container with these steps"""
    return lib.alice_codec_test_inverse_variant(kind, (C.c_int32 * 3)(*[int(s) for s in steps]), 1)


def classes(lib, kind):
    """[(class, first step, last step)] over steps 1 .. 400, in the order of the steps; the last class is still open"""
    out = []
    for s in range(1, 401):
        v = variant(lib, kind, (s, s, s))
        if out and out[-1][0] == v:
            out[-1][2] = s
        else:
            out.append([v, s, s])
    return [tuple(c) for c in out]


def edge_steps(lib, kind):
    """[(steps, class)]: the first and the last step of every class (the open end of the exact class left out)"""
    cl = classes(lib, kind)
    cases = []
    for i, (v, first, last) in enumerate(cl):
        for s in (first, last) if i + 1 < len(cl) else (first,):
            if ((s, s, s), v) not in cases:
                cases.append(((s, s, s), v))
    return cases


def step_cases(lib, kind):
    """edge_steps and the last step of the last fast class in each channel in turn, beside steps 1 and 2"""
    cases = edge_steps(lib, kind)
    assert [s[0] for s, _ in cases] == EDGE_STEPS[kind], (NAMES[kind], cases)
    v, _, top = classes(lib, kind)[-2]
    for steps in ((top, 1, 2), (2, top, 1), (1, 2, top)):
        if (steps, v) not in cases:
            cases.append((steps, v))
    return cases


def last_steps(lib, kind):
    """[(class, its last step)] of the classes that assume something (3, 2, 1)"""
    return [(v, last) for v, _, last in classes(lib, kind)[:-1]]


# ---- volumes ----
_volumes = {}


def worst_signs(kind, shape) -> np.ndarray:
    pw, ph, pf = R3.padded_dims(*shape)
    return X.worst_volume(kind, (pf, ph, pw), SHAPES[shape][1])


def volumes(kind, shape):
    """{name: [Y, Co, Cg] flat u16 symbols of the padded volume}: 'worst' and one 'loud<seed>' per seed of the shape"""
    if (kind, shape) not in _volumes:
        pw, ph, pf = R3.padded_dims(*shape)
        s = worst_signs(kind, shape)
        vols = {"worst": [X.wide_symbols_extreme(s), X.wide_symbols_extreme(-s), X.wide_symbols_extreme(s)]}
        for seed in SHAPES[shape][2]:
            vols[f"loud{seed}"] = [X.loud_random_wide((pf, ph, pw), seed + 3 * kind + c) for c in range(3)]
        vols = {k: [z.reshape(-1) for z in v] for k, v in vols.items()}
        for v in vols.values():
            for z in v:
                z.setflags(write=False)
        _volumes[(kind, shape)] = vols
    return _volumes[(kind, shape)]


def cases(lib, kind, shape):
    """[(volume name, steps, class)]: every volume at every step case"""
    return [(name, steps, v) for steps, v in step_cases(lib, kind) for name in volumes(kind, shape)]


# ---- references ----
_channels = {}


def _channel(kind, shape, name, c, step, mirrored) -> np.ndarray:
    """channel c of the volume through the mirrored (or the reference's) inverse at one step: the cropped i16 plane"""
    if name == "worst" and c == 2:
        c = 0       # the same symbols
    key = (kind, shape, name, c, int(step), mirrored)
    if key not in _channels:
        w, h, f = shape
        pw, ph, pf = R3.padded_dims(w, h, f)
        coef = X.dequantised(R3.from_wide_symbols(volumes(kind, shape)[name][c]), step)
        if mirrored:
            vol = RR.mirror_wavelet3d(kind, coef, pw, ph, pf)
        else:
            vol = o.wavelet3d(kind, coef, pw, ph, pf, inverse=True)
        plane = o._wrap16(np.asarray(vol).reshape(pf, ph, pw)[:f, :h, :w].reshape(-1))
        plane.setflags(write=False)
        _channels[key] = plane
    return _channels[key]


def reference(kind, shape, name, steps, mirrored=True) -> np.ndarray:
    """interleaved RGB: reversible_ref.inverse_quantised (mirrored) or transform_extremes.inverse_quantised_steps (the
    control) of the volume, assembled from per-channel planes that the step cases share"""
    return o.ycocg_r_to_rgb(*[_channel(kind, shape, name, c, steps[c], mirrored) for c in range(3)])


def differing_pixels(kind, shape, name, steps) -> int:
    """the number of pixels at which the mirrored and the reference's decode of the same container differ"""
    a, b = reference(kind, shape, name, steps, True), reference(kind, shape, name, steps, False)
    return int((a.reshape(-1, 3) != b.reshape(-1, 3)).any(axis=1).sum())


# ---- containers ----
_payloads = {}


def container(kind, shape, name, steps, version) -> bytes:
    """wide_ref.write_container of the volume, coded once per (wavelet, shape, volume) -- the payloads do not depend on the
    steps --, with the header's steps and byte 4 patched"""
    key = (kind, shape, name)
    if key not in _payloads:
        w, h, f = shape
        _payloads[key] = R3.write_container(kind, w, h, f, LANE_SYMBOLS, (1, 1, 1), volumes(kind, shape)[name])
    blob = bytearray(_payloads[key])
    for c in range(3):
        at = R3.FIXED + c * R3.CHANNEL
        blob[at:at + 8] = int(steps[c]).to_bytes(4, "little", signed=True) * 2       # step and dead zone
    assert R3.parse_container(bytes(blob))["step"] == list(steps)
    return RR.with_version(bytes(blob), version)


# ---- the top of the forward range ----
PAIRS = {"red/blue": ((255, 0, 0), (0, 0, 255), 1), "green/magenta": ((0, 255, 0), (255, 0, 255), 2)}   # -> the channel at +-255
FORWARD_TOP = {CDF53: 2040, CDF97: 1177, HAAR: 2040}


def top_of_range_content(kind, pair, shape=DEVICE_SHAPE) -> np.ndarray:
    """RGB whose Co (Cg) is +-255 with the signs that drive the forward transform highest"""
    w, h, f = shape
    plus, minus, _ = PAIRS[pair]
    signs = X.worst_volume(kind, (f, h, w), (1, 47, 143), inverse=False)
    return np.where(signs[..., None] > 0, np.array(plus, np.uint8), np.array(minus, np.uint8)).astype(np.uint8).reshape(-1)
