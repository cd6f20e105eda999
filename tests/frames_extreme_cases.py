"""The plan of the frame-range tests at the class edges of the inverse (DESIGN.md sections 7 and 14), CPU only: which shapes,
symbol volumes, quantiser steps and frame ranges tests/test_gpu_frames_extremes.py decodes through the window path, with the
numpy references and the containers, and what tests/test_frames_extremes_host.py holds that plan to without a device.

Volumes are those of tests/transform_extremes.py: the worst-sign volume of the shape centred on a frame T near pf / 2 (wide:
|q| = 2175 in every sample, z = 4349 / 4350, the second channel negated; version 2: the u8 symbols 255 / 254) and loud random
ones.  Steps are the class edges of tests/reversible_extreme_cases.py (versions 3 and 4) and the byte-symbol plan of
tests/transform_extremes.py (version 2).  Ranges are frames_ref.named_ranges and five around T.  Every expected pixel is the
full chunk's numpy inverse sliced to the range; nothing here calls the library but alice_codec_test_inverse_variant, which
names the steps.  Everything is built once per key and never written again; the lane-size and damage cases of the GPU module
are listed at the end."""
from __future__ import annotations

import numpy as np

import frames_ref as FR
import oracle.alice_oracle_np as o
import reversible_extreme_cases as P
import reversible_ref as RR
import split_ref as R2
import transform_extremes as X
import wide_ref as R3

CDF53, CDF97, HAAR = P.CDF53, P.CDF97, P.HAAR
KINDS = P.KINDS
NAMES = P.NAMES
VERSIONS = (2, 3, 4)
LANE_SYMBOLS = 64
# (format, wavelet, class) triples the library can reach: 11 + 10 + 10
EXPECTED = {2: X.EXPECTED_VARIANTS, 3: P.EXPECTED_CLASSES, 4: P.EXPECTED_CLASSES}

# (w, h, f) -> (band target in KiB or None, centre (t, y, x) of the worst volume, seeds of the loud volumes).  Inverse tiles
# are 96 x 32 with a halo of 4.
SHAPES = {
    (104, 40, 16): (None, (8, 31, 95), (500,)),       # tile path: two tile columns with the seam
    (99, 37, 13): (None, (7, 35, 97), (510,)),        # pad row and column; odd f with a pad frame
    (3, 40, 16): (None, (8, 21, 3), (520,)),          # generic path: the whole virtual chunk is lifted, then vol + lo * W * H
    (96, 70, 12): (1, (6, 31, 47), (530,)),           # three tile rows under a band target that cuts the slot of the kept frames
}
CASES = [(shape, kind, version) for shape in SHAPES for kind in KINDS for version in VERSIONS]


def case_id(case) -> str:
    shape, kind, version = case
    return f"{'x'.join(map(str, shape))}-{NAMES[kind].replace(' ', '').replace('/', '')}-v{version}"


def tile_eligible(shape) -> bool:
    return P.tile_eligible(shape)


def dims(shape):
    """(pw, ph, pf)"""
    return R3.padded_dims(*shape)


def centre_frame(kind, shape) -> int:
    """T: the frame the worst volume drives highest"""
    pw, ph, pf = dims(shape)
    return X.worst_position(kind, (pf, ph, pw), SHAPES[shape][1])[0]


# ---- steps ----
def variant(lib, kind, steps, version) -> int:
    return X.variant(lib, kind, steps, int(version != 2))


def step_cases(lib, kind, version):
    """[(steps, class)]"""
    return X.byte_step_cases(lib, kind) if version == 2 else P.step_cases(lib, kind)


def class_edges(lib, kind, version):
    """{class: the (s, s, s) cases at its first and its last step} (the exact class: its first step)"""
    cl = X.classes(lib, kind, int(version != 2))
    return {v: {(first,) * 3, (last,) * 3} if i + 1 < len(cl) else {(first,) * 3} for i, (v, first, last) in enumerate(cl)}


def last_steps(lib, kind, version):
    """[(class, its last step)] of the classes that assume something (3, 2, 1)"""
    return [(v, last) for v, _, last in X.classes(lib, kind, int(version != 2))[:-1]]


# ---- ranges ----
def halo_only_frame(kind, shape) -> int:
    """a frame t != T whose window holds T as a halo frame"""
    f, T, ns = shape[2], centre_frame(kind, shape), FR.LIFT_STEPS[kind]
    t = T + ns if T + ns < f else T - ns
    a, b = FR.frame_window(kind, f, t, t + 1)
    assert 0 <= t < f and t != T and a <= T < b, (kind, shape, T, t, a, b)
    return t


def ranges(kind, shape):
    """frames_ref.named_ranges, then [T, T + 1) and [T + 1, T + 2) (first - a of both parities, so the even and the odd put
    are each the first frame kept), one frame whose window holds T only as a halo frame, and [T - 1, T + 2)"""
    f, T = shape[2], centre_frame(kind, shape)
    assert 1 <= T and T + 2 <= f, (kind, shape, T)
    t = halo_only_frame(kind, shape)
    out = FR.named_ranges(kind, f) + [(T, T + 1), (T + 1, T + 2), (t, t + 1), (T - 1, T + 2)]
    return list(dict.fromkeys(out))


def range_classes(kind, shape, t0, t1) -> set:
    """which of the four kinds of window B.3 asks for this range is"""
    a, b = FR.frame_window(kind, shape[2], t0, t1)
    pf = dims(shape)[2]
    out = set()
    if a > 0 and b < pf:
        out.add("neither_end")
    if a == 0 and b < pf:
        out.add("start_only")
    if a > 0 and b == pf:
        out.add("end_only")
    if t1 - t0 == 1:
        out.add("one_frame")
    return out


WINDOW_KINDS = {"neither_end", "start_only", "end_only", "one_frame"}


# ---- volumes ----
_volumes = {}


def worst_signs(kind, shape) -> np.ndarray:
    pw, ph, pf = dims(shape)
    return X.worst_volume(kind, (pf, ph, pw), SHAPES[shape][1])


def volumes(kind, shape, version):
    """{name: [Y, Co, Cg] flat symbols of the padded volume (u8 for version 2, u16 else)}: 'worst' and 'loud<seed>'"""
    wide = version != 2
    if (kind, shape, wide) not in _volumes:
        pw, ph, pf = dims(shape)
        s = worst_signs(kind, shape)
        extreme, loud = (X.wide_symbols_extreme, X.loud_random_wide) if wide else (X.byte_symbols, X.loud_random_bytes)
        vols = {"worst": [extreme(s), extreme(-s), extreme(s)]}
        for seed in SHAPES[shape][2]:
            vols[f"loud{seed}"] = [loud((pf, ph, pw), seed + 3 * kind + c) for c in range(3)]
        vols = {k: [z.reshape(-1) for z in v] for k, v in vols.items()}
        for v in vols.values():
            for z in v:
                z.setflags(write=False)
        _volumes[(kind, shape, wide)] = vols
    return _volumes[(kind, shape, wide)]


def cases(lib, kind, shape, version):
    """[(volume name, steps, class)]: every volume at every step case"""
    return [(name, steps, v) for steps, v in step_cases(lib, kind, version) for name in volumes(kind, shape, version)]


def quantised(z, version) -> np.ndarray:
    return R3.from_wide_symbols(z) if version != 2 else o.from_symbols(np.asarray(z, np.uint8))


def inverse(kind, coef, pw, ph, pf, mirrored) -> np.ndarray:
    """the numpy inverse of one channel: (pf, ph, pw) i32"""
    if mirrored:
        vol = RR.mirror_wavelet3d(kind, coef, pw, ph, pf)
    else:
        vol = o.wavelet3d(kind, coef, pw, ph, pf, inverse=True)
    return np.asarray(vol).reshape(pf, ph, pw)


# ---- references ----
_planes = {}


def _same_channel(name, c) -> int:
    return 0 if name == "worst" and c == 2 else c      # the same symbols


def plane(kind, shape, version, name, c, step, mirrored) -> np.ndarray:
    """channel c of the full chunk through the numpy inverse at one step: the cropped i16 frames, (f, h * w).  Versions 3
    and 4 share the symbols: the key holds the inverse, not the version."""
    c = _same_channel(name, c)
    key = (kind, shape, version != 2, name, c, int(step), bool(mirrored))
    if key not in _planes:
        w, h, f = shape
        pw, ph, pf = dims(shape)
        coef = X.dequantised(quantised(volumes(kind, shape, version)[name][c], version), step)
        vol = inverse(kind, coef, pw, ph, pf, mirrored)
        p = o._wrap16(vol[:f, :h, :w].reshape(-1)).reshape(f, h * w)
        p.setflags(write=False)
        _planes[key] = p
    return _planes[key]


def window_plane(kind, shape, version, name, c, step, mirrored, a, b) -> np.ndarray:
    """channel c of the virtual chunk of window [a, b) through the numpy inverse: (b - a, h * w) cropped i16 frames, the
    halo frames included (not cached)"""
    w, h, _ = shape
    pw, ph, pf = dims(shape)
    sym = FR.window_volume(volumes(kind, shape, version)[name][_same_channel(name, c)], (pw, ph, pf), a, b)
    vol = inverse(kind, X.dequantised(quantised(sym.reshape(-1), version), step), pw, ph, b - a, mirrored)
    return o._wrap16(vol[:, :h, :w].reshape(-1)).reshape(b - a, h * w)


def reference(kind, shape, version, name, steps, t0, t1, mirrored=None) -> np.ndarray:
    """interleaved RGB of frames [t0, t1): the full chunk's numpy inverse (the mirrored one for version 4 unless told
    otherwise), sliced, then the colour step"""
    m = (version == 4) if mirrored is None else mirrored
    return o.ycocg_r_to_rgb(*[plane(kind, shape, version, name, c, steps[c], m)[t0:t1].reshape(-1) for c in range(3)])


def differing_pixels(kind, shape, name, steps, t0, t1) -> int:
    """the number of pixels of frames [t0, t1) at which the mirrored and the reference's decode of the same wide container
    differ"""
    a, b = (reference(kind, shape, 4, name, steps, t0, t1, m) for m in (True, False))
    return int((a.reshape(-1, 3) != b.reshape(-1, 3)).any(axis=1).sum())


# ---- containers ----
_payloads = {}


def container(kind, shape, name, steps, version) -> bytes:
    """split_ref / wide_ref write_container of the volume, coded once per (wavelet, shape, volume, symbol width) -- the
    payloads do not depend on the steps --, with the header's steps (and byte 4 for version 4) patched"""
    ref = R2 if version == 2 else R3
    key = (kind, shape, name, version != 2)
    if key not in _payloads:
        w, h, f = shape
        _payloads[key] = ref.write_container(kind, w, h, f, LANE_SYMBOLS, (1, 1, 1), volumes(kind, shape, version)[name])
    blob = bytearray(_payloads[key])
    for c in range(3):
        at = ref.FIXED + c * ref.CHANNEL
        blob[at:at + 8] = int(steps[c]).to_bytes(4, "little", signed=True) * 2       # step and dead zone
    assert ref.parse_container(bytes(blob))["step"] == list(steps)
    return bytes(blob) if version != 4 else RR.with_version(bytes(blob), 4)


# ---- lane sizes (C.3) ----
LANE_SHAPE = (128, 96, 40)            # 491520 symbols per channel: 60 blocks at L = 128, 15 at 512, 3.75 at 2048, one at the maximum
LANE_SIZES = {2: (128, 512, 2048, 16384), 3: (128, 512, 2048, 8192), 4: (128, 512, 2048, 8192)}
LANE_QUALITY = {2: 80, 3: 100, 4: 100}    # step 1 gives the wide symbols escapes (z up to 811); versions 3 and 4 at one
                                          # quality: their bytes differ in byte 4 only
ESCAPE_SHAPE = (104, 40, 16)          # the worst-sign wide volume, every symbol an escape
ESCAPE_LANES = (128, 512)
ESCAPE_STEPS = (2, 2, 2)
LANE_CLASSES = {"edge_inside_block", "shared_block", "short_last_block", "one_block_channel", "blocks_skipped"}


def lane_kind(version, L) -> int:
    """the wavelet of a lane-size case: all three appear at every version, and versions 3 and 4 take the same one at each L
    (their containers then differ in byte 4 only, and the reference lane decode is shared)"""
    return (LANE_SIZES[version].index(L) + (version == 2)) % 3


def lane_ranges(kind, f):
    """named_ranges and six single frames"""
    singles = [(t, t + 1) for t in (1, f // 4, f // 2 - 1, f // 2, 3 * f // 4, f - 2)]
    return list(dict.fromkeys(FR.named_ranges(kind, f) + singles))


# ---- damage (C.4) ----
DAMAGE_SHAPE, DAMAGE_KIND = (50, 38, 13), CDF97
# Planes of 1900 symbols in blocks of 4096.  No range of this shape has a clipped start, a clipped end and a shared block at
# once: the low range reaches the block in which the high range starts (block 3) only when b = pf, and then the high range
# ends with the channel.  So two ranges carry the three classes: [6, 7) (window [2, 12): both ends clipped) and [7, 10)
# (window [2, 14): clipped start, low and high range inside block 3).  With CDF 9/7 both plan all seven blocks; [12, 13)
# (window [8, 14): blocks 1 to 3 and 5 to 6, every inner edge inside a block) leaves blocks 0 and 4 unplanned.
DAMAGE_CLIPPED = (6, 7)
DAMAGE_SHARED = (7, 10)
DAMAGE_SKIPPING = (12, 13)
