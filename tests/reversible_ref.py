"""Plain numpy restatement of the reversible format (.alc version 4), written from DESIGN.md section 12 and not from the
kernels.  Version 4 is version 3 with another version byte and a decoder whose inverse lifting is the forward's mirror, so
this module holds the mirrored inverse and reuses everything else: the forward transform, quantiser, colour and padding of
oracle/alice_oracle_np.py (as wide_oracle does), and the lanes and the container of wide_ref with byte 4 changed."""
from __future__ import annotations

import numpy as np

import oracle.alice_oracle_np as o
import wide_oracle as WO
import wide_ref as W3

VERSION = 4


# ---- 12.2 the mirrored inverse ----
def mirror_axis(v, axis: int, steps, watch=None) -> np.ndarray:
    """The inverse of o._lift_axis(v, axis, steps, False) along `axis`, every line at once: interleave, then the lifting
    steps in reverse order, each one target = wrapping_sub(target, delta(neighbours, +c)) with the forward's delta and the
    forward's boundary neighbours.  watch(pair_sum, coeff): called with every wrapped neighbour sum and its coefficient."""
    v = np.moveaxis(np.asarray(v, np.int64), axis, 0).copy()
    n = v.shape[0]
    if n < 2:
        return np.moveaxis(v, 0, axis)
    half = n // 2
    t = np.zeros_like(v)
    t[0:2 * half:2] = v[:half]
    t[1:2 * half:2] = v[half:2 * half]
    v = t
    for coeff, predict in reversed(steps):
        even = v[0:2 * half:2]
        odd = v[1:2 * half:2]
        if predict:     # the odd samples lose what the forward's predict step gave them
            right = np.empty_like(even)
            right[:-1] = even[1:]
            right[-1] = v[2 * half] if 2 * half < n else even[-1]
            if watch is not None:
                watch(o._wrap32(even + right), coeff)
            v[1:2 * half:2] = o._wrap32(odd - o._delta(even, right, coeff))
        else:           # the even samples lose what the forward's update step gave them
            left = np.empty_like(odd)
            left[1:] = odd[:-1]
            left[0] = odd[0]
            if watch is not None:
                watch(o._wrap32(left + odd), coeff)
            v[0:2 * half:2] = o._wrap32(even - o._delta(left, odd, coeff))
    return np.moveaxis(v, 0, axis)


def mirror_wavelet3d(kind: int, volume, width: int, height: int, depth: int) -> np.ndarray:
    """Temporal, columns, rows -- the axis order of the reference's inverse."""
    v = np.asarray(volume, np.int64).reshape(depth, height, width)
    for axis in (0, 1, 2):
        v = mirror_axis(v, axis, o.STEPS[kind])
    return v.reshape(-1).astype(np.int32)


def per_pass_mirror(kind: int, coef_volume):
    """The mirrored twin of transform_extremes.per_pass_maxima for a (pf, ph, pw[, k]) coefficient volume:
    -> (maxima after the temporal / column / row pass, largest |neighbour sum|, largest |neighbour sum * c| + 4096), each
    per trailing index k when there is one."""
    v = np.asarray(coef_volume, np.int64)
    k = 1 if v.ndim == 3 else v.shape[3]
    pair = np.zeros(k, np.int64)
    prod = np.zeros(k, np.int64)

    def watch(s, coeff):
        m = np.abs(s).reshape(-1, k).max(axis=0)
        np.maximum(pair, m, out=pair)
        np.maximum(prod, m * abs(int(coeff)) + 4096, out=prod)

    maxima = []
    for axis in (0, 1, 2):
        v = mirror_axis(v, axis, o.STEPS[kind], watch)
        maxima.append(np.abs(v).reshape(-1, k).max(axis=0))
    if np.ndim(coef_volume) == 3:
        return tuple(int(m[0]) for m in maxima), int(pair[0]), int(prod[0])
    return tuple(maxima), pair, prod


# ---- decoder from quantised coefficients ----
def inverse_quantised(qs, steps, dims, w: int, h: int, f: int, kind: int) -> np.ndarray:
    """wide_oracle.inverse_quantised with the mirrored inverse and steps[c] for channel c; dims = (pw, ph, pf)."""
    pw, ph, pf = dims
    chans = []
    for q, step in zip(qs, steps):
        coef = o._wrap32(np.asarray(q, np.int64) * int(step))
        vol = mirror_wavelet3d(kind, coef, pw, ph, pf).reshape(pf, ph, pw)
        chans.append(o._wrap16(vol[:f, :h, :w].reshape(-1)))
    return o.ycocg_r_to_rgb(*chans)


def roundtrip(rgb, w: int, h: int, f: int, quality: int, kind: int, mirrored: bool = True) -> np.ndarray:
    """Forward pass, quantiser and dequantiser of the oracle around the mirrored (or the reference's) inverse -> RGB."""
    step, dims, qs = WO.forward_quantised(o, rgb, w, h, f, quality, kind)
    if mirrored:
        return inverse_quantised(qs, (step,) * 3, dims, w, h, f, kind)
    return WO.inverse_quantised(o, qs, step, dims, w, h, f, kind)


# ---- 12.1 container ----
def with_version(data: bytes, version: int) -> bytes:
    d = bytearray(data)
    d[4] = version
    return bytes(d)


def encode(rgb, w: int, h: int, f: int, quality: int, kind: int, L: int = 512) -> bytes:
    """The version 4 bytes: version 3's (wide_ref.write_container) with byte 4 set to 4."""
    step, _, qs = WO.forward_quantised(o, rgb, w, h, f, quality, kind)
    return with_version(W3.write_container(kind, w, h, f, L, (step,) * 3, [W3.wide_symbols(q) for q in qs]), VERSION)


def parse_container(data):
    """Refuses every version byte but 4; the rest is section 11's parser."""
    d = bytes(data)
    if len(d) >= W3.FIXED and d[:4] == b"ALCC" and d[4] != VERSION:
        raise W3.InvalidBitstream("version")
    return W3.parse_container(with_version(d, W3.VERSION) if len(d) > 4 else d)


def decode(data) -> np.ndarray:
    """-> interleaved RGB of a version 4 container.  Raises InvalidBitstream as wide_ref does."""
    info = parse_container(data)
    _, syms = W3.decode_container(with_version(bytes(data), W3.VERSION))
    w, h, f = info["width"], info["height"], info["frames"]
    if w * h * f == 0:
        return np.zeros(0, np.uint8)
    dims = W3.padded_dims(w, h, f)
    return inverse_quantised([W3.from_wide_symbols(s) for s in syms], info["step"], dims, w, h, f, info["wavelet"])
