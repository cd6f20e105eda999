"""Plain numpy restatement of the transcode of version 2, 3 and 4 chunks, written from DESIGN.md section 19 and not from the
kernels: the map of one symbol, the transcoded container, its size brackets and the budget rule.  Everything else is the
existing references': the containers and lane coders of split_ref / wide_ref (version 4 through reversible_ref.with_version),
the quantiser of oracle/alice_oracle_np.py, and the brackets and the chooser of split_rate_ref / wide_rate_ref."""
from __future__ import annotations

import functools
import struct

import numpy as np

import oracle.alice_oracle_np as o
import reversible_ref as R4
import split_rate_ref as SR
import split_ref as R2
import wide_rate_ref as WR
import wide_ref as W3
from split_ref import InvalidBitstream  # noqa: F401  (re-exported)

FIXED, CHANNEL, HEADER = R2.FIXED, R2.CHANNEL, R2.HEADER


class InvalidDimensions(Exception):
    pass


def coefficient(sym) -> np.ndarray:
    """19.1: what the container's decoder makes of a symbol (u8 of version 2, untruncated z of versions 3 and 4)."""
    z = np.asarray(sym, np.int64)
    return np.where(z & 1, (z + 1) >> 1, -(z >> 1))


def centre(sym, s1: int) -> np.ndarray:
    """19.1: m, the value the target quantiser sees -- the centre of the source interval, both divisions integer."""
    q1 = coefficient(sym)
    return np.sign(q1) * np.where(q1 == 0, 0, np.abs(q1) * s1 + s1 // 2 + s1 // 2)


def requant(sym, s1: int, s2: int, wide: bool) -> np.ndarray:
    """19.1: the symbols of a channel at target step s2; the channel is untouched unless the target is coarser."""
    if s2 <= s1:
        return np.array(sym, np.uint16 if wide else np.uint8)
    q2 = o.quantize(centre(sym, s1), s2, s2)
    return W3.wide_symbols(q2) if wide else o.to_symbols(q2)


def _version(data: bytes) -> int:
    if len(data) < FIXED:
        raise InvalidBitstream("too short")
    if data[:4] != b"ALCC":
        raise InvalidBitstream("magic")
    if not 2 <= data[4] <= 4:
        raise InvalidBitstream("version")
    return data[4]


@functools.lru_cache(maxsize=64)
def _decoded(data: bytes):
    """(version, info, [Y, Co, Cg] symbols), decoded once per container"""
    v = _version(data)
    if v == 2:
        info, syms = R2.decode_container(data)
    else:
        info, syms = W3.decode_container(R4.with_version(data, W3.VERSION))
    for s in syms:
        s.setflags(write=False)
    return v, info, syms


def _arguments(v: int, info, L: int, out_version: int):
    L = L or info["lane_symbols"]
    if not (W3.lane_ok(L) if v >= 3 else R2.lane_ok(L)):
        raise InvalidDimensions("lane_symbols")
    if not (out_version == 0 or (v >= 3 and out_version in (3, 4))):
        raise InvalidDimensions("out_version")
    return L, out_version or v


def transcode(data, quality: int, L: int = 0, out_version: int = 0) -> bytes:
    """19.1 / 19.3: the transcoded container.  Raises InvalidBitstream for a source no decode call accepts (version 1
    included) and InvalidDimensions for the two optional arguments."""
    data = bytes(data)
    v, info, syms = _decoded(data)
    L, out_v = _arguments(v, info, L, out_version)
    s2 = SR.quality_to_step(quality)
    wide = v >= 3
    steps, dead, new = [], [], []
    for c in range(3):
        s1 = info["step"][c]
        coarser = s2 > s1
        steps.append(s2 if coarser else s1)
        dead.append(s2 if coarser else info["dead_zone"][c])
        new.append(requant(syms[c], s1, s2, wide))
    write = W3.write_container if wide else R2.write_container
    out = bytearray(write(info["wavelet"], info["width"], info["height"], info["frames"], L, steps, new))
    for c in range(3):   # (the writers store dead zone = step: an untouched channel keeps its own)
        struct.pack_into("<i", out, FIXED + c * CHANNEL + 4, dead[c])
    out[4] = out_v
    return bytes(out)


def step_histograms(data) -> np.ndarray:
    """19.4: (64, 3, 256) histograms of the coded symbol of every channel at every target step; the rows at or below a
    channel's own step are its own histogram."""
    v, info, syms = _decoded(bytes(data))
    wide = v >= 3
    out = np.zeros((64, 3, 256), np.uint32)
    for c in range(3):
        for step in range(1, 65):
            z = requant(syms[c], info["step"][c], step, wide)
            out[step - 1, c] = W3.histogram(z) if wide else np.bincount(z, minlength=256)
    return out


def predict(data, L: int = 0):
    """19.4: (lo[101], hi[101]) of transcode(data, q, L)."""
    v, info, _ = _decoded(bytes(data))
    L, _ = _arguments(v, info, L, 0)
    return (WR if v >= 3 else SR).chunk_prediction(step_histograms(data), L)


def choose_transcode(data, budget: int, min_q: int, max_q: int, L: int = 0, out_version: int = 0):
    """19.4: (quality, fits, trials, bytes) of a budget transcode: split_rate_ref.choose over predict's brackets, a trial
    being the exact size of transcode at that quality."""
    data = bytes(data)
    v, info, _ = _decoded(data)
    _, out_v = _arguments(v, info, L, out_version)
    if min(min_q, 100) > min(max_q, 100):
        raise InvalidDimensions("min_quality > max_quality")
    if out_v == 4:
        raise InvalidBitstream("a version 4 result has no byte budget")
    lo, hi = predict(data, L)
    q, fits, trials = SR.choose(lo, hi, budget, min_q, max_q, lambda q: len(transcode(data, q, L, out_version)))
    return q, fits, trials, transcode(data, q, L, out_version)
