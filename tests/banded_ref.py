"""Plain numpy restatement of the banded format (.alc version 5), written from DESIGN.md section 20 and not from the
kernels: the band boxes and their raster order, one normalised table per band, the container writer and parser with the
checks in their order, a decoder with the end checks, and the repack in both directions.  The lane coders, normalisation
and containers of the base versions come from split_ref (2), wide_ref (3) and reversible_ref (4); the front end and the
inverses are those modules' too, so a banded chunk decodes through exactly the code its base chunk decodes through."""
from __future__ import annotations

import struct

import numpy as np

import oracle.alice_oracle_np as o
import reversible_ref as R4
import split_ref as R2
import wide_oracle as WO
import wide_ref as R3
from split_ref import InvalidBitstream, normalize, padded_dims  # noqa: F401  (re-exported)

VERSION = 5
FIXED = 24
BAND = 524
CHANNEL = 12 + 8 * BAND
HEADER = FIXED + 3 * CHANNEL
assert HEADER == 12636


def coder(base: int):
    return R2 if base == 2 else R3


def lane_ok(L: int, base: int) -> bool:
    return coder(base).lane_ok(L)


def band_boxes(pw: int, ph: int, pf: int):
    """The eight (t, y, x) slices of a [pf][ph][pw] volume, band k = 4 bt + 2 by + bx ascending."""
    hw, hh, ht = pw // 2, ph // 2, pf // 2
    return [(slice(bt * ht, (bt + 1) * ht), slice(by * hh, (by + 1) * hh), slice(bx * hw, (bx + 1) * hw))
            for bt in (0, 1) for by in (0, 1) for bx in (0, 1)]


def gather_bands(volume, pw: int, ph: int, pf: int):
    """-> eight 1-D arrays: each band's symbols in band order (the raster of its box)."""
    v = np.asarray(volume).reshape(pf, ph, pw)
    return [np.ascontiguousarray(v[box]).reshape(-1) for box in band_boxes(pw, ph, pf)]


def scatter_bands(bands, pw: int, ph: int, pf: int, dtype):
    v = np.zeros((pf, ph, pw), dtype)
    for box, b in zip(band_boxes(pw, ph, pf), bands):
        v[box] = np.asarray(b, dtype).reshape(v[box].shape)
    return v.reshape(-1)


def band_histogram(symbols, base: int) -> np.ndarray:
    s = np.asarray(symbols).reshape(-1).astype(np.int64)
    return np.bincount(np.minimum(s, 255) if base >= 3 else s, minlength=256).astype(np.uint32)


# ---- 20.2 container ----
def write_container(base: int, wavelet: int, w: int, h: int, f: int, L: int, steps, dead_zones, channels_symbols) -> bytes:
    """channels_symbols: three arrays (Y, Co, Cg) of the padded volume each, u8 for base 2 and u16 for bases 3 and 4."""
    assert base in (2, 3, 4) and lane_ok(L, base)
    pw, ph, pf = padded_dims(w, h, f)
    padded = pw * ph * pf
    out = bytearray(b"ALCC" + bytes([VERSION, wavelet]) + struct.pack("<IIII", w, h, f, L) + bytes([base, 0]))
    K = coder(base)
    payloads = []
    for c in range(3):
        out += struct.pack("<iiI", int(steps[c]), int(dead_zones[c]), padded)
        if padded == 0:
            out += bytes(8 * BAND)
            continue
        for band in gather_bands(channels_symbols[c], pw, ph, pf):
            freq = normalize(band_histogram(band, base))
            pay = K.encode_channel(band, freq, L)
            payloads.append(pay)
            out += struct.pack("<IQ", K.n_blocks_of(band.size, L), len(pay)) + freq.astype("<u2").tobytes()
    assert len(out) == HEADER
    for pay in payloads:
        out += pay
    return bytes(out)


def parse_container(data):
    """-> dict of the header fields, 'freq' [24][256] and 'payload' [24] bytes.  Raises InvalidBitstream, each failure with
    the name of its check; the checks run in the order of section 20.3."""
    d = bytes(data)
    if len(d) < FIXED:
        raise InvalidBitstream("fixed length")
    if d[:4] != b"ALCC":
        raise InvalidBitstream("magic")
    if d[4] != VERSION:
        raise InvalidBitstream("version")
    if d[5] > 2:
        raise InvalidBitstream("wavelet")
    w, h, f, L = struct.unpack_from("<IIII", d, 6)
    base = d[22]
    if base not in (2, 3, 4):
        raise InvalidBitstream("base")
    if d[23] != 0:
        raise InvalidBitstream("reserved")
    if not lane_ok(L, base):
        raise InvalidBitstream("lane_symbols")
    if len(d) < HEADER:
        raise InvalidBitstream("header length")
    pw, ph, pf = padded_dims(w, h, f)
    padded = pw * ph * pf
    n_band = padded // 8
    info = dict(wavelet=d[5], width=w, height=h, frames=f, lane_symbols=L, base=base, step=[], dead_zone=[], num_symbols=[],
                n_blocks=[], payload_len=[], freq=[], payload=[])
    total = HEADER
    for c in range(3):
        oc = FIXED + c * CHANNEL
        step, dz, ns = struct.unpack_from("<iiI", d, oc)
        if step < 1 or dz < 0:
            raise InvalidBitstream(f"channel {c}: quantiser step")
        if ns != padded:
            raise InvalidBitstream(f"channel {c}: num_symbols")
        info["step"].append(step); info["dead_zone"].append(dz); info["num_symbols"].append(ns)
        for k in range(8):
            ob = oc + 12 + k * BAND
            nb, plen = struct.unpack_from("<IQ", d, ob)
            freq = np.frombuffer(d, "<u2", 256, ob + 12).astype(np.uint16)
            if nb != R2.n_blocks_of(n_band, L):
                raise InvalidBitstream(f"channel {c} band {k}: n_blocks")
            if int(freq.astype(np.int64).sum()) != (R2.SCALE if padded else 0):
                raise InvalidBitstream(f"channel {c} band {k}: frequency sum")
            if plen < 132 * nb:
                raise InvalidBitstream(f"channel {c} band {k}: payload_len")
            info["n_blocks"].append(nb); info["payload_len"].append(plen); info["freq"].append(freq)
            total += plen
    if total != len(d):
        raise InvalidBitstream("total length")
    at = HEADER
    for j in range(24):
        pay = d[at:at + info["payload_len"][j]]
        nb = info["n_blocks"][j]
        blen = np.frombuffer(pay, "<u4", nb).astype(np.int64)
        if (blen < 128).any() or 4 * nb + int(blen.sum()) != len(pay):
            raise InvalidBitstream(f"channel {j // 8} band {j % 8}: block lengths")
        info["payload"].append(pay)
        at += len(pay)
    return info


def decode_container(data):
    """-> (info, [Y, Co, Cg] symbol volumes).  Raises InvalidBitstream when a lane fails its end check."""
    info = parse_container(data)
    base = info["base"]
    K = coder(base)
    pw, ph, pf = padded_dims(info["width"], info["height"], info["frames"])
    n_band = pw * ph * pf // 8
    dtype = np.uint8 if base == 2 else np.uint16
    syms = []
    for c in range(3):
        bands = []
        for k in range(8):
            j = 8 * c + k
            s, ok = K.decode_channel(info["payload"][j], info["freq"][j], info["lane_symbols"], n_band)
            if not ok:
                raise InvalidBitstream(f"stream {j}: end check")
            bands.append(s)
        syms.append(scatter_bands(bands, pw, ph, pf, dtype) if n_band else np.zeros(0, dtype))
    return info, syms


# ---- pixels ----
def base_symbols(rgb, w: int, h: int, f: int, quality: int, kind: int, base: int):
    """-> (step, the three symbol volumes of the base version)."""
    if w * h * f == 0:
        return o.quality_to_step(quality), [np.zeros(0, np.uint8 if base == 2 else np.uint16)] * 3
    step, _, qs = WO.forward_quantised(o, rgb, w, h, f, quality, kind)
    return step, [o.to_symbols(q) if base == 2 else R3.wide_symbols(q) for q in qs]


def encode_base(rgb, w: int, h: int, f: int, quality: int, kind: int, base: int, L: int = 512) -> bytes:
    """The version `base` container of the input."""
    step, syms = base_symbols(rgb, w, h, f, quality, kind, base)
    if base == 2:
        return R2.write_container(kind, w, h, f, L, (step,) * 3, syms)
    return R4.with_version(R3.write_container(kind, w, h, f, L, (step,) * 3, syms), base)


def encode(rgb, w: int, h: int, f: int, quality: int, kind: int, base: int = 2, L: int = 512) -> bytes:
    step, syms = base_symbols(rgb, w, h, f, quality, kind, base)
    return write_container(base, kind, w, h, f, L, (step,) * 3, (step,) * 3, syms)


def decode_base(data) -> np.ndarray:
    """The reference decode of a version 2, 3 or 4 container -> interleaved RGB."""
    d = bytes(data)
    version = d[4]
    if version == 4:
        return R4.decode(d)
    info, syms = (R2 if version == 2 else R3).decode_container(d)
    return pixels(info, syms, version)


def pixels(info, syms, base: int) -> np.ndarray:
    w, h, f = info["width"], info["height"], info["frames"]
    if w * h * f == 0:
        return np.zeros(0, np.uint8)
    dims = padded_dims(w, h, f)
    qs = [o.from_symbols(s) if base == 2 else R3.from_wide_symbols(s) for s in syms]
    if base == 4:
        return R4.inverse_quantised(qs, info["step"], dims, w, h, f, info["wavelet"])
    assert len(set(info["step"])) == 1
    return WO.inverse_quantised(o, qs, info["step"][0], dims, w, h, f, info["wavelet"])


def decode(data) -> np.ndarray:
    info, syms = decode_container(data)
    return pixels(info, syms, info["base"])


# ---- 20.6 repack ----
def to_banded(data, L: int = 0) -> bytes:
    d = bytes(data)
    base = d[4]
    if base not in (2, 3, 4):
        raise InvalidBitstream("version")
    if base == 4:
        R4.parse_container(d)
        info, syms = R3.decode_container(R4.with_version(d, 3))
    else:
        info, syms = coder(base).decode_container(d)
    return write_container(base, info["wavelet"], info["width"], info["height"], info["frames"], L or info["lane_symbols"], info["step"],
                           info["dead_zone"], syms)


def from_banded(data, L: int = 0) -> bytes:
    info, syms = decode_container(data)
    base = info["base"]
    L = L or info["lane_symbols"]
    K = coder(base)
    # the base writers store step as dead zone; a repack keeps the dead zone that is stored
    out = bytearray(K.write_container(info["wavelet"], info["width"], info["height"], info["frames"], L, info["step"], syms))
    out[4] = base
    for c in range(3):
        struct.pack_into("<i", out, R2.FIXED + c * R2.CHANNEL + 4, info["dead_zone"][c])
    return bytes(out)
