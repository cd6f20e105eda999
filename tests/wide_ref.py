"""Plain numpy restatement of the wide format (.alc version 3), written from DESIGN.md section 11 and not from the
kernels: the wide symbol map, the coded symbol with its escape, the per-lane rANS coder with the 12-bit residual step, the
container writer and parser, and a decoder with the end check.  Normalisation, the running sum and the padded dimensions
are version 2's (section 10.2 / 10.1) and come from split_ref.  As there, the coder is vectorised ACROSS lanes."""
from __future__ import annotations

import struct

import numpy as np

from split_ref import InvalidBitstream, cumulative, normalize, padded_dims  # noqa: F401  (re-exported)

SCALE_BITS = 12
SCALE = 1 << SCALE_BITS
RANS_L = 1 << 23
FIXED = 22
CHANNEL = 536
HEADER = FIXED + 3 * CHANNEL
ESCAPE = 255
RES_BITS = 12
RES_MAX = (1 << RES_BITS) - 1
VERSION = 3


def wide_symbols(q) -> np.ndarray:
    """11.2: z = 0 for q = 0, 2q - 1 for q > 0, -2q for q < 0; nothing is truncated."""
    q = np.asarray(q, np.int64)
    z = np.where(q > 0, 2 * q - 1, -2 * q)
    assert z.max(initial=0) <= 0xFFFF
    return z.astype(np.uint16)


def from_wide_symbols(z) -> np.ndarray:
    z = np.asarray(z, np.int64)
    return np.where(z & 1, (z + 1) >> 1, -(z >> 1)).astype(np.int32)


def coded(z) -> np.ndarray:
    return np.minimum(np.asarray(z, np.int64), ESCAPE)


def histogram(z) -> np.ndarray:
    return np.bincount(coded(z).reshape(-1), minlength=256).astype(np.uint32)


def n_blocks_of(n: int, L: int) -> int:
    return (n + 64 * L - 1) // (64 * L)


def lane_ok(L: int) -> bool:
    return 64 <= L <= 8192 and (L & (L - 1)) == 0


def stream_bound(n: int, L: int) -> int:
    """4 bytes per symbol, and per block its length, its directory and 4 state bytes per lane."""
    return n_blocks_of(n, L) * (4 + 128 + 64 * 4) + 4 * n


def _lane_counts(n: int, L: int) -> np.ndarray:
    nb = n_blocks_of(n, L)
    in_block = np.minimum(64 * L, n - np.arange(nb, dtype=np.int64) * 64 * L)
    j = np.arange(64, dtype=np.int64)
    return np.maximum(0, (in_block[:, None] - j[None, :] + 63) // 64)


# ---- 11.3 one channel ----
def encode_channel(symbols, freq, L: int) -> bytes:
    z = np.asarray(symbols, np.uint16).reshape(-1).astype(np.int64)
    n = z.size
    if n == 0:
        return b""
    assert lane_ok(L)
    if int(z.max()) - ESCAPE > RES_MAX:
        raise ValueError("a residual above 4095 has no code")
    f = np.asarray(freq, np.int64)
    assert int(f.sum()) == SCALE and np.all(f[np.unique(coded(z))] >= 1)
    c = cumulative(f)
    nb = n_blocks_of(n, L)
    k = _lane_counts(n, L).reshape(-1)
    pad = np.zeros(nb * 64 * L, np.int64)
    pad[:n] = z
    Z = pad.reshape(nb, L, 64).transpose(1, 0, 2).reshape(L, nb * 64)   # Z[i, lane]
    lanes = nb * 64
    cap = 4 * L + 4
    buf = np.zeros((lanes, cap), np.uint8)
    cur = np.full(lanes, cap, np.int64)
    x = np.full(lanes, RANS_L, np.int64)
    idx = np.arange(lanes)

    def emit(mask, byte):
        cur[mask] -= 1
        buf[idx[mask], cur[mask]] = byte[mask]

    for i in range(L - 1, -1, -1):
        act = k > i
        if not act.any():
            continue
        zi = Z[i]
        esc = act & (zi >= ESCAPE)
        if esc.any():   # the residual first: the decoder meets it after the escape
            for _ in range(2):
                m = esc & (x >= (1 << 19))
                emit(m, (x & 255).astype(np.uint8))
                x = np.where(m, x >> 8, x)
            assert not (esc & (x >= (1 << 19))).any()
            x = np.where(esc, (x << RES_BITS) + (zi - ESCAPE), x)
        s = np.minimum(zi, ESCAPE)
        fs = f[s]
        cs = c[s]
        xmax = fs << 19
        for _ in range(2):
            m = act & (x >= xmax)
            emit(m, (x & 255).astype(np.uint8))
            x = np.where(m, x >> 8, x)
        assert not (act & (x >= xmax)).any()
        fs1 = np.where(act, fs, 1)
        x = np.where(act, ((x // fs1) << SCALE_BITS) + (x % fs1) + cs, x)
        assert int(x.max()) < (1 << 31)
    has = k > 0
    for sh in (0, 8, 16, 24):
        emit(has, ((x >> sh) & 255).astype(np.uint8))
    lens = (cap - cur).astype(np.int64)
    out = bytearray()
    blocks = []
    for b in range(nb):
        body = bytearray()
        for j in range(64):
            body += struct.pack("<H", int(lens[b * 64 + j]))
        for j in range(64):
            lane = b * 64 + j
            body += buf[lane, cur[lane]:].tobytes()
        blocks.append(bytes(body))
    for blk in blocks:
        out += struct.pack("<I", len(blk))
    for blk in blocks:
        out += blk
    return bytes(out)


def decode_channel(payload, freq, L: int, n: int):
    """-> (u16 symbols, ok).  ok is False when a directory does not add up or a lane fails its end check."""
    p = np.frombuffer(bytes(payload), np.uint8)
    if n == 0:
        return np.zeros(0, np.uint16), p.size == 0
    f = np.asarray(freq, np.int64)
    assert int(f.sum()) == SCALE
    c = cumulative(f)
    c2s = np.repeat(np.arange(256), f).astype(np.int64)
    nb = n_blocks_of(n, L)
    out = np.zeros(nb * 64 * L, np.uint16)
    if 4 * nb > p.size:
        return out[:n], False
    blen = p[:4 * nb].view("<u4").astype(np.int64)
    boff = 4 * nb + np.cumsum(blen) - blen
    if (blen < 128).any() or int(boff[-1] + blen[-1]) != p.size:
        return out[:n], False
    dirs = np.stack([p[o:o + 128].view("<u2").astype(np.int64) for o in boff])
    if (dirs.sum(axis=1) + 128 != blen).any():
        return out[:n], False
    start = (boff[:, None] + 128 + np.cumsum(dirs, axis=1) - dirs).reshape(-1)
    lens = dirs.reshape(-1)
    k = _lane_counts(n, L).reshape(-1)
    lanes = nb * 64
    pos = np.zeros(lanes, np.int64)
    pz = np.concatenate([p, np.zeros(1, np.uint8)]).astype(np.int64)

    def take(mask):
        inside = mask & (pos < lens)
        byte = np.where(inside, pz[np.where(inside, start + pos, p.size)], 0)
        pos[mask] += 1
        return byte

    has = k > 0
    x = np.zeros(lanes, np.int64)
    for _ in range(4):
        x = np.where(has, (x << 8) | take(has), x)
    O = out.reshape(nb, L, 64)
    for i in range(L):
        act = k > i
        if not act.any():
            break
        slot = x & (SCALE - 1)
        s = c2s[slot]
        x = np.where(act, (f[s] * (x >> SCALE_BITS) + slot - c[s]) & 0xFFFFFFFF, x)
        for _ in range(2):
            m = act & (x < RANS_L)
            x = np.where(m, ((x << 8) | take(m)) & 0xFFFFFFFF, x)
        esc = act & (s == ESCAPE)
        zz = s.copy()
        if esc.any():
            zz = np.where(esc, ESCAPE + (x & RES_MAX), zz)
            x = np.where(esc, x >> RES_BITS, x)
            for _ in range(2):
                m = esc & (x < RANS_L)
                x = np.where(m, ((x << 8) | take(m)) & 0xFFFFFFFF, x)
        O[:, i, :] = np.where(act, zz, 0).astype(np.uint16).reshape(nb, 64)
    ok = bool(np.all(np.where(has, (x == RANS_L) & (pos == lens), lens == 0)))
    return out[:n], ok


# ---- 11.1 container ----
def write_container(wavelet: int, w: int, h: int, f: int, L: int, steps, channels_symbols) -> bytes:
    """channels_symbols: three u16 arrays (Y, Co, Cg) of the padded volume each."""
    out = bytearray(b"ALCC" + bytes([VERSION, wavelet]) + struct.pack("<IIII", w, h, f, L))
    payloads = []
    for c in range(3):
        z = np.asarray(channels_symbols[c], np.uint16).reshape(-1)
        freq = normalize(histogram(z))
        pay = encode_channel(z, freq, L)
        payloads.append(pay)
        out += struct.pack("<iiIIQ", int(steps[c]), int(steps[c]), z.size, n_blocks_of(z.size, L), len(pay))
        out += freq.astype("<u2").tobytes()
    for pay in payloads:
        out += pay
    return bytes(out)


def parse_container(data):
    """-> dict of the header fields, 'freq' [3][256] and 'payload' [3] bytes.  Raises InvalidBitstream; the checks run in
    the order of section 10.5 with the lane range of section 11."""
    d = bytes(data)
    if len(d) < FIXED:
        raise InvalidBitstream("too short")
    if d[:4] != b"ALCC":
        raise InvalidBitstream("magic")
    if d[4] != VERSION:
        raise InvalidBitstream("version")
    if d[5] > 2:
        raise InvalidBitstream("wavelet")
    w, h, f, L = struct.unpack_from("<IIII", d, 6)
    if not lane_ok(L):
        raise InvalidBitstream("lane_symbols")
    if len(d) < HEADER:
        raise InvalidBitstream("too short for the header")
    pw, ph, pf = padded_dims(w, h, f)
    padded = pw * ph * pf
    info = dict(wavelet=d[5], width=w, height=h, frames=f, lane_symbols=L, step=[], dead_zone=[], num_symbols=[], n_blocks=[],
                payload_len=[], freq=[], payload=[])
    total = HEADER
    for c in range(3):
        o = FIXED + c * CHANNEL
        step, dz, ns, nb, plen = struct.unpack_from("<iiIIQ", d, o)
        freq = np.frombuffer(d, "<u2", 256, o + 24).astype(np.uint16)
        if step < 1 or dz < 0:
            raise InvalidBitstream("quantiser step")
        if ns != padded:
            raise InvalidBitstream("num_symbols")
        if nb != n_blocks_of(padded, L):
            raise InvalidBitstream("n_blocks")
        if int(freq.astype(np.int64).sum()) != (SCALE if padded else 0):
            raise InvalidBitstream("frequency sum")
        if plen < 132 * nb:
            raise InvalidBitstream("payload_len")
        for key, v in (("step", step), ("dead_zone", dz), ("num_symbols", ns), ("n_blocks", nb), ("payload_len", plen), ("freq", freq)):
            info[key].append(v)
        total += plen
    if total != len(d):
        raise InvalidBitstream("total length")
    o = HEADER
    for c in range(3):
        pay = d[o:o + info["payload_len"][c]]
        nb = info["n_blocks"][c]
        blen = np.frombuffer(pay, "<u4", nb).astype(np.int64)
        if (blen < 128).any() or 4 * nb + int(blen.sum()) != len(pay):
            raise InvalidBitstream("block lengths")
        info["payload"].append(pay)
        o += len(pay)
    return info


def decode_container(data):
    """-> (info, [Y, Co, Cg] u16 symbols).  Raises InvalidBitstream when a lane fails its end check."""
    info = parse_container(data)
    syms = []
    for c in range(3):
        s, ok = decode_channel(info["payload"][c], info["freq"][c], info["lane_symbols"], info["num_symbols"][c])
        if not ok:
            raise InvalidBitstream("end check")
        syms.append(s)
    return info, syms
