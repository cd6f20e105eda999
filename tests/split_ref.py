"""Plain numpy restatement of the split-stream format (.alc version 2), written from DESIGN.md section 10 and not from
the kernels: normalisation, lane split, the per-lane rANS coder, the container writer and parser, and a decoder with the
end check.  The lanes of a channel are independent, so the coder is vectorised ACROSS lanes (one numpy step per symbol
position); inside a lane it is the textbook loop of section 10.3."""
from __future__ import annotations

import struct

import numpy as np

SCALE_BITS = 12
SCALE = 1 << SCALE_BITS
RANS_L = 1 << 23
FIXED = 22
CHANNEL = 536
HEADER = FIXED + 3 * CHANNEL


class InvalidBitstream(Exception):
    pass


# ---- 10.2 normalisation ----
def normalize(hist) -> np.ndarray:
    h = [int(v) for v in hist]
    assert len(h) == 256
    total = sum(h)
    f = [0] * 256
    if total == 0:
        return np.zeros(256, np.uint16)
    for s in range(256):
        if h[s]:
            f[s] = max(1, h[s] * SCALE // total)
    ssum = sum(f)
    if ssum < SCALE:
        top = max(range(256), key=lambda s: (f[s], -s))
        f[top] += SCALE - ssum
    while ssum > SCALE:
        top = max(range(256), key=lambda s: (f[s], -s))
        f[top] -= 1
        ssum -= 1
    return np.array(f, np.uint16)


def cumulative(freq) -> np.ndarray:
    f = np.asarray(freq, np.int64)
    return (np.cumsum(f) - f).astype(np.int64)


def n_blocks_of(n: int, L: int) -> int:
    return (n + 64 * L - 1) // (64 * L)


def lane_ok(L: int) -> bool:
    return 64 <= L <= 16384 and (L & (L - 1)) == 0


def _lane_counts(n: int, L: int) -> np.ndarray:
    """k[b, j]: symbols of lane j of block b."""
    nb = n_blocks_of(n, L)
    in_block = np.minimum(64 * L, n - np.arange(nb, dtype=np.int64) * 64 * L)
    j = np.arange(64, dtype=np.int64)
    return np.maximum(0, (in_block[:, None] - j[None, :] + 63) // 64)


# ---- 10.3 / 10.4 one channel ----
def encode_channel(symbols, freq, L: int) -> bytes:
    sym = np.asarray(symbols, np.uint8).reshape(-1)
    n = sym.size
    if n == 0:
        return b""
    assert lane_ok(L)
    f = np.asarray(freq, np.int64)
    assert int(f.sum()) == SCALE and np.all(f[np.unique(sym)] >= 1)
    c = cumulative(f)
    nb = n_blocks_of(n, L)
    k = _lane_counts(n, L).reshape(-1)                       # per lane (block-major)
    pad = np.zeros(nb * 64 * L, np.uint8)
    pad[:n] = sym
    S = pad.reshape(nb, L, 64).transpose(1, 0, 2).reshape(L, nb * 64)   # S[i, lane]
    lanes = nb * 64
    cap = 2 * L + 4
    buf = np.zeros((lanes, cap), np.uint8)
    cur = np.full(lanes, cap, np.int64)                      # the next byte goes to cur - 1
    x = np.full(lanes, RANS_L, np.int64)
    idx = np.arange(lanes)

    def emit(mask, byte):
        cur[mask] -= 1
        buf[idx[mask], cur[mask]] = byte[mask]

    for i in range(L - 1, -1, -1):
        act = k > i
        if not act.any():
            continue
        fs = f[S[i]]
        cs = c[S[i]]
        xmax = fs << 19
        for _ in range(2):
            m = act & (x >= xmax)
            emit(m, (x & 255).astype(np.uint8))
            x = np.where(m, x >> 8, x)
        assert not (act & (x >= xmax)).any()
        fs1 = np.where(act, fs, 1)
        x = np.where(act, ((x // fs1) << SCALE_BITS) + (x % fs1) + cs, x)
    has = k > 0
    for sh in (0, 8, 16, 24):
        emit(has, ((x >> sh) & 255).astype(np.uint8))
    lens = (cap - cur).astype(np.int64)
    out = bytearray()
    blocks = []
    for b in range(nb):
        body = bytearray()
        for j in range(64):
            lane = b * 64 + j
            body += struct.pack("<H", int(lens[lane]))
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
    """-> (symbols, ok).  ok is False when a directory does not add up or a lane fails its end check."""
    p = np.frombuffer(bytes(payload), np.uint8)
    if n == 0:
        return np.zeros(0, np.uint8), p.size == 0
    f = np.asarray(freq, np.int64)
    assert int(f.sum()) == SCALE
    c = cumulative(f)
    c2s = np.repeat(np.arange(256), f).astype(np.int64)
    nb = n_blocks_of(n, L)
    out = np.zeros(nb * 64 * L, np.uint8)
    if 4 * nb > p.size:
        return out[:n], False
    blen = p[:4 * nb].view("<u4").astype(np.int64)
    boff = 4 * nb + np.cumsum(blen) - blen
    if (blen < 128).any() or int(boff[-1] + blen[-1]) != p.size:
        return out[:n], False
    dirs = np.stack([p[o:o + 128].view("<u2").astype(np.int64) for o in boff])   # [nb, 64]
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
        O[:, i, :] = np.where(act, s, 0).astype(np.uint8).reshape(nb, 64)
    ok = bool(np.all(np.where(has, (x == RANS_L) & (pos == lens), lens == 0)))
    return out[:n], ok


# ---- 10.1 container ----
def padded_dims(w: int, h: int, f: int):
    if w == 0 or h == 0 or f == 0:
        return 0, 0, 0
    return w + (w & 1), h + (h & 1), 2 if f == 1 else f + (f & 1)


def write_container(wavelet: int, w: int, h: int, f: int, L: int, steps, channels_symbols) -> bytes:
    """channels_symbols: three u8 arrays (Y, Co, Cg) of the padded volume each."""
    out = bytearray(b"ALCC" + bytes([2, wavelet]) + struct.pack("<IIII", w, h, f, L))
    payloads = []
    for c in range(3):
        sym = np.asarray(channels_symbols[c], np.uint8).reshape(-1)
        freq = normalize(np.bincount(sym, minlength=256))
        pay = encode_channel(sym, freq, L)
        payloads.append(pay)
        out += struct.pack("<iiIIQ", int(steps[c]), int(steps[c]), sym.size, n_blocks_of(sym.size, L), len(pay))
        out += freq.astype("<u2").tobytes()
    for pay in payloads:
        out += pay
    return bytes(out)


def parse_container(data):
    """-> dict of the header fields, 'freq' [3][256] and 'payload' [3] bytes.  Raises InvalidBitstream; the checks run in
    the order of section 10.5."""
    d = bytes(data)
    if len(d) < FIXED:
        raise InvalidBitstream("too short")
    if d[:4] != b"ALCC":
        raise InvalidBitstream("magic")
    if d[4] != 2:
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
    """-> (info, [Y, Co, Cg] symbols).  Raises InvalidBitstream when a lane fails its end check."""
    info = parse_container(data)
    syms = []
    for c in range(3):
        s, ok = decode_channel(info["payload"][c], info["freq"][c], info["lane_symbols"], info["num_symbols"][c])
        if not ok:
            raise InvalidBitstream("end check")
        syms.append(s)
    return info, syms
