"""Restated rate-prediction model for the tests, built on the CPU oracle.

* fold:    a histogram of unquantised coefficients -> the symbol histogram at a quantiser step, through the oracle's
           Quantizer::quantize (dead zone = step) and to_symbols;
* table:   oracle.FrequencyTable (src/rans.rs:102-150) of a symbol histogram;
* cost:    status and stream-length bracket of a channel in integers (derivation: csrc/rate.hip), with the library's fixed-point log table (test hook),
           so that libm never decides a rounding on either side;
* chunk:   whole-.alc lo / hi / status at the 101 qualities from the 64 x 3 step histograms.
"""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np

BOUNDED, UNBOUNDED, DIVERGES = 0, 1, 2
FRAC = 24
HEADER = 18 + 3 * 1040
U64_MAX = (1 << 64) - 1


def log_table(codec):
    """(lo[4097], hi[4097], (g_up, g_dn)) from alice_codec_test_rate_log_table."""
    lib = codec.load_library()
    lo = np.zeros(4097, np.uint32); hi = np.zeros(4097, np.uint32); g = np.zeros(2, np.uint32)
    u32p = C.POINTER(C.c_uint32)
    lib.alice_codec_test_rate_log_table(lo.ctypes.data_as(u32p), hi.ctypes.data_as(u32p), g.ctypes.data_as(u32p))
    return lo, hi, (int(g[0]), int(g[1]))


def fold(oracle, values, counts, step: int) -> np.ndarray:
    """Symbol histogram at `step` of coefficients `values` occurring `counts` times."""
    sym = oracle.to_symbols(oracle.quantize_buffer(step, np.asarray(values, np.int32), step))
    return np.bincount(sym, weights=np.asarray(counts, np.float64), minlength=256).astype(np.uint64)


def channel_cost(oracle, hist, table):
    """(status, lo_bytes, hi_bytes) of one channel's stream; lo = hi = 0 unless BOUNDED."""
    lo_t, hi_t, (g_up, g_dn) = table
    hist = np.asarray(hist, np.uint64)
    ft = oracle.FrequencyTable(hist.astype(np.uint32))
    freq = ft.freq.astype(np.int64); cum = ft.cum_freq.astype(np.int64)
    status = BOUNDED
    m_lo = m_hi = n = e = 0
    for s in np.nonzero(hist)[0]:
        c, f = int(hist[s]), int(freq[s])
        n += c
        if f == 0:
            status = max(status, DIVERGES)
        elif f > 4096:
            status = max(status, UNBOUNDED)
        else:
            e = max(e, int(cum[s]) + f - 4096)
            m_lo += c * int(lo_t[f]); m_hi += c * int(hi_t[f])
    if status != BOUNDED:
        return status, 0, 0
    one = 1 << FRAC
    up = -(-(8192 + 2 * e) * 14427 // 10000) if e else g_up     # log2(1 + 2^-11 + e 2^-23) < (2^-11 + e 2^-23) * 1.4427
    hi = (m_hi + n * up) // (8 * one) + 4
    num = m_lo - n * g_dn - (9 if e else 8) * one                 # the final state may exceed 2^31 by e
    lo = (-(-num // (8 * one + g_dn)) if num > 0 else 0) + 4
    return status, lo, hi


def quality_to_step(q: int) -> int:
    return max(64 - (min(q, 100) * 63) // 100, 1)


def chunk_prediction(oracle, step_hists, table):
    """step_hists[step - 1][channel] -> (lo[101], hi[101], status[101]) as the library reports them."""
    per_step = [[channel_cost(oracle, step_hists[s][c], table) for c in range(3)] for s in range(64)]
    lo = np.zeros(101, np.uint64); hi = np.zeros(101, np.uint64); st = np.zeros(101, np.uint8)
    for q in range(101):
        ch = per_step[quality_to_step(q) - 1]
        worst = max(c[0] for c in ch)
        st[q] = worst
        lo[q] = HEADER + sum(c[1] for c in ch) if worst == BOUNDED else 0
        hi[q] = HEADER + sum(c[2] for c in ch) if worst == BOUNDED else U64_MAX
    return lo, hi, st


def header_hists(alc: bytes) -> np.ndarray:
    """The three channel histograms stored in an .alc header, (3, 256)."""
    out = np.zeros((3, 256), np.uint64)
    for c in range(3):
        off = 18 + c * 1040 + 16
        out[c] = struct.unpack_from("<256I", alc, off)
    return out


def oracle_step_hists(oracle, rgb, w, h, f, wavelet) -> np.ndarray:
    """(64, 3, 256): the header histograms of oracle.encode at a quality of every step 1..64."""
    q_of = {}
    for q in range(101):
        q_of.setdefault(quality_to_step(q), q)
    assert sorted(q_of) == list(range(1, 65))
    return np.stack([header_hists(oracle.encode(rgb, w, h, f, q_of[s], wavelet)) for s in range(1, 65)])


def choose(hi, status, budget, min_q, max_q):
    """The budget rule: (quality, fits)."""
    min_q, max_q = min(min_q, 100), min(max_q, 100)
    for q in range(max_q, min_q - 1, -1):
        if status[q] == BOUNDED and int(hi[q]) <= budget:
            return q, True
    return min_q, False
