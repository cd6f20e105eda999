"""Restated size model and budget rule of the split-stream container (.alc version 2), written from DESIGN.md section 10
(10.2 normalisation, 10.4 payload layout, 10.8 bracket and refinement rule) and not from the kernels.  Everything is Python
integers; the fixed-point log table is computed here at 60 decimal digits (the suite compares it with the library's).

Per channel, with n symbols, L = lane_symbols, B = ceil(n / 64L) blocks, K = lanes that own a symbol, one = 2^24:
    fixed = 132 B + 4 K
    hi    = fixed + floor((S_hi + n g_up) / (8 one))
    lo    = fixed + (ceil((S_lo - sub) / (8 one + g_dn)) if S_lo > sub else 0),   sub = n g_dn + 8 K one
A chunk is 1630 + the three channels."""
from __future__ import annotations

import functools
from decimal import Decimal, getcontext, ROUND_FLOOR, ROUND_CEILING

import numpy as np

import split_ref

FRAC = 24
ONE = 1 << FRAC
HEADER = 1630
REFINE_TRIALS = 4


@functools.lru_cache(maxsize=None)
def log_table():
    """(lo[4097], hi[4097], (g_up, g_dn)): floor / ceil of log2(4096 / f) * 2^24 (entry 0 unused) and the two
    ceil(+-log2(1 +- 2^-11) * 2^24) terms."""
    getcontext().prec = 60
    ln2 = Decimal(2).ln()
    scale = Decimal(ONE)
    lo = [0] * 4097
    hi = [0] * 4097
    for f in range(1, 4097):
        if f & (f - 1) == 0:
            lo[f] = hi[f] = (12 - (f.bit_length() - 1)) << FRAC
            continue
        v = (Decimal(4096) / Decimal(f)).ln() / ln2 * scale
        lo[f] = int(v.to_integral_value(ROUND_FLOOR))
        hi[f] = int(v.to_integral_value(ROUND_CEILING))
    g_up = int(((Decimal(1) + Decimal(2) ** -11).ln() / ln2 * scale).to_integral_value(ROUND_CEILING))
    g_dn = int((-(Decimal(1) - Decimal(2) ** -11).ln() / ln2 * scale).to_integral_value(ROUND_CEILING))
    return lo, hi, (g_up, g_dn)


def lanes_with_symbols(n: int, L: int) -> int:
    nb = split_ref.n_blocks_of(n, L)
    return sum(min(64, min(64 * L, n - b * 64 * L)) for b in range(nb))


def channel_bracket(hist, L: int):
    """(lo, hi) bytes of the channel payload of a histogram (its sum is the number of symbols)."""
    h = [int(v) for v in hist]
    n = sum(h)
    if n == 0:
        return 0, 0
    lo_t, hi_t, (g_up, g_dn) = log_table()
    freq = split_ref.normalize(h)
    s_lo = sum(c * lo_t[int(f)] for c, f in zip(h, freq) if c)
    s_hi = sum(c * hi_t[int(f)] for c, f in zip(h, freq) if c)
    B = split_ref.n_blocks_of(n, L)
    K = lanes_with_symbols(n, L)
    fixed = 132 * B + 4 * K
    hi = fixed + (s_hi + n * g_up) // (8 * ONE)
    sub = n * g_dn + 8 * K * ONE
    lo = fixed + (-(-(s_lo - sub) // (8 * ONE + g_dn)) if s_lo > sub else 0)
    return lo, hi


def quality_to_step(q: int) -> int:
    return max(64 - (min(q, 100) * 63) // 100, 1)


def chunk_prediction(step_hists, L: int):
    """step_hists[step - 1][channel] (256 bins each) -> (lo[101], hi[101]) of the whole container."""
    per_step = [[channel_bracket(step_hists[s][c], L) for c in range(3)] for s in range(64)]
    lo = np.zeros(101, np.uint64)
    hi = np.zeros(101, np.uint64)
    for q in range(101):
        ch = per_step[quality_to_step(q) - 1]
        lo[q] = HEADER + sum(c[0] for c in ch)
        hi[q] = HEADER + sum(c[1] for c in ch)
    return lo, hi


def choose(lo, hi, budget: int, min_q: int, max_q: int, exact_size):
    """The budget rule: (quality, fits, trials).  exact_size(q) is the length of the container at quality q."""
    min_q, max_q = min(min_q, 100), min(max_q, 100)
    q0 = None
    for q in range(max_q, min_q - 1, -1):
        if int(hi[q]) <= budget:
            q0 = q
            break
    tried = set()
    trials = 0
    for q in range(max_q, (min_q - 1) if q0 is None else q0, -1):
        if not int(lo[q]) <= budget < int(hi[q]):
            continue
        step = quality_to_step(q)
        if step in tried:
            continue
        if trials == REFINE_TRIALS:
            break
        tried.add(step)
        trials += 1
        if exact_size(q) <= budget:
            return q, True, trials
    if q0 is None:
        return min_q, False, trials
    return q0, True, trials
