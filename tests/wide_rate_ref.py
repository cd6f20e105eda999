"""Restated size model of the wide container (.alc version 3), written from DESIGN.md section 11.6 and not from the
kernels.  Everything is Python integers; the log table, the lane count, the quality scale and the budget rule are version
2's (split_rate_ref).

The histogram is of the coded symbol s = min(z, 255); E = hist[255] is the number of escapes, and each escape adds one chain
step of exactly 12 bits (the residual: frequency 1 out of 4096).  Per channel, with n symbols, L = lane_symbols,
B = ceil(n / 64L) blocks, K = lanes that own a symbol, one = 2^24, S_lo / S_hi the table sums over the rule-10.2 table:
    steps = n + E
    T_lo  = S_lo + 12 one E           T_hi = S_hi + 12 one E
    fixed = 132 B + 4 K
    hi    = fixed + floor((T_hi + steps g_up) / (8 one))
    lo    = fixed + (ceil((T_lo - sub) / (8 one + g_dn)) if T_lo > sub else 0),   sub = steps g_dn + 8 K one
A chunk is 1630 + the three channels."""
from __future__ import annotations

import numpy as np

import split_rate_ref as SR
import wide_oracle
import wide_ref
from split_rate_ref import HEADER, ONE, REFINE_TRIALS, choose, lanes_with_symbols, log_table, quality_to_step  # noqa: F401

RES_BITS = 12


def channel_bracket(hist, L: int):
    """(lo, hi) bytes of the channel payload of a histogram of coded symbols (its sum is the number of symbols)."""
    h = [int(v) for v in hist]
    assert len(h) == 256
    n = sum(h)
    if n == 0:
        return 0, 0
    lo_t, hi_t, (g_up, g_dn) = log_table()
    freq = wide_ref.normalize(h)
    s_lo = sum(c * lo_t[int(f)] for c, f in zip(h, freq) if c)
    s_hi = sum(c * hi_t[int(f)] for c, f in zip(h, freq) if c)
    E = h[255]
    steps = n + E
    t_lo = s_lo + RES_BITS * ONE * E
    t_hi = s_hi + RES_BITS * ONE * E
    B = wide_ref.n_blocks_of(n, L)
    K = lanes_with_symbols(n, L)
    fixed = 132 * B + 4 * K
    hi = fixed + (t_hi + steps * g_up) // (8 * ONE)
    sub = steps * g_dn + 8 * K * ONE
    lo = fixed + (-(-(t_lo - sub) // (8 * ONE + g_dn)) if t_lo > sub else 0)
    return lo, hi


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


def q_of_step():
    """step -> the lowest quality that has it"""
    out = {}
    for q in range(101):
        out.setdefault(quality_to_step(q), q)
    assert sorted(out) == list(range(1, 65))
    return out


def oracle_step_symbols_wide(o, rgb, w, h, f, kind):
    """[step - 1][channel]: the u16 wide symbols of the padded volume at a quality of every step 1..64"""
    q_of = q_of_step()
    out = []
    for s in range(1, 65):
        step, _, qs = wide_oracle.forward_quantised(o, rgb, w, h, f, q_of[s], kind)
        assert step == s
        out.append([wide_ref.wide_symbols(q) for q in qs])
    return out


def oracle_step_hists_wide(o, rgb, w, h, f, kind) -> np.ndarray:
    """(64, 3, 256): wide_ref.histogram of wide_ref.wide_symbols of wide_oracle.forward_quantised at a quality of every
    step 1..64."""
    return np.stack([np.stack([wide_ref.histogram(z) for z in zs]) for zs in oracle_step_symbols_wide(o, rgb, w, h, f, kind)])
