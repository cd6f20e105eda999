"""Worst-case inputs of the inverse (and forward) transform, built on the numpy oracle (oracle/alice_oracle_np.py), CPU only.

The lifting transforms are linear up to their rounding, so the 1-D transform of length n has a matrix: column j is the
response to an impulse at j.  The output sample whose row has the largest absolute sum is the one an adversary can drive
highest, by giving every input the sign of its entry in that row; that sum is the l-infinity gain of one pass.  A 3-D volume
that does this on all three axes is the outer product of three such sign vectors: after the temporal pass the line through
the chosen frame carries gain x amplitude, after the column pass gain^2, after the row pass gain^3, at the chosen sample.

Measured with these functions (any length >= 4): inverse gain 2.0 for CDF 5/3 and Haar, 1.666 for CDF 9/7; a length of 2
(a single frame, padded) has 1.75 / 1.434 / 1.5.  The forward gains are the same three numbers."""
from __future__ import annotations

import ctypes as C

import numpy as np

import oracle.alice_oracle_np as o

BYTE_MAX_Q = 128      # u8 symbols: 255 -> +128, 254 -> -127
WIDE_MAX_Q = 2175     # wide symbols: 4349 -> +2175, 4350 -> -2175
_IMPULSE = 1 << 20    # large enough that the rounding of the lifting steps is below 1e-5 of an entry

_matrices = {}


def transform_matrix(kind: int, n: int, inverse: bool) -> np.ndarray:
    """M[i, j] = output sample i per unit of input sample j of o._lift_axis (inverse: j indexes [low half | high half])."""
    key = (kind, n, inverse)
    if key not in _matrices:
        eye = np.eye(n, dtype=np.int64) * _IMPULSE
        _matrices[key] = o._lift_axis(eye, 0, o.STEPS[kind], inverse).astype(np.float64) / _IMPULSE
    return _matrices[key]


def pass_gain(kind: int, n: int, inverse: bool = True) -> float:
    return float(np.abs(transform_matrix(kind, n, inverse)).sum(axis=1).max())


def worst_row(kind: int, n: int, inverse: bool, at: int | None = None) -> int:
    """The output sample with the largest absolute row sum; of those (every second interior sample has it) the one
    nearest to `at`, the first when at is None."""
    g = np.abs(transform_matrix(kind, n, inverse)).sum(axis=1)
    best = np.flatnonzero(g >= g.max() * (1 - 1e-4))
    if at is None:
        return int(best[0])
    return int(best[np.argmin(np.abs(best - at))])


def worst_signs(kind: int, n: int, inverse: bool, at: int | None = None) -> np.ndarray:
    """+-1 per input sample: the signs that drive output sample worst_row(kind, n, inverse, at) to +gain (an input the row
    does not read gets +1)."""
    row = transform_matrix(kind, n, inverse)[worst_row(kind, n, inverse, at)]
    return np.where(row < 0, -1, 1).astype(np.int64)


def worst_position(kind: int, dims, centre=None, inverse: bool = True):
    """(t, y, x) of the sample worst_volume drives highest; dims = (pf, ph, pw), centre = (t, y, x) or None"""
    c = centre or (None, None, None)
    return tuple(worst_row(kind, n, inverse, a) for n, a in zip(dims, c))


def worst_volume(kind: int, dims, centre=None, inverse: bool = True) -> np.ndarray:
    """(pf, ph, pw) volume of +-1, the outer product of the three sign vectors; the maximum lands on
    worst_position(kind, dims, centre)."""
    c = centre or (None, None, None)
    st, sy, sx = (worst_signs(kind, n, inverse, a) for n, a in zip(dims, c))
    return st[:, None, None] * sy[None, :, None] * sx[None, None, :]


def per_pass_maxima(kind: int, coef_volume):
    """max |value| after the temporal, the column and the row pass of the inverse of a (pf, ph, pw) coefficient volume:
    three ints.  A (pf, ph, pw, k) array is k volumes at once: three int64 arrays of k."""
    v = np.asarray(coef_volume, np.int64)
    out = []
    for axis in (0, 1, 2):
        v = o._lift_axis(v, axis, o.STEPS[kind], True)
        m = np.abs(v).reshape(v.shape[0] * v.shape[1] * v.shape[2], -1).max(axis=0)
        out.append(int(m[0]) if v.ndim == 3 else m)
    return tuple(out)


# ---- symbols ----
def byte_symbols(signs) -> np.ndarray:
    """u8 symbols of the largest magnitudes: 255 (q = +128) where the sign is positive, 254 (q = -127) where it is negative"""
    return np.where(np.asarray(signs) > 0, 255, 254).astype(np.uint8)


def wide_symbols_extreme(signs) -> np.ndarray:
    """u16 symbols 4349 (q = +2175) / 4350 (q = -2175), the largest a version 3 stream decodes to"""
    return np.where(np.asarray(signs) > 0, 4349, 4350).astype(np.uint16)


def loud_random_q(shape, max_q: int, seed: int) -> np.ndarray:
    """quantised coefficients of random sign with magnitudes drawn from {max, max - 1, max / 2, 1, 0}; u8 symbols have no
    -128, so a negative value stops at -(max - 1) there (max_q = 128)"""
    rng = np.random.default_rng(seed)
    mags = np.array([max_q, max_q - 1, max_q // 2, 1, 0], np.int64)
    q = mags[rng.integers(0, 5, shape)] * rng.choice(np.array([-1, 1], np.int64), shape)
    if max_q == BYTE_MAX_Q:
        q = np.maximum(q, -(max_q - 1))
    return q


def loud_random_bytes(shape, seed: int) -> np.ndarray:
    return o.to_symbols(loud_random_q(shape, BYTE_MAX_Q, seed)).reshape(shape)


def loud_random_wide(shape, seed: int) -> np.ndarray:
    q = loud_random_q(shape, WIDE_MAX_Q, seed)
    return np.where(q > 0, 2 * q - 1, -2 * q).astype(np.uint16)


def from_wide(z) -> np.ndarray:
    """the wide symbol map backwards: odd z -> (z + 1) / 2, even z -> -z / 2"""
    z = np.asarray(z, np.int64)
    return np.where(z & 1, (z + 1) >> 1, -(z >> 1))


def dequantised(q, step: int) -> np.ndarray:
    return o._wrap32(np.asarray(q, np.int64) * int(step))


# ---- the reference's decoder from quantised coefficients, one quantiser step per channel ----
def inverse_quantised_steps(qs, steps, dims, w: int, h: int, f: int, kind: int) -> np.ndarray:
    """wide_oracle.inverse_quantised with steps[c] for channel c; dims = (pw, ph, pf) as there.  -> interleaved RGB"""
    pw, ph, pf = dims
    chans = []
    for q, step in zip(qs, steps):
        vol = o.wavelet3d(kind, dequantised(q, step), pw, ph, pf, inverse=True).reshape(pf, ph, pw)
        chans.append(o._wrap16(vol[:f, :h, :w].reshape(-1)))
    return o.ycocg_r_to_rgb(*chans)


# ---- the quantiser steps at which the launcher changes the instance class, read from the library ----
CDF53, CDF97, HAAR = 0, 1, 2
EXPECTED_VARIANTS = {CDF53: {0, 1, 2, 3}, CDF97: {0, 2, 3}, HAAR: {0, 1, 2, 3}}     # u8 symbols; CDF 9/7 has no fast i32 class


def variant(lib, kind, steps, wide=0):
    return lib.alice_codec_test_inverse_variant(kind, (C.c_int32 * 3)(*[int(s) for s in steps]), wide)


def classes(lib, kind, wide):
    """[(variant, first step, last step)] over steps 1 .. 400, in the order of the steps; the last class is still open"""
    out = []
    for s in range(1, 401):
        v = variant(lib, kind, (s, s, s), wide)
        if out and out[-1][0] == v:
            out[-1][2] = s
        else:
            out.append([v, s, s])
    return [tuple(c) for c in out]


def edge_steps(lib, kind, wide):
    """[(steps, variant)]: the first and the last step of every class (the open end of the exact class left out)"""
    cl = classes(lib, kind, wide)
    cases = []
    for i, (v, first, last) in enumerate(cl):
        for s in (first, last) if i + 1 < len(cl) else (first,):
            if ((s, s, s), v) not in cases:
                cases.append(((s, s, s), v))
    return cases


def byte_step_cases(lib, kind):
    """the step plan of the u8 symbols: edge_steps, two steps whose products wrap i32, and the last step of the last class
    before exact in another channel each time"""
    cl = classes(lib, kind, 0)
    cases = edge_steps(lib, kind, 0) + [((70000,) * 3, 0), ((1 << 20,) * 3, 0)]
    v, _, top = cl[-2]
    cases += [((top, 1, 2), v), ((2, top, 1), v), ((1, 2, top), v)]
    return cases
