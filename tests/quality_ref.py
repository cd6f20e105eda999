"""Plain numpy restatement of the quality control of DESIGN.md section 13, written from the rule in include/alice_codec.h
and not from the library: the pass threshold, the candidate steps, the search, and a chunk's squared error at a quality on
the CPU oracle (the front end and inverse of oracle/alice_oracle_np.py around the symbol map of the container)."""
from __future__ import annotations

import math

import numpy as np

import oracle.alice_oracle_np as o
import reversible_ref as RV
import wide_oracle as WO

FORMAT_SPLIT, FORMAT_WIDE, FORMAT_REVERSIBLE = 2, 3, 4
MAX_TRIALS = 8


def step_of(q: int) -> int:
    return int(o.quality_to_step(min(int(q), 100)))


def psnr_from_sse(sse: int, n_bytes: int) -> float:
    """The expression of alice_codec_psnr: mse = sse / n in f64, +inf at 0, else 10 log10(255^2 / mse)."""
    if n_bytes == 0:
        return math.inf
    mse = float(sse) / float(n_bytes)
    return math.inf if mse == 0.0 else 10.0 * math.log10(255.0 * 255.0 / mse)


def sse_max(T: float, N: int) -> int:
    """floor(65025 N / 10^(T / 10)) in f64; 0 for T = +inf (and wherever the power overflows to it)."""
    if math.isinf(T):
        return 0
    try:
        p = math.pow(10.0, T / 10.0)
    except OverflowError:
        return 0
    return int(math.floor(65025.0 * float(N) / p))


def candidates(min_q: int, max_q: int) -> list:
    """The lowest quality of every distinct step in [min_q, max_q] (qualities above 100 act as 100), coarsest first."""
    out = []
    for q in range(min(min_q, 100), min(max_q, 100) + 1):
        if not out or step_of(q) != step_of(out[-1]):
            out.append(q)
    return out


def choose(step_sse, N: int, T: float, min_q: int, max_q: int):
    """-> (quality, reached, trials).  step_sse: {quantiser step: squared error of the chunk at that step}."""
    limit = sse_max(T, N)
    cand = candidates(min_q, max_q)
    tried = []

    def passes(k):
        tried.append(k)
        return step_sse[step_of(cand[k])] <= limit

    if not passes(len(cand) - 1):
        return min(max_q, 100), False, len(tried)
    if len(cand) == 1 or passes(0):
        return cand[0], True, len(tried)
    lo, hi = 0, len(cand) - 1          # lo fails, hi passes
    while hi - lo > 1:
        mid = (lo + hi + 1) // 2       # towards the finer step
        if passes(mid):
            hi = mid
        else:
            lo = mid
    return cand[hi], True, len(tried)


def scan(step_sse, N: int, T: float, min_q: int, max_q: int):
    """The exhaustive answer: the coarsest passing step of the range -> (quality, reached)."""
    limit = sse_max(T, N)
    for q in candidates(min_q, max_q):
        if step_sse[step_of(q)] <= limit:
            return q, True
    return min(max_q, 100), False


_forward = {}


def reconstruct(version: int, rgb, w: int, h: int, f: int, quality: int, kind: int) -> np.ndarray:
    """The pixels the version's decode returns for the version's encode at this quality."""
    rgb = np.asarray(rgb, np.uint8).reshape(-1)
    if version == FORMAT_REVERSIBLE:
        return np.asarray(RV.roundtrip(rgb, w, h, f, quality, kind), np.uint8)
    key = (hash(rgb.tobytes()), w, h, f, step_of(quality), kind)
    if key not in _forward:
        if len(_forward) > 256:
            _forward.clear()
        _forward[key] = WO.forward_quantised(o, rgb, w, h, f, quality, kind)
    step, dims, qs = _forward[key]
    if version == FORMAT_SPLIT:        # the u8 symbol map of versions 1 and 2: `as u8` wraps
        qs = [o.from_symbols(o.to_symbols(q)) for q in qs]
    else:                              # the wide map is one to one on what 8-bit RGB produces
        assert version == FORMAT_WIDE
    return np.asarray(WO.inverse_quantised(o, qs, step, dims, w, h, f, kind), np.uint8)


def sse_of(a, b) -> int:
    d = np.asarray(a, np.int64).reshape(-1) - np.asarray(b, np.int64).reshape(-1)
    return int((d * d).sum())


def frame_sse(a, b, n_frames: int) -> np.ndarray:
    d = np.asarray(a, np.int64).reshape(n_frames, -1) - np.asarray(b, np.int64).reshape(n_frames, -1)
    return (d * d).sum(axis=1).astype(np.uint64)


def chunk_sse(version: int, rgb, w: int, h: int, f: int, quality: int, kind: int) -> int:
    return sse_of(rgb, reconstruct(version, rgb, w, h, f, quality, kind))


_tables = {}


def step_table(version: int, rgb, w: int, h: int, f: int, kind: int, max_q: int = 100) -> dict:
    """{step: sse} for every step of the qualities 0 .. max_q, computed once per content."""
    rgb = np.asarray(rgb, np.uint8).reshape(-1)
    key = (version, hash(rgb.tobytes()), w, h, f, kind, max_q)
    if key not in _tables:
        _tables[key] = {step_of(q): chunk_sse(version, rgb, w, h, f, q, kind) for q in candidates(0, max_q)}
    return _tables[key]


def midway_targets(table: dict, N: int) -> list:
    """A dB target midway between the values of every pair of adjacent steps whose values are finite and differ."""
    steps = sorted(table)
    out = []
    for a, b in zip(steps[:-1], steps[1:]):
        pa, pb = psnr_from_sse(table[a], N), psnr_from_sse(table[b], N)
        if math.isfinite(pa) and math.isfinite(pb) and pa != pb:
            out.append(0.5 * (pa + pb))
    return out
