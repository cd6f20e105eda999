"""The reference's buffer-model rate control (src/rate_control.rs), restated for callers who port code that uses it.

Host code only, no device.  Integer behaviour follows the Rust: ``u32::midpoint`` for the start quality, the buffer starts
half full, a 30-entry history, the +-0.3 buffer-ratio thresholds with +1 / -2 quality steps, ``clamp`` with the
configured range, and Rust's casts: ``f64 as u64`` / ``f64 as u32`` saturate (NaN -> 0, negatives -> 0), integer ``as``
casts wrap, ``mul_add`` rounds once.

What the GPU adds on top (``predict_sizes``, ``encode_to_size``) looks at the pixels; this model does not, and reacts one
chunk late.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from fractions import Fraction

_U32 = (1 << 32) - 1
_U64 = (1 << 64) - 1


def _f64_as_uint(x: float, top: int) -> int:
    """Rust ``x as u64`` / ``x as u32``: truncation toward zero, saturating; NaN -> 0."""
    if math.isnan(x) or x <= 0.0:
        return 0
    if math.isinf(x) or x >= top + 1:
        return top
    return int(x)


def _wrap_i64(v: int) -> int:
    v &= _U64
    return v - (1 << 64) if v >> 63 else v


def _wrap_i32(v: int) -> int:
    v &= _U32
    return v - (1 << 32) if v >> 31 else v


def _clamp(v: int, lo: int, hi: int) -> int:
    if lo > hi:   # Ord::clamp panics on an inverted range
        raise ValueError(f"clamp: min {lo} > max {hi}")
    return lo if v < lo else hi if v > hi else v


def _mul_add(a: float, b: float, c: float) -> float:
    """f64::mul_add: a * b + c with one rounding."""
    if not all(math.isfinite(v) for v in (a, b, c)):
        return a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))


@dataclass
class RateControlConfig:
    """src/rate_control.rs:7-31 (the defaults: 5000 kbps, 30 fps, quality 10..95, a buffer of 2 s = 10 000 000 bits)."""
    target_bitrate_kbps: int = 5_000
    framerate: float = 30.0
    min_quality: int = 10
    max_quality: int = 95
    buffer_size_bits: int = 5_000 * 1_000 * 2


class RateController:
    """src/rate_control.rs:34-190."""

    MAX_HISTORY = 30

    def __init__(self, config: RateControlConfig | None = None):    # RateController::new
        self.config = config if config is not None else RateControlConfig()
        c = self.config
        self._quality = ((c.min_quality & _U32) + (c.max_quality & _U32)) >> 1       # u32::midpoint
        self._fullness = _wrap_i64(c.buffer_size_bits) // 2 if _wrap_i64(c.buffer_size_bits) >= 0 \
            else -((-_wrap_i64(c.buffer_size_bits)) // 2)                             # i64 division truncates
        self._history: list[int] = []
        self._frames = 0

    @classmethod
    def with_defaults(cls) -> "RateController":
        return cls(RateControlConfig())

    def target_bits_per_frame(self) -> int:
        fr = float(self.config.framerate)
        if fr <= 0.0:
            return 0
        return _f64_as_uint(float(self.config.target_bitrate_kbps & _U32) * 1000.0 / fr, _U64)

    def recommended_quality(self) -> int:
        return self._quality

    def update(self, frame_size_bits: int) -> None:
        size = int(frame_size_bits) & _U64
        target = _wrap_i64(self.target_bits_per_frame())
        buf = _wrap_i64(self.config.buffer_size_bits)
        self._fullness = _wrap_i64(self._fullness + _wrap_i64(target - _wrap_i64(size)))
        self._fullness = _clamp(self._fullness, _wrap_i64(-buf), buf)
        self._history.append(size)
        if len(self._history) > self.MAX_HISTORY:
            self._history.pop(0)
        self._frames += 1
        self._adjust_quality()

    def _adjust_quality(self) -> None:
        bits = float(self.config.buffer_size_bits & _U64)
        full = float(self._fullness)
        ratio = full / bits if bits != 0.0 else (math.nan if full == 0.0 else math.copysign(math.inf, full))
        adj = 1 if ratio > 0.3 else (-2 if ratio < -0.3 else 0)
        q = _clamp(_wrap_i32(self._quality + adj), _wrap_i32(self.config.min_quality), _wrap_i32(self.config.max_quality))
        self._quality = q & _U32

    def buffer_ratio(self) -> float:
        if self.config.buffer_size_bits == 0:
            return 0.0
        return float(self._fullness) / float(self.config.buffer_size_bits & _U64)

    def average_frame_size(self) -> int:
        if not self._history:
            return 0
        return (sum(self._history) & _U64) // len(self._history)

    def frame_count(self) -> int:
        return self._frames

    def current_quality(self) -> int:
        return self._quality

    def actual_to_target_ratio(self) -> float:
        target = self.target_bits_per_frame()
        actual = self.average_frame_size()
        if target == 0:
            return 0.0
        return float(actual) / float(target)


def estimate_quality(target_bitrate_kbps: int, width: int, height: int, fps: float) -> int:
    """src/rate_control.rs:196-219: a quality from the bits per pixel the bitrate allows (no history, no pixels)."""
    fps = float(fps)
    if fps <= 0.0 or width == 0 or height == 0:
        return 50
    pixels_per_sec = float(width) * float(height) * fps
    bpp = float(target_bitrate_kbps) * 1000.0 / pixels_per_sec
    if bpp > 2.0:
        q = 95.0
    elif bpp > 0.5:
        q = _mul_add(bpp, 30.0, 35.0)
    elif bpp > 0.1:
        q = _mul_add(bpp, 75.0, 12.5)
    else:
        q = bpp * 100.0 + 5.0
    return _clamp(_f64_as_uint(q, _U32), 5, 100)


def budget_bytes_per_chunk(target_bitrate_kbps: int, framerate: float, frames: int) -> int:
    """floor(target_bits_per_frame * frames / 8): the byte budget of a chunk of ``frames`` frames at the controller's rate."""
    ctrl = RateController(RateControlConfig(target_bitrate_kbps=target_bitrate_kbps, framerate=framerate))
    return ctrl.target_bits_per_frame() * frames // 8
