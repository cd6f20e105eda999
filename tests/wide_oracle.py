"""The CPU side of the wide-format tests: the reference front end and inverse of oracle/alice_oracle_np.py around a symbol
map of the caller's choice (the u8 map of versions 1 and 2, or the wide map of version 3)."""
from __future__ import annotations

import numpy as np


def smooth_plus_noise(w: int, h: int, f: int, seed: int = 5) -> np.ndarray:
    """Interleaved RGB: slow gradients in x, y and t with full-range amplitude, plus uniform noise of +-24."""
    rng = np.random.default_rng(seed)
    t, y, x = np.meshgrid(np.arange(f), np.arange(h), np.arange(w), indexing="ij")
    base = np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y + 9 * t) * 255) // max(w + h + 9 * f - 3, 1)], axis=-1)
    noise = rng.integers(-24, 25, base.shape)
    return np.clip(base + noise, 0, 255).astype(np.uint8).reshape(-1)


def forward_quantised(o, rgb, w, h, f, quality, kind):
    """-> (step, (pw, ph, pf), [q_Y, q_Co, q_Cg]) with q the quantised coefficients (int64) of the padded volume."""
    step = o.quality_to_step(quality)
    qs = []
    for ch in o.rgb_to_ycocg_r(np.asarray(rgb, np.uint8).reshape(-1)):
        v, pw, ph, pf = o._pad(ch, w, h, f)
        qs.append(np.asarray(o.quantize(o.wavelet3d(kind, v, pw, ph, pf), step, step), np.int64))
    return step, (pw, ph, pf), qs


def inverse_quantised(o, qs, step, dims, w, h, f, kind):
    """from quantised coefficients (what from_symbols gives back) to RGB, as the reference's decoder does it"""
    pw, ph, pf = dims
    chans = []
    for q in qs:
        coef = o._wrap32(np.asarray(q, np.int64) * step)
        vol = o.wavelet3d(kind, coef, pw, ph, pf, inverse=True).reshape(pf, ph, pw)
        chans.append(o._wrap16(vol[:f, :h, :w].reshape(-1)))
    return o.ycocg_r_to_rgb(*chans)


def psnr(a, b) -> float:
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    mse = float((d * d).mean())
    return float("inf") if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)
