"""Inputs the transcode tests share (tests/test_transcode_host.py on the CPU, tests/test_gpu_transcode.py on the device):
source containers written by the CPU references from the oracle's quantised coefficients, each built once."""
from __future__ import annotations

import functools

import numpy as np

import oracle.alice_oracle_np as o
import reversible_ref as R4
import split_ref as R2
import wide_oracle as WO
import wide_ref as W3

# whole-chunk shapes at L = 64 (a block is 4096 symbols)
SHAPES = {
    "short_block_empty_lanes": (2, 2, 1),      # 8 symbols: one short block, lanes without symbols
    "one_block": (64, 32, 2),                  # exactly 4096 symbols
    "one_block_and_a_bit": (66, 32, 2),
    "padding_on_every_axis": (33, 17, 3),      # pads to 34 x 18 x 4
    "several_blocks": (130, 34, 6),
}
PAIRS = [(100, 80), (95, 60), (80, 50)]        # source quality -> target quality, the target coarser
SAME = [(90, 89), (60, 90)]                    # the same step, and a finer target: the source's bytes come back
BUDGET_SHAPE = "padding_on_every_axis"
BUDGET_RANGE = (10, 95)                        # min_quality, max_quality of the budget cases


@functools.lru_cache(maxsize=None)
def clip(w: int, h: int, f: int) -> np.ndarray:
    rgb = WO.smooth_plus_noise(w, h, f, seed=w + h + f)
    rgb.setflags(write=False)
    return rgb


@functools.lru_cache(maxsize=None)
def quantised(w: int, h: int, f: int, kind: int, quality: int):
    return WO.forward_quantised(o, clip(w, h, f), w, h, f, quality, kind)


@functools.lru_cache(maxsize=None)
def source(version: int, w: int, h: int, f: int, kind: int, quality: int, L: int = 64) -> bytes:
    """The container the encoder of `version` writes for clip(w, h, f) (the GPU test checks that it does)."""
    step, _, qs = quantised(w, h, f, kind, quality)
    if version == 2:
        return R2.write_container(kind, w, h, f, L, (step,) * 3, [o.to_symbols(q) for q in qs])
    blob = W3.write_container(kind, w, h, f, L, (step,) * 3, [W3.wide_symbols(q) for q in qs])
    return blob if version == 3 else R4.with_version(blob, 4)


@functools.lru_cache(maxsize=None)
def mixed_source(version: int) -> bytes:
    """Quantiser steps (4, 9, 20) from the writer itself: Y at 4, Co at 9, Cg at 20."""
    w, h, f = SHAPES["padding_on_every_axis"]
    _, _, qs = quantised(w, h, f, 0, 100)
    steps = (4, 9, 20)
    coarse = [o.quantize(q, s, s) for q, s in zip(qs, steps)]
    if version == 2:
        return R2.write_container(0, w, h, f, 64, steps, [o.to_symbols(q) for q in coarse])
    blob = W3.write_container(0, w, h, f, 64, steps, [W3.wide_symbols(q) for q in coarse])
    return blob if version == 3 else R4.with_version(blob, 4)


def budgets(exact_size):
    """The four budgets of the budget cases from the reference's exact sizes (exact_size(q) -> bytes)."""
    lo_q, hi_q = BUDGET_RANGE
    return [exact_size(70),             # exactly the size at q = 70
            exact_size(70) - 1,         # one byte less
            exact_size(lo_q) - 1,       # below the size at min_quality: fits = 0, still encoded
            exact_size(hi_q) + 1]       # above the size at max_quality
