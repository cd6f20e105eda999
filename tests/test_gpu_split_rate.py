"""Version 2 size prediction and budget encodes on the MI355X.  Per shape, one reference is built on the CPU and shared:
the oracle's step histograms and symbols, split_rate_ref's brackets and split_ref's containers at the 64 quantiser steps.
The GPU's lo / hi must be the reference's integers, every real container must lie inside its bracket and equal split_ref's
bytes, and the budget calls must pick the reference chooser's quality with its number of trials and write encode_split's
bytes."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rate_ref  # noqa: E402
import split_rate_ref as SR  # noqa: E402
import split_ref as R  # noqa: E402

import torch  # noqa: E402

pytestmark = pytest.mark.gpu

Q_OF_STEP = {}
for _q in range(101):
    Q_OF_STEP.setdefault(SR.quality_to_step(_q), _q)


def _source(seed, w, h, f, noise=8):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = ((x[None] * 3 + y[None] * 2 + np.arange(f)[:, None, None] * 5) % 256).astype(np.int16)
    rgb = np.stack([base, 255 - base, (base * 7) % 256], axis=3) + rng.integers(-noise, noise + 1, (f, h, w, 3))
    return np.clip(rgb, 0, 255).astype(np.uint8).reshape(-1)


# name: (w, h, f, wavelet, lane_symbols (0 = the default 512), noise)
SHAPES = {
    "tile_short_last_block": (48, 32, 10, 1, 64, 8),     # CDF 9/7, tile path, 15360 symbols = 3.75 blocks of 64 x 64
    "odd_everything": (33, 17, 5, 0, 128, 20),           # CDF 5/3, pads to 34 x 18 x 6
    "one_full_block": (64, 32, 2, 2, 64, 8),             # Haar, 4096 symbols per channel = exactly one block
    "generic_empty_lanes": (4, 4, 2, 1, 0, 40),          # generic path, 32 symbols < 64 lanes
    "one_pixel": (1, 1, 1, 0, 0, 0),
    "banded": (96, 200, 4, 1, 64, 30),                   # cut into bands by the band hook
}


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(rgb, lo[101], hi[101], {step: container bytes}) -- computed once per shape, never modified"""
    import oracle
    w, h, f, k, L, noise = SHAPES[name]
    Le = L or 512
    rgb = _source(sum(map(ord, name)), w, h, f, noise)
    rgb.setflags(write=False)
    hists = rate_ref.oracle_step_hists(oracle, rgb, w, h, f, k)
    lo, hi = SR.chunk_prediction(hists, Le)
    blobs = {}
    for step in range(1, 65):
        sym = oracle.encode_symbols(rgb, w, h, f, Q_OF_STEP[step], k).reshape(3, -1)
        assert np.array_equal(np.stack([np.bincount(s, minlength=256) for s in sym]), hists[step - 1])
        blobs[step] = R.write_container(k, w, h, f, Le, [step] * 3, sym)
    return rgb, lo, hi, blobs


def _trials(codec, n):
    out = np.zeros(max(n, 1), np.uint32)
    got = codec.load_library().alice_codec_test_last_split_trials(out.ctypes.data_as(C.POINTER(C.c_uint32)), n)
    assert got == n
    return [int(v) for v in out[:n]]


def _check_prediction(codec, name):
    w, h, f, k, L, _ = SHAPES[name]
    rgb, lo, hi, blobs = _reference(name)
    p = codec.predict_split_sizes(rgb, w, h, f, k, L)
    assert np.array_equal(p.lo, lo) and np.array_equal(p.hi, hi) and not p.status.any()
    d = torch.from_numpy(np.concatenate([rgb, rgb])).to("cuda:0")
    pd = codec.predict_split_sizes_device(d.data_ptr(), w, h, f, 2, k, L)
    for i in range(2):
        assert np.array_equal(pd.lo[i], lo) and np.array_equal(pd.hi[i], hi)
    for step, want in blobs.items():
        q = Q_OF_STEP[step]
        got = codec.encode_split(codec.FrameEncoder.with_wavelet(q, codec.WaveletType(k)), rgb, w, h, f, L)
        print(f"{name} step {step}: lo {int(lo[q])} size {len(got)} hi {int(hi[q])}")
        assert got == want, (name, step)
        assert int(lo[q]) <= len(got) <= int(hi[q]), (name, step, int(lo[q]), len(got), int(hi[q]))


@pytest.mark.parametrize("name", [n for n in SHAPES if n != "banded"])
def test_brackets_are_the_references_and_hold(gpu_codec, name):
    _check_prediction(gpu_codec, name)


def test_banded_shape(gpu_codec):
    lib = gpu_codec.load_library()
    try:
        lib.alice_codec_test_set_tuning(16)            # several bands of a few tile rows each (tests/test_gpu_bands.py)
        _check_prediction(gpu_codec, "banded")
    finally:
        lib.alice_codec_test_set_tuning(1024 * 1024)


def test_out_of_range_fallback(gpu_codec):
    lib = gpu_codec.load_library()
    try:
        lib.alice_codec_test_set_value_table_radius(24)   # coefficients outside [-24, 24): histograms from real forward passes
        for name in ("tile_short_last_block", "generic_empty_lanes"):
            w, h, f, k, L, _ = SHAPES[name]
            rgb, lo, hi, _ = _reference(name)
            p = gpu_codec.predict_split_sizes(rgb, w, h, f, k, L)
            assert np.array_equal(p.lo, lo) and np.array_equal(p.hi, hi)
    finally:
        lib.alice_codec_test_set_value_table_radius(2048)


def _budgets(lo, hi, blobs):
    mid = 60
    return [int(lo.min()) - 1,                                  # below the smallest lo: nothing can fit
            int(hi.max()) + 1,                                  # above the largest hi: max_quality at once
            len(blobs[SR.quality_to_step(mid)]),                # the exact size of a mid quality: refinement must find it
            int(hi[mid]) - 1]                                   # one below an upper bound


@pytest.mark.parametrize("name", list(SHAPES))
def test_budget_encodes_follow_the_reference_chooser(gpu_codec, name):
    a = gpu_codec
    w, h, f, k, L, _ = SHAPES[name]
    rgb, lo, hi, blobs = _reference(name)
    budgets = _budgets(lo, hi, blobs)
    want = [SR.choose(lo, hi, b, 10, 95, lambda q: len(blobs[SR.quality_to_step(q)])) for b in budgets]
    assert want[0][:2] == (10, False) and want[1] == (95, True, 0)
    mid_top = max(q for q in range(10, 96) if SR.quality_to_step(q) == SR.quality_to_step(60))
    assert want[2][1] and want[2][0] >= mid_top and (want[2][2] >= 1 or hi[want[2][0]] <= budgets[2])
    for b, (q, fits, trials) in zip(budgets, want):
        data, gq, gfits = a.encode_split_to_size(rgb, w, h, f, b, k, 10, 95, L)
        print(f"{name} budget {b}: chose {gq} fits {gfits} size {len(data)} trials {_trials(a, 1)} (reference {q} {fits} {trials})")
        assert (gq, gfits) == (q, fits)
        assert _trials(a, 1) == [trials] and trials <= SR.REFINE_TRIALS
        assert data == blobs[SR.quality_to_step(q)]
        assert data == a.encode_split(a.FrameEncoder.with_wavelet(q, a.WaveletType(k)), rgb, w, h, f, L)
        if fits:
            assert len(data) <= b
    # three chunks under three different budgets in one device call
    d = torch.from_numpy(np.concatenate([rgb] * 3)).to("cuda:0")
    stride = (max(len(v) for v in blobs.values()) + 255) & ~255
    for first in (0, 1):
        out = torch.full((3 * stride,), 0xCD, dtype=torch.uint8, device="cuda:0")
        chosen, fits, sizes = a.split_encode_to_budget_device(d.data_ptr(), w, h, f, 3, k, budgets[first:first + 3], out.data_ptr(),
                                                              stride, 10, 95, L)
        host = out.cpu().numpy().reshape(3, stride)
        assert _trials(a, 3) == [t for _, _, t in want[first:first + 3]]
        for i in range(3):
            q, fit, _ = want[first + i]
            assert (int(chosen[i]), bool(fits[i])) == (q, fit)
            assert host[i, :int(sizes[i])].tobytes() == blobs[SR.quality_to_step(q)]
            assert (host[i, int(sizes[i]):] == 0xCD).all()
