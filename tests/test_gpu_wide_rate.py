"""Version 3 size prediction and budget encodes on the MI355X.  Per shape, one reference is built on the CPU and shared:
the oracle's wide symbols and step histograms, wide_rate_ref's brackets and wide_ref's containers at the 64 quantiser
steps.  The folded device histograms must be the oracle's, the GPU's lo / hi the reference's integers, every real container
must lie inside its bracket and equal wide_ref's bytes, and the budget calls must pick the reference chooser's quality with
its number of trials and write encode_wide's bytes.  Every shape but the single pixel has escapes at step 1: without them
the test would only repeat version 2's."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_rate_ref as SR  # noqa: E402
import wide_oracle as WO  # noqa: E402
import wide_rate_ref as WR  # noqa: E402
import wide_ref as R  # noqa: E402

import torch  # noqa: E402

pytestmark = pytest.mark.gpu

Q_OF_STEP = WR.q_of_step()

# name: (w, h, f, wavelet, lane_symbols (0 = the default 512))
SHAPES = {
    "tile_short_last_block": (48, 32, 10, 1, 64),     # CDF 9/7, tile path, a short last block
    "odd_everything": (33, 17, 5, 0, 128),            # CDF 5/3, pads to 34 x 18 x 6
    "one_full_block": (64, 32, 2, 2, 64),             # Haar, 4096 symbols per channel = exactly one block
    "generic_empty_lanes": (4, 4, 2, 1, 0),           # generic path, 32 symbols < 64 lanes
    "one_pixel": (1, 1, 1, 0, 0),
    "banded": (96, 200, 4, 1, 64),                    # cut into bands by the band hook
}


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(rgb, hists (64, 3, 256), lo[101], hi[101], {step: container bytes}) -- computed once per shape, never modified"""
    import oracle.alice_oracle_np as o
    w, h, f, k, L = SHAPES[name]
    Le = L or 512
    rgb = WO.smooth_plus_noise(w, h, f, seed=w + h + f)
    rgb.setflags(write=False)
    syms = WR.oracle_step_symbols_wide(o, rgb, w, h, f, k)
    hists = WR.oracle_step_hists_wide(o, rgb, w, h, f, k)
    assert np.array_equal(hists, np.stack([np.stack([R.histogram(z) for z in zs]) for zs in syms]))
    hists.setflags(write=False)
    escapes = int(hists[0, :, 255].sum())
    print(f"{name}: {escapes} escapes at step 1 of {int(hists[0].sum())} symbols")
    if name != "one_pixel":
        assert escapes > 0, name                       # a condition of the test
    lo, hi = WR.chunk_prediction(hists, Le)
    blobs = {step: R.write_container(k, w, h, f, Le, [step] * 3, syms[step - 1]) for step in range(1, 65)}
    return rgb, hists, lo, hi, blobs


def _trials(codec, n):
    out = np.zeros(max(n, 1), np.uint32)
    got = codec.load_library().alice_codec_test_last_split_trials(out.ctypes.data_as(C.POINTER(C.c_uint32)), n)
    assert got == n
    return [int(v) for v in out[:n]]


def _check_prediction(codec, name):
    w, h, f, k, L = SHAPES[name]
    rgb, hists, lo, hi, blobs = _reference(name)
    p = codec.predict_wide_sizes(rgb, w, h, f, k, L)
    assert np.array_equal(p.lo, lo) and np.array_equal(p.hi, hi) and not p.status.any()
    d = torch.from_numpy(np.concatenate([rgb, rgb])).to("cuda:0")
    d_hist = torch.full((2 * 64 * 3 * 256,), 0x7FFFFFFF, dtype=torch.int32, device="cuda:0")
    pd = codec.predict_wide_sizes_device(d.data_ptr(), w, h, f, 2, k, L, d_step_hist=d_hist.data_ptr())
    got_hist = d_hist.cpu().numpy().view(np.uint32).reshape(2, 64, 3, 256)
    for i in range(2):
        assert np.array_equal(got_hist[i], hists), (name, i)
        assert np.array_equal(pd.lo[i], lo) and np.array_equal(pd.hi[i], hi)
    pn = codec.predict_wide_sizes_device(d.data_ptr(), w, h, f, 2, k, L)               # d_step_hist may be NULL
    assert np.array_equal(pn.lo, pd.lo) and np.array_equal(pn.hi, pd.hi)
    for step, want in blobs.items():
        q = Q_OF_STEP[step]
        got = codec.encode_wide(codec.FrameEncoder.with_wavelet(q, codec.WaveletType(k)), rgb, w, h, f, L)
        print(f"{name} step {step}: lo {int(lo[q])} size {len(got)} hi {int(hi[q])}")
        assert got == want, (name, step)
        assert int(lo[q]) <= len(got) <= int(hi[q]), (name, step, int(lo[q]), len(got), int(hi[q]))


@pytest.mark.parametrize("name", [n for n in SHAPES if n != "banded"])
def test_histograms_and_brackets_are_the_references_and_hold(gpu_codec, name):
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
        lib.alice_codec_test_set_value_table_radius(24)   # coefficients outside [-24, 24): histograms from real wide forward passes
        for name in ("tile_short_last_block", "generic_empty_lanes"):
            w, h, f, k, L = SHAPES[name]
            rgb, hists, lo, hi, _ = _reference(name)
            p = gpu_codec.predict_wide_sizes(rgb, w, h, f, k, L)
            assert np.array_equal(p.lo, lo) and np.array_equal(p.hi, hi)
            d = torch.from_numpy(rgb.copy()).to("cuda:0")
            d_hist = torch.zeros(64 * 3 * 256, dtype=torch.int32, device="cuda:0")
            pd = gpu_codec.predict_wide_sizes_device(d.data_ptr(), w, h, f, 1, k, L, d_step_hist=d_hist.data_ptr())
            assert np.array_equal(d_hist.cpu().numpy().view(np.uint32).reshape(64, 3, 256), hists)
            assert np.array_equal(pd.lo[0], lo) and np.array_equal(pd.hi[0], hi)
    finally:
        lib.alice_codec_test_set_value_table_radius(2048)


def _budgets(lo, hi, blobs):
    return [int(lo.min()) - 1,                                  # below the smallest lo: nothing can fit
            int(hi.max()) + 1,                                  # above the largest hi: max_quality at once
            len(blobs[SR.quality_to_step(100)]),                # the exact size at q = 100
            len(blobs[SR.quality_to_step(60)]),                 # the exact size at q = 60: refinement must find it
            int(hi[60]) - 1]                                    # one below an upper bound


@pytest.mark.parametrize("name", list(SHAPES))
def test_budget_encodes_follow_the_reference_chooser(gpu_codec, name):
    a = gpu_codec
    w, h, f, k, L = SHAPES[name]
    rgb, _, lo, hi, blobs = _reference(name)
    budgets = _budgets(lo, hi, blobs)
    want = [SR.choose(lo, hi, b, 10, 100, lambda q: len(blobs[SR.quality_to_step(q)])) for b in budgets]
    assert want[0][:2] == (10, False) and want[1] == (100, True, 0)
    assert want[2][1] and want[3][1]
    for b, (q, fits, trials) in zip(budgets, want):
        data, gq, gfits = a.encode_wide_to_size(rgb, w, h, f, b, k, 10, 100, L)
        print(f"{name} budget {b}: chose {gq} fits {gfits} size {len(data)} trials {_trials(a, 1)} (reference {q} {fits} {trials})")
        assert (gq, gfits) == (q, fits)
        assert _trials(a, 1) == [trials] and trials <= SR.REFINE_TRIALS == 4
        assert data == blobs[SR.quality_to_step(q)]
        assert data == a.encode_wide(a.FrameEncoder.with_wavelet(q, a.WaveletType(k)), rgb, w, h, f, L)
        if fits:
            assert len(data) <= b
    # three chunks under three different budgets in one device call
    d = torch.from_numpy(np.concatenate([rgb] * 3)).to("cuda:0")
    stride = (max(len(v) for v in blobs.values()) + 255) & ~255
    for first in (0, 2):
        out = torch.full((3 * stride + 256,), 0xCD, dtype=torch.uint8, device="cuda:0")
        chosen, fits, sizes = a.wide_encode_to_budget_device(d.data_ptr(), w, h, f, 3, k, budgets[first:first + 3], out.data_ptr(),
                                                             stride, 10, 100, L)
        host = out.cpu().numpy()
        assert (host[3 * stride:] == 0xCD).all()
        host = host[:3 * stride].reshape(3, stride)
        assert _trials(a, 3) == [t for _, _, t in want[first:first + 3]]
        for i in range(3):
            q, fit, _ = want[first + i]
            assert (int(chosen[i]), bool(fits[i])) == (q, fit)
            assert host[i, :int(sizes[i])].tobytes() == blobs[SR.quality_to_step(q)]
            assert (host[i, int(sizes[i]):] == 0xCD).all()
