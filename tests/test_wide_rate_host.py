"""Version 3 rate control without a device: the size bracket of wide_rate_ref against wide_ref's own
encoder, its reduction to version 2's bracket when nothing escapes, and the argument checks of the six new C entry points
(host code, in the order NULL arguments, dimensions, buffer size or rectangles, wavelet, lane_symbols, quality range)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_rate_ref as SR  # noqa: E402
import wide_rate_ref as WR  # noqa: E402
import wide_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["alice_codec_predict_wide_sizes", "alice_codec_dev_predict_wide_sizes", "alice_codec_encode_wide_to_size",
               "alice_codec_dev_encode_wide_regions", "alice_codec_dev_decode_wide_regions",
               "alice_codec_dev_encode_wide_to_budget"]
Z_MAX = R.ESCAPE + R.RES_MAX     # 4350: the largest symbol the format codes

# ---- the bracket against wide_ref's encoder ----

KINDS = ("geometric, no escapes", "heavy tail", "uniform 0..4350", "all 255 + 4095", "2 % escapes")


def _symbols(kind, n, rng):
    if kind == "geometric, no escapes":
        return np.minimum(rng.geometric(0.2, n) - 1, 254).astype(np.uint16)
    if kind == "heavy tail":
        return np.minimum(np.floor(rng.pareto(0.6, n) * 6), Z_MAX).astype(np.uint16)
    if kind == "uniform 0..4350":
        return rng.integers(0, Z_MAX + 1, n).astype(np.uint16)
    if kind == "all 255 + 4095":
        return np.full(n, Z_MAX, np.uint16)
    z = np.minimum(rng.geometric(0.3, n) - 1, 254).astype(np.uint16)        # 2 % escapes (at least one)
    k = max(n // 50, 1)
    z[rng.choice(n, k, replace=False)] = rng.integers(R.ESCAPE, Z_MAX + 1, k)
    return z


def _sizes(L):
    return (1, 63, 64, 65, 64 * L - 1, 64 * L, 64 * L + 1, 3 * 64 * L + 777)


@pytest.mark.parametrize("L", [64, 128, 512])
def test_bracket_contains_every_payload(L):
    rng = np.random.default_rng(3000 + L)
    checked = 0
    shares = set()
    for n in _sizes(L):
        for kind in KINDS:
            z = _symbols(kind, n, rng)
            hist = R.histogram(z)
            assert int(hist.sum()) == n and int(hist[255]) == int((z >= 255).sum())
            lo, hi = WR.channel_bracket(hist, L)
            size = len(R.encode_channel(z, R.normalize(hist), L))
            assert lo <= size <= hi, (kind, n, L, lo, size, hi)
            # the fixed part alone: block lengths, lane directories and four state bytes per lane that owns a symbol
            assert lo >= 132 * R.n_blocks_of(n, L) + 4 * WR.lanes_with_symbols(n, L)
            assert size <= R.stream_bound(n, L)
            shares.add((kind, int(hist[255]) == 0, int(hist[255]) == n))
            checked += 1
    assert checked == 8 * len(KINDS)
    assert ("geometric, no escapes", True, False) in shares and ("all 255 + 4095", False, True) in shares   # shares 0 and 1


@pytest.mark.parametrize("L", [64, 128, 512])
def test_without_escapes_it_is_version_2s_bracket(L):
    rng = np.random.default_rng(77 + L)
    for n in _sizes(L):
        for p in (0.05, 0.5):
            hist = np.bincount(np.minimum(rng.geometric(p, n) - 1, 254), minlength=256)
            assert hist[255] == 0
            assert WR.channel_bracket(hist, L) == SR.channel_bracket(hist, L)
    # and one escape moves it: one more step, twelve more bits
    hist = np.zeros(256, np.int64); hist[0] = 5000; hist[255] = 1
    assert WR.channel_bracket(hist, L)[1] > SR.channel_bracket(hist, L)[1]


def test_an_empty_channel_is_nothing():
    for L in (64, 128, 512, 8192):
        assert WR.channel_bracket(np.zeros(256, np.int64), L) == (0, 0)
    lo, hi = WR.chunk_prediction(np.zeros((64, 3, 256), np.int64), 512)
    assert np.all(lo == WR.HEADER) and np.all(hi == WR.HEADER) and WR.HEADER == 1630


# ---- the C ABI ----

def test_new_symbols_are_exported_and_declared(codec):
    lib = codec.load_library()
    hdr = open(os.path.join(ROOT, "include", "alice_codec.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
    for name in ("predict_wide_sizes", "predict_wide_sizes_device", "encode_wide_to_size", "wide_encode_regions_device",
                 "wide_decode_regions_device", "wide_encode_to_budget_device"):
        assert callable(getattr(codec, name)), name


def _err(codec, fn, *args, **kw):
    with pytest.raises(codec.CodecError) as e:
        fn(*args, **kw)
    return e.value.code


def _msg(codec):
    return codec.load_library().alice_codec_last_error_message().decode()


NULL_ARG, BUFFER, DIMS, OVERFLOW, BITSTREAM, DEVICE = 9, 1, 2, 3, 4, 8


def test_empty_chunk_predicts_and_encodes_as_its_header(codec):
    p = codec.predict_wide_sizes(np.zeros(0, np.uint8), 0, 7, 3)
    assert np.all(p.lo == WR.HEADER) and np.all(p.hi == WR.HEADER) and np.all(p.status == codec.RATE_BOUNDED)
    data, q, fits = codec.encode_wide_to_size(np.zeros(0, np.uint8), 5, 0, 2, 10_000, codec.WaveletType.Haar, 20, 150, 128)
    assert (q, fits, len(data)) == (100, True, WR.HEADER) and data[4] == 3
    assert data == codec.encode_wide(codec.FrameEncoder.with_wavelet(100, codec.WaveletType.Haar), b"", 5, 0, 2, 128)
    data, q, fits = codec.encode_wide_to_size(np.zeros(0, np.uint8), 5, 0, 2, WR.HEADER - 1, min_quality=20, max_quality=30)
    assert (q, fits) == (20, False)
    assert data == codec.encode_wide(codec.FrameEncoder.with_wavelet(20, codec.WaveletType.Cdf53), b"", 5, 0, 2)
    n = np.zeros(4, np.uint32)
    assert codec.load_library().alice_codec_test_last_split_trials(n.ctypes.data_as(C.POINTER(C.c_uint32)), 4) == 1 and n[0] == 0
    codec.encode_wide_to_size(np.zeros(0, np.uint8), 5, 0, 2, 10_000, lane_symbols=8192)      # the top of version 3's range


def test_host_calls_validate_in_order_without_a_device(codec):
    a = codec
    z = np.zeros
    rgb = z(4 * 4 * 2 * 3, np.uint8)
    for call in (lambda *x, **k: a.predict_wide_sizes(*x, **k),
                 lambda r, w, h, f, **k: a.encode_wide_to_size(r, w, h, f, 10_000, **k)):
        # dimensions first, whatever the buffer and everything after it
        assert _err(a, call, z(3, np.uint8), 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, wavelet_type=7, lane_symbols=100) == OVERFLOW
        # then the buffer size (no pixels but bytes; a short buffer)
        assert _err(a, call, z(3, np.uint8), 0, 4, 4, wavelet_type=7, lane_symbols=100) == BUFFER
        assert _err(a, call, rgb[:-1], 4, 4, 2, wavelet_type=7, lane_symbols=100) == BUFFER
        # then the wavelet, then lane_symbols: 100 is no power of two, 16384 is version 2's top and refused here
        assert _err(a, call, rgb, 4, 4, 2, wavelet_type=7, lane_symbols=100) == BITSTREAM
        for lane in (100, 16384):
            assert _err(a, call, rgb, 4, 4, 2, lane_symbols=lane) == DIMS
            assert "lane_symbols" in _msg(a) and "8192" in _msg(a)
        assert _err(a, call, z(0, np.uint8), 0, 4, 2, wavelet_type=3) == BITSTREAM
        assert _err(a, call, z(0, np.uint8), 0, 4, 2, lane_symbols=32) == DIMS
        assert _err(a, call, z(0, np.uint8), 0, 4, 2, lane_symbols=16384) == DIMS
    # the quality range comes last
    for lane in (100, 16384):
        assert _err(a, a.encode_wide_to_size, rgb, 4, 4, 2, 10_000, min_quality=60, max_quality=50, lane_symbols=lane) == DIMS
        assert "lane_symbols" in _msg(a)
    with pytest.raises(a.CodecError, match="min_quality > max_quality"):
        a.encode_wide_to_size(rgb, 4, 4, 2, 10_000, min_quality=60, max_quality=50)
    with pytest.raises(a.CodecError, match="min_quality > max_quality"):
        a.encode_wide_to_size(z(0, np.uint8), 0, 4, 2, 10_000, min_quality=60, max_quality=50)
    a.encode_wide_to_size(z(0, np.uint8), 0, 4, 2, 10_000, min_quality=200, max_quality=120)   # both act as 100
    for bad in (-1, 1 << 64):
        with pytest.raises(ValueError):
            a.encode_wide_to_size(z(0, np.uint8), 5, 0, 2, bad)
    lib = a.load_library()
    u64 = C.POINTER(C.c_uint64)
    lo = np.full(101, 77, np.uint64); hi = np.full(101, 77, np.uint64)
    assert lib.alice_codec_predict_wide_sizes(0, None, 0, 0, 0, 0, 0, None, None) == NULL_ARG
    assert lib.alice_codec_predict_wide_sizes(0, rgb.ctypes.data_as(C.POINTER(C.c_uint8)), rgb.size, 4, 4, 2, 16384,
                                              lo.ctypes.data_as(u64), hi.ctypes.data_as(u64)) == DIMS
    assert (lo == 77).all() and (hi == 77).all()                                                # sentinels untouched
    n = C.c_uint64(7)
    assert not lib.alice_codec_encode_wide_to_size(0, None, 0, 0, 0, 0, 0, 100, 10, 95, None, None, C.byref(n))
    assert lib.alice_codec_last_error() == NULL_ARG and n.value == 7
    ch = C.c_uint8(9); ok = C.c_uint8(9)
    assert not lib.alice_codec_encode_wide_to_size(0, rgb.ctypes.data_as(C.POINTER(C.c_uint8)), rgb.size, 4, 4, 2, 16384, 100, 10, 95,
                                                   C.byref(ch), C.byref(ok), C.byref(n))
    assert lib.alice_codec_last_error() == DIMS and (ch.value, ok.value, n.value) == (9, 9, 7)
    if a.device_count() < 1:   # valid arguments reach the device check, and only they
        assert _err(a, a.predict_wide_sizes, rgb, 4, 4, 2) == DEVICE
        assert _err(a, a.encode_wide_to_size, rgb, 4, 4, 2, 10_000) == DEVICE
        assert _err(a, a.predict_wide_sizes, rgb, 4, 4, 2, lane_symbols=8192) == DEVICE


def test_device_calls_validate_in_order_without_a_device(codec):
    a = codec
    lib = a.load_library()
    P = 0x1000                        # a pointer that is never followed: every check below is host code
    W, H, w, h, f, n = 70, 50, 32, 24, 6, 3
    inside = [(0, 0), (38, 26), (5, 7)]
    outside = [(0, 0), (39, 26), (5, 7)]
    sentinel = np.full(n, 77, np.uint64)
    u32, u64, u8 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)

    def regions(origins=inside, w=w, h=h, f=f, wavelet=1, quality=80, lane=0, src=P, out=P):
        o = np.array(origins, np.uint32).reshape(-1)
        return lib.alice_codec_dev_encode_wide_regions(src, W, H, o.ctypes.data_as(u32), w, h, f, len(origins), wavelet, quality, None,
                                                       lane, out, 1 << 20, sentinel.ctypes.data_as(u64), None)

    def budget(origins=inside, w=w, h=h, f=f, wavelet=1, lane=0, min_q=10, max_q=95, src=P, n=n):
        o = None if origins is None else np.array(origins, np.uint32).reshape(-1)
        b = np.full(max(n, 1), 5000, np.uint64)
        ch = np.full(max(n, 1), 9, np.uint8); ok = np.full(max(n, 1), 9, np.uint8)
        rc = lib.alice_codec_dev_encode_wide_to_budget(src, W, H, None if o is None else o.ctypes.data_as(u32), w, h, f, n, wavelet, lane,
                                                       b.ctypes.data_as(u64), min_q, max_q, ch.ctypes.data_as(u8), ok.ctypes.data_as(u8), P,
                                                       1 << 20, sentinel.ctypes.data_as(u64), None)
        assert (ch == 9).all() and (ok == 9).all()
        return rc

    for call in (regions, budget):
        assert call(src=None) == NULL_ARG
        assert call(w=0, origins=outside, wavelet=9, lane=100) == DIMS           # dimensions first
        assert call(w=0xFFFFFFFF, h=0xFFFFFFFF, f=0xFFFFFFFF, wavelet=9) == OVERFLOW
        assert call(origins=outside, wavelet=9, lane=100) == DIMS                 # then the rectangles ...
        assert "does not lie inside" in _msg(a)
        assert call(wavelet=9, lane=100) == BITSTREAM                             # ... the wavelet ...
        for lane in (100, 16384):                                                 # ... and lane_symbols
            assert call(lane=lane) == DIMS
            assert "lane_symbols" in _msg(a) and "8192" in _msg(a)
    assert regions(out=None) == NULL_ARG
    assert budget(lane=16384, min_q=60, max_q=50) == DIMS and "lane_symbols" in _msg(a)
    assert budget(min_q=60, max_q=50) == DIMS and "min_quality" in _msg(a)
    assert budget(origins=None, n=0) == DIMS                                       # an empty batch
    assert (sentinel == 77).all()
    lo = np.full(101, 77, np.uint64)

    def predict(src=P, h=4, wavelet=0, lane=0, hist=None):
        return lib.alice_codec_dev_predict_wide_sizes(src, 4, h, 2, 1, wavelet, lane, lo.ctypes.data_as(u64), lo.ctypes.data_as(u64), hist, None)

    assert predict(src=None) == NULL_ARG
    assert predict(h=0, wavelet=9, lane=100) == DIMS
    assert predict(wavelet=9, lane=100) == BITSTREAM
    assert predict(wavelet=2, lane=100) == DIMS and "lane_symbols" in _msg(a)
    assert predict(wavelet=2, lane=16384, hist=P) == DIMS and "lane_symbols" in _msg(a)
    assert (lo == 77).all()
    o = np.array([80, 0], np.uint32)
    sz = np.array([2000], np.uint64)

    def decode(alc=P, n=1):
        return lib.alice_codec_dev_decode_wide_regions(alc, 4096, sz.ctypes.data_as(u64), n, P, W, H, o.ctypes.data_as(u32), None)

    assert decode(alc=None) == NULL_ARG
    assert decode(n=0) == DIMS
    assert decode() == DIMS                                                         # the origin (80, 0) starts outside the frame
    if a.device_count() < 1:
        assert regions() == DEVICE and budget() == DEVICE and budget(origins=None) == DEVICE
        assert regions(lane=8192) == DEVICE and predict() == DEVICE and predict(hist=P) == DEVICE
        o[:] = (3, 4)
        assert decode() == DEVICE


def test_person_chunks_argument_rules(codec):
    a = codec
    with pytest.raises(a.CodecError, match="format"):
        a.encode_person_chunks(0x1000, 0x1000, 8, 8, 2, 1, 80, format="v3")
    with pytest.raises(a.CodecError, match="max_bytes"):
        a.encode_person_chunks(0x1000, 0x1000, 8, 8, 2, 1, 80, max_bytes=1000)
    with pytest.raises(a.CodecError, match="max_bytes"):
        a.encode_person_chunks(0x1000, 0x1000, 8, 8, 2, 1, 80, format="v1", max_bytes=1000)
    # format="wide" passes the format check, with and without a budget: the next refusal is another one (the width)
    for kw in ({}, {"max_bytes": 1000}):
        with pytest.raises(a.CodecError) as e:
            a.encode_person_chunks(0x1000, 0x1000, 0, 8, 2, 1, 80, format="wide", **kw)
        assert "format" not in str(e.value) and "max_bytes" not in str(e.value)
