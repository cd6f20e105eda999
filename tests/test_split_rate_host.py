"""Version 2 rate control without a device: the size bracket of split_rate_ref against split_ref's own encoder, the budget
rule on synthetic tables, and the argument checks of the new C entry points (host code: dimensions, buffer size or
regions, wavelet, lane_symbols, then the quality range)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rate_ref  # noqa: E402
import split_rate_ref as SR  # noqa: E402
import split_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["alice_codec_predict_split_sizes", "alice_codec_dev_predict_split_sizes", "alice_codec_encode_split_to_size",
               "alice_codec_dev_encode_split_regions", "alice_codec_dev_decode_split_regions",
               "alice_codec_dev_encode_split_to_budget"]


def test_own_log_table_is_the_librarys(codec):
    lo, hi, g = rate_ref.log_table(codec)
    mine = SR.log_table()
    assert [int(v) for v in lo[1:]] == mine[0][1:] and [int(v) for v in hi[1:]] == mine[1][1:] and g == mine[2]


# ---- the bracket against split_ref's encoder ----

KINDS = ("all-zero", "one symbol", "uniform 256", "geometric", "sparse")


def _symbols(kind, n, rng):
    if kind == "all-zero":
        return np.zeros(n, np.uint8)
    if kind == "one symbol":
        return np.full(n, 201, np.uint8)
    if kind == "uniform 256":
        return rng.integers(0, 256, n).astype(np.uint8)
    if kind == "geometric":
        return np.minimum(rng.geometric(0.35, n) - 1, 255).astype(np.uint8)
    s = np.zeros(n, np.uint8)                      # sparse: a few rare symbols in a sea of zeros
    k = max(n // 40, 1)
    s[rng.choice(n, k, replace=False)] = rng.integers(1, 256, k)
    return s


@pytest.mark.parametrize("L", [64, 128])
def test_bracket_contains_every_payload(L):
    rng = np.random.default_rng(1000 + L)
    checked = 0
    for n in (1, 63, 64, 65, 64 * L - 1, 64 * L, 64 * L + 1, 3 * 64 * L - 7):
        for kind in KINDS:
            sym = _symbols(kind, n, rng)
            hist = np.bincount(sym, minlength=256)
            lo, hi = SR.channel_bracket(hist, L)
            size = len(R.encode_channel(sym, R.normalize(hist), L))
            assert lo <= size <= hi, (kind, n, L, lo, size, hi)
            # the fixed part alone: block lengths, lane directories and four state bytes per lane that owns a symbol
            assert lo >= 132 * R.n_blocks_of(n, L) + 4 * SR.lanes_with_symbols(n, L)
            checked += 1
    assert checked == 8 * len(KINDS)
    assert SR.channel_bracket(np.zeros(256, np.int64), L) == (0, 0)


def test_lane_count():
    assert SR.lanes_with_symbols(1, 64) == 1 and SR.lanes_with_symbols(63, 64) == 63 and SR.lanes_with_symbols(64, 64) == 64
    assert SR.lanes_with_symbols(4096, 64) == 64 and SR.lanes_with_symbols(4097, 64) == 65
    assert SR.lanes_with_symbols(3 * 4096 - 7, 64) == 192


# ---- the budget rule on synthetic tables ----

def _tables(sizes, slack_lo, slack_hi):
    """per-quality tables from per-step exact sizes: lo = size - slack_lo, hi = size + slack_hi"""
    lo = np.zeros(101, np.int64); hi = np.zeros(101, np.int64); size = np.zeros(101, np.int64)
    for q in range(101):
        s = SR.quality_to_step(q)
        size[q] = sizes[s]; lo[q] = sizes[s] - slack_lo; hi[q] = sizes[s] + slack_hi
    return lo, hi, size


def _run(lo, hi, size, budget, min_q=10, max_q=95):
    calls = []

    def exact(q):
        calls.append(q)
        return int(size[q])

    q, fits, trials = SR.choose(lo, hi, budget, min_q, max_q, exact)
    assert trials == len(calls) <= SR.REFINE_TRIALS
    assert len({SR.quality_to_step(c) for c in calls}) == len(calls)        # no step twice
    assert calls == sorted(calls, reverse=True)                              # from the highest down
    return q, fits, calls


def test_chooser_on_synthetic_tables():
    mono = {s: 100_000 - 1000 * s for s in range(1, 65)}                     # size falls with the step
    lo, hi, size = _tables(mono, 50, 50)
    # none fits: min_q, fits = False, and nothing straddles
    assert _run(lo, hi, size, 10) == (10, False, [])
    # all fit: max_q at once
    assert _run(lo, hi, size, 10**9) == (95, True, [])
    # hi[q0] == budget exactly, the next step straddles nothing (1000 apart, brackets 100 wide)
    q0 = 50
    assert _run(lo, hi, size, int(hi[q0]))[:2] == (max(q for q in range(10, 96) if hi[q] <= hi[q0]), True)
    # the exact size of a quality: its bracket straddles, one trial finds it; the highest quality of that step is taken
    q, fits, calls = _run(lo, hi, size, int(size[60]))
    top = max(k for k in range(10, 96) if SR.quality_to_step(k) == SR.quality_to_step(60))
    assert (q, fits, calls) == (top, True, [top])
    # one byte short of that size: the trial fails, q0 (the next step down) is chosen
    q, fits, calls = _run(lo, hi, size, int(size[60]) - 1)
    assert fits and calls == [top] and SR.quality_to_step(q) == SR.quality_to_step(60) + 1
    # a budget below every hi but inside the lowest bracket: no q0, the trial decides between fits and not
    assert _run(lo, hi, size, int(size[10]))[:2] == (max(k for k in range(10, 96) if SR.quality_to_step(k) == SR.quality_to_step(10)), True)
    q, fits, calls = _run(lo, hi, size, int(size[10]) - 1)
    assert (q, fits) == (10, False) and len(calls) == 1


def test_chooser_non_monotone_and_the_cap():
    # non-monotone sizes: a higher quality that is SMALLER than its neighbours is found although lower ones do not fit
    sizes = {s: 50_000 + 700 * ((s * 37) % 11) - 300 * s for s in range(1, 65)}
    lo, hi, size = _tables(sizes, 40, 40)
    for budget in sorted({int(v) for v in size[10:96]})[::5]:
        q, fits, calls = _run(lo, hi, size, budget)
        q0 = max((k for k in range(10, 96) if hi[k] <= budget), default=None)
        if fits:
            assert size[q] <= budget and (q0 is None or q >= q0)
        else:
            assert q0 is None and q == 10
    # more than four straddling steps, none of which fits: exactly four trials, then q0
    wide = {s: 90_000 - 10 * s for s in range(1, 65)}
    lo, hi, size = _tables(wide, 2000, 2000)
    q, fits, calls = _run(lo, hi, size, int(min(size[10:96])) - 1)
    assert len(calls) == SR.REFINE_TRIALS and (q, fits) == (10, False)
    # ... and with a q0 far below, the cap still holds and q0 wins
    wide[64] = 1000
    lo, hi, size = _tables(wide, 2000, 2000)
    q, fits, calls = _run(lo, hi, size, int(min(size[11:96])) - 1, min_q=0)
    assert len(calls) == SR.REFINE_TRIALS and fits and SR.quality_to_step(q) == 64
    # repeated steps: qualities 8 and 9 share step 59 (and 5, 6 step 61): one trial per step, the higher quality stands for it
    lo, hi, size = _tables(mono_sizes(), 7000, 7000)
    q, fits, calls = _run(lo, hi, size, int(min(size[0:10])) - 1, min_q=0, max_q=9)
    assert [SR.quality_to_step(c) for c in (9, 8, 7, 6, 5, 4)] == [59, 59, 60, 61, 61, 62]
    assert calls == [9, 7, 6, 4] and (q, fits) == (0, False)


def mono_sizes():
    return {s: 100_000 - 1000 * s for s in range(1, 65)}


# ---- the C ABI ----

def test_new_symbols_are_exported_and_declared(codec):
    lib = codec.load_library()
    hdr = open(os.path.join(ROOT, "include", "alice_codec.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
    assert hasattr(lib, "alice_codec_test_last_split_trials")
    assert "alice_codec_test_last_split_trials" in open(os.path.join(ROOT, "include", "alice_codec_test.h")).read()
    assert "ALICE_SPLIT_REFINE_TRIALS = 4" in hdr


def _err(codec, fn, *args, **kw):
    with pytest.raises(codec.CodecError) as e:
        fn(*args, **kw)
    return e.value.code


NULL_ARG, BUFFER, DIMS, OVERFLOW, BITSTREAM, DEVICE = 9, 1, 2, 3, 4, 8


def test_empty_chunk_predicts_and_encodes_as_its_header(codec):
    p = codec.predict_split_sizes(np.zeros(0, np.uint8), 0, 7, 3)
    assert np.all(p.lo == SR.HEADER) and np.all(p.hi == SR.HEADER) and np.all(p.status == codec.RATE_BOUNDED)
    data, q, fits = codec.encode_split_to_size(np.zeros(0, np.uint8), 5, 0, 2, 10_000, codec.WaveletType.Haar, 20, 150, 128)
    assert (q, fits, len(data)) == (100, True, SR.HEADER)
    assert data == codec.encode_split(codec.FrameEncoder.with_wavelet(100, codec.WaveletType.Haar), b"", 5, 0, 2, 128)
    data, q, fits = codec.encode_split_to_size(np.zeros(0, np.uint8), 5, 0, 2, SR.HEADER - 1, min_quality=20, max_quality=30)
    assert (q, fits) == (20, False)
    assert data == codec.encode_split(codec.FrameEncoder.with_wavelet(20, codec.WaveletType.Cdf53), b"", 5, 0, 2)
    n = np.zeros(4, np.uint32)
    assert codec.load_library().alice_codec_test_last_split_trials(n.ctypes.data_as(C.POINTER(C.c_uint32)), 4) == 1 and n[0] == 0


def test_host_calls_validate_in_order_without_a_device(codec):
    a = codec
    z = np.zeros
    rgb = z(4 * 4 * 2 * 3, np.uint8)
    for call in (lambda *x, **k: a.predict_split_sizes(*x, **k),
                 lambda r, w, h, f, **k: a.encode_split_to_size(r, w, h, f, 10_000, **k)):
        # dimensions first, whatever the buffer and everything after it
        assert _err(a, call, z(3, np.uint8), 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, wavelet_type=7, lane_symbols=100) == OVERFLOW
        # then the buffer size (no pixels but bytes; a short buffer)
        assert _err(a, call, z(3, np.uint8), 0, 4, 4, wavelet_type=7, lane_symbols=100) == BUFFER
        assert _err(a, call, rgb[:-1], 4, 4, 2, wavelet_type=7, lane_symbols=100) == BUFFER
        # then the wavelet, then lane_symbols
        assert _err(a, call, rgb, 4, 4, 2, wavelet_type=7, lane_symbols=100) == BITSTREAM
        assert _err(a, call, rgb, 4, 4, 2, lane_symbols=100) == DIMS
        assert _err(a, call, z(0, np.uint8), 0, 4, 2, wavelet_type=3) == BITSTREAM
        assert _err(a, call, z(0, np.uint8), 0, 4, 2, lane_symbols=32) == DIMS
    # the quality range comes last
    assert _err(a, a.encode_split_to_size, rgb, 4, 4, 2, 10_000, min_quality=60, max_quality=50, lane_symbols=100) == DIMS
    with pytest.raises(a.CodecError, match="lane_symbols"):
        a.encode_split_to_size(rgb, 4, 4, 2, 10_000, min_quality=60, max_quality=50, lane_symbols=100)
    with pytest.raises(a.CodecError, match="min_quality > max_quality"):
        a.encode_split_to_size(rgb, 4, 4, 2, 10_000, min_quality=60, max_quality=50)
    with pytest.raises(a.CodecError, match="min_quality > max_quality"):
        a.encode_split_to_size(z(0, np.uint8), 0, 4, 2, 10_000, min_quality=60, max_quality=50)
    a.encode_split_to_size(z(0, np.uint8), 0, 4, 2, 10_000, min_quality=200, max_quality=120)   # both act as 100
    for bad in (-1, 1 << 64):
        with pytest.raises(ValueError):
            a.encode_split_to_size(z(0, np.uint8), 5, 0, 2, bad)
    lib = a.load_library()
    assert lib.alice_codec_predict_split_sizes(0, None, 0, 0, 0, 0, 0, None, None) == NULL_ARG
    n = C.c_uint64(7)
    assert not lib.alice_codec_encode_split_to_size(0, None, 0, 0, 0, 0, 0, 100, 10, 95, None, None, C.byref(n))
    assert lib.alice_codec_last_error() == NULL_ARG and n.value == 7
    if a.device_count() < 1:   # valid arguments reach the device check, and only they
        assert _err(a, a.predict_split_sizes, rgb, 4, 4, 2) == DEVICE
        assert _err(a, a.encode_split_to_size, rgb, 4, 4, 2, 10_000) == DEVICE


def test_device_calls_validate_in_order_without_a_device(codec):
    a = codec
    P = 0x1000                        # a pointer that is never followed: every check below is host code
    W, H, w, h, f, n = 70, 50, 32, 24, 6, 3
    inside = [(0, 0), (38, 26), (5, 7)]
    outside = [(0, 0), (39, 26), (5, 7)]
    sentinel = np.full(n, 77, np.uint64)

    def regions(origins=inside, w=w, h=h, f=f, wavelet=1, quality=80, lane=0, src=P, out=P):
        o = np.array(origins, np.uint32).reshape(-1)
        q = None
        return a.load_library().alice_codec_dev_encode_split_regions(
            src, W, H, o.ctypes.data_as(C.POINTER(C.c_uint32)), w, h, f, len(origins), wavelet, quality, q, lane, out, 1 << 20,
            sentinel.ctypes.data_as(C.POINTER(C.c_uint64)), None)

    def budget(origins=inside, w=w, h=h, f=f, wavelet=1, lane=0, min_q=10, max_q=95, src=P, n=n):
        o = None if origins is None else np.array(origins, np.uint32).reshape(-1)
        b = np.full(n, 5000, np.uint64)
        ch = np.full(n, 9, np.uint8); ok = np.full(n, 9, np.uint8)
        rc = a.load_library().alice_codec_dev_encode_split_to_budget(
            src, W, H, None if o is None else o.ctypes.data_as(C.POINTER(C.c_uint32)), w, h, f, n, wavelet, lane,
            b.ctypes.data_as(C.POINTER(C.c_uint64)), min_q, max_q, ch.ctypes.data_as(C.POINTER(C.c_uint8)),
            ok.ctypes.data_as(C.POINTER(C.c_uint8)), P, 1 << 20, sentinel.ctypes.data_as(C.POINTER(C.c_uint64)), None)
        assert (ch == 9).all() and (ok == 9).all()
        return rc

    for call in (regions, budget):
        assert call(src=None) == NULL_ARG
        assert call(w=0, origins=outside, wavelet=9, lane=100) == DIMS           # dimensions first
        assert call(w=0xFFFFFFFF, h=0xFFFFFFFF, f=0xFFFFFFFF, wavelet=9) == OVERFLOW
        assert call(origins=outside, wavelet=9, lane=100) == DIMS                 # then the rectangles ...
        assert "does not lie inside" in a.load_library().alice_codec_last_error_message().decode()
        assert call(wavelet=9, lane=100) == BITSTREAM                             # ... the wavelet ...
        assert call(lane=100) == DIMS                                             # ... and lane_symbols
        assert "lane_symbols" in a.load_library().alice_codec_last_error_message().decode()
    assert regions(out=None) == NULL_ARG
    assert budget(lane=100, min_q=60, max_q=50) == DIMS and "lane_symbols" in a.load_library().alice_codec_last_error_message().decode()
    assert budget(min_q=60, max_q=50) == DIMS and "min_quality" in a.load_library().alice_codec_last_error_message().decode()
    assert budget(origins=None, n=0) == DIMS                                       # an empty batch
    assert (sentinel == 77).all()
    lib = a.load_library()
    u64 = C.POINTER(C.c_uint64)
    lo = np.zeros(101, np.uint64)
    assert lib.alice_codec_dev_predict_split_sizes(None, 4, 4, 2, 1, 0, 0, lo.ctypes.data_as(u64), lo.ctypes.data_as(u64), None) == NULL_ARG
    assert lib.alice_codec_dev_predict_split_sizes(P, 4, 0, 2, 1, 9, 100, lo.ctypes.data_as(u64), lo.ctypes.data_as(u64), None) == DIMS
    assert lib.alice_codec_dev_predict_split_sizes(P, 4, 4, 2, 1, 9, 100, lo.ctypes.data_as(u64), lo.ctypes.data_as(u64), None) == BITSTREAM
    assert lib.alice_codec_dev_predict_split_sizes(P, 4, 4, 2, 1, 2, 100, lo.ctypes.data_as(u64), lo.ctypes.data_as(u64), None) == DIMS
    o = np.array([80, 0], np.uint32)
    sz = np.array([2000], np.uint64)
    assert lib.alice_codec_dev_decode_split_regions(None, 4096, sz.ctypes.data_as(u64), 1, P, W, H, o.ctypes.data_as(C.POINTER(C.c_uint32)), None) == NULL_ARG
    assert lib.alice_codec_dev_decode_split_regions(P, 4096, sz.ctypes.data_as(u64), 0, P, W, H, o.ctypes.data_as(C.POINTER(C.c_uint32)), None) == DIMS
    assert lib.alice_codec_dev_decode_split_regions(P, 4096, sz.ctypes.data_as(u64), 1, P, W, H, o.ctypes.data_as(C.POINTER(C.c_uint32)), None) == DIMS
    if a.device_count() < 1:
        assert regions() == DEVICE and budget() == DEVICE and budget(origins=None) == DEVICE


def test_person_chunks_refuse_a_budget_in_v1(codec):
    with pytest.raises(codec.CodecError):
        codec.encode_person_chunks(0x1000, 0x1000, 8, 8, 2, 1, 80, max_bytes=1000)
    with pytest.raises(codec.CodecError):
        codec.encode_person_chunks(0x1000, 0x1000, 8, 8, 2, 1, 80, format="v3")
