"""Quality control without a GPU: the rule of alice_codec_encode_to_psnr as tests/quality_ref.py
restates it against an exhaustive scan on the CPU oracle, the arguments every new call refuses before it looks for a
device, and the case table of the squared-error kernel against the classes the constants of csrc/kernels.h define."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quality_cases as QC  # noqa: E402
import quality_ref as Q  # noqa: E402
import wide_oracle as WO  # noqa: E402

ROOT = QC.ROOT
W, H, F = 64, 48, 8
N = W * H * F * 3
NULL_ARG, BUFFER, DIMS, OVERFLOW, BITSTREAM, DEVICE = 9, 1, 2, 3, 4, 8
NEW_SYMBOLS = ["alice_codec_dev_rgb_sse", "alice_codec_dev_trial_sse", "alice_codec_psnr_from_sse", "alice_codec_dev_encode_to_psnr",
               "alice_codec_encode_to_psnr"]


def content():
    return WO.smooth_plus_noise(W, H, F)


# ---- the threshold ----
def test_sse_max():
    assert Q.sse_max(math.inf, N) == 0
    assert Q.sse_max(5000.0, N) == 0                      # 10^500 is +inf in f64
    assert Q.sse_max(0.0, N) == 65025 * N
    assert Q.sse_max(10.0, N) == 65025 * N // 10
    assert Q.sse_max(20.0, 3) == 1950                     # floor(195075 / 100)
    assert Q.sse_max(48.13, 0) == 0
    for t in (17.3, 30.0, 41.77):                         # a trial at the threshold passes, one above it does not
        m = Q.sse_max(t, N)
        assert Q.choose({Q.step_of(50): m}, N, t, 50, 50) == (50, True, 1)
        assert Q.choose({Q.step_of(50): m + 1}, N, t, 50, 50) == (50, False, 1)


def test_psnr_from_sse_is_the_expression_of_psnr(codec):
    lib = codec.load_library()
    for sse, n in ((0, 10), (0, 0), (7, 0), (1, 1), (65025, 1), (123456789, N), (65025 * N, N), ((1 << 40) + 3, 3 << 30)):
        assert codec.psnr_from_sse(sse, n) == Q.psnr_from_sse(sse, n), (sse, n)
        assert lib.alice_codec_psnr_from_sse(sse, n) == Q.psnr_from_sse(sse, n)


def test_candidates():
    c = Q.candidates(0, 100)
    assert len(c) == 64 and c[0] == 0 and c[-1] == 100
    steps = [Q.step_of(q) for q in c]
    assert steps == sorted(steps, reverse=True) and steps[0] == 64 and steps[-1] == 1
    for q in c:                                            # the lowest quality that has the step
        assert q == 0 or Q.step_of(q - 1) != Q.step_of(q)
    assert Q.candidates(0, 255) == c and Q.candidates(200, 255) == [100]
    assert Q.candidates(97, 98) == [97] and Q.step_of(97) == Q.step_of(98) == 3


# ---- the rule against an exhaustive scan on the oracle ----
@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("version,max_q", [(Q.FORMAT_WIDE, 100), (Q.FORMAT_SPLIT, 96)])
def test_bisection_equals_the_scan_where_distortion_is_monotone(version, max_q, kind):
    table = Q.step_table(version, content(), W, H, F, kind, max_q)
    steps = sorted(table)
    assert len(steps) == (64 if max_q == 100 else 61)
    # the premise, on the oracle's numbers: distortion does not fall as the step grows
    assert all(table[a] <= table[b] for a, b in zip(steps[:-1], steps[1:])), (version, kind)
    targets = Q.midway_targets(table, N)
    assert len(targets) >= len(steps) - 2
    most = 0
    for t in targets:
        q, reached, trials = Q.choose(table, N, t, 0, max_q)
        assert (q, reached) == Q.scan(table, N, t, 0, max_q), (version, kind, t)
        assert trials <= Q.MAX_TRIALS
        most = max(most, trials)
    assert most == Q.MAX_TRIALS                            # the bound is reached: 2 + 6 for 64 steps
    # sub-ranges: the same answer as the scan of the sub-range
    for lo, hi in ((10, 95), (40, 60), (77, 77), (0, 5)):
        hi = min(hi, max_q)
        for t in targets[::5]:
            q, reached, trials = Q.choose(table, N, t, lo, hi)
            assert (q, reached) == Q.scan(table, N, t, lo, hi) and trials <= Q.MAX_TRIALS


def test_early_exits():
    table = Q.step_table(Q.FORMAT_WIDE, content(), W, H, F, 1)
    best = Q.psnr_from_sse(table[1], N)
    worst = Q.psnr_from_sse(table[64], N)
    assert Q.choose(table, N, best + 1.0, 0, 100) == (100, False, 1)          # unreachable: the finest step fails
    assert Q.choose(table, N, worst - 1.0, 0, 100) == (0, True, 2)            # met at min_q: two trials
    assert Q.choose(table, N, worst - 1.0, 37, 37) == (37, True, 1)           # one candidate: one trial
    assert Q.choose(table, N, math.inf, 0, 100) == (100, False, 1)            # the reference's inverse is not exact at step 1
    assert Q.choose(table, N, best + 1.0, 10, 250) == (100, False, 1)         # qualities above 100 act as 100
    zero = {s: 0 for s in table}                                              # a chunk without pixels: nothing differs
    assert Q.choose(zero, 0, math.inf, 20, 90) == (20, True, 2)


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_version_2_wraps_at_the_top(kind):
    """Among steps 1 to 3 (q >= 97) the u8 symbol wraps: distortion RISES towards the finest step (step 1 with every wavelet,
    steps 2 and 3 as well with CDF 9/7), the finest step fails a target that step 4 meets, and the call answers max_q,
    reached = 0."""
    table = Q.step_table(Q.FORMAT_SPLIT, content(), W, H, F, kind, 100)
    assert table[1] > table[4] and any(table[s] > table[s + 1] for s in (1, 2, 3))
    if kind == 1:
        assert table[2] > table[4] and table[3] > table[4]
    t = 0.5 * (Q.psnr_from_sse(table[4], N) + Q.psnr_from_sse(table[5], N))   # step 4 (q = 96) meets it
    assert Q.choose(table, N, t, 0, 96)[:2] == Q.scan(table, N, t, 0, 96) == (96, True)
    assert Q.choose(table, N, t, 0, 100) == (100, False, 1)
    wide = Q.step_table(Q.FORMAT_WIDE, content(), W, H, F, kind, 100)         # version 3 does not wrap
    assert wide[1] <= wide[2] <= wide[3] <= wide[4] == table[4]


def test_reversible_trials_on_the_oracle():
    rgb = content()
    for kind in (0, 1, 2):
        assert Q.chunk_sse(Q.FORMAT_REVERSIBLE, rgb, W, H, F, 100, kind) == 0
    assert Q.chunk_sse(Q.FORMAT_REVERSIBLE, rgb, W, H, F, 80, 1) > 0


# ---- the C ABI: refusals before a device is looked for ----
def test_new_symbols_are_exported_and_declared(codec):
    lib = codec.load_library()
    hdr = open(os.path.join(ROOT, "include", "alice_codec.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name + "(" in hdr, name
    test_hdr = open(os.path.join(ROOT, "include", "alice_codec_test.h")).read()
    assert hasattr(lib, "alice_codec_test_last_quality_trials") and "alice_codec_test_last_quality_trials(" in test_hdr
    assert "ALICE_FORMAT_SPLIT = 2, ALICE_FORMAT_WIDE = 3, ALICE_FORMAT_REVERSIBLE = 4" in hdr
    assert (codec.FORMAT_SPLIT, codec.FORMAT_WIDE, codec.FORMAT_REVERSIBLE) == (2, 3, 4)


def _code(codec, fn, *args, **kw):
    with pytest.raises(codec.CodecError) as e:
        fn(*args, **kw)
    return e.value.code


def _msg(codec):
    return codec.load_library().alice_codec_last_error_message().decode()


P = 0x1000   # a pointer that is never followed: every check below is host code


def test_rgb_sse_validates_without_a_device(codec):
    a = codec
    lib = a.load_library()
    packed = (4, 4, 2)
    assert _code(a, a.rgb_sse_device, 0, P, *packed, d_frame_sse_ptr=P) == NULL_ARG
    assert _code(a, a.rgb_sse_device, P, 0, *packed, d_frame_sse_ptr=P) == NULL_ARG
    assert lib.alice_codec_dev_rgb_sse(P, 12, 48, P, 12, 48, 4, 4, 2, None, None) == NULL_ARG
    for w, h, n in ((0, 4, 2), (4, 0, 2), (4, 4, 0)):
        assert _code(a, a.rgb_sse_device, P, P, w, h, n, d_frame_sse_ptr=P) == DIMS
    assert _code(a, a.rgb_sse_device, P, P, 0xFFFFFFFF, 0xFFFFFFFF, 1 << 40, d_frame_sse_ptr=P) == OVERFLOW
    assert _code(a, a.rgb_sse_device, P, P, *packed, a_pitches=(11, 48), d_frame_sse_ptr=P) == DIMS
    assert "row pitch of a" in _msg(a)
    assert _code(a, a.rgb_sse_device, P, P, *packed, b_pitches=(11, 48), d_frame_sse_ptr=P) == DIMS
    assert "row pitch of b" in _msg(a)
    assert _code(a, a.rgb_sse_device, P, P, *packed, a_pitches=(12, 47), d_frame_sse_ptr=P) == DIMS
    assert "frame pitch of a" in _msg(a)
    assert _code(a, a.rgb_sse_device, P, P, *packed, b_pitches=(16, 59), d_frame_sse_ptr=P) == DIMS   # 3 * 16 + 12 = 60
    assert "frame pitch of b" in _msg(a)
    assert _code(a, a.rgb_sse_device, P, P, 4, 4, 3, a_pitches=(12, 1 << 63), d_frame_sse_ptr=P) == OVERFLOW
    if a.device_count() < 1:   # valid arguments reach the device check, and only they
        assert _code(a, a.rgb_sse_device, P, P, *packed, b_pitches=(16, 60), d_frame_sse_ptr=P) == DEVICE


def test_trial_sse_validates_in_order_without_a_device(codec):
    a = codec
    lib = a.load_library()
    k = a.WaveletType.Cdf53
    sse = np.full(2, 77, np.uint64)
    u64 = C.POINTER(C.c_uint64)
    # null arguments first, then the format byte, dimensions, regions, the wavelet byte
    assert lib.alice_codec_dev_trial_sse(9, None, 0, 0, None, 0, 0, 0, 0, 9, 80, None, sse.ctypes.data_as(u64), None, None) == NULL_ARG
    assert lib.alice_codec_dev_trial_sse(9, P, 0, 0, None, 0, 0, 0, 0, 9, 80, None, None, None, None) == NULL_ARG
    for fmt in (0, 1, 5, 255):
        assert _code(a, a.trial_sse_device, fmt, P, 0, 0, 0, 0, 9, 80) == BITSTREAM
        assert "format byte" in _msg(a)
    with pytest.raises(a.CodecError, match="format"):
        a.trial_sse_device("v1", P, 8, 8, 2, 1, k, 80)
    for fmt in ("split", "wide", "reversible", 2, 3, 4):
        assert _code(a, a.trial_sse_device, fmt, P, 0, 8, 2, 1, 9, 80) == DIMS
        assert _code(a, a.trial_sse_device, fmt, P, 8, 8, 2, 0, 9, 80) == DIMS
        assert _code(a, a.trial_sse_device, fmt, P, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 1, 9, 80) == OVERFLOW
        assert _code(a, a.trial_sse_device, fmt, P, 8, 8, 2, 2, 9, 80, frame_width=10, frame_height=10, origins=[(0, 0), (3, 1)]) == DIMS
        assert "region 1" in _msg(a)
        assert _code(a, a.trial_sse_device, fmt, P, 8, 8, 2, 2, 9, 80, frame_width=11, frame_height=10, origins=[(0, 0), (3, 1)]) == BITSTREAM
        assert "wavelet" in _msg(a)
        assert _code(a, a.trial_sse_device, fmt, P, 8, 8, 2, 1, 3, 80) == BITSTREAM
    with pytest.raises(ValueError):
        a.trial_sse_device("wide", P, 8, 8, 2, 2, k, 80, qualities=[1, 2, 3])
    assert (sse == 77).all()
    if a.device_count() < 1:
        assert _code(a, a.trial_sse_device, "wide", P, 8, 8, 2, 1, k, 80) == DEVICE
        assert _code(a, a.trial_psnr_device, "reversible", P, 8, 8, 2, 1, k, 100) == DEVICE


def test_encode_to_psnr_device_validates_in_order_without_a_device(codec):
    a = codec
    lib = a.load_library()
    k = a.WaveletType.Cdf53

    def call(fmt, w, h, f, n, wavelet, lane, t, lo, hi, fw=0, fh=0, origins=None):
        return a._encode_container_to_psnr_device(fmt, P, w, h, f, n, wavelet, t, P, 1 << 20, lo, hi, lane, fw, fh, origins, 0)

    ch = np.full(2, 9, np.uint8); ok = np.full(2, 9, np.uint8); db = np.full(2, -3.0); sz = np.full(2, 7, np.uint64)
    u8, u64, f64 = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    outs = (ch.ctypes.data_as(u8), ok.ctypes.data_as(u8), db.ctypes.data_as(f64))
    raw = lib.alice_codec_dev_encode_to_psnr
    assert raw(9, None, 0, 0, None, 0, 0, 0, 0, 9, 3, -1.0, 60, 50, *outs, P, 0, sz.ctypes.data_as(u64), None) == NULL_ARG
    assert raw(9, P, 0, 0, None, 0, 0, 0, 0, 9, 3, -1.0, 60, 50, outs[0], outs[1], None, P, 0, sz.ctypes.data_as(u64), None) == NULL_ARG
    assert raw(9, P, 0, 0, None, 0, 0, 0, 0, 9, 3, -1.0, 60, 50, *outs, None, 0, sz.ctypes.data_as(u64), None) == NULL_ARG
    # the format byte, with everything behind it wrong too
    assert raw(9, P, 0, 0, None, 0, 0, 0, 0, 9, 3, -1.0, 60, 50, *outs, P, 0, sz.ctypes.data_as(u64), None) == BITSTREAM
    assert "format byte" in _msg(a)
    assert raw(4, P, 0, 0, None, 0, 0, 0, 0, 9, 3, -1.0, 60, 50, *outs, P, 0, sz.ctypes.data_as(u64), None) == BITSTREAM
    assert "lossless container" in _msg(a) and "no quality to search" in _msg(a)
    for fmt in ("split", "wide"):
        assert _code(a, call, fmt, 0, 8, 2, 1, 9, 3, 30.0, 60, 50) == DIMS and "dimensions" in _msg(a)
        assert _code(a, call, fmt, 8, 8, 2, 0, 9, 3, 30.0, 60, 50) == DIMS and "empty batch" in _msg(a)
        assert _code(a, call, fmt, 8, 8, 2, 2, 9, 3, 30.0, 60, 50, 10, 10, [(0, 0), (3, 1)]) == DIMS and "region 1" in _msg(a)
        assert _code(a, call, fmt, 8, 8, 2, 1, 9, 3, 30.0, 60, 50) == BITSTREAM and "wavelet" in _msg(a)
        assert _code(a, call, fmt, 8, 8, 2, 1, k, 3, 30.0, 60, 50) == DIMS and "lane_symbols" in _msg(a)
        assert _code(a, call, fmt, 8, 8, 2, 1, k, 16384 if fmt == "wide" else 32768, 30.0, 60, 50) == DIMS and "lane_symbols" in _msg(a)
        assert _code(a, call, fmt, 8, 8, 2, 1, k, 64, 30.0, 60, 50) == DIMS and "min_quality > max_quality" in _msg(a)
        # the target last; the Python wrapper checks it too, so the library is asked directly
        for bad in (float("nan"), -0.5, -math.inf):
            assert raw(a._format_byte(fmt), P, 0, 0, None, 8, 8, 2, 1, int(k), 64, bad, 10, 95, *outs, P, 1 << 20, sz.ctypes.data_as(u64),
                       None) == DIMS
            assert "min_psnr_db" in _msg(a)
            with pytest.raises(a.CodecError, match="min_psnr"):
                call(fmt, 8, 8, 2, 1, k, 64, bad, 10, 95)
        if a.device_count() < 1:
            for t in (0.0, 35.0, math.inf):
                assert _code(a, call, fmt, 8, 8, 2, 1, k, 64, t, 200, 120) == DEVICE   # both qualities act as 100
    assert _code(a, call, "reversible", 8, 8, 2, 1, k, 64, 30.0, 10, 95) == BITSTREAM
    assert (ch == 9).all() and (ok == 9).all() and (db == -3.0).all() and (sz == 7).all()


def test_encode_to_psnr_host_validates_in_order_without_a_device(codec):
    a = codec
    lib = a.load_library()
    rgb = np.zeros(4 * 4 * 2 * 3, np.uint8)
    u8, u64 = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
    ch = C.c_uint8(9); ok = C.c_uint8(9); db = C.c_double(-3.0); n = C.c_uint64(7)
    outs = (C.byref(ch), C.byref(ok), C.byref(db), C.byref(n))
    raw = lib.alice_codec_encode_to_psnr
    src = rgb.ctypes.data_as(u8)
    assert not raw(3, 0, src, rgb.size, 4, 4, 2, 0, 30.0, 10, 95, None, C.byref(ok), C.byref(db), C.byref(n))
    assert lib.alice_codec_last_error() == NULL_ARG
    assert not raw(3, 0, None, rgb.size, 4, 4, 2, 0, 30.0, 10, 95, *outs)
    assert lib.alice_codec_last_error() == NULL_ARG
    assert not raw(1, 9, src, rgb.size - 1, 4, 4, 2, 3, -1.0, 60, 50, *outs)
    assert lib.alice_codec_last_error() == BITSTREAM and "format byte" in _msg(a)
    assert not raw(4, 9, src, rgb.size - 1, 4, 4, 2, 3, -1.0, 60, 50, *outs)
    assert lib.alice_codec_last_error() == BITSTREAM and "no quality to search" in _msg(a)
    for fmt in (2, 3):
        steps = [((fmt, 9, src, rgb.size, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 3, -1.0, 60, 50), OVERFLOW, "overflow"),
                 ((fmt, 9, src, rgb.size - 1, 4, 4, 2, 3, -1.0, 60, 50), BUFFER, "buffer size"),
                 ((fmt, 9, src, rgb.size, 4, 4, 2, 3, -1.0, 60, 50), BITSTREAM, "wavelet"),
                 ((fmt, 1, src, rgb.size, 4, 4, 2, 3, -1.0, 60, 50), DIMS, "lane_symbols"),
                 ((fmt, 1, src, rgb.size, 4, 4, 2, 0, -1.0, 60, 50), DIMS, "min_quality > max_quality"),
                 ((fmt, 1, src, rgb.size, 4, 4, 2, 0, -1.0, 10, 95), DIMS, "min_psnr_db"),
                 ((fmt, 1, src, rgb.size, 4, 4, 2, 0, float("nan"), 10, 95), DIMS, "min_psnr_db")]
        for args, code, word in steps:
            assert not raw(*args, *outs)
            assert lib.alice_codec_last_error() == code and word in _msg(a), (args, _msg(a))
    assert (ch.value, ok.value, db.value, n.value) == (9, 9, -3.0, 7)
    # a chunk without pixels needs no device: nothing differs at any step
    for fn, info in ((a.encode_split_to_psnr, a.split_info), (a.encode_wide_to_psnr, a.wide_info)):
        data, q, reached, dbv = fn(np.zeros(0, np.uint8), 5, 0, 2, math.inf, a.WaveletType.Haar, 20, 150, 128)
        assert (q, reached, dbv, len(data)) == (20, True, math.inf, a.SPLIT_HEADER_BYTES)
        ci = info(data)
        assert (ci.width, ci.height, ci.frames, ci.lane_symbols) == (5, 0, 2, 128) and ci.quant_step == [Q.step_of(20)] * 3
        assert lib.alice_codec_test_last_quality_trials(None, 0) == 1
        t = np.zeros(1, np.uint32)
        lib.alice_codec_test_last_quality_trials(t.ctypes.data_as(C.POINTER(C.c_uint32)), 1)
        assert t[0] == 2
    with pytest.raises(ValueError):
        a.encode_wide_to_psnr(rgb, 4, 4, 2, 30.0, min_quality=-1)
    with pytest.raises(a.CodecError, match="min_psnr"):
        a.encode_split_to_psnr(rgb, 4, 4, 2, float("nan"))
    if a.device_count() < 1:
        assert _code(a, a.encode_wide_to_psnr, rgb, 4, 4, 2, 30.0) == DEVICE
        assert _code(a, a.encode_split_to_psnr, rgb, 4, 4, 2, math.inf) == DEVICE


def test_person_chunks_argument_rules(codec):
    a = codec
    for fmt in ("v1", "reversible"):
        with pytest.raises(a.CodecError, match="min_psnr"):
            a.encode_person_chunks(P, P, 8, 8, 2, 1, 80, format=fmt, min_psnr=30.0)
    with pytest.raises(a.CodecError, match="min_psnr"):
        a.encode_person_chunks(P, P, 8, 8, 2, 1, 80, min_psnr=30.0)              # the default format
    for fmt in ("split", "wide"):
        with pytest.raises(a.CodecError, match="min_psnr and max_bytes"):
            a.encode_person_chunks(P, P, 8, 8, 2, 1, 80, format=fmt, min_psnr=30.0, max_bytes=1000)
        with pytest.raises(a.CodecError, match="min_psnr"):
            a.encode_person_chunks(P, P, 8, 8, 2, 1, 80, format=fmt, min_psnr=float("nan"))
        with pytest.raises(a.CodecError) as e:                                   # accepted: the next refusal is the width's
            a.encode_person_chunks(P, P, 0, 8, 2, 1, 80, format=fmt, min_psnr=30.0)
        assert "min_psnr" not in str(e.value) and "format" not in str(e.value)


# ---- the kernel's case table against the classes its constants define ----
def test_constants_are_what_the_arithmetic_allows():
    assert QC.FLUSH % QC.VPL == 0 and QC.BLOCK % 64 == 0
    assert 16 * QC.MAX_TERM * QC.FLUSH < 1 << 32 <= 16 * QC.MAX_TERM * (QC.FLUSH + QC.VPL)


def test_case_table_covers_every_class():
    cases = QC.cases()
    assert len({c.name for c in cases}) == len(cases)
    seen = set()
    for c in cases:
        seen |= c.classes()
    want = {"flat", "rows", "flush:below", "flush:at", "flush:above", "run<window", "frame>vb", "grid-stride", "frames-per-workgroup>1",
            "pitches-differ", "frame>=2^32"}
    want |= {f"a%16={k}" for k in range(16)} | {f"b-a%16={k}" for k in range(16)} | {f"len%16={k}" for k in range(16)}
    assert want <= seen, sorted(want - seen)
    # both modes see every alignment of either side
    for mode in ("flat", "rows"):
        got = set()
        for c in cases:
            if mode in c.classes():
                got |= {x for x in c.classes() if x.startswith(("a%16", "b-a%16"))}
        assert len(got) == 32, (mode, sorted(got))
    by = {c.name: c for c in cases}
    # the fold under one workgroup: exactly at the limit, one virtual block before it, one window past it
    below, at, past = by["fold-limit-below"], by["fold-limit-at"], by["fold-limit-past"]
    assert (below.vb_per_frame(), at.vb_per_frame(), past.vb_per_frame()) == (QC.FLUSH_VB - 1, QC.FLUSH_VB, QC.FLUSH_VB + 1)
    assert at.vb_per_frame() < Case_vb(at.w + 1) and past.vb_per_frame() > Case_vb(past.w - 1)
    assert (past.off[0] + 3 * past.w + 15) // 16 == QC.FLUSH_VB * QC.PER_VB + 1          # the window past the limit exists
    # one whole virtual block past it: a lane that did not fold would hold FLUSH + VPL whole windows of maximal terms, too many
    whole = by["fold-limit-past-whole-block"]
    assert whole.vb_per_frame() == QC.FLUSH_VB + 1 and whole.off == (0, 0) and whole.content == "extreme" and whole.cap == 1
    assert 3 * whole.w // 16 >= (QC.FLUSH_VB + 1) * QC.PER_VB - QC.BLOCK          # whole windows: all but the last lanes' last
    assert 16 * QC.MAX_TERM * (QC.FLUSH + QC.VPL) >= 1 << 32
    mixed = by["stride-frames-and-segments"]
    assert mixed.vb_per_frame() == 3 and mixed.grid() == 7 and by["stride-frames-and-segments-rows"].vb_per_frame() >= 3
    big = [c for c in cases if c.name.startswith("fold-") and c.name.endswith("cap1") and "limit" not in c.name]
    assert big and all(3 * c.w * c.h > 66052 * QC.BLOCK and c.flush_class() == "above" and c.content == "extreme" for c in big)
    assert any(c.name.endswith("cap3") and c.cap == 3 for c in cases)
    # the shapes the issue names
    assert by["1x1x1"].run_len() == 3
    assert {3 * w % 16 for w in range(1, 18)} == set(range(16))
    assert by["300-frames"].n == 300 and by["frame-sum-2^32"].n == 2 and 3 * 160 * 140 * QC.MAX_TERM >= 1 << 32


def Case_vb(w):
    return QC.Case("probe", w, 1, 1).vb_per_frame()


def test_case_references_are_int64_numpy():
    c = next(x for x in QC.cases() if x.name == "300-frames")
    a, b, ref = c.build()
    assert list(ref) == list(range(1, 301))
    assert (a[:QC.GUARD] == 0).all() and (b[:QC.GUARD] == 255).all() and (a[-QC.GUARD:] == 0).all() and (b[-QC.GUARD:] == 255).all()
    c = next(x for x in QC.cases() if x.name == "frame-sum-2^32-rows")
    _, _, ref = c.build()
    assert list(ref) == [160 * 140 * 3 * QC.MAX_TERM] * 2 and int(ref[0]) >= 1 << 32


def test_either_band_plan_of_the_inverse_can_need_the_larger_slot(codec):
    """What a trial's scratch has to allow for: under one band target the i32 plan may cut a chunk that the i16 plan leaves
    whole, so the i16 slot (the whole frame) is the larger; with no cut at all the i32 slot is twice the i16 one."""
    lib = codec.load_library()
    try:
        lib.alice_codec_test_set_tuning(4096)
        i16, i32 = (int(lib.alice_codec_test_inverse_scratch_bytes(256, 256, 16, m)) for m in (1, 0))
        assert i16 >= 256 * 256 * 16 * 3 * 2 and i32 < i16 - (2 << 20)
    finally:
        lib.alice_codec_test_set_tuning(1024 * 1024)
    i16, i32 = (int(lib.alice_codec_test_inverse_scratch_bytes(256, 256, 16, m)) for m in (1, 0))
    assert i32 > i16 >= 256 * 256 * 16 * 3 * 2
    # the shapes at the default target where the i16 slot is the larger one
    for w, h, f in ((1920, 1080, 128), (1920, 1080, 96), (2560, 1440, 64), (3840, 2160, 32)):
        i16, i32 = (int(lib.alice_codec_test_inverse_scratch_bytes(w, h, f, m)) for m in (1, 0))
        assert i16 > i32 > 0, (w, h, f, i16, i32)
    assert lib.alice_codec_test_inverse_scratch_bytes(3, 40, 4, 1) == 0       # the generic path has no band slot
