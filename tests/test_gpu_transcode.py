"""Transcode of version 2, 3 and 4 chunks on the MI355X, bit for bit against tests/transcode_ref.py:
the stage call at every alignment, size and step pair; whole chunks of every version and wavelet; lanes and version byte
changed on the way; the device call with its refusals and its damage verdicts; the size brackets; the byte budgets.
The sources are the encoders' own containers, which must equal the references' (tests/transcode_cases.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle.alice_oracle_np as o  # noqa: E402
import reversible_ref as R4  # noqa: E402
import split_rate_ref as SR  # noqa: E402
import transcode_cases as TC  # noqa: E402
import transcode_ref as T  # noqa: E402
import wide_ref as W3  # noqa: E402

import torch  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64          # guard bytes on each side of a stage buffer
STEP_PAIRS = sorted({(s1, s2) for s1 in (1, 2, 3, 8, 13, 64) for s2 in (1, s1, s1 + 1, 2 * s1, 63, 64) if s2 <= 64})
SIZES = [1, 15, 16, 17, 63, 64, 65, 2047, 2048, 2049, 4095, 4096, 4097]     # a workgroup trip is 256 vectors: 4096 u8, 2048 u16


def _symbols(n: int, wide: bool, shift: int = 0) -> np.ndarray:
    """n symbols that hold every u8 value (every z in 0..4350 for wide) as soon as n allows, in an order that is no ramp"""
    period = 4351 if wide else 256
    i = np.arange(n, dtype=np.int64)
    return ((i * 2477 + shift) % period).astype(np.uint16 if wide else np.uint8)


def _stage(a, sym: np.ndarray, wide: bool, s1: int, s2: int, src_off: int, dst_off, hist0: int = 0):
    """One stage call on guarded device buffers; dst_off None: in place.  Checks symbols, histogram and guards."""
    e = 2 if wide else 1
    raw = sym.view(np.uint8)
    cap = GUARD + 32 + raw.size + GUARD
    src = torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda:0")
    src[GUARD + src_off:GUARD + src_off + raw.size] = torch.from_numpy(raw.copy()).to("cuda:0")
    dst = src if dst_off is None else torch.full((cap,), 0x5A, dtype=torch.uint8, device="cuda:0")
    d_off = src_off if dst_off is None else dst_off
    hist = torch.full((256,), hist0, dtype=torch.int32, device="cuda:0")
    before = src.cpu().numpy().copy()
    a.requant_symbols_device(src.data_ptr() + GUARD + src_off, dst.data_ptr() + GUARD + d_off, sym.size, wide, s1, s2, hist.data_ptr())
    want = T.requant(sym, s1, s2, wide)
    got = dst.cpu().numpy()
    body = got[GUARD + d_off:GUARD + d_off + raw.size].view(sym.dtype)
    tag = (sym.size, wide, s1, s2, src_off, dst_off)
    assert np.array_equal(body, want), tag
    fill = 0xA5 if dst_off is None else 0x5A
    assert (got[:GUARD + d_off] == fill).all() and (got[GUARD + d_off + raw.size:] == fill).all(), tag
    if dst_off is not None:
        assert np.array_equal(src.cpu().numpy(), before), tag                 # the source is only read
    coded = np.minimum(want.astype(np.int64), 255)
    assert np.array_equal(hist.cpu().numpy().view(np.uint32) - hist0, np.bincount(coded, minlength=256)), tag
    assert e * sym.size == raw.size


def test_stage_call_sizes_alignments_and_modes(gpu_codec):
    k = 0
    for wide in (False, True):
        offsets = (0, 2) if wide else (0, 1, 2, 3)
        for n in SIZES:
            for off in offsets:
                for dst_off in (None, off, (off + 16) % 32):             # in place; the same offset in 16 bytes (vectors)
                    s1, s2 = STEP_PAIRS[k % len(STEP_PAIRS)]
                    k += 1
                    _stage(gpu_codec, _symbols(n, wide, k), wide, s1, s2, off, dst_off)
        # source and destination at different offsets inside 16 bytes: every element takes the element path
        for off, dst_off in (((0, 2), (2, 0), (6, 12)) if wide else ((0, 1), (3, 0), (5, 9))):
            _stage(gpu_codec, _symbols(4097, wide), wide, 3, 8, off, dst_off)


@pytest.mark.parametrize("wide", [False, True])
def test_stage_call_every_step_pair_on_every_symbol(gpu_codec, wide):
    sym = _symbols(2 * 4351 + 3, wide)
    assert np.unique(sym).size == (4351 if wide else 256)
    for i, (s1, s2) in enumerate(STEP_PAIRS):
        _stage(gpu_codec, sym, wide, s1, s2, (i % 2) * 2, None if i % 3 else 2, hist0=7 * (i % 2))   # the histogram is added to
    big = np.arange(65536 - 9000, 65536).astype(np.uint16) if wide else sym
    _stage(gpu_codec, big, wide, 64, 64, 0, None)
    if wide:
        _stage(gpu_codec, big, True, 13, 64, 2, 0)                                                  # any u16, not only z <= 4350


@pytest.mark.parametrize("cap", [1, 3])
def test_stage_call_grid_stride_wraps(gpu_codec, cap):
    lib = gpu_codec.load_library()
    try:
        lib.alice_codec_test_set_grid_cap(cap)
        for wide in (False, True):
            n = (cap * 3 + 1) * (2048 if wide else 4096) + 37             # several trips of every workgroup, a ragged last one
            _stage(gpu_codec, _symbols(n, wide), wide, 2, 3, 2, None)
            _stage(gpu_codec, _symbols(n, wide, 5), wide, 8, 64, 2, 6)    # element path: n elements over cap workgroups
    finally:
        lib.alice_codec_test_set_grid_cap(0)


# ---- whole chunks ----

def _encode(a, version, w, h, f, kind, quality, L=64):
    enc = a.FrameEncoder.with_wavelet(quality, a.WaveletType(kind))
    fn = {2: a.encode_split, 3: a.encode_wide, 4: a.encode_reversible}[version]
    return fn(enc, TC.clip(w, h, f), w, h, f, L)


def _ref_pixels(blob: bytes, w, h, f) -> np.ndarray:
    """the pixels of a container from transcode_ref's symbols: the reference inverse (mirrored for version 4) with every
    channel's own step"""
    v, info, syms = T._decoded(blob)
    if w * h * f == 0:
        return np.zeros(0, np.uint8)
    qs = [T.coefficient(s) for s in syms]
    pw, ph, pf = W3.padded_dims(w, h, f)
    if v == 4:
        return R4.inverse_quantised(qs, info["step"], (pw, ph, pf), w, h, f, info["wavelet"])
    chans = []
    for q, step in zip(qs, info["step"]):
        vol = o.wavelet3d(info["wavelet"], o._wrap32(q * int(step)), pw, ph, pf, inverse=True).reshape(pf, ph, pw)
        chans.append(o._wrap16(vol[:f, :h, :w].reshape(-1)))
    return o.ycocg_r_to_rgb(*chans)


@pytest.mark.parametrize("name", list(TC.SHAPES))
def test_whole_chunks_match_the_reference(gpu_codec, name):
    a = gpu_codec
    w, h, f = TC.SHAPES[name]
    for version in (2, 3, 4):
        for kind in (0, 1, 2):
            for qs, qt in TC.PAIRS:
                src = _encode(a, version, w, h, f, kind, qs)
                assert src == TC.source(version, w, h, f, kind, qs), (version, kind, qs)
                got = a.transcode(src, qt)
                assert got == T.transcode(src, qt), (version, kind, qs, qt)
                assert got != src
                if name in ("padding_on_every_axis", "one_block_and_a_bit"):
                    assert np.array_equal(a.decode_alc(got), _ref_pixels(got, w, h, f)), (version, kind, qs, qt)
            for qs, qt in TC.SAME:
                src = _encode(a, version, w, h, f, kind, qs)
                assert a.transcode(src, qt) == src, (version, kind, qs, qt)


@pytest.mark.parametrize("version", [2, 3, 4])
def test_lanes_and_version_byte_change_on_the_way(gpu_codec, version):
    a = gpu_codec
    w, h, f = TC.SHAPES["several_blocks"]
    src = _encode(a, version, w, h, f, 1, 95)
    for q in (95, 60):
        got = a.transcode(src, q, 128)
        assert got == T.transcode(src, q, 128) and int.from_bytes(got[18:22], "little") == 128
        assert a.transcode(got, q, 64) == a.transcode(src, q)
        assert np.array_equal(a.decode_alc(got), a.decode_alc(a.transcode(src, q)))
    if version >= 3:
        other = 7 - version
        got = a.transcode(src, 60, 0, other)
        assert got == T.transcode(src, 60, 0, other) and got[4] == other
        assert got == R4.with_version(a.transcode(src, 60), other)
        assert a.transcode(src, 99, 0, other) == R4.with_version(src, other)       # untouched channels, another inverse
        assert np.array_equal(a.decode_alc(got), _ref_pixels(got, w, h, f))


def test_a_step_one_source_gives_the_direct_encode(gpu_codec):
    a = gpu_codec
    w, h, f = TC.SHAPES["padding_on_every_axis"]
    for kind in (0, 1):
        src = _encode(a, 3, w, h, f, kind, 100)
        for q in (0, 50, 80, 99):
            assert a.transcode(src, q) == _encode(a, 3, w, h, f, kind, q), (kind, q)
            assert a.transcode(src, q, 0, 4) == _encode(a, 4, w, h, f, kind, q), (kind, q)


@pytest.mark.parametrize("version", [2, 3, 4])
def test_per_channel_steps_one_mapped_one_at_the_boundary_one_kept(gpu_codec, version):
    a = gpu_codec
    src = TC.mixed_source(version)
    q9 = next(q for q in range(101) if SR.quality_to_step(q) == 9)
    got = a.transcode(src, q9)
    assert got == T.transcode(src, q9)
    info = {2: a.split_info, 3: a.wide_info, 4: a.reversible_info}[version](got)
    assert list(info.quant_step) == [9, 9, 20] and list(info.dead_zone) == [9, 9, 20]
    w, h, f = TC.SHAPES["padding_on_every_axis"]
    assert np.array_equal(a.decode_alc(got), _ref_pixels(got, w, h, f))
    assert a.transcode(src, 100) == src


def _device_call(a, blobs, qualities, stride, fill=0xCD, out_stride=None, **kw):
    """blobs at `stride` on the device -> (host copy of the guarded output, sizes)"""
    n = len(blobs)
    out_stride = stride if out_stride is None else out_stride
    inp = np.zeros(n * stride, np.uint8)
    for i, b in enumerate(blobs):
        inp[i * stride:i * stride + len(b)] = np.frombuffer(b, np.uint8)
    d_in = torch.from_numpy(inp).to("cuda:0")
    d_out = torch.full((n * out_stride + 256,), fill, dtype=torch.uint8, device="cuda:0")
    sizes = a.transcode_device(d_in.data_ptr(), stride, [len(b) for b in blobs], 0, d_out.data_ptr(), out_stride, qualities, **kw)
    return d_out.cpu().numpy(), sizes


@pytest.mark.parametrize("version", [2, 3, 4])
def test_device_call_three_chunks_three_qualities_and_refusals(gpu_codec, version):
    a = gpu_codec
    w, h, f = TC.SHAPES["one_block_and_a_bit"]
    srcs = [_encode(a, version, w, h, f, 0, q) for q in (100 if version > 2 else 95, 90, 80)]
    qualities = [70, 95, 20]                                                 # one mapped, one untouched, one mapped far
    stride = (max(len(s) for s in srcs) + 255) & ~255
    host, sizes = _device_call(a, srcs, qualities, stride)
    assert (host[3 * stride:] == 0xCD).all()
    for i in range(3):
        want = T.transcode(srcs[i], qualities[i])
        assert int(sizes[i]) == len(want)
        assert host[i * stride:i * stride + len(want)].tobytes() == want, i
        assert (host[i * stride + len(want):(i + 1) * stride] == 0xCD).all()
    assert T.transcode(srcs[1], 95) == srcs[1]

    def refused(blobs, code):
        with pytest.raises(a.CodecError) as e:
            _device_call(a, blobs, [50] * len(blobs), stride)
        assert e.value.code == code, str(e.value)

    # mismatched shape, wavelet, lanes or version: refused before anything is queued
    w2, h2, f2 = TC.SHAPES["one_block"]
    refused([srcs[0], _encode(a, version, w2, h2, f2, 0, 90)], 2)
    refused([srcs[0], _encode(a, version, w, h, f, 1, 90)], 2)
    refused([srcs[0], _encode(a, version, w, h, f, 0, 90, 128)], 2)
    refused([srcs[0], _encode(a, {2: 3, 3: 4, 4: 3}[version], w, h, f, 0, 90)], 2)
    refused([o.encode(TC.clip(w, h, f), w, h, f, 90, 0)], 4)                 # version 1

    # out_stride one byte short of the larger chunk: nothing of the group is written
    want = [T.transcode(s, 50) for s in srcs[:2]]
    short = max(len(x) for x in want) - 1
    inp_stride = stride
    n = 2
    inp = np.zeros(n * inp_stride, np.uint8)
    for i, b in enumerate(srcs[:2]):
        inp[i * inp_stride:i * inp_stride + len(b)] = np.frombuffer(b, np.uint8)
    d_in = torch.from_numpy(inp).to("cuda:0")
    d_out = torch.full((n * short + 256,), 0xEE, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(a.CodecError) as e:
        a.transcode_device(d_in.data_ptr(), inp_stride, [len(b) for b in srcs[:2]], 50, d_out.data_ptr(), short)
    assert e.value.code == 1 and (d_out.cpu().numpy() == 0xEE).all()
    sizes = a.transcode_device(d_in.data_ptr(), inp_stride, [len(b) for b in srcs[:2]], 50, d_out.data_ptr(), short + 1)
    assert [int(s) for s in sizes] == [len(x) for x in want]

    # damage: a flipped byte in a lane stream, a wrong block length -> InvalidBitstream, nothing written
    info = T._decoded(srcs[0])[1]
    flipped = bytearray(srcs[0]); flipped[T.HEADER + 4 * info["n_blocks"][0] + 128 + 9] ^= 0x40
    wrong_len = bytearray(srcs[0]); wrong_len[T.HEADER] ^= 0x01
    for bad in (bytes(flipped), bytes(wrong_len)):
        inp = np.zeros(2 * stride, np.uint8)
        for i, b in enumerate((srcs[1], bad)):
            inp[i * stride:i * stride + len(b)] = np.frombuffer(b, np.uint8)
        d_in = torch.from_numpy(inp).to("cuda:0")
        d_out = torch.full((2 * stride,), 0xEE, dtype=torch.uint8, device="cuda:0")
        with pytest.raises(a.CodecError) as e:
            a.transcode_device(d_in.data_ptr(), stride, [len(srcs[1]), len(bad)], 50, d_out.data_ptr(), stride)
        assert e.value.code == 4 and (d_out.cpu().numpy() == 0xEE).all()
        with pytest.raises(a.CodecError) as e:
            a.transcode(bad, 50)
        assert e.value.code == 4


# ---- prediction and budgets ----

def _budget_sources(a):
    w, h, f = TC.SHAPES[TC.BUDGET_SHAPE]
    out = []
    for version, quality in ((2, 95), (3, 100)):
        src = _encode(a, version, w, h, f, 0, quality)
        assert src == TC.source(version, w, h, f, 0, quality)
        out.append((version, src))
    return out


def test_brackets_are_the_references_and_hold_at_every_step(gpu_codec):
    a = gpu_codec
    q_of = {}
    for q in range(101):
        q_of.setdefault(SR.quality_to_step(q), q)
    sources = _budget_sources(a) + [(v, TC.mixed_source(v)) for v in (2, 3, 4)]
    for version, src in sources:
        lo, hi = T.predict(src)
        p = a.predict_transcode_sizes(src)
        assert np.array_equal(p.lo, lo) and np.array_equal(p.hi, hi), version
        for step in range(1, 65):
            q = q_of[step]
            size = len(a.transcode(src, q))
            assert int(lo[q]) <= size <= int(hi[q]), (version, step, int(lo[q]), size, int(hi[q]))
        lo128, hi128 = T.predict(src, 128)
        p = a.predict_transcode_sizes(src, 128)
        assert np.array_equal(p.lo, lo128) and np.array_equal(p.hi, hi128), version
    lib = a.load_library()
    try:
        lib.alice_codec_test_set_value_table_radius(24)      # values outside [-24, 24): the rows come from real maps
        for version, src in sources[:3]:
            lo, hi = T.predict(src)
            p = a.predict_transcode_sizes(src)
            assert np.array_equal(p.lo, lo) and np.array_equal(p.hi, hi), version
    finally:
        lib.alice_codec_test_set_value_table_radius(2048)


def _trials(a, n):
    out = np.zeros(max(n, 1), np.uint32)
    assert a.load_library().alice_codec_test_last_split_trials(out.ctypes.data_as(C.POINTER(C.c_uint32)), n) == n
    return [int(v) for v in out[:n]]


def test_budget_transcodes_follow_the_reference_chooser(gpu_codec):
    a = gpu_codec
    lo_q, hi_q = TC.BUDGET_RANGE
    for version, src in _budget_sources(a):
        budgets = TC.budgets(lambda q: len(T.transcode(src, q)))
        want = [T.choose_transcode(src, b, lo_q, hi_q) for b in budgets]
        assert want[0][1] and not want[2][1] and want[2][0] == lo_q and want[3][:2] == (hi_q, True)
        for b, (q, fits, trials, data) in zip(budgets, want):
            got, gq, gfits = a.transcode_to_size(src, b, lo_q, hi_q)
            print(f"v{version} budget {b}: chose {gq} fits {gfits} size {len(got)} trials {_trials(a, 1)} (reference {q} {fits} {trials})")
            assert (gq, gfits) == (q, fits) and _trials(a, 1) == [trials] and trials <= SR.REFINE_TRIALS
            assert got == data == a.transcode(src, q)
            if fits:
                assert len(got) <= b
        # the four budgets in one device call
        stride = (len(src) + 255) & ~255
        d_in = torch.from_numpy(np.tile(np.pad(np.frombuffer(src, np.uint8), (0, stride - len(src))), 4)).to("cuda:0")
        d_out = torch.full((4 * stride + 256,), 0xCD, dtype=torch.uint8, device="cuda:0")
        chosen, fits, sizes = a.transcode_to_budget_device(d_in.data_ptr(), stride, [len(src)] * 4, budgets, d_out.data_ptr(), stride, lo_q, hi_q)
        host = d_out.cpu().numpy()
        assert (host[4 * stride:] == 0xCD).all()
        assert _trials(a, 4) == [t for _, _, t, _ in want]
        for i, (q, fit, _, data) in enumerate(want):
            assert (int(chosen[i]), bool(fits[i]), int(sizes[i])) == (q, fit, len(data))
            assert host[i * stride:i * stride + len(data)].tobytes() == data
            assert (host[i * stride + len(data):(i + 1) * stride] == 0xCD).all()
    # a version 4 result has no budget; through out_version = 3 it has
    w, h, f = TC.SHAPES[TC.BUDGET_SHAPE]
    v4 = _encode(a, 4, w, h, f, 0, 100)
    with pytest.raises(a.CodecError) as e:
        a.transcode_to_size(v4, 10 ** 6, lo_q, hi_q)
    assert e.value.code == 4
    want = T.choose_transcode(v4, 4000, lo_q, hi_q, 0, 3)
    got, gq, gfits = a.transcode_to_size(v4, 4000, lo_q, hi_q, 0, 3)
    assert (got, gq, gfits) == (want[3], want[0], want[1]) and got[4] == 3


@pytest.mark.parametrize("wide", [False, True])
def test_bins_kernel_counts_the_value_the_map_quantises(gpu_codec, wide):
    """symbol_bins_kernel through its test hook: every size class and alignment of the stage call, bins and counter added to"""
    lib = gpu_codec.load_library()
    e = 2 if wide else 1
    for k, n in enumerate(SIZES + [2 * 4351 + 3, 5 * 4096 + 37]):
        s1 = (1, 2, 3, 8, 13, 64)[k % 6]
        off = (k % (2 if wide else 4)) * e
        sym = _symbols(n, wide, k)
        buf = torch.zeros(GUARD + sym.nbytes + GUARD, dtype=torch.uint8, device="cuda:0")
        buf[GUARD + off:GUARD + off + sym.nbytes] = torch.from_numpy(sym.view(np.uint8).copy()).to("cuda:0")
        bins = torch.full((4096,), 3, dtype=torch.int32, device="cuda:0")
        oor = torch.full((1,), 5, dtype=torch.int32, device="cuda:0")
        assert lib.alice_codec_test_symbol_bins(buf.data_ptr() + GUARD + off, n, int(wide), s1, bins.data_ptr(), oor.data_ptr(), None) == 0
        m = T.centre(sym, s1)
        inside = (m >= -2048) & (m < 2048)
        want = np.bincount(m[inside] + 2048, minlength=4096)
        assert np.array_equal(bins.cpu().numpy().view(np.uint32) - 3, want), (n, s1, off)
        assert int(oor.cpu().numpy().view(np.uint32)[0]) - 5 == int((~inside).sum()), (n, s1, off)
