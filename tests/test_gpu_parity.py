"""Parity tests proper: the HIP path, called through the C ABI, against the CPU oracle on the
same seeded inputs, against the committed golden fixtures, and -- at BASELINE.json's full
1920x1080x64 size -- byte for byte against the oracle plus size-independent properties.
Bar: bit-exact (integer / byte work).  Run with `-m gpu` on an MI355X."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from conftest import golden_cases

pytestmark = pytest.mark.gpu

WT = {0: "cdf53", 1: "cdf97", 2: "haar"}


def smooth_rgb(w, h, f, seed=1234, shift=0):
    """S-smooth synthetic input: moving sinusoid + integer noise in [-4, 4]."""
    rng = np.random.default_rng(seed)
    t, y, x = np.meshgrid(np.arange(f, dtype=np.float32), np.arange(h, dtype=np.float32),
                          np.arange(w, dtype=np.float32), indexing="ij")
    out = np.empty((f, h, w, 3), np.float32)
    for c, (s, ph) in enumerate(((23, 0), (31, 1), (17, 2))):
        out[..., c] = 128 + 90 * np.sin((x + 2 * t + shift) / s + ph) * np.cos((y - t) / (0.7 * s))
    out += rng.integers(-4, 5, out.shape, dtype=np.int8)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8).reshape(-1)


def first_diff(a: bytes, b: bytes):
    x = np.frombuffer(a, np.uint8); y = np.frombuffer(b, np.uint8)
    m = min(x.size, y.size)
    d = np.nonzero(x[:m] != y[:m])[0]
    return (len(a), len(b), int(d[0]) if d.size else None)


# ---- golden fixtures --------------------------------------------------------------------------

@pytest.mark.parametrize("path", golden_cases(), ids=lambda p: p.split("/")[-1][:-4])
def test_golden(gpu_codec, path):
    g = np.load(path)
    w, h, f, q, k = (int(g[n]) for n in ("w", "h", "f", "quality", "wavelet"))
    chunk = gpu_codec.FrameEncoder.with_wavelet(q, gpu_codec.WaveletType(k)).encode(g["rgb"], w, h, f)
    assert chunk.to_bytes() == g["alc"].tobytes(), first_diff(chunk.to_bytes(), g["alc"].tobytes())
    assert np.array_equal(gpu_codec.FrameDecoder().decode(chunk), g["decoded"])
    restored = gpu_codec.EncodedChunk.from_bytes(g["alc"].tobytes())
    assert np.array_equal(gpu_codec.FrameDecoder().decode(restored), g["decoded"])


# ---- pipeline vs oracle on seeded inputs ----------------------------------------------------------

SHAPES = [
    # w, h, f, quality, wavelet
    (4, 4, 2, 80, 0), (4, 4, 2, 90, 1), (4, 4, 1, 90, 0), (3, 4, 2, 90, 0), (4, 5, 2, 90, 0), (3, 5, 1, 90, 0),
    (1, 1, 1, 100, 0), (2, 2, 2, 0, 2), (8, 8, 2, 100, 2), (64, 64, 8, 100, 2), (5, 3, 7, 10, 1),
    (66, 34, 4, 50, 1), (130, 70, 3, 75, 1), (63, 33, 9, 85, 0), (128, 64, 17, 95, 2), (200, 100, 33, 90, 0),
    (256, 128, 64, 80, 1), (320, 180, 64, 80, 0), (1, 300, 4, 80, 1), (300, 1, 4, 80, 1), (17, 9, 63, 60, 1),
]


@pytest.mark.parametrize("w,h,f,q,k", SHAPES, ids=lambda v: str(v))
def test_encode_decode_matches_oracle(gpu_codec, oracle_mod, w, h, f, q, k):
    rng = np.random.default_rng(w * 7919 + h * 31 + f)
    inputs = {
        "grad": oracle_mod.make_gradient(w, h, f),
        "noise": rng.integers(0, 256, w * h * f * 3, dtype=np.uint8),
        "smooth": smooth_rgb(w, h, f),
    }
    enc = gpu_codec.FrameEncoder.with_wavelet(q, gpu_codec.WaveletType(k))
    for name, rgb in inputs.items():
        ref = oracle_mod.encode(rgb, w, h, f, q, k)
        chunk = enc.encode(rgb, w, h, f)
        got = chunk.to_bytes()
        assert got == ref, (name, first_diff(got, ref))
        assert (chunk.width, chunk.height, chunk.frames, int(chunk.wavelet_type)) == (w, h, f, k)
        dec = gpu_codec.FrameDecoder().decode(chunk)
        assert np.array_equal(dec, oracle_mod.decode(ref)), name


def test_more_than_64_frames(gpu_codec, oracle_mod):
    """The reference CLI encodes a whole file as one chunk (src/bin/main.rs:117-122): any frame count."""
    for w, h, f, q, k in ((20, 12, 66, 80, 1), (16, 16, 131, 90, 0)):
        rgb = smooth_rgb(w, h, f, seed=5)
        ref = oracle_mod.encode(rgb, w, h, f, q, k)
        chunk = gpu_codec.FrameEncoder.with_wavelet(q, gpu_codec.WaveletType(k)).encode(rgb, w, h, f)
        assert chunk.to_bytes() == ref
        assert np.array_equal(gpu_codec.FrameDecoder().decode(chunk), oracle_mod.decode(ref))


@pytest.mark.parametrize("k", [0, 1])
def test_every_frame_count_through_the_streaming_temporal_pass(gpu_codec, oracle_mod, k):
    """The temporal kernels run pairs in blocks of four with peeled first/last blocks: cover every residue and
    every short length (f = 1 pads to 2; odd f pads by one frame)."""
    w, h, q = 12, 10, 85
    enc = gpu_codec.FrameEncoder.with_wavelet(q, gpu_codec.WaveletType(k))
    for f in list(range(1, 28)) + [31, 32, 33, 34, 35, 40, 41]:
        rgb = np.random.default_rng(1000 + f).integers(0, 256, w * h * f * 3, dtype=np.uint8)
        ref = oracle_mod.encode(rgb, w, h, f, q, k)
        chunk = enc.encode(rgb, w, h, f)
        assert chunk.to_bytes() == ref, (f, first_diff(chunk.to_bytes(), ref))
        assert np.array_equal(gpu_codec.FrameDecoder().decode(chunk), oracle_mod.decode(ref)), f


def test_seeded_random_shapes(gpu_codec, oracle_mod):
    """150 seeded random (shape, quality, wavelet, content) cases against the oracle: tile borders, odd sizes,
    shapes below the tile kernels' minimum (generic path), every content class."""
    rng = np.random.default_rng(20260)
    for case in range(150):
        if case < 120:
            w = int(rng.integers(1, 160)); h = int(rng.integers(1, 110)); f = int(rng.integers(1, 20))
        else:   # several tiles in both directions, interior and border instances
            w = int(rng.integers(260, 700)); h = int(rng.integers(90, 420)); f = int(rng.integers(2, 12))
        q = int(rng.integers(0, 101)); k = int(rng.integers(0, 3))
        kind = case % 4
        if kind == 0:
            rgb = rng.integers(0, 256, w * h * f * 3, dtype=np.uint8)
        elif kind == 1:
            rgb = smooth_rgb(w, h, f, seed=case)
        elif kind == 2:
            rgb = oracle_mod.make_gradient(w, h, f)
        else:
            rgb = np.full(w * h * f * 3, int(rng.integers(0, 256)), dtype=np.uint8)
        ref = oracle_mod.encode(rgb, w, h, f, q, k)
        chunk = gpu_codec.FrameEncoder.with_wavelet(q, gpu_codec.WaveletType(k)).encode(rgb, w, h, f)
        got = chunk.to_bytes()
        assert got == ref, (case, w, h, f, q, k, first_diff(got, ref))
        assert np.array_equal(gpu_codec.FrameDecoder().decode(chunk), oracle_mod.decode(ref)), (case, w, h, f, q, k)


def test_empty_chunk(gpu_codec):  # src/pipeline.rs:738-743, 764-769
    c = gpu_codec.FrameEncoder(50).encode(np.zeros(0, np.uint8), 0, 0, 0)
    assert c.compressed_size() == 0 and gpu_codec.FrameDecoder().decode(c).size == 0
    r = gpu_codec.EncodedChunk.from_bytes(c.to_bytes())
    assert r.compressed_size() == 0


def test_quality_sweep(gpu_codec, oracle_mod):
    """Every quantiser step 1..64 (quality 0..100, src/pipeline.rs:456-457) on one input."""
    w, h, f = 48, 32, 8
    rgb = smooth_rgb(w, h, f, seed=9)
    for q in list(range(0, 101, 3)) + [100, 255]:
        for k in (0, 1):
            ref = oracle_mod.encode(rgb, w, h, f, q, k)
            assert gpu_codec.FrameEncoder.with_wavelet(q, gpu_codec.WaveletType(k)).encode(rgb, w, h, f).to_bytes() == ref, (q, k)


def test_decoder_follows_desynchronised_streams(gpu_codec, oracle_mod):
    """The reference's table construction makes its decoder desynchronise on most content
    (SURVEY.md fact 3): decode parity means reproducing that exact symbol sequence.  Also feeds
    corrupted payloads, truncated/short streams and foreign quantiser steps."""
    w, h, f = 64, 48, 16
    rgb = np.random.default_rng(4).integers(0, 256, w * h * f * 3, dtype=np.uint8)
    alc = bytearray(oracle_mod.encode(rgb, w, h, f, 100, 1))
    ref = oracle_mod.decode(bytes(alc))
    assert oracle_mod.psnr(rgb, ref) < 15.0  # garbage, as the reference would produce
    assert np.array_equal(gpu_codec.FrameDecoder().decode(gpu_codec.EncodedChunk.from_bytes(bytes(alc))), ref)
    rng = np.random.default_rng(5)
    for trial in range(6):
        bad = bytearray(alc)
        for _ in range(20):
            bad[3138 + int(rng.integers(0, len(bad) - 3138))] = int(rng.integers(0, 256))
        if trial >= 3:  # foreign steps / dead zones in the headers (i32 fields, src/pipeline.rs:279-284)
            for c in range(3):
                step = int(rng.choice([1, 3, 64, 1000, -7, 2**20, 2**31 - 1, -2**31]))
                bad[18 + 1040 * c + 4: 18 + 1040 * c + 8] = (step & 0xFFFFFFFF).to_bytes(4, "little")
        ref = oracle_mod.decode(bytes(bad))
        got = gpu_codec.FrameDecoder().decode(gpu_codec.EncodedChunk.from_bytes(bytes(bad)))
        assert np.array_equal(got, ref), trial


def test_stream_capacity_overflow_is_retried(gpu_codec, oracle_mod):
    """Stream regions are sized from the histograms; if a chain ever outgrew its region the kernels must not
    touch memory outside it and the host must encode again with the worst-case capacity.  The test hook shrinks
    the first capacity to 4352 bytes so that path runs."""
    w, h, f = 96, 64, 16
    rgb = np.random.default_rng(21).integers(0, 256, w * h * f * 3, dtype=np.uint8)
    ref = oracle_mod.encode(rgb, w, h, f, 90, 1)
    assert len(ref) > 3138 + 3 * 4352
    lib = gpu_codec.load_library()
    lib.alice_codec_test_force_first_cap(4352)
    try:
        got = gpu_codec.FrameEncoder.with_wavelet(90, gpu_codec.WaveletType.Cdf97).encode(rgb, w, h, f).to_bytes()
    finally:
        lib.alice_codec_test_force_first_cap(0)
    assert got == ref


def test_decode_validation_errors(gpu_codec, oracle_mod):  # src/pipeline.rs:566-576
    alc = bytearray(oracle_mod.encode(oracle_mod.make_gradient(4, 4, 2), 4, 4, 2, 80))
    bad = bytearray(alc); bad[18 + 12: 18 + 16] = (31).to_bytes(4, "little")  # num_symbols != padded
    with pytest.raises(gpu_codec.CodecError) as e:
        gpu_codec.FrameDecoder().decode(gpu_codec.EncodedChunk.from_bytes(bytes(bad)))
    assert e.value.kind == "InvalidBitstream"
    with pytest.raises(oracle_mod.OracleError):
        oracle_mod.decode(bytes(bad))


# ---- stage level vs oracle ----------------------------------------------------------------------------

def test_ffi_wavelet1d(gpu_codec, oracle_mod):  # src/ffi.rs:325-342 + odd lengths / i32 extremes
    rng = np.random.default_rng(11)
    for kind, ok in ((gpu_codec.WaveletType.Cdf53, oracle_mod.CDF53), (gpu_codec.WaveletType.Cdf97, oracle_mod.CDF97),
                     (gpu_codec.WaveletType.Haar, oracle_mod.HAAR)):
        wv = gpu_codec.Wavelet1D(kind)
        for n in (1, 2, 3, 5, 8, 64, 1023, 4096, 100001):
            s = rng.integers(-500, 500, n).astype(np.int32)
            fwd = wv.forward(s)
            assert np.array_equal(fwd, oracle_mod.wavelet1d(ok, s)), (kind, n)
            assert np.array_equal(wv.inverse(fwd), oracle_mod.wavelet1d(ok, fwd, inverse=True)), (kind, n)
        big = rng.integers(-2**31, 2**31 - 1, 257, dtype=np.int64).astype(np.int32)  # wrapping sums, 64-bit products
        assert np.array_equal(wv.forward(big), oracle_mod.wavelet1d(ok, big))
        assert np.array_equal(wv.inverse(big), oracle_mod.wavelet1d(ok, big, inverse=True))
    s = [10, 20, 30, 40, 50, 60, 70, 80]
    w53 = gpu_codec.Wavelet1D.cdf53()
    assert list(w53.inverse(w53.forward(s))) == s


def test_wavelet2d_3d(gpu_codec, oracle_mod):
    rng = np.random.default_rng(12)
    for k in (0, 1, 2):
        for (w, h) in ((2, 2), (8, 8), (5, 7), (64, 33)):
            img = rng.integers(-1000, 1000, w * h).astype(np.int32)
            f = gpu_codec.Wavelet2D(gpu_codec.WaveletType(k)).forward(img, w, h)
            assert np.array_equal(f, oracle_mod.wavelet2d(k, img, w, h))
            assert np.array_equal(gpu_codec.Wavelet2D(gpu_codec.WaveletType(k)).inverse(f, w, h), oracle_mod.wavelet2d(k, f, w, h, inverse=True))
        for (w, h, d) in ((2, 2, 2), (4, 4, 4), (32, 32, 8), (7, 5, 3), (16, 9, 70)):
            vol = rng.integers(-1000, 1000, w * h * d).astype(np.int32)
            f = gpu_codec.Wavelet3D(gpu_codec.WaveletType(k)).forward(vol, w, h, d)
            assert np.array_equal(f, oracle_mod.wavelet3d(k, vol, w, h, d))
            assert np.array_equal(gpu_codec.Wavelet3D(gpu_codec.WaveletType(k)).inverse(f, w, h, d), oracle_mod.wavelet3d(k, f, w, h, d, inverse=True))


def test_stage_wavelets_on_tile_kernels(gpu_codec, oracle_mod):
    """Wavelet2D / Wavelet3D of caller-shaped i32 data through the tile kernels' exact instances (even width and height
    >= 6, even depth): any i32 values incl. the extremes (wrapping sums, 64-bit products, src/wavelet.rs:193-194), tiles
    that overhang the image, volumes whose plane count is not a multiple of the three planes a workgroup takes; and the
    device-pointer entry points alice_codec_dev_wavelet3d_*."""
    import torch
    rng = np.random.default_rng(1212)
    lib = gpu_codec.load_library()

    def values(n, kind):
        if kind == 0:
            return rng.integers(-1000, 1000, n).astype(np.int32)
        v = rng.integers(-2**31, 2**31, n, dtype=np.int64).astype(np.int32)
        v[:: 97] = 2**31 - 1
        v[5:: 89] = -2**31
        return v

    for k in (0, 1, 2):
        for (w, h) in ((6, 6), (8, 6), (130, 42), (256, 96), (98, 34), (1920, 1080)):
            img = values(w * h, k & 1)
            f = gpu_codec.Wavelet2D(gpu_codec.WaveletType(k)).forward(img, w, h)
            assert np.array_equal(f, oracle_mod.wavelet2d(k, img, w, h)), (k, w, h)
            assert np.array_equal(gpu_codec.Wavelet2D(gpu_codec.WaveletType(k)).inverse(f, w, h), oracle_mod.wavelet2d(k, f, w, h, inverse=True)), (k, w, h)
        for (w, h, d) in ((6, 6, 2), (32, 32, 8), (16, 10, 70), (130, 44, 6), (96, 32, 4), (200, 90, 10), (64, 64, 1)):
            vol = values(w * h * d, (k + d) & 1)
            f = gpu_codec.Wavelet3D(gpu_codec.WaveletType(k)).forward(vol, w, h, d)
            assert np.array_equal(f, oracle_mod.wavelet3d(k, vol, w, h, d)), (k, w, h, d)
            assert np.array_equal(gpu_codec.Wavelet3D(gpu_codec.WaveletType(k)).inverse(f, w, h, d), oracle_mod.wavelet3d(k, f, w, h, d, inverse=True)), (k, w, h, d)
    # device pointers, incl. a shape the tiles do not cover (odd width: per-axis kernels behind the same entry point)
    for (w, h, d) in ((130, 44, 6), (33, 20, 4)):
        vol = values(w * h * d, 1)
        dv = torch.from_numpy(vol.copy()).cuda()
        tmp = torch.empty_like(dv)
        assert lib.alice_codec_dev_wavelet3d_forward(1, dv.data_ptr(), tmp.data_ptr(), w, h, d, None) == 0
        ref = oracle_mod.wavelet3d(1, vol, w, h, d)
        assert np.array_equal(dv.cpu().numpy(), ref), (w, h, d)
        assert lib.alice_codec_dev_wavelet3d_inverse(1, dv.data_ptr(), tmp.data_ptr(), w, h, d, None) == 0
        assert np.array_equal(dv.cpu().numpy(), oracle_mod.wavelet3d(1, ref, w, h, d, inverse=True)), (w, h, d)


def test_quantizers_symbols_histogram(gpu_codec, oracle_mod):
    rng = np.random.default_rng(13)
    vals = np.concatenate([rng.integers(-10000, 10001, 5000), [0, 1, -1, 2**31 - 1, -2**31, -2**31 + 1]]).astype(np.int32)
    for step in (1, 2, 7, 8, 14, 17, 64, 128):
        ref = oracle_mod.quantize_buffer(step, vals)
        assert np.array_equal(gpu_codec.Quantizer(step).quantize_buffer(vals), ref)
        fq = gpu_codec.FastQuantizer(step)
        assert np.array_equal(fq.quantize_buffer(vals), oracle_mod.fast_quantize_buffer(oracle_mod.fast_quantizer(step), vals))
        assert fq.step() == step and fq.dead_zone() == step
        assert np.array_equal(gpu_codec.Quantizer(step).dequantize_buffer(ref), oracle_mod.dequantize_buffer(step, ref))
    q = gpu_codec.Quantizer.with_dead_zone(8, 24)
    assert np.array_equal(q.quantize_buffer(vals), oracle_mod.quantize_buffer(8, vals, 24))
    assert gpu_codec.Quantizer(8).quantize(20) == 2 and gpu_codec.Quantizer(8).dequantize(2) == 16  # src/quant.rs:49-55
    fq = gpu_codec.FastQuantizer.from_quantizer(gpu_codec.Quantizer.with_dead_zone(32, 48))       # :919-934
    assert (fq.step(), fq.dead_zone()) == (32, 48)
    small = np.concatenate([np.arange(-300, 300), [2**31 - 1, -2**31, 2**30]]).astype(np.int32)
    sym = gpu_codec.to_symbols(small)
    assert np.array_equal(sym, oracle_mod.to_symbols(small))   # includes the u8 wrap for |c| > 127
    assert list(gpu_codec.to_symbols([0, 1, -1, 2, -2, 3, -3])) == [0, 1, 2, 3, 4, 5, 6]  # src/quant.rs:756-765
    assert np.array_equal(gpu_codec.from_symbols(np.arange(256, dtype=np.uint8)), oracle_mod.from_symbols(np.arange(256, dtype=np.uint8)))
    s = rng.integers(0, 256, 100000, dtype=np.uint8)
    assert np.array_equal(gpu_codec.build_histogram(s), oracle_mod.build_histogram(s))
    assert gpu_codec.build_histogram(np.zeros(0, np.uint8)).sum() == 0
    h = gpu_codec.build_histogram([0, 0, 1, 1, 1, 2, 5, 5])  # src/quant.rs:804-813
    assert (h[0], h[1], h[2], h[3], h[5]) == (2, 3, 1, 0, 2)


def test_colour(gpu_codec, oracle_mod):
    rng = np.random.default_rng(14)
    rgb = rng.integers(0, 256, 3 * 10007, dtype=np.uint8)
    y, co, cg = gpu_codec.rgb_bytes_to_ycocg_r(rgb)
    ry, rco, rcg = oracle_mod.rgb_to_ycocg_r(rgb)
    assert np.array_equal(y, ry) and np.array_equal(co, rco) and np.array_equal(cg, rcg)
    assert np.array_equal(gpu_codec.ycocg_r_to_rgb_bytes(y, co, cg), rgb)  # exact roundtrip, src/color.rs:429-495
    wild = [rng.integers(-32768, 32768, 5000).astype(np.int16) for _ in range(3)]  # i16 wrap + clamp
    assert np.array_equal(gpu_codec.ycocg_r_to_rgb_bytes(*wild), oracle_mod.ycocg_r_to_rgb(*wild))


def test_frequency_tables(gpu_codec, oracle_mod):
    rng = np.random.default_rng(15)
    hists = [np.zeros(256, np.uint32), np.ones(256, np.uint32)]
    h = np.zeros(256, np.uint32); h[100] = 1000; hists.append(h)                 # src/rans.rs:892-910
    h = np.ones(256, np.uint32); h[0] = 1000; h[1] = 500; h[2] = 100; hists.append(h)  # :756-761
    h = np.zeros(256, np.uint32); h[255] = 7; hists.append(h)
    h = np.zeros(256, np.uint32); h[:41] = rng.integers(1, 10**6, 41); hists.append(h)
    h = rng.integers(0, 2**32 - 1, 256, dtype=np.uint64).astype(np.uint32); hists.append(h)
    for _ in range(20):
        h = (rng.integers(0, 5000, 256) * (rng.random(256) < rng.random())).astype(np.uint32); hists.append(h)
    for h in hists:
        t = gpu_codec.FrequencyTable.from_histogram(h); r = oracle_mod.FrequencyTable(h)
        assert np.array_equal(t.freq, r.freq) and np.array_equal(t.cum_freq, r.cum_freq)
    u = gpu_codec.FrequencyTable.uniform(256)
    assert np.all(u.freq == 16) and u.cum_freq[255] == 4080


def test_rans_streams(gpu_codec, oracle_mod):
    rng = np.random.default_rng(16)
    uni_g, uni_o = gpu_codec.FrequencyTable.uniform(256), oracle_mod.FrequencyTable(uniform=256)
    for sym in ([42, 100, 200], [0], [42] * 500, list(range(100)), []):  # the reference's own cases, src/rans.rs:738-924
        e = gpu_codec.RansEncoder(); e.encode_symbols(sym, uni_g); b = e.finish()
        assert b == oracle_mod.rans_encode(sym, uni_o)
        assert list(gpu_codec.RansDecoder(b).decode_n(len(sym), uni_g)) == list(sym)
    for n in (1, 63, 64, 65, 1023, 1024, 1025, 4097, 200000):
        for p0 in (0.0, 0.5, 0.97):
            sym = (rng.integers(1, 256, n) * (rng.random(n) >= p0)).astype(np.uint8)
            hist = np.bincount(sym, minlength=256).astype(np.uint32)
            tg, to = gpu_codec.FrequencyTable.from_histogram(hist), oracle_mod.FrequencyTable(hist)
            e = gpu_codec.RansEncoder(); e.encode_symbols(sym, tg); b = e.finish()
            ref = oracle_mod.rans_encode(sym, to)
            assert b == ref, (n, p0, first_diff(b, ref))
            assert np.array_equal(gpu_codec.RansDecoder(ref).decode_n(n, tg), oracle_mod.rans_decode(ref, n, to))
    # tables that do not match the data: symbols with wrapped frequencies (> 4096) take the exact serial path
    hist = np.zeros(256, np.uint32); hist[3] = 1000
    tg, to = gpu_codec.FrequencyTable.from_histogram(hist), oracle_mod.FrequencyTable(hist)
    assert int(to.freq[255]) > 4096
    sym = rng.choice([3, 3, 3, 7, 255], 5000).astype(np.uint8)
    e = gpu_codec.RansEncoder(); e.encode_symbols(sym, tg)
    assert e.finish() == oracle_mod.rans_encode(sym, to)
    # decoder on short / empty / garbage input (state 0, pos < len guard: src/rans.rs:341-347, 365-368)
    for data in (b"", b"\x01", b"\x01\x02\x03", bytes(rng.integers(0, 256, 50, dtype=np.uint8)), bytes(200)):
        assert np.array_equal(gpu_codec.RansDecoder(data).decode_n(300, uni_g), oracle_mod.rans_decode(data, 300, uni_o))


def test_ssim_matches_oracle_bit_for_bit(gpu_codec, oracle_mod):
    """ssim / ms_ssim (src/ssim.rs:63-176): identical f64 values (exact block sums, ordered mean over blocks)."""
    rng = np.random.default_rng(123)
    for (w, h) in [(64, 64), (8, 8), (7, 9), (16, 8), (250, 131), (1920, 1080), (33, 64)]:
        a = rng.integers(0, 256, w * h, dtype=np.uint8)
        b = np.clip(a.astype(np.int32) + rng.integers(-12, 13, w * h), 0, 255).astype(np.uint8)
        assert gpu_codec.ssim(a, b, w, h) == oracle_mod.ssim(a, b, w, h), (w, h)
        assert gpu_codec.ms_ssim(a, b, w, h) == oracle_mod.ssim(a, b, w, h, multi_scale=True), (w, h)
        assert gpu_codec.ssim(a, a, w, h) == oracle_mod.ssim(a, a, w, h)
    e = np.zeros(0, np.uint8)
    assert gpu_codec.ssim(e, e, 0, 0) == 1.0 and gpu_codec.ms_ssim(e, e, 0, 0) == 1.0
    with pytest.raises(gpu_codec.CodecError):
        gpu_codec.ssim(np.zeros(100, np.uint8), np.zeros(200, np.uint8), 10, 10)
    with pytest.raises(gpu_codec.CodecError):
        gpu_codec.ssim(np.zeros(100, np.uint8), np.zeros(100, np.uint8), 8, 8)


def test_analytical_rdo_matches_oracle(gpu_codec, oracle_mod):
    """AnalyticalRDO::compute_quantizer (src/quant.rs:455-470): identical step and dead zone, because the f64 sum of
    squared deviations is accumulated in element order on the GPU as well."""
    rng = np.random.default_rng(99)
    assert gpu_codec.AnalyticalRDO.with_quality(80).target_bpp() == oracle_mod.rdo_target_bpp(80)
    assert [gpu_codec.SubBand3D(i).quant_strength() for i in range(8)] == [1, 2, 2, 4, 2, 4, 4, 8]
    assert gpu_codec.SubBand3D.LHH.is_temporal_high() and not gpu_codec.SubBand3D.HHL.is_temporal_high() and gpu_codec.SubBand3D.LLL.is_dc()
    for n in (0, 1, 2, 201, 4095, 4096, 4097, 100003):
        for scale in (3, 4000, 2 ** 30):
            c = rng.integers(-scale, scale + 1, n).astype(np.int32)
            for q in (0, 37, 80, 100):
                rdo = gpu_codec.AnalyticalRDO.with_quality(q)
                for sb in (0, 3, 7):
                    qz = rdo.compute_quantizer(c, gpu_codec.SubBand3D(sb))
                    assert (qz.step, qz.dead_zone) == oracle_mod.rdo_compute_quantizer(oracle_mod.rdo_target_bpp(q), c, sb), (n, scale, q, sb)
    alls = gpu_codec.AnalyticalRDO.with_quality(50).compute_all_quantizers([np.arange(-50, 51, dtype=np.int32)] * 8)
    assert all(a.step > 0 for a in alls) and alls[0].step <= alls[7].step                     # src/quant.rs:1045-1070
    assert gpu_codec.AnalyticalRDO(2.0).quality() == 75                                       # AnalyticalRDO::new, :388-393


def test_interleaved_rans_streams(gpu_codec, oracle_mod):
    """InterleavedRansEncoder / InterleavedRansDecoder (src/rans.rs:393-519): four chains on the GPU; the
    reference's own round trips (src/rans.rs:745-780) plus every length residue."""
    rng = np.random.default_rng(77)
    for n in (0, 1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 66, 67, 1000, 4097, 70001):
        sym = (rng.integers(0, 40, n) * (rng.random(n) < 0.4)).astype(np.uint8)
        hist = np.bincount(sym, minlength=256).astype(np.uint32)
        if n == 0:
            hist[:] = 1
        tg = gpu_codec.FrequencyTable.from_histogram(hist)
        to = oracle_mod.FrequencyTable(hist)
        enc = gpu_codec.InterleavedRansEncoder()
        enc.encode(sym, tg)
        got = enc.finish()
        ref = oracle_mod.rans_encode(sym, to, interleaved=True)
        assert got == ref, n
        assert np.array_equal(gpu_codec.InterleavedRansDecoder(ref).decode_n(n, tg), oracle_mod.rans_decode(ref, n, to, interleaved=True)), n
        if n >= 8:   # a prefix: the streams are walked round-robin from the start
            assert np.array_equal(gpu_codec.SimdRansDecoder(ref).decode_n(n - 5, tg),
                                  oracle_mod.rans_decode(ref, n - 5, to, interleaved=True)), n
    # header counts that are not the encoder's: streams that run out are skipped (src/rans.rs:506-509)
    sym = rng.integers(0, 6, 37).astype(np.uint8)
    hist = np.bincount(sym, minlength=256).astype(np.uint32)
    tg = gpu_codec.FrequencyTable.from_histogram(hist); to = oracle_mod.FrequencyTable(hist)
    parts = [sym[0:3], sym[3:20], sym[20:21], sym[21:37]]
    streams = [oracle_mod.rans_encode(p, to) for p in parts]
    blob = b"".join(len(s).to_bytes(4, "little") for s in streams) + b"".join(len(p).to_bytes(4, "little") for p in parts) + b"".join(streams)
    want = oracle_mod.rans_decode(blob, 37, to, interleaved=True)
    assert np.array_equal(gpu_codec.InterleavedRansDecoder(blob).decode_n(37, tg), want)
    assert np.array_equal(gpu_codec.InterleavedRansDecoder(blob).decode_n(20, tg), want[:20])
    with pytest.raises(gpu_codec.CodecError):
        gpu_codec.InterleavedRansDecoder(blob).decode_n(38, tg)      # the reference would spin forever
    with pytest.raises(gpu_codec.CodecError):
        gpu_codec.InterleavedRansDecoder(blob[:40]).decode_n(4, tg)  # the reference would index out of bounds


def test_zero_frequency_symbol_is_reported(gpu_codec, oracle_mod):
    """A histogram whose table gives symbol 255 frequency 0: counts 3842 / 254 out of 4096 normalise to
    themselves, the 254 unused symbols take one slot each, so the sum is 4096 + 254 and the "fix" on the
    last symbol (src/rans.rs:128-132) subtracts exactly its own frequency.  The reference encoder then never
    terminates on a 255 (x_max = 0, src/rans.rs:275-279); both the oracle and the GPU path report it."""
    hist = np.zeros(256, np.uint32)
    hist[0] = 3842
    hist[255] = 254
    ot = oracle_mod.FrequencyTable(hist)
    assert int(ot.freq[255]) == 0 and int(ot.freq[0]) == 3842
    tg = gpu_codec.FrequencyTable.from_histogram(hist)
    assert np.array_equal(tg.freq, ot.freq) and np.array_equal(tg.cum_freq, ot.cum_freq)
    # data without the poisoned symbol still encodes, identically
    sym = np.zeros(1000, np.uint8)
    e = gpu_codec.RansEncoder(); e.encode_symbols(sym, tg)
    assert e.finish() == oracle_mod.rans_encode(sym, ot)
    e = gpu_codec.RansEncoder()
    with pytest.raises(gpu_codec.CodecError) as err:    # inside encode_symbols, where the reference never returns
        e.encode_symbols([0, 255, 0], tg)
    assert err.value.kind == "ReferenceDiverges"
    with pytest.raises(oracle_mod.OracleError) as oerr:
        oracle_mod.rans_encode([0, 255, 0], ot)
    assert oerr.value.code == oracle_mod.ERR_REFERENCE_DIVERGES
    # the full pipeline on a chunk whose Y channel produces exactly that histogram is not constructible from
    # RGB input in general; the stage-level check above is the coverage for this divergence


def test_psnr_ffi(gpu_codec, oracle_mod):  # src/ffi.rs:448-464
    assert gpu_codec.psnr([100, 150, 200], [101, 149, 198]) > 30.0
    assert np.isinf(gpu_codec.psnr([100, 150, 200], [100, 150, 200]))
    rng = np.random.default_rng(17)
    a = rng.integers(0, 256, 100003, dtype=np.uint8); b = rng.integers(0, 256, 100003, dtype=np.uint8)
    assert gpu_codec.psnr(a, b) == oracle_mod.psnr(a, b)


def test_ffi_drop_in_sequence(gpu_codec):
    """The reference's own FFI walk-through (src/ffi.rs:366-417) through the raw 32-bit entry points."""
    lib = gpu_codec.load_library()
    enc = lib.alice_codec_encoder_create(80)
    rgb = (C.c_uint8 * 96)(*([128] * 96))
    chunk = lib.alice_codec_encode(enc, rgb, 96, 4, 4, 2)
    assert chunk
    assert (lib.alice_codec_chunk_width(chunk), lib.alice_codec_chunk_height(chunk), lib.alice_codec_chunk_frames(chunk)) == (4, 4, 2)
    n = C.c_uint32()
    dec = lib.alice_codec_decode(chunk, C.byref(n))
    assert dec and n.value == 96
    lib.alice_codec_data_free(dec, n.value)
    m = C.c_uint32()
    b = lib.alice_codec_chunk_to_bytes(chunk, C.byref(m))
    assert b and m.value == 3152
    payload = C.string_at(b, m.value)[3138:]
    assert payload.hex() == "01507fac40000080000000800000"      # SURVEY.md §8c hand-derived vector
    restored = lib.alice_codec_chunk_from_bytes(C.cast(b, C.POINTER(C.c_uint8)), m.value)
    assert restored and lib.alice_codec_chunk_width(restored) == 4
    lib.alice_codec_chunk_destroy(restored)
    lib.alice_codec_data_free(b, m.value)
    lib.alice_codec_chunk_destroy(chunk)
    lib.alice_codec_encoder_destroy(enc)


def test_concurrent_calls_on_one_handle(gpu_codec, oracle_mod):
    """FrameEncoder / EncodedChunk are Send + Sync in the reference (src/pipeline.rs:635-644)."""
    import threading
    w, h, f = 64, 32, 8
    enc = gpu_codec.FrameEncoder.with_wavelet(80, gpu_codec.WaveletType.Cdf97)
    inputs = [smooth_rgb(w, h, f, seed=100 + i) for i in range(8)]
    refs = [oracle_mod.encode(r, w, h, f, 80, 1) for r in inputs]
    out = [None] * 8
    def work(i):
        c = enc.encode(inputs[i], w, h, f)
        out[i] = (c.to_bytes(), gpu_codec.FrameDecoder().decode(c))
    th = [threading.Thread(target=work, args=(i,)) for i in range(8)]
    [t.start() for t in th]; [t.join() for t in th]
    for i in range(8):
        assert out[i][0] == refs[i]
        assert np.array_equal(out[i][1], oracle_mod.decode(refs[i]))


# ---- device-resident batches (the path bench.py times) --------------------------------------------------

def test_batch_matches_single_chunk_path(gpu_codec, oracle_mod):
    import torch
    w, h, f, B = 96, 64, 16, 5
    chunks = [smooth_rgb(w, h, f, seed=200 + i, shift=3 * i) for i in range(B)]
    rgb = torch.from_numpy(np.stack(chunks)).cuda()
    out = torch.empty_like(rgb)
    bt = gpu_codec.Batch(w, h, f, B, 80, gpu_codec.WaveletType.Cdf97)
    st = torch.cuda.current_stream().cuda_stream
    bt.encode(rgb.data_ptr(), st)
    sizes = bt.encode_finish()
    stride = bt.alc_stride
    host = []
    for i in range(B):
        t = torch.empty(int(sizes[i]), dtype=torch.uint8, device="cuda")
        gpu_hip_memcpy(t.data_ptr(), bt.alc_ptr(i), int(sizes[i]))
        host.append(bytes(t.cpu().numpy()))
    for i in range(B):
        assert host[i] == oracle_mod.encode(chunks[i], w, h, f, 80, 1), i
    bt.decode(bt.alc_ptr(0), stride, out.data_ptr(), st)
    bt.decode_finish()
    got = out.cpu().numpy()
    for i in range(B):
        assert np.array_equal(got[i], oracle_mod.decode(host[i])), i
    ms = bt.stage_ms()
    assert ms["rans_encode"] > 0 and ms["rans_decode"] > 0
    # in-place form (what bench.py runs): pixels of chunk i land over the chunk's consumed symbols
    bt.decode(bt.alc_ptr(0), stride, None, st)
    bt.decode_finish()
    for i in range(B):
        t = torch.empty(w * h * f * 3, dtype=torch.uint8, device="cuda")
        gpu_hip_memcpy(t.data_ptr(), bt.rgb_ptr(i), t.numel())
        assert np.array_equal(t.cpu().numpy(), got[i].reshape(-1)), i
    # and the batch is reusable afterwards
    bt.encode(rgb.data_ptr(), st)
    assert np.array_equal(bt.encode_finish(), sizes)


def test_batch_in_place_decode_odd_shape(gpu_codec, oracle_mod):
    """padded != real size: the in-place outputs sit at a stride of 3 * padded bytes"""
    import torch
    w, h, f, B = 45, 31, 5, 3
    chunks = [smooth_rgb(w, h, f, seed=300 + i, shift=i) for i in range(B)]
    rgb = torch.from_numpy(np.stack(chunks)).cuda()
    bt = gpu_codec.Batch(w, h, f, B, 90, gpu_codec.WaveletType.Cdf97)
    st = torch.cuda.current_stream().cuda_stream
    bt.encode(rgb.data_ptr(), st)
    sizes = bt.encode_finish()
    bt.decode(bt.alc_ptr(0), bt.alc_stride, None, st)
    bt.decode_finish()
    for i in range(B):
        t = torch.empty(w * h * f * 3, dtype=torch.uint8, device="cuda")
        gpu_hip_memcpy(t.data_ptr(), bt.rgb_ptr(i), t.numel())
        want = oracle_mod.decode(oracle_mod.encode(chunks[i], w, h, f, 90, 1))
        assert np.array_equal(t.cpu().numpy(), want), i


def test_batch_stream_capacity_overflow_is_retried(gpu_codec, oracle_mod):
    """A batch's first encode sizes its stream regions from the histograms; the test hook shrinks them to 4352 bytes, so
    every chain overflows and encode_finish must climb the capacity ladder (estimate, then the worst case) itself."""
    import torch
    w, h, f, B = 96, 64, 16, 2
    chunks = [np.random.default_rng(31 + i).integers(0, 256, w * h * f * 3, dtype=np.uint8) for i in range(B)]
    refs = [oracle_mod.encode(c, w, h, f, 90, 1) for c in chunks]
    assert all(len(r) > 3138 + 3 * 4352 for r in refs)
    rgb = torch.from_numpy(np.stack(chunks)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    lib = gpu_codec.load_library()
    lib.alice_codec_test_force_first_cap(4352)
    try:
        bt = gpu_codec.Batch(w, h, f, B, 90, gpu_codec.WaveletType.Cdf97)
        bt.encode(rgb.data_ptr(), st)
        sizes = bt.encode_finish()
    finally:
        lib.alice_codec_test_force_first_cap(0)
    for i in range(B):
        t = torch.empty(int(sizes[i]), dtype=torch.uint8, device="cuda")
        gpu_hip_memcpy(t.data_ptr(), bt.alc_ptr(i), int(sizes[i]))
        assert bytes(t.cpu().numpy()) == refs[i], i


def gpu_hip_memcpy(dst, src, n):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(dst, src, n, 3) == 0  # hipMemcpyDeviceToDevice


# ---- BASELINE.json full-size configurations ---------------------------------------------------------------

def _full_size(gpu_codec, oracle_mod, k, q, decode_too):
    w, h, f = 1920, 1080, 64
    rgb = smooth_rgb(w, h, f, seed=1234)
    chunk = gpu_codec.FrameEncoder.with_wavelet(q, gpu_codec.WaveletType(k)).encode(rgb, w, h, f)
    got = chunk.to_bytes()
    # size-independent properties first (cheap, and they localise a failure)
    assert got[:6] == b"ALCC\x01" + bytes([k])
    padded = w * h * f
    lens = []
    for c in range(3):
        base = 18 + 1040 * c
        lens.append(int.from_bytes(got[base:base + 4], "little"))
        assert int.from_bytes(got[base + 4:base + 8], "little") == oracle_mod.quality_to_step(q)
        assert int.from_bytes(got[base + 12:base + 16], "little") == padded
        assert int(np.frombuffer(got[base + 16:base + 1040], "<u4").astype(np.uint64).sum()) == padded
    assert 3138 + sum(lens) == len(got)
    ref = oracle_mod.encode(rgb, w, h, f, q, k)
    assert hashlib.sha256(got).hexdigest() == hashlib.sha256(ref).hexdigest(), first_diff(got, ref)
    if decode_too:
        dec = gpu_codec.FrameDecoder().decode(chunk)
        assert dec.size == rgb.size
        assert np.array_equal(dec, oracle_mod.decode(ref))


def test_full_size_1080p64_cdf97_q80(gpu_codec, oracle_mod):   # BASELINE.json configs[2], the headline
    _full_size(gpu_codec, oracle_mod, 1, 80, True)


def test_full_size_1080p64_cdf53_q80(gpu_codec, oracle_mod):   # BASELINE.json configs[1]
    _full_size(gpu_codec, oracle_mod, 0, 80, True)


def test_4k_frames_cdf97_q90(gpu_codec, oracle_mod):
    """The spatial size and quality of BASELINE.json configs[3] (3840x2160, q=90) on 6 frames: large tile grids,
    more than 65535 tiles per launch dimension product, a frame count that is not a multiple of 4."""
    w, h, f = 3840, 2160, 6
    rgb = smooth_rgb(w, h, f, seed=77)
    ref = oracle_mod.encode(rgb, w, h, f, 90, 1)
    chunk = gpu_codec.FrameEncoder.with_wavelet(90, gpu_codec.WaveletType.Cdf97).encode(rgb, w, h, f)
    got = chunk.to_bytes()
    assert hashlib.sha256(got).hexdigest() == hashlib.sha256(ref).hexdigest(), first_diff(got, ref)
    assert np.array_equal(gpu_codec.FrameDecoder().decode(chunk), oracle_mod.decode(ref))


def test_unaligned_widths_and_heights(gpu_codec, oracle_mod):
    """Widths that are not multiples of 4 (byte-wise RGB loads/stores), tiles that straddle every border case."""
    for w, h, f, k in ((130, 41, 4, 1), (257, 83, 3, 0), (127, 40, 2, 2), (129, 121, 5, 1), (514, 90, 2, 1)):
        rgb = np.random.default_rng(w + h).integers(0, 256, w * h * f * 3, dtype=np.uint8)
        ref = oracle_mod.encode(rgb, w, h, f, 85, k)
        chunk = gpu_codec.FrameEncoder.with_wavelet(85, gpu_codec.WaveletType(k)).encode(rgb, w, h, f)
        assert chunk.to_bytes() == ref, (w, h, f, k)
        assert np.array_equal(gpu_codec.FrameDecoder().decode(chunk), oracle_mod.decode(ref)), (w, h, f, k)
