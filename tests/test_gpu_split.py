"""The split-stream format (.alc version 2) on the MI355X against tests/split_ref.py, the numpy restatement of DESIGN.md
section 10: tables integer for integer, stage-level streams byte for byte, whole chunks (symbols = v1's forward symbols,
pixels = the oracle's inverse of those symbols), one full-size chunk through properties, the device-resident calls, and
seeded corruption whose verdict must be split_ref's."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_ref as R  # noqa: E402
from slab_oracle_stages import OracleStages  # noqa: E402

import torch  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def smooth(w, h, f, seed, noise=6):
    rng = np.random.default_rng(seed)
    t, y, x = np.meshgrid(np.arange(f), np.arange(h), np.arange(w), indexing="ij")
    base = 128 + 70 * np.sin((x + 2 * t) / 9.0 + seed) * np.cos((y - t) / 7.0)
    rgb = np.stack([base, base * 0.8 + 20, 255 - base], axis=-1) + rng.integers(-noise, noise + 1, (f, h, w, 3))
    return np.clip(rgb, 0, 255).astype(np.uint8).reshape(-1)


def skewed_symbols(seed, n, alpha=0.05):
    rng = np.random.default_rng(seed)
    return rng.choice(256, n, p=rng.dirichlet(np.ones(256) * alpha)).astype(np.uint8)


def hist_of(sym):
    return np.bincount(sym, minlength=256).astype(np.uint32)


def dev_encode(codec, sym, L, align=0, cap=None):
    """alice_codec_dev_split_encode of host symbols -> the payload bytes; the output starts `align` bytes into a buffer"""
    lib = codec.load_library()
    n = sym.size
    d_sym = torch.from_numpy(sym.copy()).to(DEV) if n else torch.zeros(1, dtype=torch.uint8, device=DEV)
    cap = codec.split_stream_bound(n, L) if cap is None else cap
    out = torch.full((cap + 16 + align,), 0xAB, dtype=torch.uint8, device=DEV)
    h = hist_of(sym)
    got = C.c_uint64(0)
    rc = lib.alice_codec_dev_split_encode(d_sym.data_ptr(), n, h.ctypes.data_as(C.POINTER(C.c_uint32)), L, out.data_ptr() + align, cap,
                                          C.byref(got), None)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    if rc == 0:
        assert (host[:align] == 0xAB).all() and (host[align + got.value:] == 0xAB).all(), "bytes outside the stream were written"
    return rc, host[align:align + got.value].tobytes()


def dev_decode(codec, payload, freq, L, n, align=0):
    """alice_codec_dev_split_decode -> (rc, symbols)"""
    lib = codec.load_library()
    buf = np.zeros(len(payload) + align + 1, np.uint8)
    buf[align:align + len(payload)] = np.frombuffer(payload, np.uint8)
    d_in = torch.from_numpy(buf).to(DEV)
    d_out = torch.zeros(max(n, 1) + 64, dtype=torch.uint8, device=DEV)
    d_out[n:] = 0xCD
    f = np.ascontiguousarray(freq, np.uint16)
    rc = lib.alice_codec_dev_split_decode(d_in.data_ptr() + align, len(payload), f.ctypes.data_as(C.POINTER(C.c_uint16)), L,
                                          d_out.data_ptr(), n, None)
    torch.cuda.synchronize()
    host = d_out.cpu().numpy()
    assert (host[n:] == 0xCD).all(), "symbols were stored outside the block"
    return rc, host[:n]


def special_histograms():
    rng = np.random.default_rng(11)
    one = np.zeros(256, np.uint32); one[77] = 12345
    dominant = np.ones(256, np.uint32); dominant[3] = 10_000_000
    floor_heavy = np.ones(256, np.uint32); floor_heavy[:56] = 1000
    out = [one, dominant, floor_heavy, np.zeros(256, np.uint32)]
    for _ in range(12):
        h = (rng.pareto(0.7, 256) * rng.integers(1, 1000)).astype(np.uint32)
        h[rng.random(256) < rng.random()] = 0
        out.append(h)
    out.append(np.full(256, 0xFFFFFF, np.uint32))        # total close to 2^32
    return out


def test_tables_equal_split_ref(gpu_codec):
    for h in special_histograms():
        got = gpu_codec.normalized_frequencies(h)
        want = R.normalize(h)
        assert np.array_equal(got, want), h.tolist()
        assert int(got.astype(np.int64).sum()) == (4096 if h.sum() else 0)


# (n, L, alpha): every allowed L at least once; n = 1, n < 64, n not a multiple of 64 L, exact multiples, several blocks
STAGE_CASES = [
    (1, 64, 0.05), (37, 64, 0.05), (64, 64, 1.0), (64 * 64 * 3 + 17, 64, 0.05), (64 * 128, 128, 0.3), (64 * 256 * 2 + 63, 256, 0.02),
    (100_000, 512, 0.05), (64 * 1024 + 65, 1024, 5.0), (150_001, 2048, 0.05), (64 * 4096 + 1, 4096, 0.1), (300_000, 8192, 0.05),
    (64 * 16384 + 700, 16384, 0.02), (5, 16384, 0.05),
]


@pytest.mark.parametrize("case", STAGE_CASES)
def test_stage_streams_equal_split_ref(gpu_codec, case):
    n, L, alpha = case
    sym = skewed_symbols(n + L, n, alpha)
    freq = R.normalize(hist_of(sym))
    want = R.encode_channel(sym, freq, L)
    assert len(want) <= gpu_codec.split_stream_bound(n, L)
    for align in range(4):
        rc, got = dev_encode(gpu_codec, sym, L, align)
        assert rc == 0 and got == want, (case, align)
        rc, dec = dev_decode(gpu_codec, want, freq, L, n, align)
        assert rc == 0 and np.array_equal(dec, sym), (case, align)
    # a capacity of exactly the stream's length is enough; one byte less is refused with nothing written
    rc, got = dev_encode(gpu_codec, sym, L, 1, cap=len(want))
    assert rc == 0 and got == want
    rc, _ = dev_encode(gpu_codec, sym, L, 0, cap=len(want) - 1)
    assert rc == 1   # InvalidBufferSize


@pytest.mark.parametrize("L", [64, 512])
def test_single_symbol_and_all_zero_channels(gpu_codec, L):
    for sym in (np.zeros(64 * L + 9, np.uint8), np.full(777, 200, np.uint8), np.zeros(1, np.uint8)):
        freq = R.normalize(hist_of(sym))
        assert int(freq.max()) == 4096
        want = R.encode_channel(sym, freq, L)
        rc, got = dev_encode(gpu_codec, sym, L, 3)
        assert rc == 0 and got == want
        rc, dec = dev_decode(gpu_codec, want, freq, L, sym.size, 1)
        assert rc == 0 and np.array_equal(dec, sym)
    # an empty channel: no payload, all-zero table
    rc, got = dev_encode(gpu_codec, np.zeros(0, np.uint8), L)
    assert rc == 0 and got == b""
    rc, _ = dev_decode(gpu_codec, b"", np.zeros(256, np.uint16), L, 0)
    assert rc == 0


# (w, h, f, wavelet, quality, L): the golden fixtures' shapes, odd sizes, f = 1, the three wavelets, generic-path shapes
# (a padded side below 6)
CHUNK_CASES = [
    (64, 64, 8, 2, 100, 64), (33, 17, 5, 1, 80, 64), (70, 50, 6, 1, 75, 128), (64, 48, 16, 1, 100, 0), (96, 64, 16, 0, 80, 256),
    (96, 64, 16, 1, 80, 1024), (13, 9, 3, 0, 50, 64), (16, 12, 1, 2, 90, 64), (3, 40, 4, 1, 80, 64), (33, 3, 2, 0, 60, 64),
    (1, 1, 1, 1, 80, 64),
]


def check_chunk(codec, oracle_mod, rgb, w, h, f, k, q, L):
    enc = codec.FrameEncoder.with_wavelet(q, codec.WaveletType(k))
    got = codec.encode_split(enc, rgb, w, h, f, L)
    Le = L or codec.SPLIT_DEFAULT_LANE_SYMBOLS
    sym = oracle_mod.encode_symbols(rgb, w, h, f, q, k).reshape(3, -1)
    step = 64 - (q * 63) // 100
    assert got == R.write_container(k, w, h, f, Le, [step] * 3, sym), (w, h, f, k, q, L)
    info, dec_sym = R.decode_container(got)
    for c in range(3):
        assert np.array_equal(dec_sym[c], sym[c])
    ci = codec.split_info(got)
    assert (ci.width, ci.height, ci.frames, ci.lane_symbols, int(ci.wavelet_type)) == (w, h, f, Le, k)
    assert ci.quant_step == [step] * 3 and ci.dead_zone == [step] * 3 and ci.payload_len == info["payload_len"]
    pw, ph, pf = R.padded_dims(w, h, f)
    want = OracleStages().inverse_symbols(torch.from_numpy(sym.reshape(3, pf, ph, pw)), w, h, f, k, [step] * 3).numpy().reshape(-1)
    assert np.array_equal(codec.decode_split(got), want), (w, h, f, k, q, L)
    return got


@pytest.mark.parametrize("case", CHUNK_CASES)
def test_whole_chunks_round_trip(gpu_codec, oracle_mod, case):
    w, h, f, k, q, L = case
    check_chunk(gpu_codec, oracle_mod, smooth(w, h, f, w + h + f + k), w, h, f, k, q, L)


def test_banded_chunk_round_trips(gpu_codec, oracle_mod):
    lib = gpu_codec.load_library()
    try:
        lib.alice_codec_test_set_tuning(96)   # one tile row per band
        check_chunk(gpu_codec, oracle_mod, smooth(256, 250, 10, 5), 256, 250, 10, 1, 80, 256)
    finally:
        lib.alice_codec_test_set_tuning(1024 * 1024)


def test_v1_parser_refuses_v2_and_v2_refuses_v1(gpu_codec):
    rgb = smooth(16, 12, 2, 3)
    enc = gpu_codec.FrameEncoder.with_wavelet(80, gpu_codec.WaveletType.Cdf97)
    v2 = gpu_codec.encode_split(enc, rgb, 16, 12, 2)
    with pytest.raises(gpu_codec.CodecError, match="unsupported version"):
        gpu_codec.EncodedChunk.from_bytes(v2 + bytes(4000))
    with pytest.raises(gpu_codec.CodecError, match="unsupported version"):
        gpu_codec.decode_split(enc.encode(rgb, 16, 12, 2).to_bytes())


def test_device_calls_many_chunks_qualities_and_stream(gpu_codec):
    w, h, f, n = 70, 50, 6, 5
    k = gpu_codec.WaveletType.Cdf97
    quals = [95, 20, 80, 50, 100]
    chunks = [smooth(w, h, f, 40 + i) for i in range(n)]
    host = [gpu_codec.encode_split(gpu_codec.FrameEncoder.with_wavelet(quals[i], k), chunks[i], w, h, f, 128) for i in range(n)]
    stride = gpu_codec.SPLIT_HEADER_BYTES + 3 * gpu_codec.split_stream_bound(R.padded_dims(w, h, f)[0] * 50 * 6, 128) + 3
    st = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(st):
        d_rgb = torch.from_numpy(np.concatenate(chunks)).to(DEV)
        d_out = torch.zeros(n * stride, dtype=torch.uint8, device=DEV)
        d_back = torch.zeros(n * w * h * f * 3, dtype=torch.uint8, device=DEV)
        sizes = gpu_codec.split_encode_device(d_rgb.data_ptr(), w, h, f, n, k, 0, d_out.data_ptr(), stride, qualities=quals,
                                              lane_symbols=128, stream=st.cuda_stream)
        gpu_codec.split_decode_device(d_out.data_ptr(), stride, sizes, d_back.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    out = d_out.cpu().numpy()
    back = d_back.cpu().numpy().reshape(n, -1)
    for i in range(n):
        assert out[i * stride:i * stride + int(sizes[i])].tobytes() == host[i], i
        assert np.array_equal(back[i], gpu_codec.decode_split(host[i])), i
    # a stride that cannot hold a chunk is refused before anything is written
    d_out.zero_()
    with pytest.raises(gpu_codec.CodecError) as e:
        gpu_codec.split_encode_device(d_rgb.data_ptr(), w, h, f, n, k, 80, d_out.data_ptr(), 2000)
    assert e.value.code == 1 and int(d_out.count_nonzero()) == 0


def test_fullsize_1080p64_chunk_properties_and_psnr(gpu_codec):
    """One 1920x1080x64 CDF 9/7 q = 80 chunk of the benchmark's content: directory sums, end checks, the symbols of the
    stage call, and the comparison the v1 suite cannot make: the v2 round trip comes back, the v1 round trip (the
    reference's frequency table, reproduced bit for bit) does not."""
    lib = gpu_codec.load_library()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    w, h, f, q = 1920, 1080, 64, 80
    assert (bench.W, bench.H, bench.F) == (w, h, f)
    k = gpu_codec.WaveletType.Cdf97
    L = gpu_codec.SPLIT_DEFAULT_LANE_SYMBOLS
    d_rgb = bench.synth_chunk(torch.device(DEV), 0).contiguous()
    n = w * h * f
    cap = gpu_codec.SPLIT_HEADER_BYTES + 3 * gpu_codec.split_stream_bound(n, L)
    d_out = torch.zeros(cap, dtype=torch.uint8, device=DEV)
    size = int(gpu_codec.split_encode_device(d_rgb.data_ptr(), w, h, f, 1, k, q, d_out.data_ptr(), cap)[0])
    alc = d_out[:size].cpu().numpy()
    info = R.parse_container(alc.tobytes())         # header fields and directory sums, restated
    ci = gpu_codec.split_info(alc)                  # the same through the C ABI
    assert ci.payload_len == info["payload_len"] and ci.n_blocks == [R.n_blocks_of(n, L)] * 3
    # the symbols of the stage call, channel by channel, through the stage-level decoder (its end checks pass)
    d_sym = torch.zeros(3 * n, dtype=torch.uint8, device=DEV)
    assert lib.alice_codec_dev_forward_symbols(d_rgb.data_ptr(), w, h, f, int(k), q, d_sym.data_ptr(), None, None) == 0
    d_dec = torch.zeros(n, dtype=torch.uint8, device=DEV)
    off = gpu_codec.SPLIT_HEADER_BYTES
    for c in range(3):
        fr = np.ascontiguousarray(info["freq"][c], np.uint16)
        rc = lib.alice_codec_dev_split_decode(d_out.data_ptr() + off, info["payload_len"][c], fr.ctypes.data_as(C.POINTER(C.c_uint16)),
                                              L, d_dec.data_ptr(), n, None)
        assert rc == 0, c
        assert torch.equal(d_dec, d_sym[c * n:(c + 1) * n]), c
        off += info["payload_len"][c]
    # the restated decoder on the chroma channel (end checks of every lane, symbols)
    s, ok = R.decode_channel(info["payload"][2], info["freq"][2], L, n)
    assert ok and np.array_equal(s, d_sym[2 * n:].cpu().numpy())
    del d_sym, d_dec
    # round trips
    d_back = torch.zeros(n * 3, dtype=torch.uint8, device=DEV)
    gpu_codec.split_decode_device(d_out.data_ptr(), cap, [size], d_back.data_ptr())
    rgb = d_rgb.cpu().numpy().reshape(-1)
    v2 = d_back.cpu().numpy()
    enc = gpu_codec.FrameEncoder.with_wavelet(q, k)
    assert np.array_equal(gpu_codec.decode_split(gpu_codec.encode_split(enc, rgb, w, h, f)), v2)   # the host route agrees
    chunk = enc.encode(rgb, w, h, f)
    v1 = gpu_codec.FrameDecoder().decode(chunk)
    p2, p1 = gpu_codec.psnr(v2, rgb), gpu_codec.psnr(v1, rgb)
    print(f"1080p x 64 CDF 9/7 q80: PSNR of the v2 round trip {p2:.2f} dB, of the v1 round trip {p1:.2f} dB; "
          f"v2 {size} bytes, v1 {len(chunk.to_bytes())} bytes")
    assert p2 > p1


def corruption_cases(payload, n, L, seed):
    """(name, bytes) -- flips inside lane streams and directories, and truncations"""
    rng = np.random.default_rng(seed)
    nb = R.n_blocks_of(n, L)
    blen = np.frombuffer(payload, "<u4", nb).astype(np.int64)
    boff = 4 * nb + np.cumsum(blen) - blen
    cases = []
    for i in range(24):
        b = int(rng.integers(nb))
        lo, hi = int(boff[b]) + 128, int(boff[b] + blen[b])
        p = bytearray(payload)
        pos = int(rng.integers(lo, hi))
        p[pos] ^= 1 << int(rng.integers(8))
        cases.append((f"stream flip {i} at {pos}", bytes(p)))
    for i in range(12):
        b = int(rng.integers(nb))
        p = bytearray(payload)
        pos = int(boff[b]) + int(rng.integers(128))
        p[pos] ^= 1 << int(rng.integers(8))
        cases.append((f"lane directory flip {i} at {pos}", bytes(p)))
    for i in range(8):
        p = bytearray(payload)
        pos = int(rng.integers(4 * nb))
        p[pos] ^= 1 << int(rng.integers(8))
        cases.append((f"block table flip {i} at {pos}", bytes(p)))
    for i in range(8):
        cases.append((f"truncation {i}", payload[:int(rng.integers(1, len(payload)))]))
    cases.append(("one byte", payload[:1]))
    cases.append(("extended", payload + b"\0\0\0"))
    return cases


@pytest.mark.parametrize("n,L,seed", [(64 * 64 * 5 + 100, 64, 1), (200_000, 512, 2), (30_000, 16384, 4)])
def test_corruption_verdicts_equal_split_ref(gpu_codec, n, L, seed):
    """Bounds safety: no case is built to fault the device; every read of the decoder is clamped to its lane stream and
    every store to its block, so a damaged payload ends in a verdict.  The process survives to make the last assertion."""
    sym = skewed_symbols(seed, n, 0.1)
    freq = R.normalize(hist_of(sym))
    payload = R.encode_channel(sym, freq, L)
    for name, bad in corruption_cases(payload, n, L, seed):
        _, ref_ok = R.decode_channel(bad, freq, L, n)
        assert not ref_ok, name      # (checked on the CPU when the cases were chosen: every one of them is detected)
        rc, _ = dev_decode(gpu_codec, bad, freq, L, n, align=seed % 4)
        assert (rc == 0) == ref_ok and rc in (0, 4), (name, rc)
    rc, dec = dev_decode(gpu_codec, payload, freq, L, n)
    assert rc == 0 and np.array_equal(dec, sym)


def test_whole_container_corruption(gpu_codec):
    w, h, f = 70, 50, 6
    rgb = smooth(w, h, f, 9)
    good = gpu_codec.encode_split(gpu_codec.FrameEncoder.with_wavelet(80, gpu_codec.WaveletType.Cdf97), rgb, w, h, f, 64)
    rng = np.random.default_rng(5)
    for i in range(40):
        p = bytearray(good)
        pos = int(rng.integers(22, len(good)))
        p[pos] ^= 1 << int(rng.integers(8))
        try:
            R.decode_container(bytes(p))
            ref_ok = True
        except R.InvalidBitstream:
            ref_ok = False
        try:
            gpu_codec.decode_split(bytes(p))
            ok = True
        except gpu_codec.CodecError as e:
            assert e.code == 4, (pos, e)
            ok = False
        # a flipped quantiser step still decodes (to other pixels): the verdicts must agree either way
        assert ok == ref_ok, pos
    assert gpu_codec.decode_split(good).size == w * h * f * 3
