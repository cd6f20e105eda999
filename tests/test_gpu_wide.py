"""The wide format (.alc version 3) on the MI355X against tests/wide_ref.py, the numpy restatement of DESIGN.md section 11:
stage-level streams byte for byte, whole chunks (symbols = the zigzag of the oracle's quantised coefficients, container =
wide_ref's, pixels = the oracle's inverse of those symbols), a banded chunk, the device-resident calls, seeded damage whose
verdict must be wide_ref's, and the separation of the three parsers."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_oracle as WO  # noqa: E402
import wide_ref as R  # noqa: E402
from test_wide_host import CASES, seeded_symbols  # noqa: E402

import torch  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64


def dev_encode(codec, z, L, align=0, cap=None):
    """alice_codec_dev_wide_encode of host symbols -> (rc, payload); the output starts `align` bytes into a guarded buffer"""
    lib = codec.load_library()
    n = z.size
    d_sym = torch.from_numpy(z.astype(np.int16).copy()).to(DEV) if n else torch.zeros(1, dtype=torch.int16, device=DEV)
    cap = codec.wide_stream_bound(n, L) if cap is None else cap
    out = torch.full((GUARD + align + cap + GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
    h = R.histogram(z)
    got = C.c_uint64(0)
    rc = lib.alice_codec_dev_wide_encode(d_sym.data_ptr(), n, h.ctypes.data_as(C.POINTER(C.c_uint32)), L, out.data_ptr() + GUARD + align,
                                         cap, C.byref(got), None)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    lo = GUARD + align
    written = int(got.value) if rc == 0 else 0
    assert (host[:lo] == 0xAB).all() and (host[lo + written:] == 0xAB).all(), "bytes outside the stream were written"
    assert np.array_equal(d_sym.cpu().numpy().view(np.uint16)[:n], z), "the symbols were modified"
    return rc, host[lo:lo + written].tobytes()


def dev_decode(codec, payload, freq, L, n, align=0):
    """alice_codec_dev_wide_decode -> (rc, u16 symbols); guard elements on both sides of the symbol buffer"""
    lib = codec.load_library()
    buf = np.zeros(len(payload) + align + 1, np.uint8)
    buf[align:align + len(payload)] = np.frombuffer(payload, np.uint8)
    d_in = torch.from_numpy(buf).to(DEV)
    d_out = torch.full((GUARD + max(n, 1) + GUARD,), 0x5A5A, dtype=torch.int16, device=DEV)
    f = np.ascontiguousarray(freq, np.uint16)
    rc = lib.alice_codec_dev_wide_decode(d_in.data_ptr() + align, len(payload), f.ctypes.data_as(C.POINTER(C.c_uint16)), L,
                                         d_out.data_ptr() + 2 * GUARD, n, None)
    torch.cuda.synchronize()
    host = d_out.cpu().numpy().view(np.uint16)
    assert (host[:GUARD] == 0x5A5A).all() and (host[GUARD + n:] == 0x5A5A).all(), "symbols were stored outside the buffer"
    assert np.array_equal(d_in.cpu().numpy(), buf), "the payload was modified"
    return rc, host[GUARD:GUARD + n]


@pytest.mark.parametrize("n,L", CASES)
@pytest.mark.parametrize("share", [0.0, 0.05, 1.0])
def test_stage_streams_equal_wide_ref(gpu_codec, n, L, share):
    z = seeded_symbols(n, share, seed=3 * n + int(share * 100))
    if n > 64 and share > 0:
        z[0] = 255; z[1] = 255 + 4095; z[n - 1] = 255 + 4095; z[n - 2] = 255
        z[((min(n, 64 * L) - 1) // 64) * 64] = 255 + 4095      # the last symbol of lane 0 of the first block
    freq = R.normalize(R.histogram(z))
    want = R.encode_channel(z, freq, L)
    assert len(want) <= gpu_codec.wide_stream_bound(n, L) == R.stream_bound(n, L)
    for align in range(4):
        rc, got = dev_encode(gpu_codec, z, L, align)
        assert rc == 0 and got == want, (n, L, share, align)
        rc, dec = dev_decode(gpu_codec, want, freq, L, n, align)
        assert rc == 0 and np.array_equal(dec, z), (n, L, share, align)
    rc, got = dev_encode(gpu_codec, z, L, 1, cap=len(want))
    assert rc == 0 and got == want
    rc, got = dev_encode(gpu_codec, z, L, 0, cap=len(want) - 1)
    assert rc == 1 and got == b""   # InvalidBufferSize, nothing written (dev_encode checks the whole buffer)


def test_residual_guard_refuses_before_a_byte_is_written(gpu_codec):
    z = seeded_symbols(5000, 0.05, 9)
    z[4321] = 255 + 4096
    rc, got = dev_encode(gpu_codec, z, 64, 2)
    assert rc == 10 and got == b""   # ALICE_ERR_INTERNAL
    assert "255 + 4095" in gpu_codec.load_library().alice_codec_last_error_message().decode()
    z[4321] = 255 + 4095
    rc, got = dev_encode(gpu_codec, z, 64, 2)
    assert rc == 0 and got == R.encode_channel(z, R.normalize(R.histogram(z)), 64)


# shape -> wavelet (0 CDF 5/3, 1 CDF 9/7, 2 Haar) and lane length: the three wavelets, odd sizes, f = 1, generic-path shapes
CHUNK_SHAPES = [(64, 64, 8, 2, 64), (33, 17, 5, 1, 64), (70, 50, 6, 1, 128), (96, 64, 16, 0, 256), (13, 9, 3, 0, 64), (16, 12, 1, 2, 64),
                (3, 40, 4, 1, 64), (33, 3, 2, 0, 64), (1, 1, 1, 1, 0)]
LARGER = {(64, 64, 8), (70, 50, 6), (96, 64, 16)}
_refs = {}


def reference(w, h, f, k, q):
    """(rgb, step, [z_Y, z_Co, z_Cg], pixels) from the CPU oracle, computed once per case"""
    import oracle.alice_oracle_np as o
    key = (w, h, f, k, q)
    if key not in _refs:
        rgb = WO.smooth_plus_noise(w, h, f, seed=w + h + f)
        step, dims, qs = WO.forward_quantised(o, rgb, w, h, f, q, k)
        z = [R.wide_symbols(v) for v in qs]
        pixels = WO.inverse_quantised(o, [R.from_wide_symbols(zz) for zz in z], step, dims, w, h, f, k)
        _refs[key] = (rgb, step, z, pixels)
    return _refs[key]


def forward_symbols_wide(codec, rgb, w, h, f, k, q):
    n = int(np.prod(R.padded_dims(w, h, f)))
    d_rgb = torch.from_numpy(rgb).to(DEV)
    d_sym = torch.full((3 * n + GUARD,), 0x5A5A, dtype=torch.int16, device=DEV)
    d_hist = torch.zeros(3 * 256, dtype=torch.int32, device=DEV)
    codec.forward_symbols_wide_device(d_rgb.data_ptr(), w, h, f, codec.WaveletType(k), q, d_sym.data_ptr(), d_hist.data_ptr())
    torch.cuda.synchronize()
    host = d_sym.cpu().numpy().view(np.uint16)
    assert (host[3 * n:] == 0x5A5A).all()
    return host[:3 * n].reshape(3, n), d_hist.cpu().numpy().view(np.uint32).reshape(3, 256)


def check_chunk(codec, w, h, f, k, q, L):
    rgb, step, z, pixels = reference(w, h, f, k, q)
    assert step == {100: 1, 95: 5, 80: 14, 0: 64}.get(q, step)
    got_z, got_hist = forward_symbols_wide(codec, rgb, w, h, f, k, q)
    for c in range(3):
        assert np.array_equal(got_z[c], z[c]), (w, h, f, k, q, c)
        assert np.array_equal(got_hist[c], R.histogram(z[c])), (w, h, f, k, q, c)
    enc = codec.FrameEncoder.with_wavelet(q, codec.WaveletType(k))
    got = codec.encode_wide(enc, rgb, w, h, f, L)
    Le = L or codec.SPLIT_DEFAULT_LANE_SYMBOLS
    assert got == R.write_container(k, w, h, f, Le, [step] * 3, z), (w, h, f, k, q, L)
    ci = codec.wide_info(got)
    assert (ci.width, ci.height, ci.frames, ci.lane_symbols, int(ci.wavelet_type)) == (w, h, f, Le, k)
    assert ci.quant_step == [step] * 3 and ci.dead_zone == [step] * 3
    dec = codec.decode_wide(got)
    assert np.array_equal(dec, pixels), (w, h, f, k, q, L)
    assert np.array_equal(codec.decode_alc(got), pixels)
    escapes = sum(int((zz >= 255).sum()) for zz in z)
    if q == 100 and (w, h, f) in LARGER:
        assert escapes > 0
    if escapes == 0:
        assert np.array_equal(dec, codec.decode_split(codec.encode_split(enc, rgb, w, h, f, L))), (w, h, f, k, q)
    return got, escapes


@pytest.mark.parametrize("q", [100, 95, 80, 0])
@pytest.mark.parametrize("shape", CHUNK_SHAPES)
def test_whole_chunks_round_trip(gpu_codec, oracle_mod, shape, q):
    w, h, f, k, L = shape
    check_chunk(gpu_codec, w, h, f, k, q, L)


@pytest.mark.parametrize("q", [100, 80])
def test_banded_chunk_round_trips(gpu_codec, oracle_mod, q):
    lib = gpu_codec.load_library()
    try:
        lib.alice_codec_test_set_tuning(96)   # one tile row per band
        _, escapes = check_chunk(gpu_codec, 256, 250, 10, 1, q, 256)
        assert (escapes > 0) == (q == 100)
    finally:
        lib.alice_codec_test_set_tuning(1024 * 1024)


def test_device_calls_many_chunks_and_qualities(gpu_codec):
    w, h, f, n = 70, 50, 6, 5
    k = gpu_codec.WaveletType.Cdf97
    quals = [100, 20, 95, 50, 100]
    chunks = [WO.smooth_plus_noise(w, h, f, seed=40 + i) for i in range(n)]
    host = [gpu_codec.encode_wide(gpu_codec.FrameEncoder.with_wavelet(quals[i], k), chunks[i], w, h, f, 128) for i in range(n)]
    stride = gpu_codec.SPLIT_HEADER_BYTES + 3 * gpu_codec.wide_stream_bound(int(np.prod(R.padded_dims(w, h, f))), 128) + 3
    st = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(st):
        d_rgb = torch.from_numpy(np.concatenate(chunks)).to(DEV)
        d_out = torch.zeros(n * stride, dtype=torch.uint8, device=DEV)
        d_back = torch.zeros(n * w * h * f * 3, dtype=torch.uint8, device=DEV)
        sizes = gpu_codec.wide_encode_device(d_rgb.data_ptr(), w, h, f, n, k, 0, d_out.data_ptr(), stride, qualities=quals,
                                             lane_symbols=128, stream=st.cuda_stream)
        gpu_codec.wide_decode_device(d_out.data_ptr(), stride, sizes, d_back.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    out = d_out.cpu().numpy()
    back = d_back.cpu().numpy().reshape(n, -1)
    for i in range(n):
        assert out[i * stride:i * stride + int(sizes[i])].tobytes() == host[i], i
        assert np.array_equal(back[i], gpu_codec.decode_wide(host[i])), i
    assert max(WO.psnr(chunks[0], back[0]), WO.psnr(chunks[4], back[4])) > 35    # q = 100 comes back
    d_out.zero_()
    with pytest.raises(gpu_codec.CodecError) as e:
        gpu_codec.wide_encode_device(d_rgb.data_ptr(), w, h, f, n, k, 80, d_out.data_ptr(), 2000)
    assert e.value.code == 1 and int(d_out.count_nonzero()) == 0


def damage_cases(payload, n, L, seed):
    """(name, bytes): single-byte flips in the block table, the lane directory, a lane's first four bytes (its state) and
    inside lane streams (with share = 1 every stream byte belongs to an escape), and truncations.  Well-formed calls only."""
    rng = np.random.default_rng(seed)
    nb = R.n_blocks_of(n, L)
    blen = np.frombuffer(payload, "<u4", nb).astype(np.int64)
    boff = 4 * nb + np.cumsum(blen) - blen
    cases = []

    def flip(name, pos):
        p = bytearray(payload)
        p[pos] ^= 1 << int(rng.integers(8))
        cases.append((f"{name} at {pos}", bytes(p)))

    for i in range(6):
        flip(f"block table flip {i}", int(rng.integers(4 * nb)))
    for i in range(10):
        flip(f"lane directory flip {i}", int(boff[rng.integers(nb)]) + int(rng.integers(128)))
    for i in range(10):
        b = int(rng.integers(nb))
        lens = np.frombuffer(payload, "<u2", 64, int(boff[b])).astype(np.int64)
        j = int(rng.integers(64))
        if lens[j] >= 4:
            flip(f"lane state flip {i}", int(boff[b]) + 128 + int(lens[:j].sum()) + int(rng.integers(4)))
    for i in range(20):
        b = int(rng.integers(nb))
        flip(f"stream flip {i}", int(rng.integers(int(boff[b]) + 128, int(boff[b] + blen[b]))))
    for i in range(6):
        cases.append((f"truncation {i}", payload[:int(rng.integers(1, len(payload)))]))
    cases.append(("extended", payload + b"\0\0\0"))
    return cases


@pytest.mark.parametrize("n,L,share,seed", [(64 * 64 * 2 + 100, 64, 0.05, 1), (20_000, 128, 1.0, 2), (30_000, 8192, 0.3, 4)])
def test_damage_verdicts_equal_wide_ref(gpu_codec, n, L, share, seed):
    """Bounds safety: every read of the decoder is clamped to its lane stream and every store to its block, so a damaged
    payload ends in a verdict (dev_decode checks the guards around the symbol buffer).  Nothing here is built to fault."""
    z = seeded_symbols(n, share, seed)
    freq = R.normalize(R.histogram(z))
    payload = R.encode_channel(z, freq, L)
    refused = 0
    for name, bad in damage_cases(payload, n, L, seed):
        if len(bad) < 132 * R.n_blocks_of(n, L):
            ref_ok = False           # the host refuses a payload that cannot hold its directories
        else:
            ref_dec, ref_ok = R.decode_channel(bad, freq, L, n)
        rc, dec = dev_decode(gpu_codec, bad, freq, L, n, align=seed % 4)
        assert (rc == 0) == ref_ok and rc in (0, 4), (name, rc)
        if ref_ok:
            assert np.array_equal(dec, ref_dec), name
        refused += not ref_ok
    assert refused > 0
    rc, dec = dev_decode(gpu_codec, payload, freq, L, n)
    assert rc == 0 and np.array_equal(dec, z)


def test_version_separation(gpu_codec):
    w, h, f = 16, 12, 2
    rgb = WO.smooth_plus_noise(w, h, f)
    enc = gpu_codec.FrameEncoder.with_wavelet(100, gpu_codec.WaveletType.Cdf97)
    v1, v2, v3 = enc.encode(rgb, w, h, f).to_bytes(), gpu_codec.encode_split(enc, rgb, w, h, f), gpu_codec.encode_wide(enc, rgb, w, h, f)
    assert [gpu_codec.alc_version(b) for b in (v1, v2, v3)] == [1, 2, 3]
    with pytest.raises(gpu_codec.CodecError, match=r"unsupported version: 3 \(expected 2\)"):
        gpu_codec.decode_split(v3)
    with pytest.raises(gpu_codec.CodecError, match=r"unsupported version: 3 \(expected 1\)"):
        gpu_codec.EncodedChunk.from_bytes(v3 + bytes(4000))
    for other, ver in ((v1, 1), (v2, 2)):
        with pytest.raises(gpu_codec.CodecError, match=rf"unsupported version: {ver} \(expected 3\)"):
            gpu_codec.decode_wide(other)
        with pytest.raises(gpu_codec.CodecError, match=rf"unsupported version: {ver} \(expected 3\)"):
            gpu_codec.wide_info(other)
    d_alc = torch.from_numpy(np.frombuffer(v2, np.uint8).copy()).to(DEV)
    d_rgb = torch.zeros(w * h * f * 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(gpu_codec.CodecError, match="unsupported version"):
        gpu_codec.wide_decode_device(d_alc.data_ptr(), len(v2), [len(v2)], d_rgb.data_ptr())
    assert int(d_rgb.count_nonzero()) == 0
    assert np.array_equal(gpu_codec.decode_alc(v2), gpu_codec.decode_split(v2))
    assert np.array_equal(gpu_codec.decode_alc(v1), gpu_codec.FrameDecoder().decode(gpu_codec.EncodedChunk.from_bytes(v1)))
