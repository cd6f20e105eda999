"""CPU-only checks of the wide format (.alc version 3): the round trip of the numpy restatement
(tests/wide_ref.py) around the block and lane boundaries and at every escape share, the header validation of the C ABI in
its fixed order, the separation of the three parsers, and the reason the format exists: at the top of the quality scale the
u8 symbol map of versions 1 and 2 wraps, the wide map does not."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_ref as R2  # noqa: E402
import wide_oracle as WO  # noqa: E402
import wide_ref as R  # noqa: E402


def seeded_symbols(n, share, seed):
    """n wide symbols of which about `share` are escapes (z >= 255); share 0: none, share 1: all."""
    rng = np.random.default_rng(seed)
    small = rng.choice(255, n, p=rng.dirichlet(np.ones(255) * 0.2)).astype(np.int64)
    big = 255 + rng.integers(0, 4096, n)
    z = np.where(rng.random(n) < share, big, small)
    if share >= 1:
        z = big
    return z.astype(np.uint16)


CASES = [(1, 64), (37, 64), (64, 64), (64 * 64 * 3 + 17, 64), (64 * 8192 + 700, 8192)]


@pytest.mark.parametrize("n,L", CASES)
@pytest.mark.parametrize("share", [0.0, 0.05, 1.0])
def test_wide_ref_round_trip(n, L, share):
    z = seeded_symbols(n, share, seed=n + int(share * 100))
    if n > 64 and share > 0:
        # an escape as the first and as the last symbol of a lane, with the smallest and the largest residual
        z[0] = 255; z[1] = 255 + 4095
        z[n - 1] = 255 + 4095; z[n - 2] = 255
        lane0_last = ((min(n, 64 * L) - 1) // 64) * 64
        z[lane0_last] = 255 + 4095
    freq = R.normalize(R.histogram(z))
    pay = R.encode_channel(z, freq, L)
    assert len(pay) <= R.stream_bound(n, L)
    dec, ok = R.decode_channel(pay, freq, L, n)
    assert ok and np.array_equal(dec, z)
    assert not R.decode_channel(pay[:-1], freq, L, n)[1]
    if share == 0:
        # without an escape the payload is version 2's of the same symbols
        assert pay == R2.encode_channel(z.astype(np.uint8), freq, L)


def test_residual_bounds_in_wide_ref():
    z = np.array([255, 255 + 4095, 0, 3], np.uint16)
    freq = R.normalize(R.histogram(z))
    pay = R.encode_channel(z, freq, 64)
    dec, ok = R.decode_channel(pay, freq, 64, 4)
    assert ok and dec.tolist() == z.tolist()
    with pytest.raises(ValueError):
        R.encode_channel(np.array([255 + 4096], np.uint16), R.normalize(R.histogram([300])), 64)
    # the symbol map
    q = np.array([0, 1, -1, 127, -128, 128, 2040, -2040])
    assert R.wide_symbols(q).tolist() == [0, 1, 2, 253, 256, 255, 4079, 4080]
    assert R.from_wide_symbols(R.wide_symbols(q)).tolist() == q.tolist()


def container(w=6, h=4, f=2, L=64, wavelet=1, seed=0):
    pw, ph, pf = R.padded_dims(w, h, f)
    sym = [seeded_symbols(pw * ph * pf, 0.1, seed + c) for c in range(3)]
    return R.write_container(wavelet, w, h, f, L, [13, 13, 13], sym), sym


def test_container_round_trip_in_wide_ref():
    data, sym = container()
    info, dec = R.decode_container(data)
    assert data[4] == 3 and info["lane_symbols"] == 64 and len(data) == R.HEADER + sum(info["payload_len"])
    for c in range(3):
        assert np.array_equal(dec[c], sym[c])


def info_rc(codec, data, fn="alice_codec_wide_info"):
    lib = codec.load_library()
    buf = np.frombuffer(bytes(data), np.uint8)
    out = (C.c_uint8 * 256)()
    ptr = buf.ctypes.data_as(C.POINTER(C.c_uint8)) if buf.size else C.cast(C.c_char_p(b"\0"), C.POINTER(C.c_uint8))
    rc = getattr(lib, fn)(ptr, buf.size, C.cast(out, C.c_void_p))
    msg = lib.alice_codec_last_error_message()
    return rc, (msg or b"").decode()


def test_wide_info_validation_has_the_fixed_order(codec):
    data, _ = container()
    i = codec.wide_info(data)
    assert (i.width, i.height, i.frames, i.lane_symbols, i.wavelet_type) == (6, 4, 2, 64, codec.WaveletType.Cdf97)
    assert i.quant_step == [13] * 3 and i.num_symbols == [48] * 3 and i.n_blocks == [1] * 3
    assert sum(i.payload_len) + codec.SPLIT_HEADER_BYTES == len(data)

    def patched(off, fmt, value, base=data):
        b = bytearray(base)
        struct.pack_into(fmt, b, off, value)
        return bytes(b)

    ch = R.FIXED
    # in the order the checks run; an entry is also tried with every LATER defect present, so the message proves the order
    defects = [
        ("data too short for the fixed fields", lambda b: b[:10]),
        ("bad magic", lambda b: b"ALCD" + b[4:]),
        ("unsupported version: 2 (expected 3)", lambda b: patched(4, "<B", 2, b)),
        ("unknown wavelet", lambda b: patched(5, "<B", 3, b)),
        ("lane_symbols 16384", lambda b: patched(18, "<I", 16384, b)),
        ("data too short for the header", lambda b: b[:800]),
        ("quantiser step", lambda b: patched(ch, "<i", 0, b)),
        ("num_symbols", lambda b: patched(ch + 8, "<I", 47, b)),
        ("n_blocks", lambda b: patched(ch + 12, "<I", 2, b)),
        ("frequencies sum", lambda b: patched(ch + 24, "<H", struct.unpack_from("<H", b, ch + 24)[0] + 1, b)),
        ("payload_len", lambda b: patched(ch + 16, "<Q", 100, b)),
        ("length mismatch", lambda b: b + b"\0"),
        ("block lengths", lambda b: patched(R.HEADER, "<I", struct.unpack_from("<I", b, R.HEADER)[0] - 1, b)),
    ]
    for k, (word, breaker) in enumerate(defects):
        rc, msg = info_rc(codec, breaker(data))
        assert rc == 4 and word in msg, (word, msg)
        if word.startswith("data too short"):
            continue
        b = data
        for later_word, later in reversed(defects[k + 1:]):
            b = later(b)
        rc, msg = info_rc(codec, breaker(b))
        assert rc == 4 and word in msg, (word, msg)
    for word, breaker in defects:
        with pytest.raises(R.InvalidBitstream):
            R.parse_container(breaker(data))
    # the lane range of version 3: 8192 is the last accepted length (the n_blocks check answers next: 1 block either way)
    for L, ok in ((0, False), (32, False), (100, False), (8192, True), (16384, False), (32768, False)):
        rc, msg = info_rc(codec, patched(18, "<I", L))
        assert (rc == 0) == ok, (L, rc, msg)
        assert ok or "[64, 8192]" in msg
    rc, msg = info_rc(codec, patched(4, "<B", 1))
    assert rc == 4 and "unsupported version: 1 (expected 3)" in msg
    # decode runs the same checks before it looks for a device
    lib = codec.load_library()
    n = C.c_uint64(5)
    bad = np.frombuffer(defects[9][1](data), np.uint8)
    assert not lib.alice_codec_decode_wide(bad.ctypes.data_as(C.POINTER(C.c_uint8)), bad.size, C.byref(n))
    assert lib.alice_codec_last_error() == 4 and n.value == 5


def test_the_three_parsers_keep_apart(codec):
    v3, _ = container()
    v2 = bytes(bytearray(v3[:4]) + b"\x02" + bytearray(v3[5:]))
    rc, msg = info_rc(codec, v3, "alice_codec_split_info")
    assert rc == 4 and "unsupported version: 3 (expected 2)" in msg
    with pytest.raises(codec.CodecError, match=r"unsupported version: 3 \(expected 1\)"):
        codec.EncodedChunk.from_bytes(v3 + bytes(4000))
    with pytest.raises(codec.CodecError, match=r"unsupported version: 2 \(expected 3\)"):
        codec.wide_info(v2)
    v1 = codec.FrameEncoder.with_wavelet(50, codec.WaveletType.Haar).encode(np.zeros(0, np.uint8), 0, 3, 3).to_bytes()
    with pytest.raises(codec.CodecError, match=r"unsupported version: 1 \(expected 3\)"):
        codec.wide_info(v1)
    with pytest.raises(codec.CodecError, match=r"unsupported version: 1 \(expected 3\)"):
        codec.decode_wide(v1)
    assert codec.alc_version(v3) == 3
    # decode_alc dispatches on the version byte: each refusal below is worded by the parser of that version
    for blob, want in ((v3[:900], "expected 3"), (v2[:900], "expected 2")):
        with pytest.raises(codec.CodecError) as e:
            codec.decode_alc(bytes(blob[:5]) + b"\x07" + bytes(blob[6:]))   # a wavelet byte no parser accepts
        assert "unknown wavelet" in str(e.value)
    assert codec.decode_alc(v1).size == 0


def test_empty_chunk_and_argument_checks(codec):
    lib = codec.load_library()
    enc = codec.FrameEncoder.with_wavelet(100, codec.WaveletType.Cdf97)
    b = codec.encode_wide(enc, np.zeros(0, np.uint8), 0, 4, 4)
    assert len(b) == codec.SPLIT_HEADER_BYTES and b[4] == 3
    i = codec.wide_info(b)
    assert i.num_symbols == [0] * 3 and i.n_blocks == [0] * 3 and i.payload_len == [0] * 3 and i.lane_symbols == 512
    assert i.quant_step == [1] * 3
    assert codec.decode_wide(b).size == 0 and codec.decode_alc(b).size == 0
    info, sym = R.decode_container(b)
    assert all(s.size == 0 for s in sym)
    rgb = np.zeros(4 * 4 * 2 * 3, np.uint8)
    for args, code in (((rgb[:-1], 4, 4, 2), 1), ((rgb[:-1], 4, 4, 2, 100), 1), ((rgb, 4, 4, 2, 100), 2), ((rgb, 4, 4, 2, 16384), 2)):
        with pytest.raises(codec.CodecError) as e:
            codec.encode_wide(enc, *args)
        assert e.value.code == code
    n = C.c_uint64(9)
    assert not lib.alice_codec_encode_wide(None, None, 0, 0, 0, 0, 0, C.byref(n)) and lib.alice_codec_last_error() == 9 and n.value == 9
    assert codec.wide_stream_bound(1000, 96) == 0 and codec.wide_stream_bound(1000, 16384) == 0
    for n_sym, L in ((1000, 64), (64 * 8192 + 700, 8192), (1, 8192)):
        assert codec.wide_stream_bound(n_sym, L) == R.stream_bound(n_sym, L)
    if codec.device_count() < 1:   # without a device the compute calls fail loudly
        with pytest.raises(codec.CodecError) as e:
            codec.encode_wide(enc, rgb, 4, 4, 2)
        assert e.value.code == 8
        data, _ = container()
        with pytest.raises(codec.CodecError) as e:
            codec.decode_wide(data)
        assert e.value.code == 8


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_fidelity_statement(oracle_mod, kind):
    """decode(encode(x)) against x on 64x48x8 smooth-plus-noise content, u8 symbol map against the wide one."""
    import oracle.alice_oracle_np as o
    w, h, f = 64, 48, 8
    rgb = WO.smooth_plus_noise(w, h, f)
    out = {}
    for q in (100, 80):
        step, dims, qs = WO.forward_quantised(o, rgb, w, h, f, q, kind)
        z = [R.wide_symbols(v) for v in qs]
        share = sum(int((zz >= 255).sum()) for zz in z) / sum(zz.size for zz in z)
        narrow = WO.inverse_quantised(o, [o.from_symbols(o.to_symbols(v)) for v in qs], step, dims, w, h, f, kind)
        wide = WO.inverse_quantised(o, [R.from_wide_symbols(zz) for zz in z], step, dims, w, h, f, kind)
        out[q] = (share, WO.psnr(rgb, narrow), WO.psnr(rgb, wide), np.array_equal(narrow, wide))
        print(f"wavelet {kind} q={q}: share of z >= 255 {share:.4f}, PSNR u8 symbols {out[q][1]:.2f} dB, wide symbols {out[q][2]:.2f} dB")
    assert out[100][0] > 0
    assert out[100][2] > out[100][1]
    assert out[80][3]


def test_cpp_mirror_host_checks_match_python(codec, tmp_path):
    """include/alice_codec.hpp: wide_info, its validation order, wide_stream_bound -- tests/cpp/test_cpp_wide.cpp built with g++
    against the library, its lines compared with the same questions put to the Python mirror."""
    data, _ = container(10, 6, 3, 128, 2, seed=4)
    empty = codec.encode_wide(codec.FrameEncoder.with_wavelet(37, codec.WaveletType.Haar), np.zeros(0, np.uint8), 5, 0, 2, 2048)
    ch = R.FIXED

    def patched(off, fmt, value):
        b = bytearray(data)
        struct.pack_into(fmt, b, off, value)
        return bytes(b)

    files = [data, empty, data[:10], b"ALCD" + data[4:], patched(4, "<B", 2), patched(4, "<B", 1), patched(5, "<B", 9), patched(18, "<I", 16384),
             data[:900], patched(ch + R.CHANNEL, "<i", 0), patched(ch + 8, "<I", 1), patched(ch + 2 * R.CHANNEL + 12, "<I", 0),
             patched(ch + 24 + 2 * 255, "<H", 9), patched(ch + 16, "<Q", 7), data + b"x",
             patched(R.HEADER, "<I", struct.unpack_from("<I", data, R.HEADER)[0] + 1),
             patched(4, "<B", 2)[:900], (b"ALCD" + patched(18, "<I", 5)[4:])]
    paths = []
    for k, b in enumerate(files):
        p = tmp_path / f"f{k}.alc"
        p.write_bytes(b)
        paths.append(str(p))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "alice-codec_amd")
    exe = str(tmp_path / "test_cpp_wide")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "test_cpp_wide.cpp"), "-L", libdir, "-lalice_codec",
                           "-Wl,-rpath," + libdir, "-o", exe])
    env = dict(os.environ, LD_LIBRARY_PATH=libdir + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    out = subprocess.run([exe] + paths, env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    want = [f"bound {codec.wide_stream_bound(1000, 64)} {codec.wide_stream_bound(1000, 96)} {codec.wide_stream_bound(1000, 16384)} "
            f"{codec.wide_stream_bound(132710400)}", f"consts {codec.WIDE_MAX_LANE_SYMBOLS}"]
    n_ok = 0
    for k, b in enumerate(files, 1):
        head = f"file {k} version {codec.alc_version(b)}: "
        try:
            i = codec.wide_info(b)
            n_ok += 1
            want.append(head + f"{i.width}x{i.height}x{i.frames} L={i.lane_symbols} wavelet={int(i.wavelet_type)}" + "".join(
                f" [{i.quant_step[c]} {i.dead_zone[c]} {i.num_symbols[c]} {i.n_blocks[c]} {i.payload_len[c]}]" for c in range(3)))
        except codec.CodecError as e:
            want.append(head + f"error {e.code}: {str(e).split(': ', 1)[1]}")
        for name, fn in (("v2", codec.split_info), ("v1", codec.EncodedChunk.from_bytes)):
            try:
                fn(b)
                want.append(f"file {k} {name}: accepted")
            except codec.CodecError as e:
                want.append(f"file {k} {name}: error {e.code}")
    assert n_ok == 2 and all(": error 4" in w for w in want if " v1: " in w)
    assert sum(" v2: accepted" in w for w in want) == 1     # the one whose version byte was patched to 2
    assert out.stdout.splitlines() == want
