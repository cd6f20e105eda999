"""CPU-only checks of the split-stream format (.alc version 2): the normalisation rule and the round trip of the numpy
restatement (tests/split_ref.py), and the header validation of the C ABI, which is host code and needs no device: every
malformed field is InvalidBitstream, in the fixed order of DESIGN.md section 10.5."""
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_ref as R  # noqa: E402
import wide_ref as RW  # noqa: E402


def seeded_histograms():
    rng = np.random.default_rng(2)
    one = np.zeros(256, np.int64); one[200] = 7
    dominant = np.ones(256, np.int64); dominant[0] = 50_000_000
    # 56 equal symbols + 200 singletons: the floors sum to 56 * 73 + 200 = 4288; taking the excess of 192 from ONE symbol
    # would leave it negative, so the rule has to walk down the currently largest ones
    floor_heavy = np.ones(256, np.int64); floor_heavy[:56] = 1000
    out = [one, dominant, floor_heavy, np.zeros(256, np.int64)]
    for _ in range(40):
        h = (rng.pareto(0.6, 256) * rng.integers(1, 5000)).astype(np.int64)
        h[rng.random(256) < rng.random()] = 0
        out.append(h)
    return out


def test_normalisation_properties():
    for h in seeded_histograms():
        f = R.normalize(h).astype(np.int64)
        if h.sum() == 0:
            assert not f.any()
            continue
        assert f.sum() == 4096
        assert (f[h > 0] >= 1).all() and (f[h == 0] == 0).all()
        c = R.cumulative(f)
        assert c[0] == 0 and (np.diff(c) == f[:-1]).all() and c[-1] + f[-1] == 4096
    f = R.normalize(seeded_histograms()[2]).astype(np.int64)
    assert (f[56:] == 1).all() and f[:56].min() >= 69 and f[:56].max() - f[:56].min() <= 1
    f = R.normalize(seeded_histograms()[0])
    assert f[200] == 4096


@pytest.mark.parametrize("n,L", [(1, 64), (63, 64), (64 * 64, 64), (64 * 64 * 2 + 5, 64), (50_000, 256), (70_000, 16384)])
def test_split_ref_round_trips_its_own_streams(n, L):
    rng = np.random.default_rng(n)
    sym = rng.choice(256, n, p=rng.dirichlet(np.ones(256) * 0.05)).astype(np.uint8)
    freq = R.normalize(np.bincount(sym, minlength=256))
    pay = R.encode_channel(sym, freq, L)
    nb = R.n_blocks_of(n, L)
    # layout: block table, then per block 64 u16 and the lane streams; a lane of k symbols is at most 2 k + 4 bytes
    blen = np.frombuffer(pay, "<u4", nb)
    assert 4 * nb + int(blen.sum()) == len(pay)
    lens = np.frombuffer(pay, "<u2", 64, 4 * nb)
    assert int(lens.sum()) + 128 == int(blen[0]) and lens.max() <= 2 * L + 4
    if n < 64:
        assert (lens[n:] == 0).all() and (lens[:n] >= 4).all()
    dec, ok = R.decode_channel(pay, freq, L, n)
    assert ok and np.array_equal(dec, sym)
    assert not R.decode_channel(pay[:-1], freq, L, n)[1]


def starved_full_block(version):
    """(symbols, histogram, L): the longest lane stream a format can hold -- one full block plus 5 symbols at the largest
    lane length, every coded step at frequency 1.  Version 2: 12 bits per symbol, 16384 symbols per lane; version 3: 24 bits
    per symbol (escape and residual), 8192 per lane.  Either way a lane stream of 3 * 8192 + 4 = 24580 bytes."""
    L = 16384 if version == 2 else 8192
    n = 64 * L + 5
    hist = np.zeros(256, np.uint32)
    hist[3] = n - 1
    if version == 2:
        hist[7] = 1
        return np.full(n, 7, np.uint8), hist, L
    hist[255] = 1
    return np.full(n, 255 + 4095, np.uint16), hist, L


# version -> (largest lane directory entry, payload bytes, the stream bound)
LONGEST = {2: (24580, 1_573_409, 2_097_938), 3: (24580, 1_573_419, 2_097_948)}


def lane_directories(payload, n, L):
    """(block lengths, [n_blocks, 64] lane lengths) of a channel payload"""
    nb = R.n_blocks_of(n, L)
    blen = np.frombuffer(payload, "<u4", nb).astype(np.int64)
    boff = 4 * nb + np.cumsum(blen) - blen
    return blen, np.stack([np.frombuffer(payload, "<u2", 64, int(o)).astype(np.int64) for o in boff])


@pytest.mark.parametrize("version", [2, 3])
def test_longest_lane_stream_fits_its_directory_entry_and_the_bound(codec, version):
    """What tests/test_gpu_lane_fuzz.py runs on the device, pinned without one: with a histogram that starves the one symbol
    of the data, a full-length lane takes 24580 bytes -- below the 65536 of its u16 directory entry -- and the payload stays
    within the stream bound."""
    ref = R if version == 2 else RW
    sym, hist, L = starved_full_block(version)
    n = sym.size
    freq = ref.normalize(hist)
    assert freq[3] == 4095 and int(freq.max(initial=0, where=np.arange(256) != 3)) == 1
    pay = ref.encode_channel(sym, freq, L)
    lane, length, bound = LONGEST[version]
    got_bound = codec.split_stream_bound(n, L) if version == 2 else codec.wide_stream_bound(n, L)
    assert len(pay) == length <= bound == got_bound
    blen, dirs = lane_directories(pay, n, L)
    assert dirs.shape == (2, 64) and (dirs[0] == lane).all() and int(dirs.max()) == lane < 65536
    assert (dirs[1, :5] == (5 if version == 2 else 7)).all() and not dirs[1, 5:].any()
    assert (blen == dirs.sum(axis=1) + 128).all() and 4 * 2 + int(blen.sum()) == len(pay)
    dec, ok = ref.decode_channel(pay, freq, L, n)
    assert ok and np.array_equal(dec, sym)


def test_stage_encode_argument_checks_need_no_device(codec):
    """alice_codec_dev_split_encode / _dev_wide_encode answer a null argument, a bad lane_symbols, too many symbols and a
    histogram whose total is not n, in that order, before they look for a device (the pointers are never followed)."""
    lib = codec.load_library()
    somewhere = 0x1000
    hist = np.zeros(256, np.uint32)
    hist[5] = 100
    hp = hist.ctypes.data_as(C.POINTER(C.c_uint32))

    def call(fn, n, L, h=hp, sym=somewhere, out=somewhere, cap=1 << 20):
        got = C.c_uint64(77)
        rc = getattr(lib, fn)(sym, n, h, L, out, cap, C.byref(got), None)
        return rc, (lib.alice_codec_last_error_message() or b"").decode(), lib.alice_codec_last_error()

    for fn, top in (("alice_codec_dev_split_encode", 16384), ("alice_codec_dev_wide_encode", 8192)):
        rc, msg, last = call(fn, 101, 64)
        assert rc == last == 1 and msg == "the histogram counts 100 symbols, n is 101"
        rc, msg, _ = call(fn, 99, top)
        assert rc == 1 and msg == "the histogram counts 100 symbols, n is 99"
        rc, msg, _ = call(fn, 0, 0)
        assert rc == 1 and msg == "the histogram counts 100 symbols, n is 0"
        for L in (32, 96, 2 * top, 1 << 31):
            rc, msg, last = call(fn, 100, L)
            assert rc == last == 2 and f"[64, {top}]" in msg, (fn, L, msg)
        # the earlier check answers: lane_symbols before the total, too many symbols before the total, null before all
        assert call(fn, 101, 100)[0] == 2
        assert call(fn, 1 << 32, 64)[0] == 3 and call(fn, 1 << 32, 100)[0] == 2
        assert call(fn, 101, 100, sym=None)[0] == 9 and call(fn, 101, 100, h=None)[0] == 9
        assert call(fn, 101, 100, out=None)[0] == 9 and call(fn, 101, 100, out=None, cap=0)[0] == 2
        # an empty channel with an empty histogram is no payload, without a device
        empty = np.zeros(256, np.uint32)
        got = C.c_uint64(77)
        assert getattr(lib, fn)(None, 0, empty.ctypes.data_as(C.POINTER(C.c_uint32)), 64, None, 0, C.byref(got), None) == 0 and got.value == 0


def container(w=6, h=4, f=2, L=64, wavelet=1, seed=0):
    rng = np.random.default_rng(seed)
    pw, ph, pf = R.padded_dims(w, h, f)
    sym = [rng.choice(256, pw * ph * pf, p=rng.dirichlet(np.ones(256) * 0.1)).astype(np.uint8) for _ in range(3)]
    return R.write_container(wavelet, w, h, f, L, [13, 13, 13], sym), sym


def test_container_round_trip_in_split_ref():
    data, sym = container()
    info, dec = R.decode_container(data)
    assert info["lane_symbols"] == 64 and info["step"] == [13] * 3 and len(data) == R.HEADER + sum(info["payload_len"])
    for c in range(3):
        assert np.array_equal(dec[c], sym[c])


def info_rc(codec, data):
    lib = codec.load_library()
    buf = np.frombuffer(bytes(data), np.uint8)
    out = (C.c_uint8 * 256)()
    ptr = buf.ctypes.data_as(C.POINTER(C.c_uint8)) if buf.size else C.cast(C.c_char_p(b"\0"), C.POINTER(C.c_uint8))
    rc = lib.alice_codec_split_info(ptr, buf.size, C.cast(out, C.c_void_p))
    msg = lib.alice_codec_last_error_message()
    return rc, (msg or b"").decode()


def test_header_validation_needs_no_device_and_has_a_fixed_order(codec):
    data, _ = container()
    i = codec.split_info(data)
    assert (i.width, i.height, i.frames, i.lane_symbols, i.wavelet_type) == (6, 4, 2, 64, codec.WaveletType.Cdf97)
    assert i.quant_step == [13] * 3 and i.num_symbols == [48] * 3 and i.n_blocks == [1] * 3
    assert sum(i.payload_len) + codec.SPLIT_HEADER_BYTES == len(data) == sum(i.payload_len) + R.HEADER

    def patched(off, fmt, value, base=data):
        b = bytearray(base)
        struct.pack_into(fmt, b, off, value)
        return bytes(b)

    ch = R.FIXED   # first channel header
    # each entry breaks one field; the list is in the order the checks run, and an entry also carries every LATER defect
    # of the list before it was added, so the message proves the order
    defects = [
        ("data too short for the fixed fields", lambda b: b[:10]),
        ("bad magic", lambda b: b"ALCD" + b[4:]),
        ("unsupported version", lambda b: patched(4, "<B", 3, b)),
        ("unknown wavelet", lambda b: patched(5, "<B", 3, b)),
        ("lane_symbols", lambda b: patched(18, "<I", 96, b)),
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
        # with every later defect present as well, the earlier check still answers first
        if word.startswith("data too short"):
            continue
        b = data
        for later_word, later in reversed(defects[k + 1:]):
            b = later(b)
        rc, msg = info_rc(codec, breaker(b))
        assert rc == 4 and word in msg, (word, msg)
    # a step below 1 and a negative dead zone, on any channel
    for off, v in ((ch, -3), (ch + 4, -1), (ch + R.CHANNEL, 0), (ch + 2 * R.CHANNEL + 4, -7)):
        rc, msg = info_rc(codec, patched(off, "<i", v))
        assert rc == 4 and "quantiser step" in msg
        with pytest.raises(R.InvalidBitstream):
            R.parse_container(patched(off, "<i", v))
    assert info_rc(codec, patched(ch + 4, "<i", 0))[0] == 0     # a dead zone of 0 is a quantiser
    # lane_symbols out of range on both sides and not a power of two
    for L in (0, 32, 32768, 100):
        assert info_rc(codec, patched(18, "<I", L))[0] == 4
    # num_symbols is compared in 64 bits: 65536 x 65536 x 2 pads to 2^33 symbols, which no u32 field equals
    rc, msg = info_rc(codec, patched(6, "<I", 65536, patched(10, "<I", 65536)))
    assert rc == 4 and "num_symbols" in msg
    # split_ref refuses every one of them too
    for word, breaker in defects:
        with pytest.raises(R.InvalidBitstream):
            R.parse_container(breaker(data))
    # decode runs the same checks before it looks for a device
    lib = codec.load_library()
    n = C.c_uint64(5)
    bad = np.frombuffer(defects[9][1](data), np.uint8)
    assert not lib.alice_codec_decode_split(bad.ctypes.data_as(C.POINTER(C.c_uint8)), bad.size, C.byref(n))
    assert lib.alice_codec_last_error() == 4 and n.value == 5


def test_v1_parser_still_refuses_a_v2_file(codec):
    data, _ = container()
    with pytest.raises(codec.CodecError, match=r"unsupported version: 2 \(expected 1\)"):
        codec.EncodedChunk.from_bytes(data + bytes(4000))
    assert codec.alc_version(data) == 2


def test_empty_chunk_and_argument_checks(codec):
    lib = codec.load_library()
    enc = codec.FrameEncoder.with_wavelet(80, codec.WaveletType.Cdf97)
    # an empty chunk is its header, on the host (as alice_codec_encode64 answers it without a device)
    b = codec.encode_split(enc, np.zeros(0, np.uint8), 0, 4, 4)
    assert len(b) == codec.SPLIT_HEADER_BYTES
    i = codec.split_info(b)
    assert i.num_symbols == [0] * 3 and i.n_blocks == [0] * 3 and i.payload_len == [0] * 3 and i.lane_symbols == 512
    assert codec.decode_split(b).size == 0
    info, sym = R.decode_container(b)
    assert all(s.size == 0 for s in sym)
    # alice_codec_encode64's validation, in its order, then lane_symbols
    rgb = np.zeros(4 * 4 * 2 * 3, np.uint8)
    with pytest.raises(codec.CodecError) as e:
        codec.encode_split(enc, rgb[:-1], 4, 4, 2)
    assert e.value.code == 1
    with pytest.raises(codec.CodecError) as e:
        codec.encode_split(enc, rgb[:-1], 4, 4, 2, 100)     # the buffer is checked before lane_symbols
    assert e.value.code == 1
    with pytest.raises(codec.CodecError) as e:
        codec.encode_split(enc, rgb, 4, 4, 2, 100)
    assert e.value.code == 2
    n = C.c_uint64(9)
    assert not lib.alice_codec_encode_split(None, None, 0, 0, 0, 0, 0, C.byref(n)) and lib.alice_codec_last_error() == 9 and n.value == 9
    assert codec.split_stream_bound(1000, 96) == 0 and codec.split_stream_bound(1000, 64) >= 2 * 1000 + 4 * 64 + 132
    if codec.device_count() < 1:   # without a device the compute calls fail loudly
        with pytest.raises(codec.CodecError) as e:
            codec.encode_split(enc, rgb, 4, 4, 2)
        assert e.value.code == 8
        with pytest.raises(codec.CodecError) as e:
            codec.normalized_frequencies(np.ones(256))
        assert e.value.code == 8
        data, _ = container()
        with pytest.raises(codec.CodecError) as e:
            codec.decode_split(data)
        assert e.value.code == 8


def test_cpp_mirror_host_checks_match_python(codec, tmp_path):
    """include/alice_codec.hpp: split_info, the validation order, alc_version, split_stream_bound -- tests/cpp/test_cpp_split.cpp
    built with g++ against the library, its lines compared with the same questions put to the Python mirror."""
    import subprocess
    data, _ = container(10, 6, 3, 128, 2, seed=4)
    empty = codec.encode_split(codec.FrameEncoder.with_wavelet(37, codec.WaveletType.Haar), np.zeros(0, np.uint8), 5, 0, 2, 2048)
    ch = R.FIXED

    def patched(off, fmt, value):
        b = bytearray(data)
        struct.pack_into(fmt, b, off, value)
        return bytes(b)

    files = [data, empty, data[:10], b"ALCD" + data[4:], patched(4, "<B", 1), patched(5, "<B", 9), patched(18, "<I", 100), data[:900],
             patched(ch + R.CHANNEL, "<i", 0), patched(ch + 8, "<I", 1), patched(ch + 2 * R.CHANNEL + 12, "<I", 0),
             patched(ch + 24 + 2 * 255, "<H", 9), patched(ch + 16, "<Q", 7), data + b"x",
             patched(R.HEADER, "<I", struct.unpack_from("<I", data, R.HEADER)[0] + 1),
             # two defects: the earlier check answers
             patched(4, "<B", 3)[:900], (b"ALCD" + patched(18, "<I", 5)[4:])]
    paths = []
    for k, b in enumerate(files):
        p = tmp_path / f"f{k}.alc"
        p.write_bytes(b)
        paths.append(str(p))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "alice-codec_amd")
    exe = str(tmp_path / "test_cpp_split")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "test_cpp_split.cpp"), "-L", libdir, "-lalice_codec",
                           "-Wl,-rpath," + libdir, "-o", exe])
    env = dict(os.environ, LD_LIBRARY_PATH=libdir + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    out = subprocess.run([exe] + paths, env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    want = [f"bound {codec.split_stream_bound(1000, 64)} {codec.split_stream_bound(1000, 96)} {codec.split_stream_bound(132710400)}",
            f"consts {codec.SPLIT_DEFAULT_LANE_SYMBOLS} {codec.SPLIT_HEADER_BYTES}"]
    n_ok = 0
    for k, b in enumerate(files, 1):
        head = f"file {k} version {codec.alc_version(b)}: "
        try:
            i = codec.split_info(b)
            n_ok += 1
            want.append(head + f"{i.width}x{i.height}x{i.frames} L={i.lane_symbols} wavelet={int(i.wavelet_type)}" + "".join(
                f" [{i.quant_step[c]} {i.dead_zone[c]} {i.num_symbols[c]} {i.n_blocks[c]} {i.payload_len[c]}]" for c in range(3)))
        except codec.CodecError as e:
            want.append(head + f"error {e.code}: {str(e).split(': ', 1)[1]}")
        try:
            codec.EncodedChunk.from_bytes(b)
            want.append(f"file {k} v1: accepted")
        except codec.CodecError as e:
            want.append(f"file {k} v1: error {e.code}")
    assert n_ok == 2 and all("v1: error 4" in w for w in want if " v1: " in w)
    assert out.stdout.splitlines() == want
