"""CPU-only checks of the banded format (.alc version 5): the numpy restatement (tests/banded_ref.py)
round-trips to the base version's pixels and repacks byte for byte; the library's host validation refuses every damaged
header with its own message, in the order of section 20.3; the parsers of versions 1 to 5 keep apart; and the size
condition the format exists for holds at chunk size and fails, as documented, at thumbnail size."""
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import banded_ref as B  # noqa: E402
import wide_oracle as WO  # noqa: E402

CDF53, CDF97, HAAR = 0, 1, 2
SHAPES = [(64, 48, 8), (33, 17, 5), (7, 3, 1), (1, 1, 1)]


def clip(w, h, f):
    return WO.smooth_plus_noise(w, h, f)


@pytest.mark.parametrize("kind", [CDF53, CDF97, HAAR])
@pytest.mark.parametrize("shape", SHAPES)
def test_reference_round_trips_and_repacks(shape, kind):
    w, h, f = shape
    rgb = clip(w, h, f)
    for base in (2, 3, 4):
        q = 100 if base == 4 else 80
        plain = B.encode_base(rgb, w, h, f, q, kind, base, 64)
        banded = B.encode(rgb, w, h, f, q, kind, base, 64)
        info = B.parse_container(banded)
        assert banded[4] == 5 and info["base"] == base and len(info["payload"]) == 24
        assert B.HEADER + sum(info["payload_len"]) == len(banded)
        pix = B.decode(banded)
        assert np.array_equal(pix, B.decode_base(plain)), (shape, kind, base)
        if base == 4:
            assert np.array_equal(pix, rgb), (shape, kind)
        assert B.to_banded(plain) == banded, (shape, kind, base)
        assert B.from_banded(banded) == plain, (shape, kind, base)
        if shape == (33, 17, 5):     # a changed L on the way, and back
            assert B.to_banded(plain, 128) == B.encode(rgb, w, h, f, q, kind, base, 128)
            assert B.from_banded(B.to_banded(plain, 128), 64) == plain


def test_band_order_is_the_raster_of_each_box():
    pw, ph, pf = 6, 4, 2
    v = np.arange(pw * ph * pf, dtype=np.uint16)
    bands = B.gather_bands(v, pw, ph, pf)
    assert [b.size for b in bands] == [6] * 8
    assert bands[0].tolist() == [0, 1, 2, 6, 7, 8] and bands[1].tolist() == [3, 4, 5, 9, 10, 11]
    assert bands[2][0] == 12 and bands[4][0] == 24 and bands[7].tolist() == [39, 40, 41, 45, 46, 47]
    assert np.array_equal(B.scatter_bands(bands, pw, ph, pf, np.uint16), v)


# ---- validation (20.3) ----
def small(base=2, L=64):
    w, h, f = 6, 4, 2
    return B.encode(clip(w, h, f), w, h, f, 80, CDF53, base, L)


def info_rc(codec, data, fn="alice_codec_banded_info"):
    lib = codec.load_library()
    buf = np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(1, np.uint8)
    out = (C.c_uint8 * 512)()
    rc = getattr(lib, fn)(buf.ctypes.data_as(C.POINTER(C.c_uint8)), len(data), C.cast(out, C.c_void_p))
    return rc, (lib.alice_codec_last_error_message() or b"").decode()


def patched(blob, at, value: bytes):
    d = bytearray(blob)
    d[at:at + len(value)] = value
    return bytes(d)


def band_at(c, k):
    return B.FIXED + c * B.CHANNEL + 12 + k * B.BAND


def u32(v):
    return struct.pack("<I", v)


# (name of the reference's check, patch, the library's message) in the order of section 20.3
def failures(blob):
    ch = B.FIXED + B.CHANNEL           # channel 1
    last = band_at(2, 7)
    pay0 = B.HEADER                    # band 0's block-length table (one block at this size)
    return [
        ("fixed length", blob[:23], "too short for the fixed fields"),
        ("magic", patched(blob, 0, b"ALCX"), "bad magic"),
        ("version", patched(blob, 4, b"\x06"), "unsupported version: 6 (expected 5)"),
        ("wavelet", patched(blob, 5, b"\x03"), "unknown wavelet type byte: 3"),
        ("base", patched(blob, 22, b"\x05"), "unknown base version: 5"),
        ("base", patched(blob, 22, b"\x01"), "unknown base version: 1"),
        ("reserved", patched(blob, 23, b"\x01"), "reserved byte is 1"),
        ("lane_symbols", patched(blob, 18, u32(96)), "lane_symbols 96 is not a power of two in [64, 16384]"),
        ("lane_symbols", patched(blob, 18, u32(32768)), "lane_symbols 32768"),
        ("header length", blob[:B.HEADER - 1], "too short for the header"),
        ("channel 0: quantiser step", patched(blob, B.FIXED, u32(0)), "channel 0: quantiser step 0"),
        ("channel 0: num_symbols", patched(blob, B.FIXED + 8, u32(47)), "channel 0: num_symbols 47 != padded_pixels 48"),
        ("channel 0 band 3: n_blocks", patched(blob, band_at(0, 3), u32(2)), "channel 0 band 3: n_blocks 2"),
        ("channel 1: quantiser step", patched(blob, ch + 4, struct.pack("<i", -1)), "channel 1: quantiser step 14 / dead zone -1"),
        ("channel 2 band 7: frequency sum", patched(blob, last + 12, b"\xff\xff"), "channel 2 band 7: frequencies sum to"),
        ("channel 2 band 7: payload_len", patched(blob, last + 4, struct.pack("<Q", 131)), "channel 2 band 7: payload_len 131"),
        ("total length", blob + b"\x00", "length mismatch"),
        ("total length", blob[:-1], "length mismatch"),
        ("channel 0 band 0: block lengths", patched(blob, pay0, u32(127)), "channel 0 band 0: block 0 is shorter"),
        ("channel 0 band 0: block lengths", patched(blob, pay0, u32(129)), "channel 0 band 0: block lengths sum to"),
    ]


def test_every_validation_failure_has_its_own_message(codec):
    blob = small()
    rc, msg = info_rc(codec, blob)
    assert rc == 0, msg
    for name, bad, words in failures(blob):
        with pytest.raises(B.InvalidBitstream) as e:
            B.parse_container(bad)
        assert str(e.value) == name, (name, str(e.value))
        rc, msg = info_rc(codec, bad)
        assert rc == 4 and words in msg, (name, rc, msg)
        # the decode, the repack and the automatic format run the same checks before they look for a device
        for fn in (codec.decode_banded, codec.from_banded, codec.decode_alc):
            if name == "version" and fn is codec.decode_alc:
                continue                          # byte 4 sends the file to another parser
            with pytest.raises(codec.CodecError) as ce:
                fn(bad)
            assert ce.value.code == 4 and words in str(ce.value), (name, fn.__name__, str(ce.value))
    # the wide range for bases 3 and 4
    for base in (3, 4):
        rc, msg = info_rc(codec, patched(small(base), 18, u32(16384)))
        assert rc == 4 and "[64, 8192]" in msg, msg
    assert info_rc(codec, patched(small(2), 18, u32(16384)))[0] == 0      # base 2 takes 16384 (one block either way at this size)


def test_the_first_applicable_check_wins(codec):
    blob = small()
    cases = failures(blob)
    # every later damage added to an earlier one leaves the earlier message: patch pairs (i, j), i < j, of header fields
    header_only = [c for c in cases if len(c[1]) == len(blob) and c[0] not in ("total length",)]
    for i in range(len(header_only)):
        for j in range(i + 1, len(header_only)):
            (name_i, bad_i, words_i), (name_j, bad_j, _) = header_only[i], header_only[j]
            if name_i == name_j:
                continue
            both = bytearray(bad_i)
            for at in range(len(blob)):
                if bad_j[at] != blob[at]:
                    both[at] = bad_j[at]
            if bytes(both) == bad_i or any(bad_i[at] != blob[at] and bad_j[at] != blob[at] for at in range(B.HEADER + 4)):
                continue
            rc, msg = info_rc(codec, bytes(both))
            assert rc == 4 and words_i in msg, (name_i, name_j, msg)
            with pytest.raises(B.InvalidBitstream) as e:
                B.parse_container(bytes(both))
            assert str(e.value) == name_i, (name_i, name_j, str(e.value))
    # a truncated file with a bad magic is still "too short" below 24 bytes, and "bad magic" from 24 on
    assert "too short for the fixed fields" in info_rc(codec, b"XXXX" + blob[4:20])[1]
    assert "bad magic" in info_rc(codec, b"XXXX" + blob[4:24])[1]


def test_the_parsers_keep_apart(codec):
    v5 = small(3)
    i = codec.banded_info(v5)
    assert (i.width, i.height, i.frames, i.lane_symbols, i.base, int(i.wavelet_type)) == (6, 4, 2, 64, 3, CDF53)
    assert i.num_symbols == [48] * 3 and i.n_blocks == [1] * 24 and sum(i.payload_len) + codec.BANDED_HEADER_BYTES == len(v5)
    assert codec.BANDED_HEADER_BYTES == B.HEADER == 12636 and codec.alc_version(v5) == 5
    # the parsers of versions 1 to 4 and the partial calls refuse version 5 ...
    for fn, ver in (("alice_codec_split_info", 2), ("alice_codec_wide_info", 3), ("alice_codec_reversible_info", 4)):
        rc, msg = info_rc(codec, v5, fn)
        assert rc == 4 and f"unsupported version: 5 (expected {ver})" in msg, msg
    with pytest.raises(codec.CodecError, match=r"unsupported version: 5 \(expected 1\)"):
        codec.EncodedChunk.from_bytes(v5)
    for fn, ver in ((codec.decode_split, 2), (codec.decode_wide, 3), (codec.decode_reversible, 4)):
        with pytest.raises(codec.CodecError, match=rf"unsupported version: 5 \(expected {ver}\)"):
            fn(v5)
    for call in (lambda: codec.transcode(v5, 50), lambda: codec.to_banded(v5)):
        with pytest.raises(codec.CodecError, match="unsupported version: 5"):
            call()
    # ... and the version 5 parser refuses 1 to 4
    w, h, f = 6, 4, 2
    v1 = codec.FrameEncoder.with_wavelet(50, codec.WaveletType.Haar).encode(np.zeros(0, np.uint8), 0, 3, 3).to_bytes()
    others = {1: v1 + bytes(64), 2: B.encode_base(clip(w, h, f), w, h, f, 80, CDF53, 2, 64), 3: B.encode_base(clip(w, h, f), w, h, f, 80, CDF53, 3, 64),
              4: B.encode_base(clip(w, h, f), w, h, f, 100, CDF53, 4, 64)}
    for ver, blob in others.items():
        rc, msg = info_rc(codec, blob)
        assert rc == 4 and f"unsupported version: {ver} (expected 5)" in msg, msg
        for fn in (codec.decode_banded, codec.from_banded):
            with pytest.raises(codec.CodecError, match=rf"unsupported version: {ver} \(expected 5\)"):
                fn(blob)
        with pytest.raises(B.InvalidBitstream):
            B.parse_container(blob)


def test_empty_chunk_and_argument_checks(codec):
    lib = codec.load_library()
    enc = codec.FrameEncoder.with_wavelet(50, codec.WaveletType.Cdf97)
    none = np.zeros(0, np.uint8)
    for base in (2, 3, 4):
        b = codec.encode_banded(enc, none, 0, 4, 4, 0, base)
        assert len(b) == 12636 and b == B.encode(none, 0, 4, 4, 50, CDF97, base, 512)
        i = codec.banded_info(b)
        assert i.base == base and i.num_symbols == [0] * 3 and i.payload_len == [0] * 24 and i.n_blocks == [0] * 24 and i.quant_step == [33] * 3
        assert codec.decode_banded(b).size == 0 and codec.decode_alc(b).size == 0
        plain = {2: codec.encode_split, 3: codec.encode_wide, 4: codec.encode_reversible}[base](enc, none, 0, 4, 4)
        assert codec.to_banded(plain) == b and codec.from_banded(b) == plain
        assert codec.to_banded(plain, 64) == B.encode(none, 0, 4, 4, 50, CDF97, base, 64)
    rgb = np.zeros(4 * 4 * 2 * 3, np.uint8)
    # encode_split's order (buffer size: 1), then base (2), then lane_symbols against the base's range (2)
    for args, code, words in (((rgb[:-1], 4, 4, 2, 100, 9), 1, "buffer size"), ((rgb, 4, 4, 2, 100, 9), 2, "base 9"),
                              ((rgb, 4, 4, 2, 100, 2), 2, "[64, 16384]"), ((rgb, 4, 4, 2, 16384, 3), 2, "[64, 8192]")):
        with pytest.raises(codec.CodecError) as e:
            codec.encode_banded(enc, *args)
        assert e.value.code == code and words in str(e.value), str(e.value)
    for base, n, L, want in ((2, 4096, 64, 388 + 2 * 4096), (3, 4097, 64, 2 * 388 + 4 * 4097), (4, 1, 8192, 388 + 4), (2, 1, 8192 * 4, 0),
                             (3, 1, 16384, 0), (5, 1, 64, 0), (2, 1 << 29, 64, 0)):
        assert codec.banded_stream_bound(n, L, base) == want
    n = C.c_uint64(9)
    assert not lib.alice_codec_encode_banded(None, None, 0, 0, 0, 0, 0, 2, C.byref(n)) and lib.alice_codec_last_error() == 9 and n.value == 9
    for fn in (lib.alice_codec_decode_banded,):
        assert not fn(None, 0, C.byref(n)) and lib.alice_codec_last_error() == 9
    for fn in (lib.alice_codec_to_banded, lib.alice_codec_from_banded):
        assert not fn(None, 0, 0, C.byref(n)) and lib.alice_codec_last_error() == 9
    bad_L = patched(small(3), 0, b"ALCC")
    with pytest.raises(codec.CodecError) as e:
        codec.from_banded(bad_L, 16384)          # base 3 has no lanes of 16384
    assert e.value.code == 2
    if codec.device_count() < 1:   # without a device the compute calls fail loudly
        for call in (lambda: codec.encode_banded(enc, rgb, 4, 4, 2), lambda: codec.decode_banded(small()), lambda: codec.from_banded(small())):
            with pytest.raises(codec.CodecError) as e:
                call()
            assert e.value.code == 8


# ---- the size condition ----
@pytest.mark.parametrize("kind", [CDF53, CDF97, HAAR])
def test_banded_is_smaller_at_chunk_size(kind):
    """wide_oracle.smooth_plus_noise 160x96x16, L = 512."""
    w, h, f = 160, 96, 16
    rgb = clip(w, h, f)
    for q in (50, 80):
        for base in (2, 3):
            step, syms = B.base_symbols(rgb, w, h, f, q, kind, base)
            K = B.coder(base)
            plain = K.write_container(kind, w, h, f, 512, (step,) * 3, syms)
            banded = B.write_container(base, kind, w, h, f, 512, (step,) * 3, (step,) * 3, syms)
            print(f"wavelet {kind} q={q} base {base}: banded {len(banded)} / plain {len(plain)} = {len(banded) / len(plain):.3f}")
            assert len(banded) < len(plain), (kind, q, base, len(banded), len(plain))


def test_banded_is_larger_at_thumbnail_size():
    """The caveat of DESIGN.md 20.7: at 64x48x8 with L = 64 the header and 24 lane directories dominate."""
    w, h, f = 64, 48, 8
    rgb = clip(w, h, f)
    for kind in (CDF53, CDF97):
        for q in (50, 80):
            plain = B.encode_base(rgb, w, h, f, q, kind, 2, 64)
            banded = B.encode(rgb, w, h, f, q, kind, 2, 64)
            print(f"wavelet {kind} q={q}: banded {len(banded)} / plain {len(plain)} = {len(banded) / len(plain):.3f}")
            assert len(banded) > len(plain), (kind, q)
