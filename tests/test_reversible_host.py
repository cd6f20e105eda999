"""CPU-only checks of the reversible format (.alc version 4): the numpy restatement
(tests/reversible_ref.py) returns the input exactly at quality 100, where the reference's inverse does not; the PSNR table of
the two inverses at lossy steps (printed, nothing asserted about which is higher); the separation of the four parsers; and
the mirrored twin of tests/test_inverse_bounds_host.py: the class inverse_bounds picks (read through
alice_codec_test_inverse_variant with wide = 1) is sound for the MIRRORED arithmetic on the worst-sign volumes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reversible_ref as RR  # noqa: E402
import transform_extremes as X  # noqa: E402
import wide_oracle as WO  # noqa: E402
import wide_ref as R3  # noqa: E402

CDF53, CDF97, HAAR = 0, 1, 2
NAMES = {CDF53: "CDF 5/3", CDF97: "CDF 9/7", HAAR: "Haar"}
SHAPES = [(64, 48, 8), (33, 17, 5), (7, 3, 1), (1, 1, 1)]
CONTENTS = ("smooth_plus_noise", "uniform_noise", "random_0_255")


def content(name, w, h, f, seed=11):
    rng = np.random.default_rng(seed + w + h + f)
    if name == "smooth_plus_noise":
        return WO.smooth_plus_noise(w, h, f)
    if name == "uniform_noise":
        return rng.integers(0, 256, w * h * f * 3, dtype=np.uint8)
    return (rng.integers(0, 2, w * h * f * 3) * 255).astype(np.uint8)


@pytest.mark.parametrize("kind", [CDF53, CDF97, HAAR])
@pytest.mark.parametrize("shape", SHAPES)
def test_the_mirrored_inverse_is_lossless_at_quality_100(shape, kind):
    w, h, f = shape
    worst_q = 0
    for name in CONTENTS:
        rgb = content(name, w, h, f)
        step, dims, qs = WO.forward_quantised(RR.o, rgb, w, h, f, 100, kind)
        assert step == 1
        worst_q = max(worst_q, max(int(np.abs(q).max()) for q in qs))
        assert np.array_equal(RR.inverse_quantised(qs, (1, 1, 1), dims, w, h, f, kind), rgb), (shape, NAMES[kind], name)
        # through the container as well: symbols, lanes and header are version 3's, byte 4 is 4
        if w * h * f <= 33 * 17 * 5:
            blob = RR.encode(rgb, w, h, f, 100, kind, 64)
            assert blob[4] == 4 and np.array_equal(RR.decode(blob), rgb)
    assert worst_q <= X.WIDE_MAX_Q        # inside version 3's residual range (z <= 255 + 4095)


def test_the_reference_inverse_is_not_lossless():
    """The gap version 4 closes: the same coefficients through the reference's inverse (versions 1 to 3)."""
    w, h, f = 64, 48, 8
    rgb = content("smooth_plus_noise", w, h, f)
    for kind in (CDF53, CDF97, HAAR):
        back = RR.roundtrip(rgb, w, h, f, 100, kind, mirrored=False)
        p = WO.psnr(rgb, back)
        print(f"{NAMES[kind]} q=100 reference inverse: {p:.2f} dB (mirrored: exact)")
        assert not np.array_equal(back, rgb) and 35 < p < 70


def test_psnr_table_at_lossy_steps():
    """The table DESIGN.md section 12 quotes.  Nothing is asserted about which inverse is higher."""
    w, h, f = 64, 48, 8
    for name in CONTENTS:
        rgb = content(name, w, h, f)
        for kind in (CDF53, CDF97, HAAR):
            for q in (90, 80, 50):
                m = WO.psnr(rgb, RR.roundtrip(rgb, w, h, f, q, kind))
                r = WO.psnr(rgb, RR.roundtrip(rgb, w, h, f, q, kind, mirrored=False))
                print(f"{name:18s} {NAMES[kind]:8s} q={q}: mirrored {m:6.2f} dB, reference {r:6.2f} dB, difference {m - r:+.2f}")
                assert np.isfinite(m) and np.isfinite(r)


# ---- parsers ----
def info_rc(codec, data, fn):
    lib = codec.load_library()
    buf = np.frombuffer(bytes(data), np.uint8)
    out = (C.c_uint8 * 256)()
    rc = getattr(lib, fn)(buf.ctypes.data_as(C.POINTER(C.c_uint8)), buf.size, C.cast(out, C.c_void_p))
    return rc, (lib.alice_codec_last_error_message() or b"").decode()


def small_container():
    w, h, f = 6, 4, 2
    rgb = content("uniform_noise", w, h, f)
    return RR.encode(rgb, w, h, f, 100, CDF97, 64), rgb


def test_the_four_parsers_keep_apart(codec):
    v4, rgb = small_container()
    i = codec.reversible_info(v4)
    assert (i.width, i.height, i.frames, i.lane_symbols, int(i.wavelet_type)) == (6, 4, 2, 64, CDF97)
    assert i.quant_step == [1] * 3 and sum(i.payload_len) + codec.SPLIT_HEADER_BYTES == len(v4)
    assert codec.alc_version(v4) == 4
    v1 = codec.FrameEncoder.with_wavelet(50, codec.WaveletType.Haar).encode(np.zeros(0, np.uint8), 0, 3, 3).to_bytes()
    others = {1: v1, 2: RR.with_version(v4, 2), 3: RR.with_version(v4, 3)}
    # the version 4 parser refuses 1, 2 and 3 ...
    for ver, blob in others.items():
        rc, msg = info_rc(codec, blob, "alice_codec_reversible_info")
        assert rc == 4 and f"unsupported version: {ver} (expected 4)" in msg, msg
        with pytest.raises(codec.CodecError, match=rf"unsupported version: {ver} \(expected 4\)"):
            codec.decode_reversible(blob)
        with pytest.raises(R3.InvalidBitstream):
            RR.parse_container(blob)
    # ... and the parsers of versions 1, 2 and 3 refuse 4, in the same words
    for fn, ver in (("alice_codec_split_info", 2), ("alice_codec_wide_info", 3)):
        rc, msg = info_rc(codec, v4, fn)
        assert rc == 4 and f"unsupported version: 4 (expected {ver})" in msg, msg
    with pytest.raises(codec.CodecError, match=r"unsupported version: 4 \(expected 1\)"):
        codec.EncodedChunk.from_bytes(v4 + bytes(4000))
    with pytest.raises(codec.CodecError, match=r"unsupported version: 4 \(expected 3\)"):
        codec.decode_wide(v4)
    with pytest.raises(codec.CodecError, match=r"unsupported version: 4 \(expected 2\)"):
        codec.decode_split(v4)
    assert codec.wide_info(others[3]).payload_len == i.payload_len      # the same bytes behind byte 4
    # decode_alc dispatches on 4: the refusal is worded by the version 4 parser (the lane range is the wide one)
    with pytest.raises(codec.CodecError, match="unknown wavelet"):
        codec.decode_alc(v4[:5] + b"\x07" + v4[6:])
    bad = bytearray(v4)
    bad[18:22] = (16384).to_bytes(4, "little")
    with pytest.raises(codec.CodecError, match=r"\[64, 8192\]"):
        codec.reversible_info(bytes(bad))
    with pytest.raises(R3.InvalidBitstream):
        RR.parse_container(bytes(bad))


def test_empty_chunk_and_argument_checks(codec):
    lib = codec.load_library()
    enc = codec.FrameEncoder.with_wavelet(100, codec.WaveletType.Cdf53)
    b = codec.encode_reversible(enc, np.zeros(0, np.uint8), 0, 4, 4)
    assert len(b) == codec.SPLIT_HEADER_BYTES and b[4] == 4
    assert b == RR.with_version(codec.encode_wide(enc, np.zeros(0, np.uint8), 0, 4, 4), 4)
    i = codec.reversible_info(b)
    assert i.num_symbols == [0] * 3 and i.payload_len == [0] * 3 and i.lane_symbols == 512 and i.quant_step == [1] * 3
    assert codec.decode_reversible(b).size == 0 and codec.decode_alc(b).size == 0
    assert codec.encode_lossless(np.zeros(0, np.uint8), 0, 4, 4) == b
    rgb = np.zeros(4 * 4 * 2 * 3, np.uint8)
    # the order of the wide twin: buffer size before lane_symbols
    for args, code in (((rgb[:-1], 4, 4, 2), 1), ((rgb[:-1], 4, 4, 2, 100), 1), ((rgb, 4, 4, 2, 100), 2), ((rgb, 4, 4, 2, 16384), 2)):
        for fn in (codec.encode_reversible, codec.encode_wide):
            with pytest.raises(codec.CodecError) as e:
                fn(enc, *args)
            assert e.value.code == code
    n = C.c_uint64(9)
    assert not lib.alice_codec_encode_reversible(None, None, 0, 0, 0, 0, 0, C.byref(n)) and lib.alice_codec_last_error() == 9 and n.value == 9
    assert not lib.alice_codec_decode_reversible(None, 0, C.byref(n)) and lib.alice_codec_last_error() == 9
    if codec.device_count() < 1:   # without a device the compute calls fail loudly
        with pytest.raises(codec.CodecError) as e:
            codec.encode_lossless(rgb, 4, 4, 2)
        assert e.value.code == 8
        with pytest.raises(codec.CodecError) as e:
            codec.decode_reversible(small_container()[0])
        assert e.value.code == 8


# ---- the bound: inverse_bounds with kWideMaxQ is sound for the mirrored arithmetic ----
STEPS = np.arange(1, 41)   # the wide classes end below step 21 (exact from 20 / 3 / 13 on)
DIMS = (8, 16, 16)         # (pf, ph, pw), as tests/test_inverse_bounds_host.py
I16_MAX = 32767
OPERAND_LIMIT = 1 << 23    # |a + b| < 2^23: the signed 24-bit operand of v_mad_i32_i24
PRODUCT_LIMIT = (1 << 31) - 1


def variant(lib, kind, step):
    s = (C.c_int32 * 3)(int(step), int(step), int(step))
    return lib.alice_codec_test_inverse_variant(kind, s, 1)


def violations(v, m_t, m_c, pair, prod):
    bad = []
    if v >= 2 and m_t > I16_MAX:
        bad.append(f"i16 band slot holds {m_t}")
    if v == 3 and m_c > I16_MAX:
        bad.append(f"packed i16 tile holds {m_c}")
    if v >= 1 and pair >= OPERAND_LIMIT:
        bad.append(f"a neighbour sum of {pair} leaves the 24-bit operand")
    if v >= 1 and prod >= PRODUCT_LIMIT:
        bad.append(f"|sum * c| + 4096 = {prod} leaves 31 bits")
    return bad


@pytest.mark.parametrize("kind", [CDF53, CDF97, HAAR])
def test_every_class_is_sound_for_the_mirrored_inverse(codec, kind):
    lib = codec.load_library()
    got = np.array([variant(lib, kind, s) for s in STEPS])
    assert got[-1] == 0 and np.all(np.diff(got) <= 0)
    signs = X.worst_volume(kind, DIMS)
    seen = 0
    for v in (3, 2, 1):
        steps = STEPS[got == v]
        if steps.size == 0:
            continue
        seen += 1
        for s in sorted({int(steps[0]), int(steps[-1])}):        # the class's first and last step
            for centre in (None, (5, 9, 9)):
                vol = X.worst_volume(kind, DIMS, centre) if centre else signs
                for sign in (1, -1):                             # q = +2175 and -2175 are both decodable
                    coef = X.dequantised(sign * vol * X.WIDE_MAX_Q, s)
                    (m_t, m_c, m_r), pair, prod = RR.per_pass_mirror(kind, coef)
                    ref = X.per_pass_maxima(kind, coef)
                    if centre is None and sign == 1:     # shown with -s: what each class is handed at its ends
                        print(f"{NAMES[kind]} class {v} step {s}: mirrored maxima {m_t} / {m_c} / {m_r} (reference {ref}), "
                              f"largest neighbour sum {pair}, largest |sum * c| + 4096 {prod}")
                    assert not violations(v, m_t, m_c, pair, prod), (NAMES[kind], v, s, violations(v, m_t, m_c, pair, prod))
                    # the mirrored step differs from the reference's by at most one per step: the maxima stay together
                    assert all(abs(a - b) <= 64 for a, b in zip((m_t, m_c, m_r), ref))
    assert seen >= 1


def test_the_mirrored_soundness_check_bites(codec):
    """A class one higher than inverse_bounds allows must be reported: CDF 5/3 (gain 2.0 per pass on 2175 * step) leaves the
    packed tile at step 3 and the i16 slot at step 7."""
    lib = codec.load_library()
    got = {int(s): variant(lib, CDF53, s) for s in STEPS}
    first_slot = min(s for s, v in got.items() if v == 2)        # leaves the packed tile here
    first_i32 = min(s for s, v in got.items() if v == 1)         # leaves the i16 slot here
    for s, wrong in ((first_i32, 2), (first_slot, 3)):
        coef = X.dequantised(X.worst_volume(CDF53, DIMS) * X.WIDE_MAX_Q, s)
        (m_t, m_c, _), pair, prod = RR.per_pass_mirror(CDF53, coef)
        assert not violations(got[s], m_t, m_c, pair, prod)
        # the bound is rigorous, not tight: one class too high need not overflow at the class's first step, but it does
        # two steps on for this wavelet (gain 2.0 per pass on 2175 * step)
        coef2 = X.dequantised(X.worst_volume(CDF53, DIMS) * X.WIDE_MAX_Q, 2 * s + 2)
        (t2, c2, _), p2, pr2 = RR.per_pass_mirror(CDF53, coef2)
        assert violations(wrong, t2, c2, p2, pr2)
    assert violations(1, 0, 0, OPERAND_LIMIT, 0) and violations(1, 0, 0, 0, PRODUCT_LIMIT) and not violations(0, 1 << 40, 1 << 40, 1 << 40, 1 << 40)
