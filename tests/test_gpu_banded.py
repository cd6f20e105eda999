"""The banded format (.alc version 5) on the MI355X.  Containers are compared byte for byte with
tests/banded_ref.py, pixels bit for bit with the base version's GPU decode: the geometry at which the band addressing can
go wrong, the content that bends the tables, the histogram stage call on its own, the device calls with their groups and
refusals, the repack in both directions, and the damage verdicts."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import banded_ref as B  # noqa: E402
import wide_oracle as WO  # noqa: E402

import torch  # noqa: E402

pytestmark = pytest.mark.gpu

CDF53, CDF97 = 0, 1
GUARD = 64

# (shape, L): what each exercises is in DESIGN.md 20.8
GEOMETRY = [
    ((1, 1, 1), 64),        # one symbol per band, 63 empty lanes
    ((6, 4, 1), 64),        # hw = 3: a 64-lane step crosses rows and the frame edge; ht = 1 from f = 1
    ((33, 17, 5), 64),      # odd everything, one short block per band
    ((126, 6, 4), 64), ((128, 6, 4), 64), ((130, 6, 4), 64),     # hw = 63, 64, 65
    ((64, 32, 16), 64),     # n_band = 4096: exactly one block
    ((126, 130, 2), 64),    # n_band = 4095
    ((34, 482, 2), 64),     # n_band = 4097: a block of one symbol
    ((160, 96, 16), 64), ((160, 96, 16), 512),                   # several blocks per band; the size condition's shape
]


def n_band(shape):
    pw, ph, pf = B.padded_dims(*shape)
    return pw * ph * pf // 8


def test_the_geometry_list_is_what_it_says():
    assert [n_band(s) for s, _ in GEOMETRY[:3]] == [1, 6, 17 * 9 * 3]
    assert [B.padded_dims(*s)[0] // 2 for s, _ in GEOMETRY[3:6]] == [63, 64, 65]
    assert [n_band(s) for s, _ in GEOMETRY[6:9]] == [4096, 4095, 4097]


@functools.lru_cache(maxsize=None)
def clip(name, shape):
    w, h, f = shape
    rng = np.random.default_rng(29 + w + h + f)
    if name == "smooth_plus_noise":
        return WO.smooth_plus_noise(w, h, f)
    if name == "uniform_noise":
        return rng.integers(0, 256, w * h * f * 3, dtype=np.uint8)
    if name == "flat_grey":
        return np.full(w * h * f * 3, 128, np.uint8)
    assert name == "smooth"         # gradients without noise: at step 1 the low band escapes and no high band does
    t, y, x = np.meshgrid(np.arange(f), np.arange(h), np.arange(w), indexing="ij")
    base = np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y + 2 * t) * 255) // max(w + h + 2 * f - 3, 1)], axis=-1)
    return base.astype(np.uint8).reshape(-1)


BASE_ENCODE = {2: "encode_split", 3: "encode_wide", 4: "encode_reversible"}


def check_chunk(a, rgb, shape, kind, q, base, L):
    """encode == reference bytes; decode == the base version's GPU decode (and the reference's); -> the banded bytes"""
    w, h, f = shape
    enc = a.FrameEncoder.with_wavelet(q, a.WaveletType(kind))
    got = a.encode_banded(enc, rgb, w, h, f, L, base)
    tag = (shape, kind, q, base, L)
    assert got == B.encode(rgb, w, h, f, q, kind, base, L), tag
    plain = getattr(a, BASE_ENCODE[base])(enc, rgb, w, h, f, L)
    pix = a.decode_banded(got)
    assert np.array_equal(pix, a.decode_alc(plain)), tag
    assert np.array_equal(a.decode_alc(got), pix), tag
    return got, plain, pix


@pytest.mark.parametrize("shape,L", GEOMETRY, ids=[f"{s[0]}x{s[1]}x{s[2]}-L{L}" for s, L in GEOMETRY])
def test_geometry(gpu_codec, shape, L):
    a = gpu_codec
    rgb = clip("smooth_plus_noise", shape)
    for kind in (CDF53, CDF97):
        for base in (2, 3):
            got, plain, _ = check_chunk(a, rgb, shape, kind, 80, base, L)
            assert a.to_banded(plain) == got and a.from_banded(got) == plain, (shape, kind, base)
            i = a.banded_info(got)
            assert i.base == base and i.n_blocks == [B.R2.n_blocks_of(n_band(shape), L)] * 24
        _, _, pix = check_chunk(a, rgb, shape, kind, 100, 4, L)
        assert np.array_equal(pix, rgb), (shape, kind)          # base 4 at quality 100 is lossless


def test_size_condition_on_the_device(gpu_codec):
    """the containers of the size condition's shape, made by the GPU: smaller than the base's at L = 512"""
    a = gpu_codec
    shape = (160, 96, 16)
    rgb = clip("smooth_plus_noise", shape)
    for kind in (CDF53, CDF97):
        for q in (50, 80):
            enc = a.FrameEncoder.with_wavelet(q, a.WaveletType(kind))
            banded = a.encode_banded(enc, rgb, *shape, 512, 2)
            plain = a.encode_split(enc, rgb, *shape, 512)
            print(f"wavelet {kind} q={q}: banded {len(banded)} / version 2 {len(plain)} = {len(banded) / len(plain):.3f}")
            assert len(banded) < len(plain)


@pytest.mark.parametrize("name", ["uniform_noise", "flat_grey"])
def test_content(gpu_codec, name):
    a = gpu_codec
    shape = (33, 17, 5)
    rgb = clip(name, shape)
    for kind in (CDF53, CDF97):
        for base in (2, 3):
            got, _, _ = check_chunk(a, rgb, shape, kind, 80, base, 64)
            if name == "flat_grey":
                # seven bands per channel hold one symbol: one frequency of 4096, four state bytes per lane that has symbols
                info = B.parse_container(got)
                nb = n_band(shape)
                for c in range(3):
                    for k in range(1, 8):
                        assert int(info["freq"][8 * c + k].max()) == 4096
                        assert info["payload_len"][8 * c + k] == 4 + 128 + 4 * min(nb, 64)
        _, _, pix = check_chunk(a, rgb, shape, kind, 100, 4, 64)
        assert np.array_equal(pix, rgb)


def test_low_band_escapes_alone(gpu_codec):
    a = gpu_codec
    shape = (32, 16, 4)
    rgb = clip("smooth", shape)
    pw, ph, pf = B.padded_dims(*shape)
    for kind in (CDF53, CDF97):
        _, syms = B.base_symbols(rgb, *shape, 100, kind, 3)
        tops = [[int(b.max()) for b in B.gather_bands(s, pw, ph, pf)] for s in syms]
        assert tops[0][0] >= 255 and all(t < 255 for ch in tops for t in ch[1:]), tops      # the content is what it says
        for base in (3, 4):
            got, _, pix = check_chunk(a, rgb, shape, kind, 100, base, 64)
            info = B.parse_container(got)
            assert info["freq"][0][255] > 0 and all(info["freq"][k][255] == 0 for k in range(1, 8))
            if base == 4:
                assert np.array_equal(pix, rgb)


# ---- the histogram stage call ----

def vbs_per_channel(pw, ph, pf):
    """virtual blocks of band_hist_kernel per channel: whole rows, 256 sixteen-symbol units at most"""
    units = (pw + 15) // 16
    if units > 256:
        return ph * pf * ((units + 255) // 256)
    per = 256 // units
    return (ph * pf + per - 1) // per


def check_hist(a, pw, ph, pf, wide, offset=0, seed=3):
    rng = np.random.default_rng(seed + pw + ph + pf)
    n = 3 * pw * ph * pf
    if wide:
        sym = rng.integers(0, 700, n).astype(np.uint16)
        sym[rng.integers(0, n, n // 7 + 1)] = 0
    else:
        sym = rng.integers(0, 256, n).astype(np.uint8)
    raw = sym.view(np.uint8)
    buf = torch.full((GUARD + 16 + raw.size + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    buf[GUARD + offset:GUARD + offset + raw.size] = torch.from_numpy(raw.copy()).to("cuda:0")
    hist = torch.full((3 * 8 * 256 + 8,), 77, dtype=torch.int32, device="cuda:0")
    a.band_histograms_device(buf.data_ptr() + GUARD + offset, pw, ph, pf, wide, hist.data_ptr())
    got = hist.cpu().numpy()
    assert (got[3 * 8 * 256:] == 77).all()
    want = np.stack([[np.bincount(np.minimum(b.astype(np.int64), 255), minlength=256) for b in B.gather_bands(ch, pw, ph, pf)]
                     for ch in sym.reshape(3, -1)])
    assert np.array_equal(got[:3 * 8 * 256].reshape(3, 8, 256), want), (pw, ph, pf, wide, offset)
    assert np.array_equal(buf.cpu().numpy()[GUARD + offset:GUARD + offset + raw.size], raw)      # the symbols are only read


@pytest.mark.parametrize("wide", [False, True], ids=["u8", "u16"])
def test_band_histograms_widths_and_alignments(gpu_codec, wide):
    # pw puts the hw edge at every offset mod 4 and mod 64 (hw = 1, 3, 33, 63, 65), at 16 (pw = 32) and past one row segment
    for pw in (2, 6, 66, 126, 130, 32, 4100):
        check_hist(gpu_codec, pw, 6, 4, wide)
    for offset in ((2, 4, 8) if wide else (1, 2, 4, 8)):      # the row start allows 2-, 4- and 8-byte loads (u8: bytes too)
        for pw in (32, 130):
            check_hist(gpu_codec, pw, 4, 2, wide, offset)
    check_hist(gpu_codec, 2, 2, 2, wide)


@pytest.mark.parametrize("cap", [1, 3, 4])
def test_band_histograms_grid_stride(gpu_codec, cap):
    """3 v virtual blocks over `cap` workgroups, v = 1, 2, 3: with 3 workgroups exactly one, two and three trips, with 4 a
    launch smaller than the cap, one-and-a-bit and two-and-a-bit trips, with 1 every block in one workgroup"""
    lib = gpu_codec.load_library()
    try:
        lib.alice_codec_test_set_grid_cap(cap)
        for wide in (False, True):
            for pw in (2, 66, 130):
                per = 256 // ((pw + 15) // 16)
                for v in (1, 2, 3):
                    rows = (per * (v - 1)) // 4 * 4 + 4          # ph * pf: the smallest multiple of 4 above (v - 1) blocks
                    assert vbs_per_channel(pw, 2, rows // 2) == v
                    check_hist(gpu_codec, pw, 2, rows // 2, wide)
            check_hist(gpu_codec, 4100, 2, 2, wide)              # 8 virtual blocks per channel
    finally:
        lib.alice_codec_test_set_grid_cap(0)


# ---- device calls ----

def dev(arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).to("cuda:0")


SHAPE3 = (33, 17, 5)
QUALS = (40, 80, 95)


@functools.lru_cache(maxsize=None)
def three_chunks(base, kind):
    w, h, f = SHAPE3
    rgb = [clip(n, SHAPE3) for n in ("smooth_plus_noise", "uniform_noise", "flat_grey")]
    want = [B.encode(r, w, h, f, q, kind, base, 64) for r, q in zip(rgb, QUALS)]
    return np.concatenate(rgb), want


def encode_three(a, base, kind, stride):
    rgb, want = three_chunks(base, kind)
    out = torch.full((GUARD + 3 * stride + GUARD,), 0x5A, dtype=torch.uint8, device="cuda:0")
    d_rgb = dev(rgb)
    sizes = a.banded_encode_device(d_rgb.data_ptr(), *SHAPE3, 3, a.WaveletType(kind), 0, out.data_ptr() + GUARD, stride,
                                   qualities=QUALS, lane_symbols=64, base=base)
    return out, sizes, want


@pytest.mark.parametrize("group", [0, 2])
def test_device_calls_three_chunks(gpu_codec, group):
    a = gpu_codec
    lib = a.load_library()
    w, h, f = SHAPE3
    try:
        lib.alice_codec_test_set_group_chunks(group)       # 2: a second group runs
        for base, kind in ((2, CDF53), (3, CDF97), (4, CDF53)):
            _, want = three_chunks(base, kind)
            stride = max(len(x) for x in want) + 3
            out, sizes, _ = encode_three(a, base, kind, stride)
            got = out.cpu().numpy()
            assert (got[:GUARD] == 0x5A).all() and (got[GUARD + 3 * stride:] == 0x5A).all()
            for i in range(3):
                assert int(sizes[i]) == len(want[i])
                chunk = got[GUARD + i * stride:GUARD + i * stride + len(want[i])]
                assert chunk.tobytes() == want[i], (base, kind, i)
                assert (got[GUARD + i * stride + len(want[i]):GUARD + (i + 1) * stride] == 0x5A).all()
            # decode: all three at once, from an unaligned d_alc
            for off in (0, 1, 2, 3):
                alc = torch.zeros(off + 3 * stride, dtype=torch.uint8, device="cuda:0")
                alc[off:] = out[GUARD:GUARD + 3 * stride]
                pix = torch.full((3 * w * h * f * 3 + GUARD,), 0x33, dtype=torch.uint8, device="cuda:0")
                a.banded_decode_device(alc.data_ptr() + off, stride, sizes, pix.data_ptr())
                p = pix.cpu().numpy()
                assert (p[3 * w * h * f * 3:] == 0x33).all()
                for i in range(3):
                    assert np.array_equal(p[i * w * h * f * 3:(i + 1) * w * h * f * 3], a.decode_alc(B.from_banded(want[i]))), (base, kind, i, off)
    finally:
        lib.alice_codec_test_set_group_chunks(0)


def test_out_stride_too_small_writes_nothing_of_the_group(gpu_codec):
    a = gpu_codec
    lib = a.load_library()
    _, want = three_chunks(2, CDF53)
    stride = max(len(x) for x in want) - 1                  # the largest chunk (uniform noise, index 1) does not fit
    assert len(want[1]) > stride >= len(want[0]) and stride >= len(want[2])
    with pytest.raises(a.CodecError) as e:
        encode_three(a, 2, CDF53, stride)
    assert e.value.code == 1 and "chunk 1 needs" in str(e.value)
    rgb, _ = three_chunks(2, CDF53)
    out = torch.full((GUARD + 3 * stride + GUARD,), 0x5A, dtype=torch.uint8, device="cuda:0")
    d_rgb = dev(rgb)
    with pytest.raises(a.CodecError):
        a.banded_encode_device(d_rgb.data_ptr(), *SHAPE3, 3, a.WaveletType(CDF53), 0, out.data_ptr() + GUARD, stride, qualities=QUALS,
                               lane_symbols=64, base=2)
    assert (out.cpu().numpy() == 0x5A).all()                 # nothing of the group was written
    try:
        lib.alice_codec_test_set_group_chunks(1)            # groups of one: chunk 0 is complete, chunks 1 and 2 untouched
        with pytest.raises(a.CodecError):
            a.banded_encode_device(d_rgb.data_ptr(), *SHAPE3, 3, a.WaveletType(CDF53), 0, out.data_ptr() + GUARD, stride, qualities=QUALS,
                                   lane_symbols=64, base=2)
        got = out.cpu().numpy()
        assert got[GUARD:GUARD + len(want[0])].tobytes() == want[0] and (got[GUARD + stride:] == 0x5A).all()
    finally:
        lib.alice_codec_test_set_group_chunks(0)


# ---- repack on the device ----

@pytest.mark.parametrize("base", [2, 3, 4])
def test_repack_on_the_device(gpu_codec, base):
    a = gpu_codec
    w, h, f = SHAPE3
    kind = CDF97
    qs = (100, 100, 100) if base == 4 else QUALS
    names = ("smooth_plus_noise", "uniform_noise", "flat_grey")
    plain = [getattr(a, BASE_ENCODE[base])(a.FrameEncoder.with_wavelet(q, a.WaveletType(kind)), clip(n, SHAPE3), w, h, f, 64)
             for n, q in zip(names, qs)]
    for L_to, L_back in ((0, 0), (128, 64)):
        Le = L_to or 64
        banded = [a.encode_banded(a.FrameEncoder.with_wavelet(q, a.WaveletType(kind)), clip(n, SHAPE3), w, h, f, Le, base)
                  for n, q in zip(names, qs)]
        assert banded[0] == B.to_banded(plain[0], Le)
        stride_in = max(len(x) for x in plain) + 1
        src = torch.zeros(3 * stride_in, dtype=torch.uint8, device="cuda:0")
        for i, x in enumerate(plain):
            src[i * stride_in:i * stride_in + len(x)] = dev(np.frombuffer(x, np.uint8))
        stride = max(len(x) for x in banded) + 5
        out = torch.full((GUARD + 3 * stride,), 0x5A, dtype=torch.uint8, device="cuda:0")
        sizes = a.to_banded_device(src.data_ptr(), stride_in, [len(x) for x in plain], out.data_ptr() + GUARD, stride, lane_symbols=L_to)
        got = out.cpu().numpy()
        assert (got[:GUARD] == 0x5A).all()
        for i in range(3):
            assert got[GUARD + i * stride:GUARD + i * stride + int(sizes[i])].tobytes() == banded[i], (base, L_to, i)
            assert a.to_banded(plain[i], L_to) == banded[i]
        # and back: the base's bytes
        back = torch.full((3 * stride_in + GUARD,), 0x5A, dtype=torch.uint8, device="cuda:0")
        sizes2 = a.from_banded_device(out.data_ptr() + GUARD, stride, sizes, back.data_ptr(), stride_in, lane_symbols=L_back)
        got2 = back.cpu().numpy()
        assert (got2[3 * stride_in:] == 0x5A).all()
        for i in range(3):
            assert got2[i * stride_in:i * stride_in + int(sizes2[i])].tobytes() == plain[i], (base, L_back, i)
            assert a.from_banded(banded[i], L_back) == plain[i]
    # an output stride below the header is refused before anything is written
    with pytest.raises(a.CodecError) as e:
        a.to_banded_device(src.data_ptr(), stride_in, [len(x) for x in plain], out.data_ptr() + GUARD, 100)
    assert e.value.code == 1


# ---- damage ----

def test_damage(gpu_codec):
    a = gpu_codec
    w, h, f = SHAPE3
    for base in (2, 3):
        _, want = three_chunks(base, CDF53)
        blob = want[0]
        info = B.parse_container(blob)
        plen = info["payload_len"]
        first_lane = B.HEADER + 4 + 128 + 5              # band 0, block 0: a byte inside the first lanes' streams
        last_band = len(blob) - plen[23]
        cases = {
            "lane of band 0": (first_lane, "stream 0: a lane failed its end check"),
            "last band of the last channel": (len(blob) - 3, "stream 23: a lane failed its end check"),
            "lane directory": (last_band + 4 + 6, "stream 23: block or lane directory does not add up"),
        }
        n_px = w * h * f * 3
        for name, (at, words) in cases.items():
            bad = bytearray(blob)
            bad[at] ^= 0x40
            with pytest.raises(a.CodecError) as e:
                a.decode_banded(bytes(bad))
            assert e.value.code == 4 and words in str(e.value), (name, str(e.value))
            with pytest.raises(a.CodecError) as e:
                a.from_banded(bytes(bad))
            assert e.value.code == 4 and words in str(e.value), (name, str(e.value))
            with pytest.raises(B.InvalidBitstream):
                B.decode(bytes(bad))
        # found by the host validation: the output is untouched.  As chunk 1 of a device call of two.
        for name, bad, words in (("block-length table", bytes(blob[:B.HEADER]) + bytes([blob[B.HEADER] ^ 1]) + blob[B.HEADER + 1:], "length"),
                                 ("truncated", blob[:-7], "length mismatch")):
            with pytest.raises(a.CodecError) as e:
                a.decode_banded(bad)
            assert e.value.code == 4 and ("block lengths sum" in str(e.value) or words in str(e.value)), (name, str(e.value))
            stride = len(blob) + 8
            alc = torch.zeros(2 * stride, dtype=torch.uint8, device="cuda:0")
            alc[:len(blob)] = dev(np.frombuffer(blob, np.uint8))
            alc[stride:stride + len(bad)] = dev(np.frombuffer(bad, np.uint8))
            pix = torch.full((2 * n_px,), 0x33, dtype=torch.uint8, device="cuda:0")
            with pytest.raises(a.CodecError) as e:
                a.banded_decode_device(alc.data_ptr(), stride, [len(blob), len(bad)], pix.data_ptr())
            assert e.value.code == 4
            if name == "truncated":
                assert (pix.cpu().numpy() == 0x33).all()
            else:
                assert "stream 24" in str(e.value), str(e.value)     # the scan kernel finds it: stream j, j = 24 * chunk + band
