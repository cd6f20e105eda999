"""The reversible format (.alc version 4) on the MI355X against tests/reversible_ref.py, the numpy
restatement of the mirrored inverse.  Shapes are chosen for the kernels' geometry (inverse tile 96 x 32, halo 4): 300x104x4
has an interior tile at bx = 1, 2 and by = 1 with edge tiles around it, 100x36x6 two partial tiles each way, 33x17x5 odd
sizes and padding on all three axes, 8x6x2 and 6x6x1 are the smallest tile-eligible shapes (one pair, a single frame), and
5x3x1, 4x4x2 and 1x1x1 take the generic path."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reversible_ref as RR  # noqa: E402
import wide_oracle as WO  # noqa: E402
import wide_ref as R3  # noqa: E402
from test_reversible_host import CONTENTS, content  # noqa: E402
from test_gpu_wide_region import _person_frames  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 256
SENTINEL = 0xA5
CDF53, CDF97, HAAR = 0, 1, 2
SHAPES = [(300, 104, 4), (100, 36, 6), (33, 17, 5), (8, 6, 2), (6, 6, 1), (5, 3, 1), (4, 4, 2), (1, 1, 1)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _stride(a, w, h, f, L):
    return (a.SPLIT_HEADER_BYTES + 3 * a.wide_stream_bound(int(np.prod(R3.padded_dims(w, h, f))), L) + 255) & ~255


# ---- lossless ----
@pytest.mark.parametrize("kind", [CDF53, CDF97, HAAR])
@pytest.mark.parametrize("shape", SHAPES)
def test_lossless(gpu_codec, shape, kind):
    a = gpu_codec
    w, h, f = shape
    wt = a.WaveletType(kind)
    for name in CONTENTS:
        rgb = content(name, w, h, f)
        blob = a.encode_lossless(rgb, w, h, f, wt, 64)
        assert a.alc_version(blob) == 4 and a.reversible_info(blob).quant_step == [1, 1, 1]
        assert np.array_equal(a.decode_reversible(blob), rgb), (shape, kind, name)
        assert np.array_equal(a.decode_alc(blob), rgb)
    # the control: version 3 of the same input at quality 100 gives the reference inverse's pixels, which are not the input
    rgb = content("smooth_plus_noise", w, h, f)
    v3 = a.decode_wide(a.encode_wide(a.FrameEncoder.with_wavelet(100, wt), rgb, w, h, f, 64))
    want = RR.roundtrip(rgb, w, h, f, 100, kind, mirrored=False)
    assert np.array_equal(v3, want)
    if w * h * f >= 8 * 6 * 2 and kind != CDF97:     # every odd neighbour sum is off by one for c = -4096
        assert not np.array_equal(v3, rgb), "the version 3 decode is expected to differ from its input"
    print(f"{w}x{h}x{f} wavelet {kind}: version 3 at q = 100 gives {WO.psnr(rgb, v3):.2f} dB, version 4 the input")


# ---- bit-exact at lossy steps: every instance the launcher can pick ----
STEP_OF = {100: 1, 95: 5, 80: 14, 0: 64}          # wide classes 3, 2, 1, 0 for CDF 5/3


@pytest.mark.parametrize("q", sorted(STEP_OF, reverse=True))
@pytest.mark.parametrize("kind", [CDF53, CDF97, HAAR])
@pytest.mark.parametrize("shape", [(100, 36, 6), (33, 17, 5)])
def test_pixels_equal_the_reference_at_every_class(gpu_codec, shape, kind, q):
    a = gpu_codec
    w, h, f = shape
    step = STEP_OF[q]
    variant = a.load_library().alice_codec_test_inverse_variant(kind, (C.c_int32 * 3)(step, step, step), 1)
    rgb = content("random_0_255" if q == 100 else "smooth_plus_noise", w, h, f)     # 0/255: the largest magnitudes
    enc = a.FrameEncoder.with_wavelet(q, a.WaveletType(kind))
    blob = a.encode_reversible(enc, rgb, w, h, f, 64)
    assert a.reversible_info(blob).quant_step == [step] * 3
    want = RR.roundtrip(rgb, w, h, f, q, kind)
    got = a.decode_reversible(blob)
    assert np.array_equal(got, want), (shape, kind, q, variant)
    if shape == (33, 17, 5):
        assert blob == RR.encode(rgb, w, h, f, q, kind, 64)            # the container, byte for byte
        assert np.array_equal(RR.decode(blob), want)                   # and the reference's own decode of it
    print(f"{w}x{h}x{f} wavelet {kind} q={q} step {step}: instance class {variant}, {WO.psnr(rgb, got):.2f} dB")


def test_the_classes_above_covered_every_instance(gpu_codec):
    """CDF 5/3 and Haar (NS = 2) reach classes 3, 2, 1 and 0 at steps 1, 5, 14 and 64; CDF 9/7 (NS = 4) has only 2 and 0
    in the wide class table (tests/test_inverse_bounds_host.py, FIRST_STEP)."""
    lib = gpu_codec.load_library()
    table = {(k, s): lib.alice_codec_test_inverse_variant(k, (C.c_int32 * 3)(s, s, s), 1) for k in (0, 1, 2) for s in STEP_OF.values()}
    assert {table[(CDF53, s)] for s in STEP_OF.values()} == {0, 1, 2, 3}
    assert [table[(CDF53, s)] for s in (1, 5, 14, 64)] == [3, 2, 1, 0]
    assert {table[(CDF97, s)] for s in STEP_OF.values()} == {0, 2}


# ---- bands ----
def test_banded_chunk_is_lossless_and_equals_the_uncut_decode(gpu_codec):
    a = gpu_codec
    lib = a.load_library()
    w, h, f = 300, 104, 4
    for kind, q in ((CDF53, 100), (CDF97, 100), (HAAR, 95)):
        rgb = content("uniform_noise", w, h, f)
        blob = a.encode_reversible(a.FrameEncoder.with_wavelet(q, a.WaveletType(kind)), rgb, w, h, f, 256)
        uncut = a.decode_reversible(blob)
        try:
            lib.alice_codec_test_set_tuning(96)       # one tile row per band: four bands of the 104 rows
            cut_blob = a.encode_reversible(a.FrameEncoder.with_wavelet(q, a.WaveletType(kind)), rgb, w, h, f, 256)
            cut = a.decode_reversible(blob)
        finally:
            lib.alice_codec_test_set_tuning(1024 * 1024)
        assert cut_blob == blob and np.array_equal(cut, uncut), (kind, q)
        if q == 100:
            assert np.array_equal(cut, rgb), kind
        else:
            assert np.array_equal(cut, RR.roundtrip(rgb, w, h, f, q, kind)), kind


# ---- bytes ----
@pytest.mark.parametrize("shape,kind,q", [((100, 36, 6), CDF97, 100), ((33, 17, 5), CDF53, 80), ((5, 3, 1), HAAR, 100)])
def test_bytes_are_version_3s_except_byte_4(gpu_codec, shape, kind, q):
    a = gpu_codec
    w, h, f = shape
    rgb = content("smooth_plus_noise", w, h, f)
    enc = a.FrameEncoder.with_wavelet(q, a.WaveletType(kind))
    v4, v3 = a.encode_reversible(enc, rgb, w, h, f, 128), a.encode_wide(enc, rgb, w, h, f, 128)
    assert len(v4) == len(v3) and v4[4] == 4 and v3[4] == 3
    assert v4[:4] == v3[:4] and v4[5:] == v3[5:]
    p = a.predict_wide_sizes(rgb, w, h, f, kind, 128)
    assert int(p.lo[q]) <= len(v4) <= int(p.hi[q]), (int(p.lo[q]), len(v4), int(p.hi[q]))


# ---- device batch ----
def test_device_batch_with_per_chunk_qualities(gpu_codec):
    a = gpu_codec
    w, h, f, n, L = 100, 36, 6, 3, 128
    kind = CDF53
    quals = [100, 100, 80]
    chunks = [content(name, w, h, f, seed=30 + i) for i, name in enumerate(("uniform_noise", "random_0_255", "smooth_plus_noise"))]
    stride = _stride(a, w, h, f, L)
    d_rgb = _dev(np.concatenate(chunks))
    d_out = torch.zeros(n * stride, dtype=torch.uint8, device=DEV)
    d_back = torch.full((GUARD + n * w * h * f * 3 + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    sizes = a.reversible_encode_device(d_rgb.data_ptr(), w, h, f, n, kind, 0, d_out.data_ptr(), stride, qualities=quals, lane_symbols=L)
    a.reversible_decode_device(d_out.data_ptr(), stride, sizes, d_back.data_ptr() + GUARD)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    host = d_back.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[-GUARD:] == SENTINEL).all()
    back = host[GUARD:-GUARD].reshape(n, -1)
    for i in range(n):
        blob = out[i * stride:i * stride + int(sizes[i])].tobytes()
        assert blob == a.encode_reversible(a.FrameEncoder.with_wavelet(quals[i], a.WaveletType(kind)), chunks[i], w, h, f, L), i
    assert np.array_equal(back[0], chunks[0]) and np.array_equal(back[1], chunks[1])
    assert np.array_equal(back[2], RR.roundtrip(chunks[2], w, h, f, 80, kind))
    # encode_lossless_device: quality 100 for every chunk
    d_out.zero_()
    sizes2 = a.encode_lossless_device(d_rgb.data_ptr(), w, h, f, n, d_out.data_ptr(), stride, kind, L)
    d_back.fill_(SENTINEL)
    a.reversible_decode_device(d_out.data_ptr(), stride, sizes2, d_back.data_ptr() + GUARD)
    torch.cuda.synchronize()
    assert np.array_equal(d_back.cpu().numpy()[GUARD:-GUARD], np.concatenate(chunks))
    assert int(sizes2[0]) == int(sizes[0]) and int(sizes2[1]) == int(sizes[1])


# ---- regions ----
@pytest.mark.parametrize("kind", [CDF53, CDF97])
def test_regions_of_640x360_frames(gpu_codec, kind):
    a = gpu_codec
    W, H, bw, bh, f, L = 640, 360, 100, 36, 2, 64
    origins = [(13, 7), (48, 32), (540, 324)]        # x0 % 4 != 0; x0 % 4 == 0; pushed into the bottom right corner
    n = len(origins)
    rng = np.random.default_rng(77 + kind)
    src = rng.integers(0, 256, (n * f, H, W, 3), dtype=np.uint8)
    d = _dev(src)
    stride = _stride(a, bw, bh, f, L)
    out = torch.full((n * stride,), 0xCD, dtype=torch.uint8, device=DEV)
    sizes = a.reversible_encode_regions_device(d.data_ptr(), W, H, origins, bw, bh, f, kind, 100, out.data_ptr(), stride, None, L)
    host = out.cpu().numpy().reshape(n, stride)
    for i, (x0, y0) in enumerate(origins):
        crop = np.ascontiguousarray(src[i * f:(i + 1) * f, y0:y0 + bh, x0:x0 + bw]).reshape(-1)
        assert host[i, :int(sizes[i])].tobytes() == a.encode_lossless(crop, bw, bh, f, kind, L), i
        assert (host[i, int(sizes[i]):] == 0xCD).all()
    total = n * f * H * W * 3
    frames_out = torch.full((GUARD + total + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    a.reversible_decode_regions_device(out.data_ptr(), stride, sizes, frames_out.data_ptr() + GUARD, W, H, origins)
    torch.cuda.synchronize()
    got = frames_out.cpu().numpy()
    assert (got[:GUARD] == SENTINEL).all() and (got[-GUARD:] == SENTINEL).all(), "guard bytes were written"
    want = np.full((n * f, H, W, 3), SENTINEL, np.uint8)
    for i, (x0, y0) in enumerate(origins):
        want[i * f:(i + 1) * f, y0:y0 + bh, x0:x0 + bw] = src[i * f:(i + 1) * f, y0:y0 + bh, x0:x0 + bw]
    assert np.array_equal(got[GUARD:-GUARD].reshape(want.shape), want)    # exact inside the boxes, untouched outside
    assert np.array_equal(d.cpu().numpy(), src)
    with pytest.raises(a.CodecError) as e:
        a.reversible_encode_regions_device(d.data_ptr(), W, H, [(W - bw + 1, 0)] * n, bw, bh, f, kind, 100, out.data_ptr(), stride, None, L)
    assert e.value.code == 2


# ---- person flow ----
def test_person_chunks_in_v4_and_a_list_of_all_four_versions(gpu_codec):
    a = gpu_codec
    W, H, f, n, bg, frames = _person_frames()
    L, q = 64, 100
    d_frames, d_bg = _dev(frames), _dev(bg)
    v1 = a.encode_person_chunks(d_frames, d_bg, W, H, f, n, q)
    v2 = a.encode_person_chunks(d_frames, d_bg, W, H, f, n, q, format="split", lane_symbols=L)
    v3 = a.encode_person_chunks(d_frames, d_bg, W, H, f, n, q, format="wide", lane_symbols=L)
    v4 = a.encode_person_chunks(d_frames, d_bg, W, H, f, n, q, format="reversible", lane_symbols=L)
    assert [b for b, _ in v4] == [b for b, _ in v1]
    for c, (bbox, alc) in enumerate(v4):
        assert a.alc_version(alc) == 4 and alc[5:] == v3[c][1][5:]
        if c == 2:
            assert bbox == [0, 0, 0, 0] and alc == a.encode_reversible(a.FrameEncoder(q, a.WaveletType.Cdf53), b"", 0, 0, f, L)

    def decoded(chunks):
        out = _dev(np.repeat(bg[None], n * f, axis=0))
        a.decode_person_chunks(chunks, out, W, H, f)
        return out.cpu().numpy().reshape(n * f, H, W, 3)

    back = decoded(v4)
    want = np.repeat(bg[None], n * f, axis=0)
    for c, (b, _) in enumerate(v4):
        want[c * f:(c + 1) * f, b[1]:b[1] + b[3], b[0]:b[0] + b[2]] = frames[c * f:(c + 1) * f, b[1]:b[1] + b[3], b[0]:b[0] + b[2]]
    assert np.array_equal(back, want)             # the boxes exactly, the background untouched
    mixed = [v1[0], v2[1], v3[2], v4[3]]
    assert [a.alc_version(x) for _, x in mixed] == [1, 2, 3, 4]
    pasted = np.repeat(bg[None], n * f, axis=0).reshape(n * f, H, 3 * W)
    for c, (bbox, alc) in enumerate(mixed):
        bx, by, bw, bh = bbox
        if bw * bh:
            dec = a.decode_alc(alc).reshape(f, -1)
            for t in range(f):
                a.paste_bbox_numpy(pasted[c * f + t], dec[t], [3 * bx, by, 3 * bw, bh])
    assert np.array_equal(decoded(mixed).reshape(n * f, H, 3 * W), pasted)
    assert np.array_equal(decoded([v4[0], v3[1], v1[2], v2[3]])[:f], want[:f])
    with pytest.raises(a.CodecError):
        a.encode_person_chunks(d_frames, d_bg, W, H, f, n, q, format="reversible", max_bytes=10**6)


# ---- refusals and damage ----
def dev_decode(a, fn, blob, n_out):
    """a device decode of one container into a guarded, sentinel-filled buffer -> (error code or 0, message, pixels)"""
    d_alc = _dev(np.frombuffer(blob + b"\0\0\0\0", np.uint8).copy())
    d_rgb = torch.full((GUARD + n_out + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    code, msg = 0, ""
    try:
        fn(d_alc.data_ptr(), len(blob), [len(blob)], d_rgb.data_ptr() + GUARD)
    except a.CodecError as e:
        code, msg = e.code, str(e)
    torch.cuda.synchronize()
    host = d_rgb.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[-GUARD:] == SENTINEL).all(), "memory outside the output was written"
    return code, msg, host[GUARD:-GUARD]


def test_the_wide_and_reversible_calls_refuse_each_other(gpu_codec):
    a = gpu_codec
    w, h, f = 33, 17, 5
    rgb = content("smooth_plus_noise", w, h, f)
    enc = a.FrameEncoder.with_wavelet(100, a.WaveletType.Cdf53)
    v4, v3 = a.encode_reversible(enc, rgb, w, h, f, 64), a.encode_wide(enc, rgb, w, h, f, 64)
    n_out = w * h * f * 3
    for fn, blob, words in ((a.wide_decode_device, v4, "unsupported version: 4 (expected 3)"),
                            (a.reversible_decode_device, v3, "unsupported version: 3 (expected 4)"),
                            (a.split_decode_device, v4, "unsupported version: 4 (expected 2)")):
        code, msg, pixels = dev_decode(a, fn, blob, n_out)
        assert code == 4 and words in msg and (pixels == SENTINEL).all()
    for fn, blob, words in ((a.decode_wide, v4, "unsupported version: 4 (expected 3)"), (a.decode_reversible, v3, "unsupported version: 3 (expected 4)"),
                            (a.wide_info, v4, "unsupported version: 4 (expected 3)"), (a.reversible_info, v3, "unsupported version: 3 (expected 4)")):
        with pytest.raises(a.CodecError) as e:
            fn(blob)
        assert e.value.code == 4 and words in str(e.value)
    frames_out = torch.full((f * 40 * 60 * 3,), SENTINEL, dtype=torch.uint8, device=DEV)
    for fn, blob in ((a.wide_decode_regions_device, v4), (a.reversible_decode_regions_device, v3)):
        d_alc = _dev(np.frombuffer(blob, np.uint8).copy())
        with pytest.raises(a.CodecError, match="unsupported version"):
            fn(d_alc.data_ptr(), len(blob), [len(blob)], frames_out.data_ptr(), 60, 40, [(3, 2)])
        assert (frames_out.cpu().numpy() == SENTINEL).all()
    code, _, pixels = dev_decode(a, a.reversible_decode_device, v4, n_out)
    assert code == 0 and np.array_equal(pixels, rgb)


def test_damage_decodes_or_fails_as_version_3_does(gpu_codec):
    """Truncations and byte flips behind the directories: the verdict is version 3's on the same damage (the parser, the
    lanes and the end checks are shared), nothing outside the output is written, and where the stream still passes its end
    checks the pixels are the mirrored inverse of the symbols it holds.  Bounds safety only: nothing here is built to fault."""
    a = gpu_codec
    w, h, f, L = 33, 17, 5, 64
    rgb = content("uniform_noise", w, h, f)
    v4 = a.encode_reversible(a.FrameEncoder.with_wavelet(100, a.WaveletType.Haar), rgb, w, h, f, L)
    info = a.reversible_info(v4)
    rng = np.random.default_rng(5)
    first_stream = R3.HEADER + 4 * info.n_blocks[0] + 128      # behind the block table and the first lane directory
    cases = [("truncated to the header", v4[:R3.HEADER]), ("truncated mid payload", v4[:len(v4) - 777]), ("one byte short", v4[:-1]),
             ("extended", v4 + b"\0")]
    for i in range(10):
        pos = int(rng.integers(first_stream, len(v4)))
        b = bytearray(v4)
        b[pos] ^= 1 << int(rng.integers(8))
        cases.append((f"flip at {pos}", bytes(b)))
    n_out = w * h * f * 3
    verdicts = set()
    for name, bad in cases:
        c4, m4, p4 = dev_decode(a, a.reversible_decode_device, bad, n_out)
        c3, m3, _ = dev_decode(a, a.wide_decode_device, RR.with_version(bad, 3), n_out)
        assert c4 == c3 and m4.replace("(expected 4)", "") == m3.replace("(expected 3)", ""), (name, c4, c3, m4, m3)
        verdicts.add(c4)
        if c4 == 0:
            assert np.array_equal(p4, RR.decode(bad)), name
        try:
            host4 = a.decode_reversible(bad)
            assert c4 == 0 and np.array_equal(host4, p4), name
        except a.CodecError as e:
            assert e.code == c4, name
    assert 4 in verdicts


# ---- the generic kernels' geometry ----
@pytest.fixture
def grid_cap(gpu_codec):
    lib = gpu_codec.load_library()
    yield lambda max_blocks: lib.alice_codec_test_set_grid_cap(max_blocks)
    lib.alice_codec_test_set_grid_cap(0)


def test_generic_mirrored_inverse_under_small_grids(gpu_codec, grid_cap):
    """5x3x2 (24 pairs a step: a partial trip), 4x4x32 (256: exactly one trip of one workgroup) and 4x4x40 (320: several
    trips at a cap of 1, a partial one at 3) through the mirrored axis_lift_kernel; the result does not depend on the cap."""
    a = gpu_codec
    for (w, h, f) in ((5, 3, 2), (4, 4, 32), (4, 4, 40)):
        for kind, q in ((CDF53, 100), (CDF97, 100), (HAAR, 80)):
            rgb = content("random_0_255", w, h, f)
            want = RR.roundtrip(rgb, w, h, f, q, kind)
            if q == 100:
                assert np.array_equal(want, rgb)
            enc = a.FrameEncoder.with_wavelet(q, a.WaveletType(kind))
            blob = a.encode_reversible(enc, rgb, w, h, f, 64)
            for cap in (1, 3, 0):
                grid_cap(cap)
                assert a.encode_reversible(enc, rgb, w, h, f, 64) == blob, (w, h, f, kind, cap)
                assert np.array_equal(a.decode_reversible(blob), want), (w, h, f, kind, q, cap)
