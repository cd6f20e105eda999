"""alice_codec_dev_trial_sse against the CPU oracle (tests/quality_ref.py) and, as a consequence of the contract, against the
library's own encode -> decode of each container: the trial's number IS the squared error of the decoded pixels."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quality_ref as Q  # noqa: E402
import wide_oracle as WO  # noqa: E402

import torch  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(33, 17, 5), (64, 48, 8), (96, 64, 16)]
QUALITIES = {Q.FORMAT_SPLIT: (50, 80, 96), Q.FORMAT_WIDE: (50, 80, 95, 100), Q.FORMAT_REVERSIBLE: (100, 80)}
NAMES = {Q.FORMAT_SPLIT: "split", Q.FORMAT_WIDE: "wide", Q.FORMAT_REVERSIBLE: "reversible"}
_content = {}


def content(kind: str, w, h, f, seed=None):
    key = (kind, w, h, f, seed)
    if key not in _content:
        if kind == "smooth":
            _content[key] = WO.smooth_plus_noise(w, h, f, seed=(w + h + f) if seed is None else seed)
        else:
            rng = np.random.default_rng(w * 7 + h if seed is None else seed)
            _content[key] = (rng.integers(0, 2, w * h * f * 3, dtype=np.uint8) * 255).astype(np.uint8)
    return _content[key]


def library_roundtrip(codec, version, rgb, w, h, f, k, q):
    enc = codec.FrameEncoder.with_wavelet(q, codec.WaveletType(k))
    encode = {2: codec.encode_split, 3: codec.encode_wide, 4: codec.encode_reversible}[version]
    decode = {2: codec.decode_split, 3: codec.decode_wide, 4: codec.decode_reversible}[version]
    return decode(encode(enc, rgb, w, h, f))


@pytest.mark.parametrize("what", ["smooth", "binary"])
@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_trial_equals_the_oracle_and_the_decode(gpu_codec, shape, k, what):
    a = gpu_codec
    w, h, f = shape
    rgb = content(what, w, h, f)
    d_rgb = torch.from_numpy(rgb).to(DEV)
    for version, qualities in QUALITIES.items():
        for q in qualities:
            d_fs = torch.full((f + 2,), -7, dtype=torch.int64, device=DEV)
            sse = a.trial_sse_device(version, d_rgb.data_ptr(), w, h, f, 1, a.WaveletType(k), q, d_frame_sse_ptr=d_fs.data_ptr() + 8)
            pixels = Q.reconstruct(version, rgb, w, h, f, q, k)
            want = Q.sse_of(rgb, pixels)
            print(f"{NAMES[version]} {w}x{h}x{f} wavelet {k} q {q} {what}: trial {int(sse[0])}, oracle {want}")
            assert int(sse[0]) == want, (version, shape, k, q)
            fs = d_fs.cpu().numpy()
            assert fs[0] == -7 and fs[-1] == -7
            per_frame = fs[1:-1].view(np.uint64)
            assert np.array_equal(per_frame, Q.frame_sse(rgb, pixels, f)) and int(per_frame.sum()) == int(sse[0])
            # the contract, as a consequence: what the library's own decode of its own encode returns
            assert Q.sse_of(rgb, library_roundtrip(a, version, rgb, w, h, f, k, q)) == int(sse[0]), (version, shape, k, q)
            if version == Q.FORMAT_REVERSIBLE and q == 100:
                assert int(sse[0]) == 0
            # the name and the byte select the same container; without d_frame_sse the call lends its own memory
            assert int(a.trial_sse_device(NAMES[version], d_rgb.data_ptr(), w, h, f, 1, a.WaveletType(k), q)[0]) == want
    assert torch.equal(d_rgb.cpu(), torch.from_numpy(rgb))


def test_per_chunk_qualities_and_psnr(gpu_codec):
    a = gpu_codec
    w, h, f, k = 64, 48, 8, 1
    chunks = [content("smooth", w, h, f, seed=11), content("binary", w, h, f, seed=12), content("smooth", w, h, f, seed=13)]
    d_rgb = torch.from_numpy(np.concatenate(chunks)).to(DEV)
    n = w * h * f * 3
    for version, quals in ((2, [50, 96, 80]), (3, [100, 50, 95]), (4, [100, 80, 100])):
        d_fs = torch.zeros(3 * f, dtype=torch.int64, device=DEV)
        sse = a.trial_sse_device(version, d_rgb.data_ptr(), w, h, f, 3, a.WaveletType(k), 0, qualities=quals, d_frame_sse_ptr=d_fs.data_ptr())
        fs = d_fs.cpu().numpy().view(np.uint64).reshape(3, f)
        for i in range(3):
            pixels = Q.reconstruct(version, chunks[i], w, h, f, quals[i], k)
            assert int(sse[i]) == Q.sse_of(chunks[i], pixels), (version, i)
            assert np.array_equal(fs[i], Q.frame_sse(chunks[i], pixels, f)), (version, i)
        db = a.trial_psnr_device(version, d_rgb.data_ptr(), w, h, f, 3, a.WaveletType(k), 0, qualities=quals)
        assert list(db) == [Q.psnr_from_sse(int(s), n) for s in sse]
        same = a.trial_sse_device(version, d_rgb.data_ptr(), w, h, f, 3, a.WaveletType(k), quals[1])
        assert int(same[1]) == int(sse[1])


def test_groups_do_not_change_the_numbers(gpu_codec):
    """A shape the tile kernels do not cover (padded width below 6) runs the generic path; many chunks in one call."""
    a = gpu_codec
    w, h, f, k, n = 3, 40, 4, 0, 7
    chunks = [content("smooth", w, h, f, seed=60 + i) for i in range(n)]
    d_rgb = torch.from_numpy(np.concatenate(chunks)).to(DEV)
    for version in (2, 3, 4):
        sse = a.trial_sse_device(version, d_rgb.data_ptr(), w, h, f, n, a.WaveletType(k), 80)
        assert [int(s) for s in sse] == [Q.chunk_sse(version, c, w, h, f, 80, k) for c in chunks]


def test_trials_of_a_chunk_cut_into_bands(gpu_codec):
    """Under a 4 MiB band target a 256x256x16 chunk is cut into four bands by the inverse's i32 plan (1.5 MiB per tile row) and
    not at all by its i16 plan (0.75 MiB per tile row: fewer than two bands' worth), whose slot is then the whole frame and the
    larger of the two.  Steps of either sample width run through one call's buffers; the numbers are the oracle's and those of
    the library's own encode -> decode under the same plan."""
    a = gpu_codec
    lib = a.load_library()
    w, h, f, k = 256, 256, 16, 1
    rgb = content("smooth", w, h, f, seed=2)
    d_rgb = torch.from_numpy(rgb).to(DEV)
    cases = [(2, 80), (3, 80), (3, 100), (4, 100)]
    variants = set()
    for version, q in cases:
        step = (C.c_int32 * 3)(*[Q.step_of(q)] * 3)
        variants.add(int(lib.alice_codec_test_inverse_variant(k, step, int(version != 2))) >= 2)
    assert True in variants, "no case takes the i16 band plan"
    try:
        lib.alice_codec_test_set_tuning(4096)
        i16, i32 = (int(lib.alice_codec_test_inverse_scratch_bytes(w, h, f, m)) for m in (1, 0))
        assert i16 > i32 + (2 << 20) and i16 >= 256 * 256 * 16 * 3 * 2, (i16, i32)   # the whole frame in i16 against a quarter in i32
        for version, q in cases:
            sse = a.trial_sse_device(version, d_rgb.data_ptr(), w, h, f, 1, a.WaveletType(k), q)
            assert int(sse[0]) == Q.chunk_sse(version, rgb, w, h, f, q, k), (version, q)
            assert Q.sse_of(rgb, library_roundtrip(a, version, rgb, w, h, f, k, q)) == int(sse[0]), (version, q)
        # one call, one set of buffers, steps of both sample widths
        three = torch.from_numpy(np.concatenate([rgb, rgb, rgb])).to(DEV)
        quals = [100, 80, 50]
        sse = a.trial_sse_device(3, three.data_ptr(), w, h, f, 3, a.WaveletType(k), 0, qualities=quals)
        assert [int(s) for s in sse] == [Q.chunk_sse(3, rgb, w, h, f, q, k) for q in quals]
        # and the search, whose trials share one set of buffers across steps
        t = 0.5 * (Q.psnr_from_sse(Q.chunk_sse(3, rgb, w, h, f, 80, k), rgb.size) + Q.psnr_from_sse(Q.chunk_sse(3, rgb, w, h, f, 100, k), rgb.size))
        data, q, reached, db = a.encode_wide_to_psnr(rgb, w, h, f, t, a.WaveletType(k), 50, 100)
        assert reached and 80 < q <= 100
        assert db == Q.psnr_from_sse(Q.sse_of(rgb, a.decode_wide(data)), rgb.size) >= t
    finally:
        lib.alice_codec_test_set_tuning(1024 * 1024)
    assert torch.equal(d_rgb.cpu(), torch.from_numpy(rgb))


def test_regions_ignore_what_lies_outside(gpu_codec):
    a = gpu_codec
    W, H, w, h, f, k = 640, 360, 97, 51, 4, 1
    origins = [(3, 5), (541, 307), (1, 0)]
    n = len(origins)
    rng = np.random.default_rng(21)
    frames = rng.integers(0, 256, (n * f, H, W, 3), dtype=np.uint8)             # noise everywhere
    crops = []
    for i, (x0, y0) in enumerate(origins):
        crop = content("smooth", w, h, f, seed=30 + i).reshape(f, h, w, 3)
        frames[i * f:(i + 1) * f, y0:y0 + h, x0:x0 + w] = crop
        crops.append(crop.reshape(-1))
    d_frames = torch.from_numpy(frames.reshape(-1)).to(DEV)
    for version, q in ((2, 80), (3, 95), (4, 100)):
        d_fs = torch.zeros(n * f, dtype=torch.int64, device=DEV)
        sse = a.trial_sse_device(version, d_frames.data_ptr(), w, h, f, n, a.WaveletType(k), q, frame_width=W, frame_height=H,
                                 origins=origins, d_frame_sse_ptr=d_fs.data_ptr())
        fs = d_fs.cpu().numpy().view(np.uint64).reshape(n, f)
        for i in range(n):
            pixels = Q.reconstruct(version, crops[i], w, h, f, q, k)
            assert int(sse[i]) == Q.sse_of(crops[i], pixels), (version, i)
            assert np.array_equal(fs[i], Q.frame_sse(crops[i], pixels, f))
        # other noise outside the rectangles: the same numbers
        other = rng.integers(0, 256, frames.shape, dtype=np.uint8)
        for i, (x0, y0) in enumerate(origins):
            other[i * f:(i + 1) * f, y0:y0 + h, x0:x0 + w] = frames[i * f:(i + 1) * f, y0:y0 + h, x0:x0 + w]
        d_other = torch.from_numpy(other.reshape(-1)).to(DEV)
        again = a.trial_sse_device(version, d_other.data_ptr(), w, h, f, n, a.WaveletType(k), q, frame_width=W, frame_height=H,
                                   origins=origins)
        assert list(again) == list(sse)
    assert torch.equal(d_frames.cpu(), torch.from_numpy(frames.reshape(-1)))     # the source is only read
