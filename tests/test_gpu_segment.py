"""Person segmentation (src/segment.rs) on the MI355X: the reference's inline tests through the GPU entry points,
bit-exact parity with the vectorised restatement (tests/segment_ref.py) over shapes that straddle the 64-pixel words,
radii up to 2^32-1, both reference strides and batches of frames, the fused RGB chroma call, the RLE and
extract_person_rgb, and the hybrid flow (segment, union bbox, crop, encode, decode, paste)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segment_ref as R  # noqa: E402

import torch  # noqa: E402

pytestmark = pytest.mark.gpu
BIG = 2 ** 32 - 1


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _frames(rng, n, h, w):
    """reference frames and current frames with moving rectangles and speckles"""
    ref = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    cur = ref.copy()
    for f in range(n):
        for _ in range(3):
            y0, x0 = rng.integers(0, h), rng.integers(0, w)
            y1, x1 = min(h, y0 + rng.integers(1, max(2, h // 2))), min(w, x0 + rng.integers(1, max(2, w // 2)))
            cur[f, y0:y1, x0:x1] = 255 - cur[f, y0:y1, x0:x1]
        speck = rng.random((h, w)) < 0.01
        cur[f][speck] = rng.integers(0, 256, int(speck.sum()), dtype=np.uint8)
    return cur, ref


def _device_motion(codec, cur, ref, shared, thr, rd, re, with_mask=True):
    n, h, w = cur.shape
    dc, dr = _dev(cur), _dev(ref[:1] if shared else ref)
    stats = torch.zeros(n * 5, dtype=torch.int32, device="cuda:0")
    mask = torch.full((n, h, w), 7, dtype=torch.uint8, device="cuda:0") if with_mask else None
    codec.segment_motion_device(dc.data_ptr(), dr.data_ptr(), 0 if shared else w * h, w, h, n, stats.data_ptr(),
                                mask.data_ptr() if with_mask else None, codec.SegmentConfig(thr, 100, rd, re))
    st = stats.cpu().numpy().view(np.uint32).reshape(n, 5).astype(np.int64)
    return (mask.cpu().numpy() if with_mask else None), st


# ---- the reference's inline tests through the GPU entry points ----

def test_reference_kats_on_gpu(gpu_codec):
    a = gpu_codec
    cur = np.zeros(200, np.uint8)
    for y in range(3, 7):
        cur[y * 20 + 5:y * 20 + 15] = 200
    r = a.segment_by_motion(cur, np.zeros(200, np.uint8), 20, 10, a.SegmentConfig(50, 100, 0, 0))
    assert r.foreground_count == 40 and r.bbox == [5, 3, 10, 4] and 0.0 < r.coverage() < 0.5
    cur = np.zeros(600, np.uint8)
    for y in range(5, 15):
        cur[y * 30 + 8:y * 30 + 22] = 180
    r = a.segment_by_motion(cur, np.zeros(600, np.uint8), 30, 20, a.SegmentConfig(30, 100, 2, 1))
    assert 0.1 < r.coverage() < 0.8
    assert list(r.mask) == R.lit_motion(list(cur), [0] * 600, 30, 20, 30, 2, 1)[0]
    r = a.segment_by_motion(np.full(100, 100, np.uint8), np.full(100, 100, np.uint8), 10, 10, a.SegmentConfig(25, 100, 0, 0))
    assert r.foreground_count == 0 and r.bbox == [0, 0, 0, 0]
    r = a.segment_by_motion(np.full(64, 255, np.uint8), np.zeros(64, np.uint8), 8, 8, a.SegmentConfig(50, 100, 0, 0))
    assert r.foreground_count == 64 and r.coverage() == 1.0
    m = np.zeros(25, np.uint8); m[12] = 1          # the dilate cross, :597-614, as a motion mask
    r = a.segment_by_motion(m, np.zeros(25, np.uint8), 5, 5, a.SegmentConfig(0, 100, 1, 0))
    assert r.mask.reshape(5, 5)[1:4, 1:4].all() and r.foreground_count == 9
    m = np.zeros((10, 10), np.uint8); m[2:7, 3:8] = 1
    r = a.segment_by_motion(m, np.zeros(100, np.uint8), 10, 10, a.SegmentConfig(0, 100, 0, 0))
    assert (r.bbox, r.foreground_count) == ([3, 2, 5, 5], 25)
    m = np.zeros(100, np.uint8); m[55] = 1
    assert a.segment_by_motion(m, np.zeros(100, np.uint8), 10, 10, a.SegmentConfig(0, 100, 0, 0)).bbox == [5, 5, 1, 1]
    cg = np.full(50, 100, np.int16)
    for row in range(1, 4):
        cg[row * 10 + 2:row * 10 + 8] = -10
    r = a.segment_by_chroma(None, None, cg, 10, 5, 50)
    assert r.foreground_count > 0 and list(r.mask) == R.lit_chroma(list(cg), 10, 5, 50)[0]
    m = np.zeros(40, np.uint8); m[10:30] = 1
    assert len(a.rle_encode_mask(m)) == 9
    assert a.rle_encode_mask(np.zeros(100, np.uint8)) == bytes([100, 0, 0])
    assert a.rle_encode_mask(np.ones(50, np.uint8)) == bytes([50, 0, 1])
    rgb = np.zeros(150, np.uint8); mk = np.zeros(50, np.uint8)
    for y in range(2, 4):
        for x in range(3, 6):
            rgb[(y * 10 + x) * 3:(y * 10 + x) * 3 + 3] = [255, 128, 64]; mk[y * 10 + x] = 1
    person = a.SegmentResult(mk, [3, 2, 3, 2], 6, 10, 5).extract_person_rgb(rgb)
    assert len(person) == 18 and person[:3] == bytes([255, 128, 64])


def test_erosion_keeps_the_border_and_big_radii(gpu_codec):
    a = gpu_codec
    ones = np.full(35, 200, np.uint8)
    for re in (1, 3, BIG):
        r = a.segment_by_motion(ones, np.zeros(35, np.uint8), 7, 5, a.SegmentConfig(0, 100, 0, re))
        assert r.foreground_count == 35
    m = np.zeros(30, np.uint8); m[7] = 1
    r = a.segment_by_motion(m, np.zeros(30, np.uint8), 6, 5, a.SegmentConfig(0, 100, BIG, 0))
    assert r.foreground_count == 30
    m = np.ones(30, np.uint8); m[29] = 0
    r = a.segment_by_motion(m, np.zeros(30, np.uint8), 6, 5, a.SegmentConfig(0, 100, 0, BIG))
    assert r.foreground_count == 0 and r.bbox == [0, 0, 0, 0]
    for t, want in ((255, 0), (0, 3)):
        r = a.segment_by_motion(np.array([0, 255, 3, 3], np.uint8), np.array([255, 0, 3, 4], np.uint8), 2, 2,
                                a.SegmentConfig(t, 100, 0, 0))
        assert r.foreground_count == want


# ---- parity with restatement (b) ----

RADII = [(0, 0), (1, 1), (2, 7), (64, 65), (65, 64), (300, 2), (7, 300), (BIG, 1), (2, BIG)]


@pytest.mark.parametrize("w", [1, 63, 64, 65, 127, 1920])
@pytest.mark.parametrize("h", [1, 2, 1080])
def test_motion_parity_grid(gpu_codec, w, h):
    rng = np.random.default_rng(w * 7919 + h)
    big = w * h >= 100000
    n = 8 if not big else 2
    cur, ref = _frames(rng, n, h, w)
    radii = RADII if not big else [(2, 1), (64, 65), (300, 300), (BIG, 1)]
    for i, (rd, re) in enumerate(radii):
        thr = int(rng.choice([0, 25, 100]))
        for shared in (True, False):
            frames = n if (i + shared) % 2 == 0 else 1
            c = cur[:frames]
            rr = ref[:1] if shared else ref[:frames]
            mask, st = _device_motion(gpu_codec, c, rr, shared, thr, rd, re)
            want_m, want_st = R.vec_motion(c, rr, thr, rd, re)
            assert np.array_equal(mask, want_m), (w, h, rd, re, shared, frames)
            assert np.array_equal(st, want_st), (w, h, rd, re, shared, frames, st, want_st)


def test_full_hd_batch_and_stats_only(gpu_codec):
    rng = np.random.default_rng(5)
    cur, ref = _frames(rng, 8, 1080, 1920)
    for shared in (True, False):
        rr = ref[:1] if shared else ref
        mask, st = _device_motion(gpu_codec, cur, rr, shared, 25, 2, 1)
        want_m, want_st = R.vec_motion(cur, rr, 25, 2, 1)
        assert np.array_equal(mask, want_m) and np.array_equal(st, want_st)
        _, st2 = _device_motion(gpu_codec, cur, rr, shared, 25, 2, 1, with_mask=False)
        assert np.array_equal(st2, st)


def test_wide_rows_of_many_chunks(gpu_codec):
    """rows of more than 64 words (4096 pixels) take the two-sweep horizontal pass"""
    rng = np.random.default_rng(9)
    for w, h in ((9000, 3), (70000, 1), (4097, 5)):
        cur, ref = _frames(rng, 2, h, w)
        cur[:, :, 100:] = ref[:, :, 100:]            # sparse: set pixels far apart along the row
        cur[:, 0, w - 5] = ref[:, 0, w - 5] ^ 0xFF
        for rd, re in ((1, 0), (3000, 1), (5000, 4500), (BIG, 0)):
            mask, st = _device_motion(gpu_codec, cur, ref, False, 25, rd, re)
            want_m, want_st = R.vec_motion(cur, ref, 25, rd, re)
            assert np.array_equal(mask, want_m), (w, h, rd, re)
            assert np.array_equal(st, want_st)


def test_chroma_host_and_fused_rgb(gpu_codec):
    a = gpu_codec
    rng = np.random.default_rng(11)
    for w, h, n in ((65, 33, 3), (1920, 1080, 2)):
        rgb = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
        rgb[:, h // 4:h // 2, w // 3:w // 2, 1] = 255        # greener block
        thr = 10
        d = _dev(rgb)
        stats = torch.zeros(n * 5, dtype=torch.int32, device="cuda:0")
        mask = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda:0")
        a.segment_chroma_rgb_device(d.data_ptr(), w, h, n, thr, stats.data_ptr(), mask.data_ptr())
        st = stats.cpu().numpy().view(np.uint32).reshape(n, 5)
        for f in range(n):
            _, _, cg = a.rgb_bytes_to_ycocg_r(rgb[f])
            r = a.segment_by_chroma(None, None, cg, w, h, thr)
            assert np.array_equal(mask[f].cpu().numpy().reshape(-1), r.mask)
            assert list(st[f]) == r.bbox + [r.foreground_count]
        want_m, want_st = R.vec_chroma(R.vec_cg_of_rgb(rgb), thr)
        assert np.array_equal(mask.cpu().numpy(), want_m) and np.array_equal(st.astype(np.int64), want_st)


# ---- RLE and extract_person_rgb ----

def test_rle_parity(gpu_codec):
    a = gpu_codec
    rng = np.random.default_rng(3)
    cases = [np.zeros(1920 * 1080, np.uint8),                                   # 31 full runs of 65535 and the rest
             (np.arange(1920 * 1080) & 1).astype(np.uint8),                           # alternating: the 3n worst case
             rng.integers(0, 4, 100000, dtype=np.uint8),                          # bytes other than 0 / 1
             np.repeat(rng.integers(0, 2, 300, dtype=np.uint8), rng.integers(1, 200000, 300)),
             np.array([5], np.uint8)]
    for m in cases:
        got = a.rle_encode_mask(m)
        assert got == R.vec_rle(m)
        d = _dev(m)
        out = torch.zeros(a.rle_bound(m.size), dtype=torch.uint8, device="cuda:0")
        n = a.rle_encode_mask_device(d.data_ptr(), m.size, out.data_ptr(), out.numel())
        assert out[:n].cpu().numpy().tobytes() == got
    assert len(a.rle_encode_mask(cases[0])) == 32 * 3
    assert len(a.rle_encode_mask(cases[1])) == 3 * cases[1].size
    with pytest.raises(a.CodecError):
        a.rle_encode_mask_device(d.data_ptr(), 10, out.data_ptr(), 29)


def test_extract_person_rgb_parity(gpu_codec):
    a = gpu_codec
    rng = np.random.default_rng(4)
    w, h = 129, 70
    mask = rng.integers(0, 4, w * h, dtype=np.uint8)          # byte 3 is not foreground here
    rgb = rng.integers(0, 256, w * h * 3, dtype=np.uint8)
    for bbox in ([0, 0, w, h], [5, 7, 60, 30], [100, 60, 50, 20], [0, 0, 0, 0], [3, 3, 1, 1]):
        want = R.vec_extract(mask, w, bbox, rgb)
        assert a.extract_person_rgb(mask, w, bbox, rgb) == want
        assert a.extract_person_rgb(mask, w, bbox, rgb[:-4]) == R.vec_extract(mask, w, bbox, rgb[:-4])   # short rgb
        dm, dr = _dev(mask), _dev(rgb)
        out = torch.zeros(max(1, 3 * bbox[2] * bbox[3]), dtype=torch.uint8, device="cuda:0")
        n = a.extract_person_rgb_device(dm.data_ptr(), w, h, bbox, dr.data_ptr(), out.data_ptr(), 3 * bbox[2] * bbox[3])
        assert out[:n].cpu().numpy().tobytes() == want


# ---- the hybrid flow ----

def test_hybrid_flow(gpu_codec, oracle_mod):
    a, o = gpu_codec, oracle_mod
    rng = np.random.default_rng(21)
    n, h, w = 8, 96, 160
    bg = rng.integers(0, 256, (h, w), dtype=np.uint8)
    luma = np.repeat(bg[None], n, axis=0)
    rgb = np.repeat(luma[..., None], 3, axis=3).copy()
    for f in range(n):                                         # a "person" walking across the frame
        luma[f, 30:70, 20 + 8 * f:50 + 8 * f] ^= 0x80
        rgb[f, 30:70, 20 + 8 * f:50 + 8 * f] = [200, 120, 90]
    d_cur, d_ref = _dev(luma), _dev(bg)
    stats = torch.zeros(n * 5, dtype=torch.int32, device="cuda:0")
    a.segment_motion_device(d_cur.data_ptr(), d_ref.data_ptr(), 0, w, h, n, stats.data_ptr())
    st = stats.cpu().numpy().view(np.uint32).reshape(n, 5).astype(np.int64)
    assert np.array_equal(st, R.vec_motion(luma, bg[None], 25, 2, 1)[1])
    x0, y0 = st[:, 0].min(), st[:, 1].min()
    x1, y1 = (st[:, 0] + st[:, 2]).max(), (st[:, 1] + st[:, 3]).max()
    bw, bh = int(x1 - x0), int(y1 - y0)
    vol = rgb.reshape(n * h, w * 3)                            # frames stacked: crop rows of every frame
    crops = [a.crop_to_bbox(rgb[f].reshape(-1), w * 3, [int(x0) * 3, int(y0), bw * 3, bh]) for f in range(n)]
    crop = np.frombuffer(b"".join(crops), np.uint8)
    assert crop.size == n * bh * bw * 3 and vol.size == rgb.size
    chunk = a.FrameEncoder(90).encode(crop, bw, bh, n)
    assert chunk.to_bytes() == o.encode(crop, bw, bh, n, 90, int(a.WaveletType.Cdf53))
    dec = a.FrameDecoder().decode(chunk)
    assert np.array_equal(dec, o.decode(chunk.to_bytes()))
    out = np.zeros_like(rgb)
    per = bh * bw * 3
    for f in range(n):
        a.paste_from_bbox(out[f], w * 3, dec[f * per:(f + 1) * per], [int(x0) * 3, int(y0), bw * 3, bh])
    assert np.array_equal(out[:, y0:y1, x0:x1].reshape(-1), dec)
    assert not out[:, :y0].any() and not out[:, y1:].any()
