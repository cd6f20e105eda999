"""Person segmentation (src/segment.rs) without a GPU: the reference's inline tests (:443-781) on the two restatements of
tests/segment_ref.py, their agreement on random cases, the host-side crop/paste mirrors, and the C ABI's validation
(errors come back before any device work; valid arguments report DeviceError on a host without one)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segment_ref as R  # noqa: E402

BIG = 2 ** 32 - 1


# ---- the reference's inline tests, exact values where it has them ----

def test_separable_dilate_basic():            # :597-614
    m = [0] * 25
    m[12] = 1
    out = R.lit_dilate(m, 5, 5, 1)
    for i in (6, 7, 8, 11, 12, 13, 16, 17, 18):
        assert out[i] == 1
    assert sum(out) == 9
    assert np.array_equal(R.vec_dilate(np.array(m, bool).reshape(5, 5), 1).reshape(-1).astype(int), out)


def test_separable_erode_basic():             # :617-637
    m = [1] * 49
    for x in range(7):
        m[x] = m[42 + x] = 0
    for y in range(7):
        m[y * 7] = m[y * 7 + 6] = 0
    out = R.lit_erode(m, 7, 7, 1)
    assert sum(out) < sum(m) and out[24] == 1
    assert out == list(R.vec_erode(np.array(m, bool).reshape(7, 7), 1).reshape(-1).astype(int))


def test_bbox_fast_and_single_pixel():        # :640-651, :774-780
    m = np.zeros((10, 10), np.uint8)
    m[2:7, 3:8] = 1
    assert R.lit_bbox(list(m.reshape(-1)), 10, 10) == ([3, 2, 5, 5], 25)
    assert R.vec_bbox(m.astype(bool)) == ([3, 2, 5, 5], 25)
    m = [0] * 100
    m[55] = 1
    assert R.lit_bbox(m, 10, 10) == ([5, 5, 1, 1], 1)


def test_motion_segmentation_kats():         # :448-471, :474-497, :545-558, :666-682
    cur = [0] * 200
    for y in range(3, 7):
        for x in range(5, 15):
            cur[y * 20 + x] = 200
    _, bbox, count = R.lit_motion(cur, [0] * 200, 20, 10, 50, 0, 0)
    assert count == 40 and bbox == [5, 3, 10, 4]
    cur = [0] * 600
    for y in range(5, 15):
        for x in range(8, 22):
            cur[y * 30 + x] = 180
    _, _, count = R.lit_motion(cur, [0] * 600, 30, 20, 30, 2, 1)
    assert 0.1 < count / 600 < 0.8
    assert R.lit_motion([100] * 100, [100] * 100, 10, 10, 25, 0, 0)[1:] == ([0, 0, 0, 0], 0)
    assert R.lit_motion([255] * 64, [0] * 64, 8, 8, 50, 0, 0)[1:] == ([0, 0, 8, 8], 64)


def test_chroma_segmentation_kat():           # :749-771
    cg = [100] * 50
    for row in range(1, 4):
        for col in range(2, 8):
            cg[row * 10 + col] = -10
    mask, _, count = R.lit_chroma(cg, 10, 5, 50)
    assert count > 0
    m2, st = R.vec_chroma(np.array(cg, np.int16).reshape(1, 5, 10), 50)
    assert list(m2.reshape(-1)) == mask and st[0, 4] == count


def test_rle_kats():                          # :500-518, :685-729
    m = [0] * 40
    m[10:30] = [1] * 20
    assert len(R.lit_rle(m)) == 9
    assert R.lit_rle([]) == b"" and R.vec_rle([]) == b""
    assert R.lit_rle([0] * 100) == bytes([100, 0, 0])
    assert R.lit_rle([1] * 50) == bytes([50, 0, 1])
    assert R.vec_rle(m) == R.lit_rle(m)


def test_extract_person_kat():                # :561-594
    rgb = bytearray(150)
    mask = [0] * 50
    for y in range(2, 4):
        for x in range(3, 6):
            i = (y * 10 + x) * 3
            rgb[i:i + 3] = bytes([255, 128, 64])
            mask[y * 10 + x] = 1
    out = R.lit_extract(mask, 10, [3, 2, 3, 2], rgb)
    assert len(out) == 18 and out[:3] == bytes([255, 128, 64])
    assert R.vec_extract(mask, 10, [3, 2, 3, 2], rgb) == out


def test_crop_and_paste_kats(codec):          # :521-542, :741-746
    frame = np.zeros(100, np.uint8)
    for y in range(2, 5):
        frame[y * 10 + 3:y * 10 + 7] = 100
    bbox = [3, 2, 4, 3]
    crop = codec.crop_to_bbox(frame, 10, bbox)
    assert len(crop) == 12 and set(crop) == {100} and crop == R.lit_crop(frame.tobytes(), 10, bbox)
    restored = codec.paste_from_bbox(np.zeros(100, np.uint8), 10, crop, bbox)
    for y in range(2, 5):
        assert list(restored[y * 10 + 3:y * 10 + 7]) == [100] * 4
    assert codec.crop_to_bbox(np.full(100, 42, np.uint8), 10, [0, 0, 0, 0]) == b""


def test_config_defaults_and_coverage(codec):  # :731-738, :653-663, :666-682
    c = codec.SegmentConfig()
    assert (c.motion_threshold, c.min_region_size, c.dilate_radius, c.erode_radius) == (25, 100, 2, 1)
    assert codec.SegmentResult(b"", [0, 0, 0, 0], 0, 0, 0).coverage() == 0.0
    assert codec.SegmentResult(bytes([1] * 64), [0, 0, 8, 8], 64, 8, 8).coverage() == 1.0
    r = codec.SegmentResult(bytes(600), [0, 0, 0, 0], 7, 30, 20)
    assert r.coverage() == float(np.float32(7) * (np.float32(1.0) / np.float32(600)))
    assert codec.SegmentResult(b"", [0, 0, 0, 0], 0, 0, 0).rle_encode_mask() == b""


# ---- (a) and (b) agree ----

def _random_case(rng):
    w = int(rng.choice([1, 2, 3, 5, 8, 13, 17]))
    h = int(rng.choice([1, 2, 3, 5, 8, 11]))
    if rng.random() < 0.15:
        w, h = (1, int(rng.integers(1, 40))) if rng.random() < 0.5 else (int(rng.integers(1, 40)), 1)
    density = rng.choice([0.02, 0.2, 0.5, 0.9])
    ref = rng.integers(0, 256, w * h)
    cur = np.where(rng.random(w * h) < density, rng.integers(0, 256, w * h), ref)
    radii = [0, 1, 2, w, h, w + 3, BIG]
    return w, h, cur, ref, int(rng.choice(radii)), int(rng.choice(radii)), int(rng.choice([0, 1, 25, 100, 255]))


def test_literal_and_vectorised_agree():
    rng = np.random.default_rng(1234)
    for _ in range(300):
        w, h, cur, ref, rd, re, thr = _random_case(rng)
        mask, bbox, count = R.lit_motion(list(cur), list(ref), w, h, thr, rd, re)
        vm, st = R.vec_motion(cur.reshape(1, h, w), ref.reshape(1, h, w), thr, rd, re)
        assert list(vm.reshape(-1)) == mask, (w, h, rd, re, thr)
        assert list(st[0]) == bbox + [count]
        assert R.vec_rle(mask) == R.lit_rle(mask)
    for t in (0, 255):   # threshold 255 gives an empty mask; 0 marks any difference
        cur = np.array([0, 255, 3, 3])
        ref = np.array([255, 0, 3, 4])
        assert R.lit_motion(list(cur), list(ref), 2, 2, t, 0, 0)[0] == ([0, 0, 0, 0] if t == 255 else [1, 1, 0, 1])


def test_big_radius_fills_and_empties():
    m = [0] * 30
    m[7] = 1
    assert R.lit_dilate(m, 6, 5, BIG) == [1] * 30
    m = [1] * 30
    m[29] = 0
    assert R.lit_erode(m, 6, 5, BIG) == [0] * 30


def test_erosion_does_not_eat_in_from_the_border():
    assert R.lit_erode([1] * 35, 7, 5, 1) == [1] * 35
    assert R.lit_erode([1] * 35, 7, 5, BIG) == [1] * 35
    assert np.all(R.vec_erode(np.ones((1, 5, 7), bool), 3))


def test_rle_long_runs_and_odd_bytes():
    m = [0] * (65535 * 2 + 10) + [3, 1, 2]
    lit = R.lit_rle(m)
    assert lit == bytes([255, 255, 0, 255, 255, 0, 10, 0, 0, 2, 0, 1, 1, 0, 0])
    assert R.vec_rle(m) == lit


def test_extract_rgb_mask_byte_three_and_short_rgb():
    mask = [1, 3, 1, 1]
    rgb = bytes(range(11))   # the last pixel's rgb_idx + 2 = 11 is out of range
    assert R.lit_extract(mask, 2, [0, 0, 2, 2], rgb) == bytes([0, 1, 2, 6, 7, 8])
    assert R.vec_extract(mask, 2, [0, 0, 2, 2], rgb) == R.lit_extract(mask, 2, [0, 0, 2, 2], rgb)


def test_crop_paste_skip_partial_rows(codec):
    frame = np.arange(30, dtype=np.uint8)   # 6 x 5
    bbox = [3, 3, 3, 3]                      # rows 3, 4, 5: row 4 ends at 30 and fits, row 5 ends at 36 and is skipped
    assert codec.crop_to_bbox(frame, 6, bbox) == R.lit_crop(frame.tobytes(), 6, bbox) == bytes([21, 22, 23, 27, 28, 29])
    got = codec.paste_from_bbox(np.zeros(30, np.uint8), 6, bytes([9] * 9), bbox)
    assert got.tobytes() == bytes(R.lit_paste(bytes(30), 6, bytes([9] * 9), bbox))
    with pytest.raises(codec.CodecError) as e:
        codec.crop_to_bbox(frame, 2 ** 31, [0, 2, 1, 1])
    assert e.value.kind == "DimensionOverflow"


def test_numpy_aliases_shapes(codec):
    f = np.arange(20, dtype=np.uint8).reshape(4, 5)
    c = codec.crop_bbox_numpy(f, [1, 1, 2, 2])
    assert c.shape == (2, 2) and c.tolist() == [[6, 7], [11, 12]]
    g = np.zeros((4, 5), np.uint8)
    assert codec.paste_bbox_numpy(g, c.reshape(-1), [1, 1, 2, 2]) is None
    assert g[1:3, 1:3].tolist() == [[6, 7], [11, 12]]


# ---- the C ABI's validation, before any device work ----

def _err(codec, fn):
    with pytest.raises(codec.CodecError) as e:
        fn()
    return e.value.kind


def test_validation_errors(codec):
    assert _err(codec, lambda: codec.segment_by_motion(bytes(99), bytes(99), 10, 10)) == "InvalidBufferSize"
    assert _err(codec, lambda: codec.segment_by_motion(bytes(100), bytes(99), 10, 10)) == "InvalidBufferSize"
    assert _err(codec, lambda: codec.segment_by_motion(bytes(1), bytes(1), 65536, 65536)) == "DimensionOverflow"
    assert _err(codec, lambda: codec.segment_by_chroma(None, None, np.zeros(49, np.int16), 10, 5, 30)) == "InvalidBufferSize"
    assert _err(codec, lambda: codec.segment_by_chroma(None, None, np.zeros(1, np.int16), 2 ** 20, 2 ** 20, 30)) == "DimensionOverflow"
    assert _err(codec, lambda: codec.extract_person_rgb(bytes(4), 2 ** 31, [0, 2, 1, 1], bytes(12))) == "DimensionOverflow"


def test_short_current_reported_before_short_reference(codec):
    lib = codec.load_library()
    import ctypes as C
    bbox = (C.c_uint32 * 4)()
    cnt = C.c_uint32()
    cur = (C.c_uint8 * 5)()
    ref = (C.c_uint8 * 3)()
    mask = (C.c_uint8 * 10)()
    rc = lib.alice_codec_segment_by_motion(cur, 5, ref, 3, 5, 2, 25, 2, 1, mask, 10, bbox, C.byref(cnt))
    assert rc == 1 and b"got 5" in lib.alice_codec_last_error_message()


def test_valid_arguments_need_a_device(codec):
    # empty inputs need no device
    assert codec.segment_by_motion(b"", b"", 0, 7).bbox == [0, 0, 0, 0]
    assert codec.rle_encode_mask(b"") == b""
    assert codec.extract_person_rgb(b"", 4, [0, 0, 2, 2], b"") == b""
    if codec.device_count() > 0:   # (the GPU suite covers these calls on a device)
        return
    assert _err(codec, lambda: codec.segment_by_motion(bytes(100), bytes(100), 10, 10)) == "DeviceError"
    assert _err(codec, lambda: codec.segment_by_chroma(None, None, np.zeros(50, np.int16), 10, 5, 30)) == "DeviceError"
    assert _err(codec, lambda: codec.rle_encode_mask(bytes(10))) == "DeviceError"
    assert _err(codec, lambda: codec.extract_person_rgb(bytes([1] * 4), 2, [0, 0, 2, 2], bytes(12))) == "DeviceError"
