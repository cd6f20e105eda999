"""Person segmentation (src/segment.rs) without a GPU: the reference's inline tests (:443-781) on the two restatements of
tests/segment_ref.py, their agreement on random cases, the host-side crop/paste mirrors, and the C ABI's validation
(errors come back before any device work; valid arguments report DeviceError on a host without one)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segment_ref as R  # noqa: E402
import segment_cases as K  # noqa: E402

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


# ---- the references and case tables of tests/test_gpu_segment_geometry.py ----

def test_vec_stats_is_vec_bbox_frame_by_frame():
    rng = np.random.default_rng(77)
    for _ in range(40):
        h, w = int(rng.integers(1, 12)), int(rng.integers(1, 70))
        m = rng.random((8, h, w)) < rng.choice([0.0, 0.01, 0.1, 0.6, 1.0], size=(8, 1, 1))
        st = R.vec_stats(m)
        assert st.shape == (8, 5) and st.dtype == np.int64
        for f in range(8):
            bbox, count = R.vec_bbox(m[f])
            assert list(st[f]) == bbox + [count], (h, w, f)
    assert R.vec_stats(np.zeros((3, 2, 2), bool)).tolist() == [[0] * 5] * 3


def _box(h, w, y, x, r):
    out = np.zeros((h, w), bool)
    out[max(0, y - r):min(h, y + r + 1), max(0, x - r):min(w, x + r + 1)] = True
    return out


def _lit_of_pattern(m, rd, re):
    """lit_motion of a 0/255 frame against zeros: bool [h, w] -> (bool [h, w], stats)"""
    h, w = m.shape
    mask, bbox, count = R.lit_motion(list(m.reshape(-1).astype(int) * 255), [0] * (w * h), w, h, 100, rd, re)
    return np.array(mask, bool).reshape(h, w), bbox + [count]


def test_single_pixel_and_single_hole_give_the_clipped_box():
    """what the GPU sweep relies on: one set pixel dilates to exactly the (2r+1)^2 box clipped to the frame, one hole
    erodes to its complement, in both restatements"""
    for h, w in ((3, 70), (5, 130), (66, 2)):
        for r in (1, 2, 62, 63, 64, w + 1, BIG):
            for y, x in ((0, 0), (h - 1, w - 1), (h // 2, 63 % w), (min(h - 1, 64), 64 % w), (1, w // 2)):
                m = np.zeros((h, w), bool)
                m[y, x] = True
                want = _box(h, w, y, x, min(r, h + w))
                assert np.array_equal(R.vec_dilate(m, r), want), (h, w, r, y, x)
                assert np.array_equal(R.vec_erode(~m, r), ~want), (h, w, r, y, x)
                if r in (1, 63, BIG):
                    got, st = _lit_of_pattern(m, r, 0)
                    assert np.array_equal(got, want) and st == R.vec_bbox(want)[0] + [int(want.sum())]
                    assert np.array_equal(_lit_of_pattern(~m, 0, r)[0], ~want)


def test_pattern_families_literal_vs_vectorised():
    """reduced versions of the GPU sweep's patterns (widths that still cross a 64-pixel word; one row that crosses a
    4096-pixel chunk) through both restatements, every radius class of dilate_word"""
    rng = np.random.default_rng(5)
    cases = []
    for w, h in ((65, 2), (130, 3), (129, 5)):
        for r in (0, 1, 62, 63, 64, w, w + 5):
            singles = [[p] for p in (0, 63, 64, w - 1)]
            pairs = [[63 - d // 2, 63 - d // 2 + d] for d in (r - 1, r, r + 1) if d >= 1 and 63 - d // 2 >= 0 and 63 - d // 2 + d < w]
            for f, xs in enumerate(singles + pairs + [[]]):
                m = np.zeros((h, w), bool)
                m[f % h, xs] = True
                cases.append((m, r))
    for r in (1, 62, 64):                       # a chunk edge: 64 words of 64 pixels
        for p, q in K.row_pairs(4100, r):
            m = np.zeros((1, 4100), bool)
            m[0, [p, q]] = True
            cases.append((m, r))
    for h in (3, 5, 65):                        # the column pass's patterns at a width of one word
        for c in K.column_cases(h)[::17]:
            if c["w"] == 1 and max(c["rd"], c["re"]) < BIG:
                cases.append((K.column_pattern(c, rng)[0], c["rd"], c["re"]))
    assert len(cases) > 150
    for case in cases:
        m = case[0]
        for rd, re, pat in ([(case[1], 0, m), (0, case[1], ~m)] if len(case) == 2 else [(case[1], case[2], m)]):
            got, st = _lit_of_pattern(pat, rd, re)
            vm, vst = R.vec_motion_batch(pat[None].astype(np.uint8) * 255, np.zeros((1,) + m.shape, np.uint8), 100, rd, re)
            assert np.array_equal(vm[0].astype(bool), got), (m.shape, rd, re)
            assert list(vst[0]) == st
            om, ost = R.vec_motion(pat[None].astype(np.uint8) * 255, np.zeros((1,) + m.shape, np.uint8), 100, rd, re)
            assert np.array_equal(om, vm) and np.array_equal(ost, vst)


def test_segment_geometry_known_answers():
    g = R.segment_geometry(4096, 5, 3, 1, 0)
    assert g["words_per_row @133"] == 64 and g["chunks_per_row @133"] == 1 and g["row_of_64_words @215"]
    assert g["block @505"] == {1: (3, {"<64"})} and g["pick @146"] == {0, 1} and g["last_step_partial @286"]
    assert R.segment_geometry(4096, 6, 3, 1, 0)["pick @146"] == {0, 1, 2}     # row 5: window rows 4..5 inside block 3..5
    g = R.segment_geometry(4097, 64, 1, BIG, 31)
    assert g["chunks_per_row @133"] == 2 and g["row_path @213-220"] == {"many_chunks", "plain"}
    assert g["block @505"] == {BIG: (64, {"==64", "clamped"}), 31: (63, {"<64", "==h-1"})}
    assert g["block_starts_on_lane63 @294"] and not g["block_starts_on_lane0 @292"] and g["last_step_partial @286"] is False
    assert g["smear @90"] == {"<63", ">=63"}
    g = R.segment_geometry(1, 1, 4_300_000, 0, 0)
    assert g["row_grid_loops @135"] and not g["column_grid_loops @281"] and g["block @505"] == {}
    assert R.segment_geometry(1, 1, 4_300_000, 1, 1)["column_grid_loops @281"]
    assert not R.segment_geometry(1, 1, 4 << 20, 1, 1)["column_grid_loops @281"]
    assert R.segment_geometry(257, 257, 1, 1, 0)["block_starts_on_lane0 @292"]
    assert R.segment_geometry(1, 129, 1, 32, 0)["block_ends_on_lane0 @308"]
    for g in (R.segment_geometry(5, 6, 530_000, 1, 1), R.segment_geometry(70, 200, 2, 40, 0)):
        assert R.geometry_classes(g) <= R.ALL_CLASSES


def test_case_table_reaches_every_geometry_class():
    """the closure that tests/test_gpu_segment_geometry.py asserts after its sweep: an edit of the tables fails here first"""
    missing = R.ALL_CLASSES - K.reached_classes(K.all_segment_calls())
    assert not missing, sorted(missing)


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
