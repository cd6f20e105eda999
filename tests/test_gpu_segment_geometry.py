"""The internal geometry of csrc/segment.hip on the MI355X, bit-exact against tests/segment_ref.py: the column pass at
heights around its 64-row steps with block lengths below, at and above 64 and the height; the row pass at rows of exactly
64 words and of two chunks, at the radii where dilate_word switches, with set pixels whose nearest neighbour lies in the
other chunk; launches past the cap of 2^20 workgroups, where the grid-stride loops run a second time; the chroma
thresholds at the ends of i16; the compaction at its tile and scan-round sizes and at runs around 65535.

Content is a single set pixel (a single hole for an erosion) beside random frames, so a window one pixel off is not
hidden by neighbours.  Every device output lies inside a buffer with GUARD bytes of 0xA5 on both sides, which must come
back untouched, and is itself pre-filled with 0xA5.  The case tables live in tests/segment_cases.py; the last test holds
them to every class of segment_ref.segment_geometry."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segment_cases as K  # noqa: E402
import segment_ref as R  # noqa: E402

import torch  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD, FILL = 64, 0xA5


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


class Guarded:
    """nbytes of device memory with GUARD bytes of FILL before and after, all of it FILL to begin with"""

    def __init__(self, nbytes):
        self.n = int(nbytes)
        self.t = torch.full((self.n + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
        self.ptr = self.t.data_ptr() + GUARD
        assert self.ptr % 4 == 0

    def take(self, dtype=np.uint8):
        host = self.t.cpu().numpy()
        assert (host[:GUARD] == FILL).all(), "bytes before the output changed"
        assert (host[GUARD + self.n:] == FILL).all(), "bytes after the output changed"
        return host[GUARD:GUARD + self.n].view(dtype)


def _frames_of(m, shared, rng):
    """current and reference frames whose difference exceeds 100 exactly where m is set"""
    n = len(m)
    ref = rng.integers(0, 256, (1 if shared else n,) + m.shape[1:], dtype=np.uint8)
    return np.where(m, ref ^ 0x80, ref).astype(np.uint8), ref


def _motion(codec, cur, ref, shared, rd, re, with_mask=True, thr=100):
    """-> (mask [n, h, w] or None, stats int64 [n, 5]) out of guarded buffers"""
    n, h, w = cur.shape
    dc, dr = _dev(cur), _dev(ref)
    stats = Guarded(n * 5 * 4)
    mask = Guarded(n * h * w) if with_mask else None
    codec.segment_motion_device(dc.data_ptr(), dr.data_ptr(), 0 if shared else w * h, w, h, n, stats.ptr,
                                mask.ptr if with_mask else None, codec.SegmentConfig(thr, 100, rd, re))
    return (mask.take().reshape(n, h, w) if with_mask else None), stats.take(np.uint32).reshape(n, 5).astype(np.int64)


def _check_motion(codec, m, shared, rd, re, rng, stats_only=False):
    cur, ref = _frames_of(m, shared, rng)
    want = R.vec_cleanup(m, rd, re)
    want_st = R.vec_stats(want)
    mask, st = _motion(codec, cur, ref, shared, rd, re)
    assert np.array_equal(mask, want.astype(np.uint8)), "mask"
    assert np.array_equal(st, want_st), ("stats", st.tolist(), want_st.tolist())
    if stats_only:
        _, st2 = _motion(codec, cur, ref, shared, rd, re, with_mask=False)
        assert np.array_equal(st2, st), "stats of the call without a mask"


# ---- (a) column geometry ----

@pytest.mark.parametrize("h", K.COLUMN_HEIGHTS)
def test_column_geometry(gpu_codec, h):
    rng = np.random.default_rng(1000 + h)
    cases = K.column_cases(h)
    assert {c["mode"] for c in cases} == {"dilate", "erode", "both"} and {c["shared"] for c in cases} == {True, False}
    assert sum(c["stats_only"] for c in cases) * 3 >= len(cases)
    for c in cases:
        try:
            _check_motion(gpu_codec, K.column_pattern(c, rng), c["shared"], c["rd"], c["re"], rng, c["stats_only"])
        except AssertionError as e:
            raise AssertionError(f"{c}: {e}") from None


# ---- (b) row geometry ----

@pytest.mark.parametrize("w", K.ROW_WIDTHS)
def test_row_geometry(gpu_codec, w):
    rng = np.random.default_rng(2000 + w)
    for i, c in enumerate(K.row_cases(w)):
        r = max(c["rd"], c["re"])
        m = K.row_pattern(w, c["h"], r)
        assert len(m) == c["n"] and not m[-1].any() and (m[:-1].reshape(len(m) - 1, -1).sum(axis=1) >= 1).all()
        if c["mode"] == "erode":
            m = ~m
        try:
            _check_motion(gpu_codec, m, i % 2 == 0, c["rd"], c["re"], rng)
        except AssertionError as e:
            raise AssertionError(f"{c}: {e}") from None


# ---- (c) grid-stride loops ----

def _grid_mask(rng, n, h, w):
    """about 10 % of the pixels set; every 16th frame, and a stretch at the end, empty"""
    m = rng.random((n, h, w)) < 0.1
    m[::16] = False
    m[-1000:] = False
    m[-1, h - 1, w - 1] = True      # (the last workgroup of the last turn of the loop has something to report)
    return m


@pytest.mark.parametrize("w,h,n", K.GRID_SHAPES)
def test_motion_grids_past_the_cap(gpu_codec, w, h, n):
    rng = np.random.default_rng(n)
    m = _grid_mask(rng, n, h, w)
    for c in K.grid_cases():
        if (c["w"], c["h"], c["n"]) != (w, h, n):
            continue
        g = R.segment_geometry(w, h, n, c["rd"], c["re"])
        assert g["row_grid_loops @135"] and (g["column_grid_loops @281"] or not c["rd"] or h > 1)
        _check_motion(gpu_codec, m, True, c["rd"], c["re"], rng)


def test_chroma_rgb_grid_past_the_cap(gpu_codec):
    w, h, n = K.GRID_SHAPES[1]
    rng = np.random.default_rng(31)
    rgb = rng.integers(0, 100, (n, h, w, 3), dtype=np.uint8)
    rgb[..., 1] += 140                                     # green everywhere: Cg > 10 ...
    rgb[rng.random((n, h, w)) < 0.02] = [255, 0, 255]      # ... but for 2 % of the pixels: half of the frames have none
    want_m, want_st = _chroma_want(rgb, 10)
    assert 0.02 < want_m.mean() < 0.98 and (want_st[:, 4] == 0).any()
    mask, st = _chroma_rgb(gpu_codec, rgb, 10)
    assert np.array_equal(mask, want_m) and np.array_equal(st, want_st)


# ---- (d) chroma thresholds ----

THRESHOLDS = [-32768, -256, -255, -1, 0, 254, 255, 32767]


def _chroma_want(cg_or_rgb, thr):
    cg = R.vec_cg_of_rgb(cg_or_rgb) if cg_or_rgb.dtype == np.uint8 else cg_or_rgb
    m = R.vec_erode(R.vec_dilate(cg <= int(thr), 2), 1)
    return m.astype(np.uint8), R.vec_stats(m)


def _chroma_rgb(codec, rgb, thr):
    n, h, w, _ = rgb.shape
    d = _dev(rgb)
    stats, mask = Guarded(n * 5 * 4), Guarded(n * h * w)
    codec.segment_chroma_rgb_device(d.data_ptr(), w, h, n, thr, stats.ptr, mask.ptr)
    return mask.take().reshape(n, h, w), stats.take(np.uint32).reshape(n, 5).astype(np.int64)


def _chroma_planar(codec, cg, thr):
    """alice_codec_segment_by_chroma of one plane, its host mask inside guard bytes too"""
    h, w = cg.shape
    buf = np.full(w * h + 2 * GUARD, FILL, np.uint8)
    bbox, cnt = (C.c_uint32 * 4)(), C.c_uint32()
    cgc = np.ascontiguousarray(cg, np.int16)
    rc = codec.load_library().alice_codec_segment_by_chroma(cgc.ctypes.data_as(C.POINTER(C.c_int16)), cgc.size, w, h, thr,
                                                            buf[GUARD:].ctypes.data_as(C.POINTER(C.c_uint8)), w * h, bbox,
                                                            C.byref(cnt))
    assert rc == 0
    assert (buf[:GUARD] == FILL).all() and (buf[GUARD + w * h:] == FILL).all()
    return buf[GUARD:GUARD + w * h].reshape(h, w), list(bbox) + [cnt.value]


def test_chroma_thresholds(gpu_codec):
    rng = np.random.default_rng(41)
    n, h, w = 3, 33, 65
    rgb = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    rgb[:, ::5, ::7] = [255, 0, 255]              # Cg = -255
    rgb[:, 2::5, 3::7] = [0, 255, 0]              # Cg = +255
    rgb[0, 10:18, 20:28] = [0, 255, 0]           # a block of it, which the cleanup does not close: 254 and 255 differ
    rgb[2, :, :, 1] = 255                        # a frame without negative Cg
    cg = R.vec_cg_of_rgb(rgb)
    assert cg.min() == -255 and cg.max() == 255
    wide = rng.integers(-32768, 32768, (n, h, w)).astype(np.int16)    # planar input is any i16
    wide[0, 0, 0], wide[0, 32, 64], wide[1, 5, 5] = -32768, 32767, -32768
    for thr in THRESHOLDS:
        want_m, want_st = _chroma_want(rgb, thr)
        mask, st = _chroma_rgb(gpu_codec, rgb, thr)
        assert np.array_equal(mask, want_m) and np.array_equal(st, want_st), thr
        for plane, (pm, pst) in ((cg, (want_m, want_st)), (wide, _chroma_want(wide, thr))):
            for f in range(n):
                got_m, got_st = _chroma_planar(gpu_codec, plane[f], thr)
                assert np.array_equal(got_m, pm[f]) and got_st == list(pst[f]), (thr, f)
    assert _chroma_want(rgb, -256)[1][:, 4].sum() == 0 and _chroma_want(rgb, 255)[0].all()
    assert 0 < _chroma_want(rgb, -255)[1][:, 4].sum() < _chroma_want(rgb, 254)[1][:, 4].sum() < n * h * w
    assert _chroma_want(rgb, -255)[1][2, 4] == 0


# ---- (e) compaction: RLE ----

TILE = 4096                      # kCompactTile
RLE_SIZES = [TILE - 1, TILE, TILE + 1, 2 * TILE, 256 * TILE - 1, 256 * TILE, 256 * TILE + 1]


def _mask_of_runs(lens, first=0):
    vals = (np.arange(len(lens)) + first) & 1
    return np.repeat(vals.astype(np.uint8), lens)


def _rle_masks(n, rng):
    out = {"alternating": (np.arange(n) & 1).astype(np.uint8), "one run": np.ones(n, np.uint8)}
    lens = rng.geometric(1 / 300.0, n // 100 + 50)
    out["random runs"] = _mask_of_runs(lens)[:n]
    chg = np.zeros(n, np.uint8)   # a change on the last item of a tile, on the first item of one, and on both
    for t in range(1, (n + TILE - 1) // TILE + 1, 3):
        for at in (t * TILE - 1, (t + 1) * TILE, (t + 2) * TILE - 1, (t + 2) * TILE):
            if at < n:
                chg[at] = 1
    chg[n - 1] ^= 1
    out["changes at tile edges"] = (np.cumsum(chg, dtype=np.int64) & 1).astype(np.uint8)
    return {k: v for k, v in out.items() if v.size == n}


def _check_rle(codec, m, rng):
    want = R.vec_rle(m)
    dirty = m | (rng.integers(0, 128, m.size, dtype=np.uint8) << 1)       # only bit 0 counts
    for mm in (m, dirty):
        assert codec.rle_encode_mask(mm) == want
        d = _dev(mm)
        cap = codec.rle_bound(mm.size)
        assert cap == 3 * mm.size
        out = Guarded(cap)
        got = codec.rle_encode_mask_device(d.data_ptr(), mm.size, out.ptr, cap)
        host = out.take()
        assert got == len(want) and host[:got].tobytes() == want
        assert (host[got:] == FILL).all(), "bytes past the code changed"


@pytest.mark.parametrize("n", RLE_SIZES)
def test_rle_tile_sizes(gpu_codec, n):
    rng = np.random.default_rng(n)
    masks = _rle_masks(n, rng)
    assert len(masks) == 4
    for name, m in masks.items():
        try:
            _check_rle(gpu_codec, m, rng)
        except AssertionError as e:
            raise AssertionError(f"n={n} {name}: {e}") from None
    assert len(R.vec_rle(masks["alternating"])) == 3 * n                   # the code fills the capacity exactly


def test_rle_run_lengths_around_65535(gpu_codec):
    rng = np.random.default_rng(6)
    runs = [65535, 65536, 131070, 131071, 196605]
    assert [len(R.vec_rle(np.ones(r, np.uint8))) // 3 for r in runs] == [1, 2, 2, 3, 3]
    for r in runs:
        _check_rle(gpu_codec, np.ones(r, np.uint8), rng)
    for lead in (0, 1, TILE - 1, TILE):               # the runs in a row; each lead moves their starts against the tiles
        m = _mask_of_runs([lead] * (lead > 0) + runs + [7] + runs[::-1] + [1])
        _check_rle(gpu_codec, m, rng)
    # a run of 65535 and one of 131071 that start on the last item of a tile
    m = _mask_of_runs([TILE - 1, 65535, 17 * TILE - 65535, 131071, 3])
    assert m[TILE - 2] != m[TILE - 1] and m[18 * TILE - 2] != m[18 * TILE - 1]
    _check_rle(gpu_codec, m, rng)


# ---- (e) compaction: extract_person_rgb ----

EXTRACT_W, EXTRACT_H = 200, 120
EXTRACT_BBOXES = [
    [3, 2, 63, 65], [137, 57, 63, 65], [0, 0, 65, 63], [0, 0, 91, 45],       # 4095 items
    [9, 11, 64, 64], [0, 0, 128, 32], [72, 88, 128, 32],                      # 4096
    [0, 0, 241, 17], [7, 3, 241, 17],          # 4097 = 17 * 241: wider than the frame, the walk wraps into the next rows
    [0, 0, 17, 241], [150, 5, 17, 241],        # ... and taller than it: the rows past the last fail the mask_len guard
    [0, 0, 12289, 1], [100, 50, 12289, 1],     # 12289 is prime: one row that wraps through 61 frame rows
    [100, 80, 12289, 1], [5, 0, 1, 12289],     # ... that runs past the mask's end; one column that does
]


def test_extract_person_rgb_tiles(gpu_codec):
    a = gpu_codec
    rng = np.random.default_rng(8)
    w, h = EXTRACT_W, EXTRACT_H
    assert sorted({b[2] * b[3] for b in EXTRACT_BBOXES}) == [4095, 4096, 4097, 12289]
    rgb = rng.integers(0, 256, w * h * 3, dtype=np.uint8)
    masks = {"none": np.zeros(w * h, np.uint8), "all": np.ones(w * h, np.uint8),
             "half": rng.integers(0, 2, w * h, dtype=np.uint8), "bytes 0..3": rng.integers(0, 4, w * h, dtype=np.uint8)}
    d_rgb = _dev(rgb)
    for name, mask in masks.items():
        d_mask = _dev(mask)
        for bbox in EXTRACT_BBOXES:
            want = R.vec_extract(mask, w, bbox, rgb)
            items = bbox[2] * bbox[3]
            if bbox[3] == 1:      # a walk of 12289 items is linear: kept pixels in its first tile and after it
                kept = mask[bbox[1] * w + bbox[0]:][:items] == 1
                assert name == "none" or (kept[:TILE].any() and kept[TILE:].any())
            if name == "all":     # the walk keeps everything below the mask's end, also where it wraps
                assert len(want) == 3 * min(items, bbox[2] * max(0, h - bbox[1]) if bbox[3] > 1 else w * h - bbox[1] * w - bbox[0])
            assert a.extract_person_rgb(mask, w, bbox, rgb) == want, (name, bbox)
            out = Guarded(3 * items)
            n = a.extract_person_rgb_device(d_mask.data_ptr(), w, h, bbox, d_rgb.data_ptr(), out.ptr, 3 * items)
            host = out.take()
            assert n == len(want) and host[:n].tobytes() == want, (name, bbox)
            assert (host[n:] == FILL).all(), (name, bbox)


# ---- (f) coverage closure ----

def test_sweeps_reach_every_geometry_class():
    calls = K.all_segment_calls()
    missing = R.ALL_CLASSES - K.reached_classes(calls)
    assert not missing, sorted(missing)
    assert len(set(calls)) > 1900
