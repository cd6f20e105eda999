"""Many frame ranges and rectangles in one call without a device: every refusal of
alice_codec_decode_rects and alice_codec_dev_decode_rects that is host code, with its code and the index of the item that
decided it, that a refusal leaves `offsets` and the statistics hook alone, the layout of alice_codec_rect_item against the
ctypes mirror, the output-disjointness rule through alice_codec_test_rects_outputs_disjoint, and that the new symbols are
declared in every mirror."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle.alice_oracle_np as o  # noqa: E402
import frames_ref as FR  # noqa: E402
import wide_oracle as WO  # noqa: E402
from test_frames_host import _encode_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_ITEM = 0xFFFFFFFF
SENTINEL = 0x5A5A5A5A5A5A5A5A
W, H, F = 33, 17, 5
_made = {}


def _blobs():
    if not _made:
        rgb = WO.smooth_plus_noise(W, H, F)
        _made["good"] = [np.frombuffer(_encode_ref(v, rgb, W, H, F, 80, FR.CDF53, 64), np.uint8) for v in (2, 3, 4)]
        _made["v1"] = np.frombuffer(bytes(o.encode(rgb, W, H, F, 80, FR.CDF53)), np.uint8)
    return _made["good"], _made["v1"]


def _items(codec, rows):
    """rows of (array or None, len or None, first, count, (x, y, w, h)[, rgb_out, row_pitch, frame_pitch])"""
    arr = (codec.RectItem * max(len(rows), 1))()
    for i, row in enumerate(rows):
        buf, length, first, count, rect = row[:5]
        out, rp, fp = row[5:] if len(row) > 5 else (None, 0, 0)
        arr[i] = codec.RectItem(None if buf is None else buf.ctypes.data, (0 if buf is None else buf.size) if length is None else length,
                                first, count, *rect, out, rp, fp)
    return arr


def _host(codec, rows, n=None, null_offsets=False):
    """-> (pointer, code, bad_item, offsets, message) of alice_codec_decode_rects"""
    lib = codec.load_library()
    offsets = np.full(len(rows) + 1, SENTINEL, np.uint64)
    bad = C.c_uint32(7)
    ptr = lib.alice_codec_decode_rects(_items(codec, rows), len(rows) if n is None else n,
                                       None if null_offsets else offsets.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(bad))
    msg = lib.alice_codec_last_error_message()
    return ptr, lib.alice_codec_last_error(), bad.value, offsets, (msg or b"").decode()


def _dev(codec, rows):
    """-> (code, bad_item, message) of alice_codec_dev_decode_rects"""
    lib = codec.load_library()
    bad = C.c_uint32(7)
    code = lib.alice_codec_dev_decode_rects(_items(codec, rows), len(rows), C.byref(bad), None)
    return code, bad.value, (lib.alice_codec_last_error_message() or b"").decode()


def test_call_level_refusals(codec):
    lib = codec.load_library()
    good, _ = _blobs()
    stats = codec._test_last_rects_stats()
    bad = C.c_uint32(7)
    offsets = np.full(4, SENTINEL, np.uint64)
    op = offsets.ctypes.data_as(C.POINTER(C.c_uint64))
    assert not lib.alice_codec_decode_rects(None, 3, op, C.byref(bad)) and lib.alice_codec_last_error() == 9 and bad.value == NO_ITEM
    assert lib.alice_codec_dev_decode_rects(None, 3, C.byref(bad), None) == 9 and bad.value == NO_ITEM
    assert lib.alice_codec_dev_decode_rects(None, 3, None, None) == 9, "bad_item may be NULL"
    rows = [(good[0], None, 0, 1, (0, 0, 0, 0))] * 3
    ptr, code, b, off, msg = _host(codec, rows, n=0)
    assert not ptr and code == 2 and b == NO_ITEM and "at least one item" in msg
    ptr, code, b, off, msg = _host(codec, [(good[0], None, 0, 1, (1, 1, 2, 2))] * 1025)
    assert not ptr and code == 2 and b == NO_ITEM and "1025 items" in msg and "1024" in msg
    assert (off == SENTINEL).all()
    ptr, code, b, off, msg = _host(codec, rows, null_offsets=True)
    assert not ptr and code == 9 and b == NO_ITEM
    assert (offsets == SENTINEL).all()
    assert codec._test_last_rects_stats() == stats, "a refused call must not report work"
    assert codec.RECTS_MAX_ITEMS == 1024
    for call in (codec.decode_rects, codec.rects_decode_device):
        with pytest.raises(codec.CodecError) as e:
            call([])
        assert e.value.code == 2 and e.value.bad_item is None


@pytest.mark.parametrize("k", [0, 2, 4])
def test_item_refusals_name_the_item(codec, k):
    """item k of five is the one at fault, the others are fine items on containers of the three versions"""
    lib = codec.load_library()
    good, v1 = _blobs()
    stats = (codec._test_last_rects_stats(), codec._test_last_previews_stats(), codec._test_last_rect_stats())
    rects = [(0, 0, 0, 0), (2, 3, 4, 5), (0, 0, W, H), (W - 1, H - 1, 1, 1), (5, 0, 20, H)]
    fine = [(good[i % 3], None, i % F, 1, rects[i]) for i in range(5)]

    def with_item(row):
        rows = list(fine)
        rows[k] = row
        ptr, code, b, off, msg = _host(codec, rows)
        assert not ptr and (off == SENTINEL).all(), "a refusal wrote its offsets"
        assert b == k and msg.startswith(f"item {k}: "), (b, msg)
        return code, msg

    assert with_item((None, 100, 0, 1, (0, 0, 0, 0)))[0] == 9
    code, msg = with_item((good[0][:10], None, 0, 1, (0, 0, 1, 1)))
    assert code == 4 and "too short" in msg
    code, msg = with_item((good[1][:-1], None, 0, 1, (0, 0, 1, 1)))
    assert code == 4 and "length mismatch" in msg
    code, msg = with_item((v1, None, 0, 1, (0, 0, 1, 1)))
    assert code == 4 and "version 1 has no random access (one serial chain per channel)" in msg
    other = good[0].copy()
    other[0] = ord("B")
    code, msg = with_item((other, None, 0, 1, (0, 0, 1, 1)))
    assert code == 4 and "bad magic" in msg
    for first, count in ((0, 0), (0, F + 1), (F, 1), (2, F - 1), (0xFFFFFFFF, 2)):
        for rect in ((0, 0, 0, 0), (0, 0, 1, 1), (W, 0, 1, 1)):               # the range comes before the rectangle
            code, msg = with_item((good[2], None, first, count, rect))
            assert code == 2 and "frames" in msg, (first, count, msg)
    for rect in ((0, 0, 0, 1), (0, 0, 1, 0), (0, 0, 0, H), (3, 0, 0, 0), (W, 0, 1, 1), (0, H, 1, 1), (1, 0, W, 1), (0, 1, 1, H),
                 (0xFFFFFFFF, 0, 2, 1), (0, 0xFFFFFFFF, 1, 2)):
        code, msg = with_item((good[2], None, 0, 1, rect))
        assert code == 2 and "rectangle" in msg, (rect, msg)
    # the first item that fails decides: a later bad rectangle does not hide an earlier bad container, nor the other way round
    rows = list(fine)
    rows[k] = (v1, None, 0, 1, (0, 0, 1, 1))
    if k + 1 < len(rows):
        rows[k + 1] = (good[0], None, 0, 1, (W, 0, 1, 1))
    ptr, code, b, off, msg = _host(codec, rows)
    assert not ptr and code == 4 and b == k
    if k > 0:
        rows[k - 1] = (good[0], None, 0, 1, (W, 0, 1, 1))
        ptr, code, b, off, msg = _host(codec, rows)
        assert not ptr and code == 2 and b == k - 1 and "rectangle" in msg
    # the device twin: the null checks of every item come before the device is asked for
    dev_rows = [(good[0], None, 0, 1, (0, 0, 0, 0), 0x1000 + 0x100000 * i, 0, 0) for i in range(5)]
    dev_rows[k] = dev_rows[k][:5] + (None, 0, 0)
    assert _dev(codec, dev_rows)[:2] == (9, k)
    dev_rows[k] = (None, 100) + dev_rows[k][2:5] + (0x1000, 0, 0)
    assert _dev(codec, dev_rows)[:2] == (9, k)
    assert (codec._test_last_rects_stats(), codec._test_last_previews_stats(), codec._test_last_rect_stats()) == stats, \
        "a refused call must not report work"
    # the Python mirror carries the index
    with pytest.raises(codec.CodecError) as e:
        codec.decode_rects([(good[0], 0, 1)] * k + [(good[1], 0, 1, W, 0, 1, 1)] + [(good[1], 0, 1, 0, 0, 2, 2)])
    assert e.value.code == 2 and e.value.bad_item == k and f"item {k}: " in str(e.value)


def test_struct_layout_equals_the_header(codec):
    fields = ["alc", "len", "first", "count", "x", "y", "w", "h", "rgb_out", "row_pitch", "frame_pitch"]
    src = ('#include <stddef.h>\n#include <stdio.h>\n#include "alice_codec.h"\n'
           'int main(void) { printf("%zu %u", sizeof(alice_codec_rect_item), ALICE_RECTS_MAX_ITEMS);\n' +
           "".join(f'printf(" %zu", offsetof(alice_codec_rect_item, {n}));\n' for n in fields) + 'printf("\\n"); return 0; }\n')
    d = tempfile.mkdtemp(prefix="alice_rects_layout_")
    with open(os.path.join(d, "layout.c"), "w") as f:
        f.write(src)
    exe = os.path.join(d, "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(d, "layout.c"), "-o", exe])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    R = codec.RectItem
    assert got == [C.sizeof(R), codec.RECTS_MAX_ITEMS] + [getattr(R, n).offset for n in fields]
    assert got == [64, 1024, 0, 8, 16, 20, 24, 28, 32, 36, 40, 48, 56]


# ---- the disjointness rule ----
BASE = 0x10000


def _mosaic(rw=20, rh=12, count=2, gap=8):
    """a 2 x 2 mosaic of rw x rh crops of `count` frames in one pitched surface: rows of (rgb_out, count, w, h, row_pitch, frame_pitch)"""
    rp = 3 * 2 * rw + gap
    fp = rp * 2 * rh + 40
    return [(BASE + j * rh * rp + i * 3 * rw, count, rw, rh, rp, fp) for j in range(2) for i in range(2)], rp, fp


def test_a_mosaic_is_accepted_and_a_shifted_tile_is_not(codec):
    rule = codec._test_rects_outputs_disjoint
    rows, rp, fp = _mosaic()
    assert rule(rows) is None
    assert rule(rows[::-1]) is None
    for k, shift in ((1, -3), (0, 3), (2, -rp), (3, -3), (3, -rp)):        # one pixel, or one row, into a neighbour
        moved = list(rows)
        moved[k] = (rows[k][0] + shift,) + rows[k][1:]
        hit = rule(moved)
        other = {(1, -3): 0, (0, 3): 1, (2, -rp): 0, (3, -3): 2, (3, -rp): 1}[(k, shift)]
        assert hit == max(k, other), (k, shift, hit)
    # the later item of the FIRST conflicting pair in item order
    moved = list(rows)
    moved[3] = (rows[3][0] - 3,) + rows[3][1:]
    moved[1] = (rows[1][0] - 3,) + rows[1][1:]
    assert rule(moved) == 1
    # the message names the pair
    lib = codec.load_library()
    assert "item 1: its output overlaps the output of item 0" in lib.alice_codec_last_error_message().decode()
    assert lib.alice_codec_last_error() == 2


def test_packed_outputs(codec):
    rule = codec._test_rects_outputs_disjoint
    n = 2 * 5 * 4 * 3
    assert rule([(BASE, 2, 4, 5, 0, 0), (BASE + n, 2, 4, 5, 0, 0)]) is None, "back to back"
    assert rule([(BASE + n, 2, 4, 5, 0, 0), (BASE, 2, 4, 5, 0, 0)]) is None
    assert rule([(BASE, 2, 4, 5, 0, 0), (BASE + n - 1, 2, 4, 5, 0, 0)]) == 1, "one byte"
    assert rule([(BASE + n - 1, 2, 4, 5, 0, 0), (BASE, 2, 4, 5, 0, 0)]) == 1
    assert rule([(BASE, 2, 4, 5, 0, 0), (BASE + n, 1, 7, 3, 0, 0), (BASE + n + 62, 1, 1, 1, 0, 0)]) == 2
    assert rule([(BASE, 1, 4, 5, 0, 0)]) is None


def test_interleaved_ranges_that_are_no_boxes_of_one_surface(codec):
    rule = codec._test_rects_outputs_disjoint
    # equal pitches, but the second item's rows wrap past row_pitch: x_byte + 3 w > row_pitch
    rp, fp = 100, 100 * 10
    assert rule([(BASE, 1, 10, 4, rp, fp), (BASE + 50, 1, 10, 4, rp, fp)]) is None, "two columns of one surface"
    assert rule([(BASE, 1, 10, 4, rp, fp), (BASE + 80, 1, 10, 4, rp, fp)]) == 1, "bytes 80 .. 110 of a 100-byte row"
    # ... or its rows leave the frame: (y + h) row_pitch > frame_pitch
    assert rule([(BASE, 2, 10, 4, rp, fp), (BASE + 8 * rp + 50, 2, 10, 4, rp, fp)]) == 1
    assert rule([(BASE, 2, 10, 4, rp, fp), (BASE + 6 * rp + 50, 2, 10, 4, rp, fp)]) is None
    # different pitches with interleaved ranges: refused although the bytes may be disjoint
    assert rule([(BASE, 1, 10, 4, 100, 1000), (BASE + 50, 1, 10, 4, 200, 1000)]) == 1
    assert rule([(BASE, 2, 10, 4, 100, 1000), (BASE + 50, 2, 10, 4, 100, 2000)]) == 1
    # different pitches, ranges apart: accepted
    assert rule([(BASE, 1, 10, 4, 100, 1000), (BASE + 400, 1, 10, 4, 200, 1000)]) is None


def test_the_same_rows_of_different_frames(codec):
    rule = codec._test_rects_outputs_disjoint
    rp, fp = 3 * 40, 3 * 40 * 24
    at = 5 * rp + 30
    assert rule([(BASE + at, 2, 10, 6, rp, fp), (BASE + at + 2 * fp, 3, 10, 6, rp, fp)]) is None, "frames 0-1 and 2-4"
    assert rule([(BASE + at + 2 * fp, 3, 10, 6, rp, fp), (BASE + at, 2, 10, 6, rp, fp)]) is None
    assert rule([(BASE + at, 3, 10, 6, rp, fp), (BASE + at + 2 * fp, 3, 10, 6, rp, fp)]) == 1, "frame 2 twice"
    # same frames, rows apart; same rows, columns apart
    assert rule([(BASE + at, 2, 10, 6, rp, fp), (BASE + at + 6 * rp, 2, 10, 6, rp, fp)]) is None
    assert rule([(BASE + at, 2, 10, 6, rp, fp), (BASE + at + 5 * rp, 2, 10, 6, rp, fp)]) == 1
    assert rule([(BASE + at, 2, 10, 6, rp, fp), (BASE + at + 30, 2, 10, 6, rp, fp)]) is None
    assert rule([(BASE + at, 2, 10, 6, rp, fp), (BASE + at + 29, 2, 10, 6, rp, fp)]) == 1


def test_the_rule_refuses_what_it_cannot_judge(codec):
    lib = codec.load_library()
    bad = C.c_uint32(7)
    assert lib.alice_codec_test_rects_outputs_disjoint(None, 2, C.byref(bad)) == 9 and bad.value == NO_ITEM
    assert codec._test_rects_outputs_disjoint([(BASE, 1, 4, 4, 0, 0), (BASE + 4096, 1, 0, 0, 0, 0)]) == 1       # no explicit rectangle
    assert lib.alice_codec_last_error() == 2
    assert codec._test_rects_outputs_disjoint([(BASE, 1, 4, 4, 11, 0)]) == 0                                    # a pitch below 3 w
    assert "pitches" in lib.alice_codec_last_error_message().decode()
    # many items: the sweep and the pairwise search agree
    rows = [(BASE + 64 * i, 1, 4, 4, 0, 0) for i in range(1024)]
    assert codec._test_rects_outputs_disjoint(rows) is None
    rows[700] = (BASE + 64 * 300 + 47, 1, 4, 4, 0, 0)
    assert codec._test_rects_outputs_disjoint(rows) == 700


def test_new_symbols_are_exported_and_declared(codec):
    lib = codec.load_library()
    pub = open(os.path.join(ROOT, "include", "alice_codec.h")).read()
    tst = open(os.path.join(ROOT, "include", "alice_codec_test.h")).read()
    hpp = open(os.path.join(ROOT, "include", "alice_codec.hpp")).read()
    rs = open(os.path.join(ROOT, "bindings", "rust", "alice_codec_gpu.rs")).read()
    for name in ("alice_codec_decode_rects", "alice_codec_dev_decode_rects"):
        assert hasattr(lib, name) and re.search(r"\b" + name + r"\s*\(", pub), name
        assert name in hpp and name in rs, name
    for name in ("alice_codec_test_last_rects_stats", "alice_codec_test_rects_outputs_disjoint"):
        assert hasattr(lib, name) and re.search(r"\b" + name + r"\s*\(", tst), name
    for name in ("decode_rects", "rects_decode_device"):
        assert callable(getattr(codec, name))
        assert re.search(r"\binline [^;{]*\b" + name + r"\(", hpp) and re.search(r"\bpub (unsafe )?fn " + name + r"\(", rs), name
    assert len(codec._test_last_rects_stats()) == 11
    assert "conservative" in pub[pub.index("Many frame ranges and rectangles in one call"):], "the header states what the rule is"
