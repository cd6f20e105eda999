"""Many previews in one call without a device: every refusal of alice_codec_decode_previews and
alice_codec_dev_decode_previews that is host code, with its code and the index of the item that decided it, that a refusal
leaves `offsets` and the statistics hook alone, the layout of alice_codec_preview_item against the ctypes mirror, and that
the new symbols are declared in every mirror."""
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


def _blobs():
    rgb = WO.smooth_plus_noise(W, H, F)
    good = [np.frombuffer(_encode_ref(v, rgb, W, H, F, 80, FR.CDF53, 64), np.uint8) for v in (2, 3, 4)]
    v1 = np.frombuffer(bytes(o.encode(rgb, W, H, F, 80, FR.CDF53)), np.uint8)
    return good, v1


def _host(codec, rows, n=None, null_offsets=False):
    """-> (pointer, code, bad_item, offsets) of alice_codec_decode_previews over rows of (array or None, len or None, first, count)"""
    lib = codec.load_library()
    arr = (codec.PreviewItem * max(len(rows), 1))()
    for i, (buf, length, first, count) in enumerate(rows):
        arr[i] = codec.PreviewItem(None if buf is None else buf.ctypes.data, (0 if buf is None else buf.size) if length is None else length,
                                   first, count, None)
    offsets = np.full(len(rows) + 1, SENTINEL, np.uint64)
    bad = C.c_uint32(7)
    ptr = lib.alice_codec_decode_previews(arr, len(rows) if n is None else n, None if null_offsets else offsets.ctypes.data_as(C.POINTER(C.c_uint64)),
                                          C.byref(bad))
    msg = lib.alice_codec_last_error_message()
    return ptr, lib.alice_codec_last_error(), bad.value, offsets, (msg or b"").decode()


def test_call_level_refusals(codec):
    lib = codec.load_library()
    good, _ = _blobs()
    stats = codec._test_last_previews_stats()
    bad = C.c_uint32(7)
    offsets = np.full(4, SENTINEL, np.uint64)
    op = offsets.ctypes.data_as(C.POINTER(C.c_uint64))
    assert not lib.alice_codec_decode_previews(None, 3, op, C.byref(bad)) and lib.alice_codec_last_error() == 9 and bad.value == NO_ITEM
    assert lib.alice_codec_dev_decode_previews(None, 3, C.byref(bad), None) == 9 and bad.value == NO_ITEM
    assert lib.alice_codec_dev_decode_previews(None, 3, None, None) == 9, "bad_item may be NULL"
    rows = [(good[0], None, 0, 1)] * 3
    ptr, code, b, off, msg = _host(codec, rows, n=0)
    assert not ptr and code == 2 and b == NO_ITEM and "at least one item" in msg
    ptr, code, b, off, msg = _host(codec, [(good[0], None, 0, 1)] * 1025)
    assert not ptr and code == 2 and b == NO_ITEM and "1025 items" in msg and "1024" in msg
    assert (off == SENTINEL).all()
    ptr, code, b, off, msg = _host(codec, rows, null_offsets=True)
    assert not ptr and code == 9 and b == NO_ITEM
    assert (offsets == SENTINEL).all()
    assert codec._test_last_previews_stats() == stats, "a refused call must not report work"
    assert codec.PREVIEWS_MAX_ITEMS == 1024
    with pytest.raises(codec.CodecError) as e:
        codec.decode_previews([])
    assert e.value.code == 2 and e.value.bad_item is None
    with pytest.raises(codec.CodecError) as e:
        codec.previews_decode_device([])
    assert e.value.code == 2 and e.value.bad_item is None


@pytest.mark.parametrize("k", [0, 2, 4])
def test_item_refusals_name_the_item(codec, k):
    """item k of five is the one at fault, the others are fine containers of the three versions"""
    lib = codec.load_library()
    good, v1 = _blobs()
    stats = codec._test_last_previews_stats()
    fine = [(good[i % 3], None, i % F, 1) for i in range(5)]

    def with_item(row):
        rows = list(fine)
        rows[k] = row
        ptr, code, b, off, msg = _host(codec, rows)
        assert not ptr and (off == SENTINEL).all(), "a refusal wrote its offsets"
        assert b == k and msg.startswith(f"item {k}: "), (b, msg)
        return code, msg

    assert with_item((None, 100, 0, 1))[0] == 9
    code, msg = with_item((good[0][:10], None, 0, 1))
    assert code == 4 and "too short" in msg
    code, msg = with_item((good[1][:-1], None, 0, 1))
    assert code == 4 and "length mismatch" in msg
    code, msg = with_item((v1, None, 0, 1))
    assert code == 4 and "version 1 has no random access (one serial chain per channel)" in msg
    for first, count in ((0, 0), (0, F + 1), (F, 1), (2, F - 1), (0xFFFFFFFF, 2)):
        code, msg = with_item((good[2], None, first, count))
        assert code == 2 and "frames" in msg, (first, count, msg)
    other = good[0].copy()
    other[0] = ord("B")
    code, msg = with_item((other, None, 0, 1))
    assert code == 4 and "bad magic" in msg
    # the first item that fails decides: a later bad range does not hide behind an earlier bad container, nor before it
    rows = list(fine)
    rows[k] = (v1, None, 0, 1)
    if k + 1 < len(rows):
        rows[k + 1] = (good[0], None, F, 1)
    ptr, code, b, off, msg = _host(codec, rows)
    assert not ptr and code == 4 and b == k
    # the device twin: the null checks of every item come before the device is asked for
    arr = (codec.PreviewItem * 5)()
    for i in range(5):
        arr[i] = codec.PreviewItem(good[0].ctypes.data, good[0].size, 0, 1, 0x1000)
    arr[k].rgb_out = None
    bad = C.c_uint32(9)
    assert lib.alice_codec_dev_decode_previews(arr, 5, C.byref(bad), None) == 9 and bad.value == k
    arr[k].rgb_out = 0x1000
    arr[k].alc = None
    assert lib.alice_codec_dev_decode_previews(arr, 5, C.byref(bad), None) == 9 and bad.value == k
    assert codec._test_last_previews_stats() == stats, "a refused call must not report work"
    # the Python mirror carries the index
    with pytest.raises(codec.CodecError) as e:
        codec.decode_previews([(good[0], 0, 1)] * k + [(v1, 0, 1)] + [(good[1], 0, 1)])
    assert e.value.code == 4 and e.value.bad_item == k and f"item {k}: " in str(e.value)


def test_struct_layout_equals_the_header(codec):
    src = ('#include <stddef.h>\n#include <stdio.h>\n#include "alice_codec.h"\n'
           'int main(void) { printf("%zu %zu %zu %zu %zu %zu %u\\n", sizeof(alice_codec_preview_item), offsetof(alice_codec_preview_item, alc), '
           'offsetof(alice_codec_preview_item, len), offsetof(alice_codec_preview_item, first), offsetof(alice_codec_preview_item, count), '
           'offsetof(alice_codec_preview_item, rgb_out), ALICE_PREVIEWS_MAX_ITEMS); return 0; }\n')
    d = tempfile.mkdtemp(prefix="alice_previews_layout_")
    with open(os.path.join(d, "layout.c"), "w") as f:
        f.write(src)
    exe = os.path.join(d, "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(d, "layout.c"), "-o", exe])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    P = codec.PreviewItem
    assert got == [C.sizeof(P), P.alc.offset, P.len.offset, P.first.offset, P.count.offset, P.rgb_out.offset, codec.PREVIEWS_MAX_ITEMS]
    assert got == [32, 0, 8, 16, 20, 24, 1024]


def test_new_symbols_are_exported_and_declared(codec):
    lib = codec.load_library()
    pub = open(os.path.join(ROOT, "include", "alice_codec.h")).read()
    tst = open(os.path.join(ROOT, "include", "alice_codec_test.h")).read()
    hpp = open(os.path.join(ROOT, "include", "alice_codec.hpp")).read()
    rs = open(os.path.join(ROOT, "bindings", "rust", "alice_codec_gpu.rs")).read()
    for name in ("alice_codec_decode_previews", "alice_codec_dev_decode_previews"):
        assert hasattr(lib, name) and re.search(r"\b" + name + r"\s*\(", pub), name
        assert name in hpp and name in rs, name
    assert hasattr(lib, "alice_codec_test_last_previews_stats") and re.search(r"\balice_codec_test_last_previews_stats\s*\(", tst)
    for name in ("decode_previews", "previews_decode_device"):
        assert callable(getattr(codec, name))
        assert re.search(r"\binline [^;{]*\b" + name + r"\(", hpp) and re.search(r"\bpub (unsafe )?fn " + name + r"\(", rs), name
    assert callable(codec._test_last_previews_stats)
    assert len(codec._test_last_previews_stats()) == 9
