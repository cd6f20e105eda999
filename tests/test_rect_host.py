"""Spatial rectangles of frame ranges without a device: the window rule on three axes against both
inverse restatements, that it is tight on x and on y, the plan figures of the design note, the case table of
tests/test_gpu_rect.py held to the plan classes it claims, alice_codec_rect_window through the C ABI and every refusal of
alice_codec_decode_rect that is host code, in order."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle.alice_oracle_np as o  # noqa: E402
import frames_ref as FR  # noqa: E402
import rect_ref as RF  # noqa: E402
import reversible_ref as RR  # noqa: E402
import wide_oracle as WO  # noqa: E402
from test_frames_host import _encode_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

AXIS_INVERSES = {
    "reference": lambda v, axis, kind: o._lift_axis(v, axis, o.STEPS[kind], True),
    "mirrored": lambda v, axis, kind: RR.mirror_axis(v, axis, o.STEPS[kind]),
}
VOLUMES = [(14, 10, 8), (22, 18, 12)]          # w, h, f: even, so the padded volume is the volume


def _inverse3(v, kind, axis_inverse):
    """temporal, columns, rows: the axis order of the container's inverse"""
    for axis in (0, 1, 2):
        v = axis_inverse(v, axis, kind)
    return v


def _random_window(rng, w, h, f):
    t0 = int(rng.integers(0, f)); t1 = int(rng.integers(t0 + 1, f + 1))
    x = int(rng.integers(0, w)); rw = int(rng.integers(1, w - x + 1))
    y = int(rng.integers(0, h)); rh = int(rng.integers(1, h - y + 1))
    return t0, t1, (x, y, rw, rh)


def _mismatches(kind, name, halo_of, n_windows=150):
    """(windows tried, windows whose virtual chunk's inverse differs from the slice of the full inverse) over n_windows random
    (frame range x rectangle) windows on each of the two volumes; halo_of(ns) = the halo per axis (t, y, x)"""
    inv = AXIS_INVERSES[name]
    rng = np.random.default_rng(300 + kind)
    ns = RF.LIFT_STEPS[kind]
    tried = bad = 0
    for w, h, f in VOLUMES:
        coef = rng.integers(-20000, 20001, (f, h, w)).astype(np.int64)
        full = _inverse3(coef, kind, inv)
        for _ in range(n_windows):
            t0, t1, rect = _random_window(rng, w, h, f)
            x, y, rw, rh = rect
            win = RF.windows(kind, w, h, f, t0, t1, rect, halo_of(ns))
            (ta, tb), (ya, yb), (xa, xb) = win
            for (a, b), c0, c1, pn in (((ta, tb), t0, t1, f), ((ya, yb), y, y + rh, h), ((xa, xb), x, x + rw, w)):
                assert a % 2 == 0 and b % 2 == 0 and 0 <= a <= c0 and c1 <= b <= pn
            virt = RF.cut(coef, (w, h, f), win)
            assert virt.shape == (tb - ta, yb - ya, xb - xa)
            got = _inverse3(virt, kind, inv)[t0 - ta:t1 - ta, y - ya:y + rh - ya, x - xa:x + rw - xa]
            tried += 1
            bad += not np.array_equal(got, full[t0:t1, y:y + rh, x:x + rw])
    return tried, bad


@pytest.mark.parametrize("name", sorted(AXIS_INVERSES))
@pytest.mark.parametrize("kind", RF.WAVELETS)
def test_rule_is_exact_and_tight_on_every_axis(kind, name):
    assert RF.LIFT_STEPS[kind] == len(o.STEPS[kind])
    tried, bad = _mismatches(kind, name, lambda ns: (ns, ns, ns))
    assert tried == 300 and bad == 0
    for axis, halo_of in (("x", lambda ns: (ns, ns, ns - 1)), ("y", lambda ns: (ns, ns - 1, ns))):
        tried, bad = _mismatches(kind, name, halo_of)
        print(f"wavelet {kind}, {name} inverse: a halo of NS - 1 on {axis} fails {bad} of {tried} windows")
        assert bad > 0, f"a halo of NS - 1 on {axis} must fail somewhere: the rule is tight, not just safe"


def test_windows_and_the_cut():
    assert RF.windows(RF.CDF97, 1920, 1080, 64, 31, 32, (832, 412, 256, 256)) == ((26, 36), (408, 672), (828, 1092))
    assert RF.windows(RF.CDF53, 33, 17, 5, 0, 5, (0, 0, 33, 17)) == ((0, 6), (0, 18), (0, 34))
    assert RF.windows(RF.HAAR, 33, 17, 5, 4, 5, (32, 16, 1, 1)) == ((2, 6), (14, 18), (30, 34))
    assert RF.windows(RF.CDF97, 64, 64, 16, 0, 1, (4, 5, 1, 1)) == ((0, 6), (0, 10), (0, 10))
    assert RF.axis_indices(14, 10, 14) == [5, 6, 12, 13]
    # on t the rule is frames_ref's
    for kind in RF.WAVELETS:
        for f in (1, 2, 5, 13, 16):
            for t0 in range(f):
                for t1 in range(t0 + 1, f + 1):
                    assert RF.windows(kind, 8, 8, f, t0, t1, (0, 0, 8, 8))[0] == FR.frame_window(kind, f, t0, t1)
    pos = np.arange(6 * 4 * 4).reshape(4, 4, 6)
    got = RF.cut(pos, (6, 4, 4), ((0, 2), (2, 4), (0, 6)))
    assert got.shape == (2, 2, 6) and got[:, :, 0].tolist() == [[6, 18], [54, 66]]


def test_plan_figures_of_the_design_note():
    """1920 x 1080 x 64, CDF 9/7, L = 512: a 256 x 256 rectangle at (832, 412) of frame 31"""
    p = RF.rect_plan(RF.CDF97, 1920, 1080, 64, 512, 31, 32, (832, 412, 256, 256), classes=False)
    q = FR.frame_plan(FR.CDF97, 1920, 1080, 64, 512, 31, 32)
    assert (p["n_blocks"], p["n_planned"], q["n_planned"]) == (4050, 174, 636)
    assert p["per_channel"] == 696960 and p["stored"] == 3 * 696960 and p["vdims"] == (264, 264, 10)
    assert 1920 * 1080 * 10 == 20736000
    whole = RF.rect_plan(RF.CDF97, 1920, 1080, 64, 512, 31, 32, (0, 0, 1920, 1080), classes=False)
    assert whole["planned"] == q["planned"] and whole["per_channel"] == 20736000
    assert (whole["ta"], whole["tb"]) == (q["a"], q["b"])


def test_whole_frame_plans_are_the_frame_range_plans():
    for shape in RF.SHAPES:
        w, h, f = shape
        for kind in RF.WAVELETS:
            for t0, t1 in RF.ranges_for(shape):
                p = RF.rect_plan(kind, w, h, f, RF.LANE, t0, t1, (0, 0, w, h))
                q = FR.frame_plan(kind, w, h, f, RF.LANE, t0, t1)
                assert p["planned"] == q["planned"] and (p["ta"], p["tb"]) == (q["a"], q["b"]), (shape, kind, t0, t1)
                assert {"x_full", "y_full"} <= p["classes"]


def test_case_table_reaches_every_plan_class():
    cases = RF.all_cases()
    assert len(cases) == 627
    assert RF.SHAPES == [(64, 64, 16), (50, 38, 13), (33, 17, 5), (160, 104, 6), (224, 104, 4), (5, 3, 7), (40, 24, 1)]
    seen = {}
    by_shape = {}
    for shape, kind, (t0, t1), rect in cases:
        p = RF.rect_plan(kind, *shape, RF.LANE, t0, t1, rect)
        for c in p["classes"]:
            seen.setdefault(c, (shape, kind, (t0, t1), rect))
            by_shape.setdefault(shape, set()).add(c)
    assert set(seen) == RF.REQUIRED_CLASSES, (RF.REQUIRED_CLASSES - set(seen), set(seen) - RF.REQUIRED_CLASSES)
    # the classes the shapes were chosen for, by shape
    assert "virtual_interior_tile" in by_shape[(224, 104, 4)]
    assert "gap_inside_plane" in by_shape[(160, 104, 6)]
    assert {"plane_below_64", "virtual_generic", "pad_column", "pad_row"} <= by_shape[(5, 3, 7)]
    assert {"one_block_channel", "pad_column", "pad_row"} <= by_shape[(33, 17, 5)]
    assert {"short_last_block", "block_partial"} <= by_shape[(50, 38, 13)]
    assert {"block_whole", "blocks_skipped"} <= by_shape[(64, 64, 16)]
    # every kind of rectangle and range the table promises is in it
    for shape in RF.SHAPES:
        w, h, f = shape
        for kind in RF.WAVELETS:
            rs = RF.rects_for(shape, kind)
            m = RF.LIFT_STEPS[kind] + 2
            assert {(0, 0, w, h), (0, 0, 1, 1), (w - 1, h - 1, 1, 1), (w // 2, h // 2, 1, 1)} <= set(rs)
            assert ((m, m, w - 2 * m, h - 2 * m) in rs) == (w > 2 * m and h > 2 * m)
            assert ((m + 1, m, 3, 2) in rs) == (m + 4 <= w and m + 2 <= h)
            assert all(x + rw <= w and y + rh <= h and rw >= 1 and rh >= 1 for x, y, rw, rh in rs)
            assert {(0, 1), (f - 1, f), (0, f), (f // 2, f // 2 + 1)} == set(RF.ranges_for(shape))
            assert RF.named_rects(shape, kind) <= set(rs)


# ---- the C ABI, no device ----
def test_rect_window_through_the_c_abi(codec):
    rng = np.random.default_rng(5)
    for kind in RF.WAVELETS:
        for w, h in ((1, 1), (2, 2), (5, 3), (33, 17), (64, 64), (1920, 1080), (0xFFFFFFFE, 0xFFFFFFFD)):
            rects = [(0, 0, w, h), (0, 0, 1, 1), (w - 1, h - 1, 1, 1), (w // 2, h // 2, 1, 1)]
            for _ in range(40):
                x = int(rng.integers(0, w)); y = int(rng.integers(0, h))
                rects.append((x, y, int(rng.integers(1, w - x + 1)), int(rng.integers(1, h - y + 1))))
            for rect in rects:
                _, (ya, yb), (xa, xb) = RF.windows(kind, w, h, 1, 0, 1, rect)
                assert codec.rect_window(codec.WaveletType(kind), w, h, *rect) == (xa, xb, ya, yb), (kind, w, h, rect)
    for args, code in (((0, 8, 8, 0, 0, 0, 1), 2), ((0, 8, 8, 0, 0, 1, 0), 2), ((0, 8, 8, 8, 0, 1, 1), 2), ((0, 8, 8, 0, 8, 1, 1), 2),
                       ((0, 8, 8, 4, 0, 5, 1), 2), ((0, 8, 8, 0, 4, 1, 5), 2), ((0, 8, 8, 0xFFFFFFFF, 0, 2, 1), 2),
                       ((0, 8, 8, 0, 0xFFFFFFFF, 1, 2), 2), ((0, 0, 8, 0, 0, 1, 1), 2), ((3, 8, 8, 0, 0, 1, 1), 4),
                       ((0, 0xFFFFFFFF, 8, 0, 0, 1, 1), 3), ((0, 8, 0xFFFFFFFF, 0, 0, 1, 1), 3)):
        with pytest.raises(codec.CodecError) as e:
            codec.rect_window(*args)
        assert e.value.code == code, args
    lib = codec.load_library()
    v = [C.c_uint32(0) for _ in range(4)]
    for missing in range(4):
        ptrs = [None if i == missing else C.byref(c) for i, c in enumerate(v)]
        assert lib.alice_codec_rect_window(0, 8, 8, 0, 0, 1, 1, *ptrs) == 9


def _refused(codec, blob, first, count, rect=(0, 0, 1, 1)):
    with pytest.raises(codec.CodecError) as e:
        codec.decode_rect(blob, first, count, *rect)
    return e.value.code, str(e.value)


def test_decode_rect_validation_order(codec):
    """frames_validate's checks in its order and with its codes, then the rectangle; all host code"""
    lib = codec.load_library()
    w, h, f = 33, 17, 5
    rgb = WO.smooth_plus_noise(w, h, f)
    v1 = bytearray(o.encode(rgb, w, h, f, 80, FR.CDF53))
    n = C.c_uint64(7)
    assert not lib.alice_codec_decode_rect(None, 100, 0, 1, 0, 0, 1, 1, C.byref(n)) and lib.alice_codec_last_error() == 9
    buf = np.frombuffer(bytes(v1), np.uint8)
    assert not lib.alice_codec_decode_rect(buf.ctypes.data_as(C.POINTER(C.c_uint8)), buf.size, 0, 1, 0, 0, 1, 1, None)
    assert lib.alice_codec_last_error() == 9
    assert lib.alice_codec_dev_decode_rect(None, 100, 0, 1, 0, 0, 1, 1, None, 0, 0, None) == 9
    stats = codec._test_last_rect_stats()
    # version 1: refused with the message that says why, before the range and the rectangle are looked at
    for first, count, rect in ((0, 1, (0, 0, 1, 1)), (0, 0, (0, 0, 1, 1)), (9, 9, (0, 0, 0, 0)), (0, 1, (40, 40, 1, 1))):
        code, msg = _refused(codec, bytes(v1), first, count, rect)
        assert code == 4 and "version 1 has no random access (one serial chain per channel)" in msg
    bad = bytearray(v1)
    bad[0] = ord("B")
    code, msg = _refused(codec, bytes(bad), 0, 1)
    assert code == 4 and "bad magic" in msg
    assert _refused(codec, bytes(v1[:10]), 0, 1)[0] == 4
    outside = ((0, 0, 0, 1), (0, 0, 1, 0), (w, 0, 1, 1), (0, h, 1, 1), (1, 0, w, 1), (0, 1, 1, h), (0xFFFFFFFF, 0, 2, 1),
               (0, 0xFFFFFFFF, 1, 2), (0, 0, 0xFFFFFFFF, 1), (0, 0, w + 1, h))
    for version in (2, 3, 4):
        blob = _encode_ref(version, rgb, w, h, f, 80, FR.CDF53, 64)
        # the range comes before the rectangle
        for first, count in ((0, 0), (3, 0), (0, f + 1), (f, 1), (2, f - 1), (0xFFFFFFFF, 2)):
            for rect in ((0, 0, 1, 1), outside[0], outside[2]):
                code, msg = _refused(codec, blob, first, count, rect)
                assert code == 2 and "frames" in msg and "rectangle" not in msg, (version, first, count, rect, msg)
        for rect in outside:
            code, msg = _refused(codec, blob, 0, 1, rect)
            assert code == 2 and "rectangle" in msg and f"{w}x{h} frame" in msg and "frames [" not in msg, (version, rect, msg)
        # an unknown version, then a header check (the wavelet byte), then the length: all before the range and the rectangle
        other = bytearray(blob)
        other[4] = 5
        code, msg = _refused(codec, bytes(other), 0, 0, outside[0])
        assert code == 4 and "unsupported version: 5" in msg
        other = bytearray(blob)
        other[5] = 3
        code, msg = _refused(codec, bytes(other), 0, 0, outside[0])
        assert code == 4 and "wavelet" in msg
        code, msg = _refused(codec, blob[:-1], 0, 0, outside[0])
        assert code == 4 and "length mismatch" in msg
    # an empty chunk refuses every range and rectangle
    enc = codec.FrameEncoder.with_wavelet(80, codec.WaveletType.Cdf97)
    for make in (codec.encode_split, codec.encode_wide, codec.encode_reversible):
        for dims in ((0, 4, 4), (4, 4, 0)):
            empty = make(enc, np.zeros(0, np.uint8), *dims)
            for first, count in ((0, 1), (0, 0), (0, 4)):
                assert _refused(codec, empty, first, count)[0] == 2
    assert codec._test_last_rect_stats() == stats, "a refused call must not report work"


def test_new_symbols_are_exported_and_declared(codec):
    lib = codec.load_library()
    pub = open(os.path.join(ROOT, "include", "alice_codec.h")).read()
    tst = open(os.path.join(ROOT, "include", "alice_codec_test.h")).read()
    hpp = open(os.path.join(ROOT, "include", "alice_codec.hpp")).read()
    rs = open(os.path.join(ROOT, "bindings", "rust", "alice_codec_gpu.rs")).read()
    for name in ("alice_codec_rect_window", "alice_codec_decode_rect", "alice_codec_dev_decode_rect"):
        assert hasattr(lib, name) and re.search(r"\b" + name + r"\s*\(", pub), name
        assert name in hpp and name in rs, name
    assert hasattr(lib, "alice_codec_test_last_rect_stats") and re.search(r"\balice_codec_test_last_rect_stats\s*\(", tst)
    for name in ("rect_window", "decode_rect", "rect_decode_device"):
        assert callable(getattr(codec, name))
        assert re.search(r"\binline [^;{]*\b" + name + r"\(", hpp) and re.search(r"\bpub (unsafe )?fn " + name + r"\(", rs), name
    assert callable(codec._test_last_rect_stats)
