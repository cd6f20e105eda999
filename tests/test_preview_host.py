"""Half-resolution preview without a device: the gain constant from the lifting steps, the window
rule on the restatement of tests/preview_ref.py, its fidelity against the 2x2 box average of the full decode, the case table
of tests/test_gpu_preview.py held to the plan classes it claims, and the host side of the C ABI."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle.alice_oracle_np as o  # noqa: E402
import frames_ref as FR  # noqa: E402
import preview_ref as PR  # noqa: E402
import temporal_cases as TC  # noqa: E402
import wide_oracle as WO  # noqa: E402
import wide_ref as R3  # noqa: E402
from test_frames_host import _encode_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gain_constant_from_the_lifting_steps():
    assert [PR.gain_constant(k) for k in (PR.CDF53, PR.CDF97, PR.HAAR)] == [65536, 47484, 65536]
    assert PR.dc_gain(PR.CDF53) == 1 and PR.dc_gain(PR.HAAR) == 1
    g = PR.dc_gain(PR.CDF97)
    assert abs(float(g) - 1.17480326) < 1e-8 and abs(65536 / float(g * g) - 47484.257) < 1e-3
    assert PR.K == {k: PR.gain_constant(k) for k in PR.WAVELETS}
    # K = 65536 is the identity of step 4 for every i32
    v = np.array([-2**31, -32769, -1, 0, 1, 32767, 2**31 - 1], np.int64)
    assert np.array_equal((v * 65536 + 32768) >> 16, v)


@pytest.mark.parametrize("version", [3, 4])      # the reference's inverse and the mirrored one
@pytest.mark.parametrize("kind", PR.WAVELETS)
def test_window_rule_on_the_preview(kind, version):
    """The preview of every (t0, t1) equals the slice of the preview of [0, f): every even pf from 2 to 24."""
    rng = np.random.default_rng(200 + kind)
    pw, ph = 6, 4
    q = (pw // 2) * (ph // 2) * 3
    tried = 0
    for pf in range(2, 25, 2):
        dims = (pw, ph, pf)
        syms = [R3.wide_symbols(rng.integers(-600, 601, pw * ph * pf)) for _ in range(3)]
        steps = (3, 5, 7)
        full = PR.preview(syms, dims, pf, kind, steps, version, 0, pf)
        for t0 in range(pf):
            for t1 in range(t0 + 1, pf + 1):
                got = PR.preview(syms, dims, pf, kind, steps, version, t0, t1)
                assert np.array_equal(got, full[t0 * q:t1 * q]), (kind, version, pf, t0, t1)
                tried += 1
    assert tried == 1378


# ---- fidelity floor, on the restatement alone ----
def _clip():
    w, h, f = 64, 48, 8
    t, y, x = np.meshgrid(np.arange(f), np.arange(h), np.arange(w), indexing="ij")
    r = 128 + 100 * np.sin((x + 3 * t) / 17) * np.cos(y / 23)
    g = 128 + 90 * np.sin((x + y + 2 * t) / 31)
    b = 128 + 80 * np.cos((x - y - t) / 13)
    rgb = np.stack([r, g, b], axis=-1) + np.random.default_rng(1).normal(0, 4, (f, h, w, 3))
    return np.clip(np.rint(rgb), 0, 255).astype(np.uint8).reshape(-1), w, h, f


def test_fidelity_floor():
    rgb, w, h, f = _clip()
    for kind in PR.WAVELETS:
        for q in (50, 80):
            step, dims, qs = WO.forward_quantised(o, rgb, w, h, f, q, kind)
            syms = [o.to_symbols(x) for x in qs]
            full = WO.inverse_quantised(o, [o.from_symbols(s) for s in syms], step, dims, w, h, f, kind)
            want = PR.box_average(full, w, h, f).reshape(-1)
            db = WO.psnr(PR.preview(syms, dims, f, kind, (step,) * 3, 2, 0, f), want)
            print(f"wavelet {kind} q {q}: preview against the box average {db:.1f} dB")
            assert db >= 25.0, (kind, q, db)
            if kind == PR.CDF97:
                raw = WO.psnr(PR.preview(syms, dims, f, kind, (step,) * 3, 2, 0, f, normalise=False), want)
                print(f"wavelet {kind} q {q}: without step 4 {raw:.1f} dB")
                assert raw <= 16.0, (q, raw)


# ---- the plan ----
def test_plan_figures_of_the_design():
    """blocks per channel of one 1920x1080x64 chunk at L = 512: frame-range decode against preview"""
    for kind, r, frames, prev in ((PR.CDF97, (31, 32), 636, 328), (PR.CDF97, (0, 1), 380, 194), (PR.CDF97, (24, 40), 1522, 782),
                                  (PR.CDF97, (0, 64), 4050, 2086), (PR.CDF53, (31, 32), 382, 196)):
        assert FR.frame_plan(kind, 1920, 1080, 64, 512, *r)["n_planned"] == frames
        assert PR.preview_plan(kind, 1920, 1080, 64, 512, *r)["n_planned"] == prev


def test_planned_blocks_hold_every_quadrant_symbol_and_nothing_more():
    for shape, kind, (t0, t1) in PR.all_cases():
        w, h, f = shape
        p = PR.preview_plan(kind, w, h, f, PR.LANE, t0, t1)
        pw, ph, pf = p["dims"]
        pos = np.arange(pw * ph * pf).reshape(pf, ph, pw)
        need = FR.window_volume(pos, p["dims"], p["a"], p["b"])[:, :p["qh"], :p["qw"]].reshape(-1)
        assert sorted(set((need // (64 * PR.LANE)).tolist())) == p["planned"], (shape, kind, (t0, t1))
        assert p["stored"] == 3 * need.size
        assert set(p["planned"]) <= set(FR.frame_plan(kind, w, h, f, PR.LANE, t0, t1)["planned"])


def test_case_table_reaches_every_plan_class():
    seen = {}
    for shape, kind, (t0, t1) in PR.all_cases():
        for c in PR.plan_classes(kind, *shape, PR.LANE, t0, t1):
            seen.setdefault(c, (shape, kind, (t0, t1)))
    assert PR.REQUIRED_CLASSES <= set(seen), PR.REQUIRED_CLASSES - set(seen)

    def classes(shape):
        out = set()
        for kind in PR.WAVELETS:
            for r in PR.ranges_for(shape, kind):
                out |= PR.plan_classes(kind, *shape, PR.LANE, *r)
        return out
    c = classes((128, 128, 8))
    assert {"blocks_skipped_inside_a_plane", "plane_end_aligned", "q_mod4_0"} <= c and "plane_end_clipped" not in c
    p = PR.preview_plan(PR.CDF53, 128, 128, 8, PR.LANE, 0, 8)
    assert p["n_blocks"] == 32 and p["planned"] == [b for b in range(32) if b % 4 < 2]       # half of them
    assert {"plane_end_clipped", "blocks_skipped_inside_a_plane"} <= classes((200, 120, 6))
    assert {"block_shared_by_two_planes", "short_last_block", "pad_frame", "qw_odd", "q_mod4_3"} <= classes((50, 38, 13))
    assert {"one_block_channel", "q_mod4_1"} <= classes((33, 17, 5))
    assert {"qw_odd", "q_mod4_2"} <= classes((5, 3, 7))
    assert {"qw_one", "one_frame_chunk", "q_mod4_1"} <= classes((2, 2, 1))
    assert {"one_frame_chunk", "window_touches_both_ends"} <= classes((40, 24, 1))
    assert len(PR.ranges_for(PR.ALL_RANGES_SHAPE, PR.CDF97)) == 13 * 14 // 2


def test_every_frame_count_class_is_reached_by_a_window():
    """(b - a) / 2 is the half the finish kernel's stream runs over"""
    for kind in PR.WAVELETS:
        seen = set()
        for f in TC.FRAMES:
            for t0, t1 in PR.class_ranges(kind, f):
                a, b = FR.frame_window(kind, f, t0, t1)
                seen.add(TC.inverse_class((b - a) // 2))
        assert seen >= set(TC.INVERSE_CLASSES), (kind, set(TC.INVERSE_CLASSES) - seen)


# ---- the C ABI, no device ----
def test_preview_dims(codec):
    for w, h in ((1, 1), (2, 2), (3, 5), (1920, 1080), (0xFFFFFFFF, 0xFFFFFFFE)):
        assert codec.preview_dims(w, h) == PR.preview_dims(w, h)
    for w, h in ((0, 4), (4, 0), (0, 0)):
        with pytest.raises(codec.CodecError) as e:
            codec.preview_dims(w, h)
        assert e.value.code == 2
    lib = codec.load_library()
    v = C.c_uint32(0)
    assert lib.alice_codec_preview_dims(4, 4, None, C.byref(v)) == 9
    assert lib.alice_codec_preview_dims(4, 4, C.byref(v), None) == 9


def _refused(codec, blob, first, count):
    with pytest.raises(codec.CodecError) as e:
        codec.decode_preview(blob, first, count)
    return e.value.code, str(e.value)


def test_decode_preview_validation_order(codec):
    """frames_validate's checks, in its order and with its codes; all host code"""
    lib = codec.load_library()
    w, h, f = 33, 17, 5
    rgb = WO.smooth_plus_noise(w, h, f)
    v1 = bytearray(o.encode(rgb, w, h, f, 80, FR.CDF53))
    n = C.c_uint64(7)
    assert not lib.alice_codec_decode_preview(None, 100, 0, 1, C.byref(n)) and lib.alice_codec_last_error() == 9
    buf = np.frombuffer(bytes(v1), np.uint8)
    assert not lib.alice_codec_decode_preview(buf.ctypes.data_as(C.POINTER(C.c_uint8)), buf.size, 0, 1, None) and lib.alice_codec_last_error() == 9
    assert lib.alice_codec_dev_decode_preview(None, 100, 0, 1, None, None) == 9
    stats = codec._test_last_preview_stats()
    for first, count in ((0, 1), (0, 0), (9, 9)):
        code, msg = _refused(codec, bytes(v1), first, count)
        assert code == 4 and "version 1 has no random access (one serial chain per channel)" in msg
    bad = bytearray(v1)
    bad[0] = ord("B")
    code, msg = _refused(codec, bytes(bad), 0, 1)
    assert code == 4 and "bad magic" in msg
    assert _refused(codec, bytes(v1[:10]), 0, 1)[0] == 4
    for version in (2, 3, 4):
        blob = _encode_ref(version, rgb, w, h, f, 80, FR.CDF53, 64)
        for first, count in ((0, 0), (3, 0), (0, f + 1), (f, 1), (2, f - 1), (0xFFFFFFFF, 2)):
            code, msg = _refused(codec, blob, first, count)
            assert code == 2 and "frames" in msg, (version, first, count, msg)
        other = bytearray(blob)
        other[4] = 5
        code, msg = _refused(codec, bytes(other), 0, 0)
        assert code == 4 and "unsupported version: 5" in msg
        other = bytearray(blob)
        other[5] = 3
        code, msg = _refused(codec, bytes(other), 0, 0)
        assert code == 4 and "wavelet" in msg
        code, msg = _refused(codec, blob[:-1], 0, 0)
        assert code == 4 and "length mismatch" in msg
    enc = codec.FrameEncoder.with_wavelet(80, codec.WaveletType.Cdf97)
    for make in (codec.encode_split, codec.encode_wide, codec.encode_reversible):
        for dims in ((0, 4, 4), (4, 4, 0)):
            empty = make(enc, np.zeros(0, np.uint8), *dims)
            for first, count in ((0, 1), (0, 0), (0, 4)):
                assert _refused(codec, empty, first, count)[0] == 2
    assert codec._test_last_preview_stats() == stats, "a refused call must not report work"


def test_new_symbols_are_exported_and_declared(codec):
    lib = codec.load_library()
    pub = open(os.path.join(ROOT, "include", "alice_codec.h")).read()
    tst = open(os.path.join(ROOT, "include", "alice_codec_test.h")).read()
    hpp = open(os.path.join(ROOT, "include", "alice_codec.hpp")).read()
    rs = open(os.path.join(ROOT, "bindings", "rust", "alice_codec_gpu.rs")).read()
    for name in ("alice_codec_preview_dims", "alice_codec_decode_preview", "alice_codec_dev_decode_preview"):
        assert hasattr(lib, name) and re.search(r"\b" + name + r"\s*\(", pub), name
        assert name in hpp and name in rs, name
    assert hasattr(lib, "alice_codec_test_last_preview_stats") and re.search(r"\balice_codec_test_last_preview_stats\s*\(", tst)
    for name in ("preview_dims", "decode_preview", "preview_decode_device"):
        assert callable(getattr(codec, name))
        assert re.search(r"\binline [^;{]*\b" + name + r"\(", hpp) and re.search(r"\bpub (unsafe )?fn " + name + r"\(", rs), name
    assert callable(codec._test_last_preview_stats)
