"""Frame ranges and half-size previews of a banded chunk without a device: the case table of
tests/test_gpu_banded_partial.py held to the plan classes it claims, the rule restated in numpy against the full reference
decode, the block counts of the design's table, and the host side of the C ABI with its refusals in their order."""
import ctypes as C
import os
import re
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import banded_partial_ref as BP  # noqa: E402
import banded_ref as B  # noqa: E402
import frames_ref as FR  # noqa: E402
import preview_ref as PR  # noqa: E402
import temporal_cases as TC  # noqa: E402
import wide_oracle as WO  # noqa: E402
from test_banded_host import band_at, clip, failures, patched, small, u32  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U8P = C.POINTER(C.c_uint8)


# ---- the plan ----
def test_case_table_reaches_every_plan_class():
    seen = {}
    for shape, kind, (t0, t1) in BP.all_cases():
        for mode in (BP.FRAMES, BP.PREVIEW):
            p = BP.plan(mode, kind, *shape, BP.LANE, t0, t1)
            assert p["blocks_total"] == 3 * len(p["bands"]) * p["blk_count"]
            assert p["stored"] == 3 * (p["b"] - p["a"]) * (p["dims"][0] * p["dims"][1] if mode == BP.FRAMES else p["Q"])
            for c in p["classes"]:
                seen.setdefault(c, (shape, kind, (t0, t1)))
    assert BP.REQUIRED_CLASSES <= set(seen), BP.REQUIRED_CLASSES - set(seen)

    def classes(shape):
        out = set()
        for kind in BP.kinds_for(shape):
            for r in BP.ranges_for(shape, kind):
                out |= BP.plan(BP.FRAMES, kind, *shape, BP.LANE, *r)["classes"]
        return out
    c = classes((128, 128, 16))
    assert "edges_on_block_edges" in c and not c & {"first_block_clipped", "last_block_clipped", "range_inside_one_block"}
    c = classes((160, 96, 16))
    assert {"first_block_clipped", "last_block_clipped", "short_last_block_planned", "q_mod4_0"} <= c
    p = BP.plan(BP.FRAMES, BP.CDF53, 160, 96, 16, BP.LANE, 15, 16)
    assert (p["Q"], p["n_band"], p["n_blocks"], p["idx_hi"]) == (3840, 30720, 8, 30720) and "short_last_block_planned" in p["classes"]
    assert "plane_longer_than_block" in classes((200, 120, 6))
    assert {"one_block_band", "pad_frame", "q_mod4_3", "window_touches_neither_end", "window_touches_both_ends"} <= classes((50, 38, 13))
    assert len(BP.ranges_for((50, 38, 13), BP.CDF97)) == 13 * 14 // 2
    assert "q_mod4_1" in classes((33, 17, 5))
    p = BP.plan(BP.PREVIEW, BP.CDF97, 5, 3, 7, BP.LANE, 0, 7)
    assert (p["Q"], p["n_band"]) == (6, 24) and {"q_below_64", "q_mod4_2", "one_block_band"} <= p["classes"]
    p = BP.plan(BP.FRAMES, BP.CDF53, 6, 4, 64, BP.LANE, 31, 32)
    assert (p["Q"], p["n_band"], p["idx_lo"], p["idx_hi"]) == (6, 192, 84, 102) and "q_below_64" in p["classes"]
    p = BP.plan(BP.FRAMES, BP.CDF53, 18, 10, 200, BP.LANE, 0, 200)
    assert (p["Q"], p["n_band"], p["blk_count"]) == (45, 4500, 2) and "q_below_64_two_blocks" in p["classes"]
    assert "range_inside_one_block" in classes((18, 10, 200))
    assert {"n_band_one", "one_frame_chunk", "q_mod4_1"} <= classes((2, 2, 1))
    assert BP.plan(BP.FRAMES, BP.CDF97, 40, 24, 1, BP.LANE, 0, 1)["dims"][2] == 2


def test_case_table_reaches_every_frame_count_class():
    """(b - a) / 2 is the half the finish kernels' temporal stream runs over (tests/temporal_cases.py)"""
    seen = {BP.window_class(kind, shape[2], t0, t1) for shape, kind, (t0, t1) in BP.all_cases()}
    assert seen >= set(TC.INVERSE_CLASSES), set(TC.INVERSE_CLASSES) - seen
    for kind in BP.WAVELETS:        # and the long windows under every wavelet, on the shape that carries them
        mine = {BP.window_class(kind, 64, *r) for r in BP.ranges_for(BP.CLASS_SHAPE, kind)}
        assert mine >= {c for c in TC.INVERSE_CLASSES if c[0] != "short"}, kind


def test_block_counts_of_the_design_table():
    """blocks per channel of one 1920x1080x64 chunk at L = 512, CDF 9/7 (a band is 507 blocks, a channel 4056)"""
    for r, prev, frames in (((31, 32), 160, 640), ((0, 64), 1014, 4056)):
        p = BP.plan(BP.PREVIEW, BP.CDF97, 1920, 1080, 64, 512, *r)
        assert p["n_blocks"] == 507 and p["blocks_total"] // 3 == prev, (r, p["blocks_total"])
        p = BP.plan(BP.FRAMES, BP.CDF97, 1920, 1080, 64, 512, *r)
        assert p["blocks_total"] // 3 == frames, (r, p["blocks_total"])
    # the base version's figures beside them
    assert PR.preview_plan(PR.CDF97, 1920, 1080, 64, 512, 31, 32)["n_planned"] == 328
    assert FR.frame_plan(FR.CDF97, 1920, 1080, 64, 512, 31, 32)["n_planned"] == 636


# ---- the rule in numpy ----
@pytest.mark.parametrize("kind", BP.WAVELETS)
@pytest.mark.parametrize("shape", [(50, 38, 13), (5, 3, 7)])
def test_the_rule_against_the_full_reference_decode(shape, kind):
    w, h, f = shape
    dims = BP.padded(w, h, f)
    pw, ph, pf = dims
    rgb = WO.smooth_plus_noise(w, h, f, seed=w + f)
    for base in (2, 3, 4):
        x = B.encode(rgb, w, h, f, 100 if base == 4 else 80, kind, base, BP.LANE)
        info, syms = B.decode_container(x)
        full = B.decode(x).reshape(f, h, w, 3)
        for t0, t1 in list(dict.fromkeys(FR.named_ranges(kind, f) + [(f // 2, f // 2 + 1), (f // 2, f // 2 + 2), (1, 2)])):
            tag = (shape, kind, base, (t0, t1))
            pf_, pp = BP.plan(BP.FRAMES, kind, w, h, f, BP.LANE, t0, t1), BP.plan(BP.PREVIEW, kind, w, h, f, BP.LANE, t0, t1)
            a, b = pf_["a"], pf_["b"]
            assert (a, b) == (pp["a"], pp["b"]) == FR.frame_window(kind, f, t0, t1)
            # frames: the gathered runs are the virtual chunk's volume, and its decode is the slice of the full decode
            vols = [BP.frames_volume(s, dims, pf_) for s in syms]
            for v, s in zip(vols, syms):
                assert np.array_equal(v, FR.window_volume(s, dims, a, b)), tag
            virt_info = dict(info, frames=b - a)
            virt = B.pixels(virt_info, [v.reshape(-1).astype(syms[0].dtype) for v in vols], base).reshape(b - a, h, w, 3)
            assert np.array_equal(virt[t0 - a:t1 - a], full[t0:t1]), tag
            # preview: bands 0 and 4 are the low-low quadrants of the window's planes; preview_ref on a virtual chunk that
            # holds nothing else equals preview_ref on the whole chunk's symbols
            want = PR.preview(syms, dims, f, kind, info["step"], base, t0, t1)
            virt_syms = []
            for s in syms:
                q = BP.preview_volume(s, dims, pp)
                assert np.array_equal(q, FR.window_volume(s, dims, a, b)[:, :ph // 2, :pw // 2]), tag
                v = np.zeros((b - a, ph, pw), syms[0].dtype)
                v[:, :ph // 2, :pw // 2] = q
                virt_syms.append(v.reshape(-1))
            got = PR.preview(virt_syms, (pw, ph, b - a), b - a, kind, info["step"], base, t0 - a, t1 - a)
            assert np.array_equal(got, want), tag


# ---- the C ABI, no device ----
CALLS = ("decode_banded_frames", "decode_banded_preview")


def _refused(codec, call, blob, first, count):
    with pytest.raises(codec.CodecError) as e:
        getattr(codec, call)(blob, first, count)
    return e.value.code, str(e.value)


def _stats(codec):
    return codec._test_last_banded_partial_stats("frames"), codec._test_last_banded_partial_stats("preview")


def test_null_arguments(codec):
    lib = codec.load_library()
    buf = np.frombuffer(small(), np.uint8)
    n = C.c_uint64(7)
    for name in ("alice_codec_decode_banded_frames", "alice_codec_decode_banded_preview"):
        fn = getattr(lib, name)
        assert not fn(None, 100, 0, 1, C.byref(n)) and lib.alice_codec_last_error() == 9 and n.value == 7
        assert not fn(buf.ctypes.data_as(U8P), buf.size, 0, 1, None) and lib.alice_codec_last_error() == 9
        assert not fn(None, 0, 0, 0, None) and lib.alice_codec_last_error() == 9       # before the header and the range
    for name in ("alice_codec_dev_decode_banded_frames", "alice_codec_dev_decode_banded_preview"):
        fn = getattr(lib, name)
        assert fn(None, 100, 0, 1, None, None) == 9
        assert fn(None, 100, 0, 0, C.c_void_p(256), None) == 9 and fn(C.c_void_p(256), 100, 0, 0, None, None) == 9


def test_every_header_failure_with_its_message(codec):
    """section 20.3's checks through the new calls, each ahead of a bad range; the directory checks after a good one"""
    blob = small()
    stats = _stats(codec)
    for name, bad, words in failures(blob):
        directory = name.endswith("block lengths")
        for call in CALLS:
            code, msg = _refused(codec, call, bad, 0, 1)
            assert code == 4 and words in msg, (name, call, msg)
            code, msg = _refused(codec, call, bad, 0, 0)          # a bad range as well
            if directory:
                assert code == 2 and "frames" in msg, (name, call, msg)      # the range is checked before the tables
            else:
                assert code == 4 and words in msg, (name, call, msg)
    for base in (3, 4):
        for call in CALLS:
            code, msg = _refused(codec, call, patched(small(base), 18, u32(16384)), 0, 1)
            assert code == 4 and "[64, 8192]" in msg
    assert _stats(codec) == stats, "a refused call must not report work"


def test_other_versions_bad_ranges_and_empty_chunks(codec):
    w, h, f = 6, 4, 2
    stats = _stats(codec)
    v1 = codec.FrameEncoder.with_wavelet(50, codec.WaveletType.Haar).encode(np.zeros(0, np.uint8), 0, 3, 3).to_bytes()
    others = {1: v1 + bytes(64), 2: B.encode_base(clip(w, h, f), w, h, f, 80, 0, 2, 64), 3: B.encode_base(clip(w, h, f), w, h, f, 80, 0, 3, 64),
              4: B.encode_base(clip(w, h, f), w, h, f, 100, 0, 4, 64)}
    for ver, blob in others.items():
        for call in CALLS:
            for first, count in ((0, 1), (0, 0)):
                code, msg = _refused(codec, call, blob, first, count)
                assert code == 4 and f"unsupported version: {ver} (expected 5)" in msg, (ver, call, msg)
    for base in (2, 3, 4):
        blob = small(base)
        for call in CALLS:
            for first, count in ((0, 0), (f, 1), (0, f + 1), (0xFFFFFFFF, 2)):
                code, msg = _refused(codec, call, blob, first, count)
                assert code == 2 and "frames [" in msg and f"chunk's {f} frames" in msg, (base, call, first, count, msg)
    enc = codec.FrameEncoder.with_wavelet(50, codec.WaveletType.Cdf97)
    for base in (2, 3, 4):
        for dims in ((0, 4, 4), (4, 4, 0)):
            empty = codec.encode_banded(enc, np.zeros(0, np.uint8), *dims, 0, base)
            assert len(empty) == B.HEADER
            for call in CALLS:
                for first, count in ((0, 1), (0, 0), (0, 4), (3, 1)):
                    assert _refused(codec, call, empty, first, count)[0] == 2, (base, dims, call, first, count)
    assert _stats(codec) == stats, "a refused call must not report work"


def test_a_short_table_entry_in_any_band_is_refused_on_the_host(codec):
    """all 24 block-length tables are checked on the way up: also those of bands a preview does not keep"""
    blob = small()
    info = B.parse_container(blob)
    at = B.HEADER
    for j in range(24):
        c, k = divmod(j, 8)
        for call in CALLS:
            code, msg = _refused(codec, call, patched(blob, at, u32(127)), 0, 1)
            assert code == 4 and f"channel {c} band {k}: block 0 is shorter than its lane directory" in msg, (j, call, msg)
            code, msg = _refused(codec, call, patched(blob, at, u32(struct.unpack_from("<I", blob, at)[0] + 1)), 0, 1)
            assert code == 4 and f"channel {c} band {k}: block lengths sum to" in msg, (j, call, msg)
        at += info["payload_len"][j]
    assert at == len(blob) and band_at(0, 1) - band_at(0, 0) == B.BAND
    if codec.device_count() < 1:   # without a device a call that passes every host check fails loudly
        for call in CALLS:
            assert _refused(codec, call, blob, 0, 1)[0] == 8


def test_new_symbols_are_exported_and_declared(codec):
    lib = codec.load_library()
    pub = open(os.path.join(ROOT, "include", "alice_codec.h")).read()
    tst = open(os.path.join(ROOT, "include", "alice_codec_test.h")).read()
    hpp = open(os.path.join(ROOT, "include", "alice_codec.hpp")).read()
    rs = open(os.path.join(ROOT, "bindings", "rust", "alice_codec_gpu.rs")).read()
    for name in ("alice_codec_decode_banded_frames", "alice_codec_dev_decode_banded_frames", "alice_codec_decode_banded_preview",
                 "alice_codec_dev_decode_banded_preview"):
        assert hasattr(lib, name) and re.search(r"\b" + name + r"\s*\(", pub), name
        assert name in hpp and name in rs, name
    for name in ("alice_codec_test_last_banded_frames_stats", "alice_codec_test_last_banded_preview_stats"):
        assert hasattr(lib, name) and re.search(r"\b" + name + r"\s*\(", tst), name
    for name in ("decode_banded_frames", "banded_frames_decode_device", "decode_banded_preview", "banded_preview_decode_device"):
        assert callable(getattr(codec, name))
        assert re.search(r"\binline [^;{]*\b" + name + r"\(", hpp) and re.search(r"\bpub (unsafe )?fn " + name + r"\(", rs), name
    assert len(codec._test_last_banded_partial_stats("frames")) == 6 and len(codec._test_last_banded_partial_stats("preview")) == 6
