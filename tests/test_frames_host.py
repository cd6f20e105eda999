"""Frame ranges without a device: the window rule against both inverse restatements, the plan
end to end on the CPU for each lane format, alice_codec_frames_window through the C ABI, the validation order of
alice_codec_decode_frames, and the case table of tests/test_gpu_frames.py held to the plan classes it claims."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle.alice_oracle_np as o  # noqa: E402
import frames_ref as FR  # noqa: E402
import reversible_ref as RR  # noqa: E402
import split_ref as R2  # noqa: E402
import wide_oracle as WO  # noqa: E402
import wide_ref as R3  # noqa: E402

INVERSES = {
    "reference": lambda v, kind: o._lift_axis(v, 0, o.STEPS[kind], True),
    "mirrored": lambda v, kind: RR.mirror_axis(v, 0, o.STEPS[kind]),
}


def _window_mismatches(kind, inverse, halo):
    """(windows tried, windows whose windowed inverse differs from the slice of the full one) over every even pf in 2..24
    and every (t0, t1), on random coefficients."""
    rng = np.random.default_rng(100 + kind)
    tried = bad = 0
    for pf in range(2, 25, 2):
        coef = rng.integers(-20000, 20001, (pf, 7)).astype(np.int64)
        full = inverse(coef, kind)
        half = pf // 2
        for t0 in range(pf):
            for t1 in range(t0 + 1, pf + 1):
                a, b = FR.frame_window(kind, pf, t0, t1, halo)
                assert a % 2 == 0 and b % 2 == 0 and 0 <= a <= t0 and t1 <= b <= pf
                virt = np.concatenate([coef[a // 2:b // 2], coef[half + a // 2:half + b // 2]], axis=0)
                got = inverse(virt, kind)[t0 - a:t1 - a]
                tried += 1
                bad += not np.array_equal(got, full[t0:t1])
    return tried, bad


@pytest.mark.parametrize("name", sorted(INVERSES))
@pytest.mark.parametrize("kind", FR.WAVELETS)
def test_window_rule_is_exact_and_tight(kind, name):
    ns = FR.LIFT_STEPS[kind]
    assert ns == len(o.STEPS[kind])
    tried, bad = _window_mismatches(kind, INVERSES[name], None)
    assert tried == 1378 and bad == 0
    tried, bad = _window_mismatches(kind, INVERSES[name], ns - 1)
    print(f"wavelet {kind}, {name} inverse: halo {ns - 1} fails {bad} of {tried} windows")
    assert bad > 0, "a halo of NS - 1 must fail somewhere: the rule is tight, not just safe (Haar included)"


def test_window_formula_and_planes():
    assert FR.frame_window(FR.CDF97, 64, 31, 32) == (26, 36) and len(FR.window_planes(64, 26, 36)) == 10
    assert FR.frame_window(FR.CDF53, 64, 31, 32) == (28, 34) and FR.frame_window(FR.HAAR, 64, 31, 32) == (28, 34)
    assert FR.frame_window(FR.CDF97, 1, 0, 1) == (0, 2) and FR.frame_window(FR.CDF53, 13, 12, 13) == (10, 14)
    assert FR.window_planes(14, 10, 14) == [5, 6, 12, 13]
    # the figures of DESIGN.md 14: one middle frame of 1920 x 1080 x 64 at L = 512
    p97 = FR.frame_plan(FR.CDF97, 1920, 1080, 64, 512, 31, 32)
    p53 = FR.frame_plan(FR.CDF53, 1920, 1080, 64, 512, 31, 32)
    assert (p97["n_blocks"], p97["n_planned"], p53["n_planned"]) == (4050, 636, 382)


# ---- the plan end to end on the CPU, one case per version ----
def _encode_ref(version, rgb, w, h, f, q, kind, L):
    step, dims, qs = WO.forward_quantised(o, rgb, w, h, f, q, kind)
    if version == 2:
        return R2.write_container(kind, w, h, f, L, (step,) * 3, [o.to_symbols(x) for x in qs])
    blob = R3.write_container(kind, w, h, f, L, (step,) * 3, [R3.wide_symbols(x) for x in qs])
    return blob if version == 3 else RR.with_version(blob, 4)


def _decode_syms(version, blob):
    """-> (info, symbols per channel, symbols -> quantised coefficients, coefficients -> RGB for (dims, f))"""
    if version == 2:
        info, syms = R2.decode_container(blob)
        unmap = o.from_symbols
    else:
        info, syms = R3.decode_container(RR.with_version(blob, 3))
        unmap = R3.from_wide_symbols
    w, h, kind, steps = info["width"], info["height"], info["wavelet"], info["step"]

    def to_rgb(qs, dims, f):
        if version == 4:
            return RR.inverse_quantised(qs, steps, dims, w, h, f, kind)
        assert len(set(steps)) == 1
        return WO.inverse_quantised(o, qs, steps[0], dims, w, h, f, kind)
    return info, syms, unmap, to_rgb


@pytest.mark.parametrize("version,kind,q", [(2, FR.CDF97, 80), (3, FR.CDF53, 95), (4, FR.HAAR, 100)])
@pytest.mark.parametrize("shape", [(33, 17, 5), (50, 38, 13)])
def test_plan_end_to_end_on_the_cpu(shape, version, kind, q):
    w, h, f = shape
    L = FR.LANE
    rgb = WO.smooth_plus_noise(w, h, f, seed=w + f)
    blob = _encode_ref(version, rgb, w, h, f, q, kind, L)
    info, syms, unmap, to_rgb = _decode_syms(version, blob)
    dims = R2.padded_dims(w, h, f)
    full = to_rgb([unmap(s) for s in syms], dims, f).reshape(f, h, w, 3)
    if version == 4:
        assert np.array_equal(full.reshape(-1), rgb)
    for t0, t1 in FR.named_ranges(kind, f) + [(f // 2, f // 2 + 1), (f // 2, f // 2 + 2)]:
        p = FR.frame_plan(kind, w, h, f, L, t0, t1)
        a, b = p["a"], p["b"]
        assert p["dims"] == dims
        # every symbol of the window lies in a planned block, and the ranges are the planes' positions
        pos = np.arange(dims[0] * dims[1] * dims[2]).reshape(dims[2], dims[1], dims[0])
        wpos = FR.window_volume(pos, dims, a, b).reshape(-1)
        assert set(np.unique(wpos // (64 * L)).tolist()) == set(p["planned"])
        assert np.array_equal(wpos, np.concatenate([np.arange(lo, hi) for lo, hi in p["ranges"]]))
        vdims = (dims[0], dims[1], b - a)
        virt = to_rgb([unmap(FR.window_volume(s, dims, a, b).reshape(-1)) for s in syms], vdims, b - a).reshape(b - a, h, w, 3)
        assert np.array_equal(virt[t0 - a:t1 - a], full[t0:t1]), (shape, version, kind, (t0, t1))


# ---- the C ABI, no device ----
def test_frames_window_through_the_c_abi(codec):
    for kind in FR.WAVELETS:
        for f in list(range(1, 27)) + [63, 64, 0xFFFFFFFE]:
            firsts = range(f) if f < 30 else (0, 1, 5, f // 2, f - 9, f - 1)
            for t0 in firsts:
                for t1 in sorted({t0 + 1, min(t0 + 3, f), f}):
                    assert codec.frames_window(codec.WaveletType(kind), f, t0, t1 - t0) == FR.frame_window(kind, f, t0, t1), (kind, f, t0, t1)
    for args, code in (((0, 8, 0, 0), 2), ((0, 8, 8, 1), 2), ((0, 8, 3, 6), 2), ((1, 0, 0, 1), 2), ((2, 8, 0xFFFFFFFF, 2), 2), ((3, 8, 0, 1), 4),
                       ((0, 0xFFFFFFFF, 0, 1), 3)):
        with pytest.raises(codec.CodecError) as e:
            codec.frames_window(*args)
        assert e.value.code == code, args
    lib = codec.load_library()
    a = C.c_uint32(0)
    assert lib.alice_codec_frames_window(0, 8, 0, 1, None, C.byref(a)) == 9
    assert lib.alice_codec_frames_window(0, 8, 0, 1, C.byref(a), None) == 9


def _refused(codec, blob, first, count):
    with pytest.raises(codec.CodecError) as e:
        codec.decode_frames(blob, first, count)
    return e.value.code, str(e.value)


def test_decode_frames_validation_order(codec):
    """Null arguments, fixed fields and magic, the version byte, that version's header checks, then the range -- all on
    the host, so none of it needs a device."""
    lib = codec.load_library()
    w, h, f = 33, 17, 5
    rgb = WO.smooth_plus_noise(w, h, f)
    v1 = bytearray(o.encode(rgb, w, h, f, 80, FR.CDF53))
    assert v1[:4] == b"ALCC" and v1[4] == 1
    n = C.c_uint64(7)
    assert not lib.alice_codec_decode_frames(None, 100, 0, 1, C.byref(n)) and lib.alice_codec_last_error() == 9
    buf = np.frombuffer(bytes(v1), np.uint8)
    assert not lib.alice_codec_decode_frames(buf.ctypes.data_as(C.POINTER(C.c_uint8)), buf.size, 0, 1, None) and lib.alice_codec_last_error() == 9
    assert lib.alice_codec_dev_decode_frames(None, 100, 0, 1, None, None) == 9
    # version 1: refused with the message that says why, before the range is looked at
    for first, count in ((0, 1), (0, 0), (9, 9)):
        code, msg = _refused(codec, bytes(v1), first, count)
        assert code == 4 and "version 1 has no random access (one serial chain per channel)" in msg
    # the magic comes before the version
    bad = bytearray(v1)
    bad[0] = ord("B")
    code, msg = _refused(codec, bytes(bad), 0, 1)
    assert code == 4 and "bad magic" in msg
    assert _refused(codec, bytes(v1[:10]), 0, 1)[0] == 4            # too short for the fixed fields
    for version in (2, 3, 4):
        blob = _encode_ref(version, rgb, w, h, f, 80, FR.CDF53, 64)
        for first, count in ((0, 0), (3, 0), (0, f + 1), (f, 1), (2, f - 1), (0xFFFFFFFF, 2)):
            code, msg = _refused(codec, blob, first, count)
            assert code == 2 and "frames" in msg, (version, first, count, msg)
        # an unknown version, then a header check (the wavelet byte): both before the range
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
    # an empty chunk refuses every range
    enc = codec.FrameEncoder.with_wavelet(80, codec.WaveletType.Cdf97)
    for make in (codec.encode_split, codec.encode_wide, codec.encode_reversible):
        for dims in ((0, 4, 4), (4, 4, 0)):
            empty = make(enc, np.zeros(0, np.uint8), *dims)
            for first, count in ((0, 1), (0, 0), (0, 4)):
                assert _refused(codec, empty, first, count)[0] == 2


# ---- the case table reaches every class of the plan ----
def test_case_table_reaches_every_plan_class():
    seen = {}
    for shape, kind, (t0, t1) in FR.all_cases():
        p = FR.frame_plan(kind, *shape, FR.LANE, t0, t1)
        for c in p["classes"]:
            seen.setdefault(c, (shape, kind, (t0, t1)))
    assert set(seen) == FR.REQUIRED_CLASSES, (FR.REQUIRED_CLASSES - set(seen), set(seen) - FR.REQUIRED_CLASSES)
    # the classes the shapes were chosen for, by shape
    def classes(shape, kind):
        out = set()
        for r in FR.ranges_for(shape, kind):
            out |= FR.frame_plan(kind, *shape, FR.LANE, *r)["classes"]
        return out
    assert {"start_aligned", "end_aligned", "gap_between_ranges", "blocks_skipped", "separate_blocks"} <= classes((64, 64, 16), FR.CDF53)
    assert "edge_inside_block" not in classes((64, 64, 16), FR.CDF97)
    assert {"start_clipped", "end_clipped", "shared_block", "short_last_block", "pad_frame"} <= classes((50, 38, 13), FR.CDF97)
    assert "one_block_channel" in classes((33, 17, 5), FR.HAAR)
    for shape in ((40, 24, 1), (40, 24, 2)):
        assert all(FR.frame_plan(k, *shape, FR.LANE, *r)["classes"] >= {"merged"} for k in FR.WAVELETS for r in FR.ranges_for(shape, k))
    assert len(FR.ranges_for(*FR.ALL_RANGES_CASE)) == 13 * 14 // 2
