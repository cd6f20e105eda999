"""Transcode without a device: the properties of the map over every pair of quantiser steps, the
integer arithmetic of the kernel restated in numpy against the rule's divisions, the reference transcoder on whole
containers, the kept-row rule of the size prediction, the refusals of the C ABI (all of them host code that runs before a
device is looked for), and one printed table of what a transcode costs in PSNR against a direct encode."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle.alice_oracle_np as o  # noqa: E402
import reversible_ref as R4  # noqa: E402
import split_rate_ref as SR  # noqa: E402
import split_ref as R2  # noqa: E402
import transcode_cases as TC  # noqa: E402
import transcode_ref as T  # noqa: E402
import wide_oracle as WO  # noqa: E402
import wide_ref as W3  # noqa: E402

U8 = np.arange(256, dtype=np.int64)
Z = np.arange(4351, dtype=np.int64)            # every z a version 3 / 4 lane stream decodes to


def kernel_map(z, s1: int, s2: int, wide: bool) -> np.ndarray:
    """requant_sym1 of csrc/transcode.hip, operation by operation, in unsigned 64-bit numpy: the reciprocal multiply, the
    saturating subtractions and the sign bit instead of the rule's divisions and signs."""
    z = np.asarray(z, np.uint64)
    if s2 <= s1:
        return z.astype(np.int64)
    hdz, magic = np.uint64(s2 // 2), np.uint64(((1 << 32) + s2 - 1) // s2)
    a = (z + np.uint64(1)) >> np.uint64(1)
    m = np.where(a > 0, a * np.uint64(s1) + np.uint64(2 * (s1 // 2)), np.uint64(0))
    adj = np.where(m > hdz, m - hdz, np.uint64(0))
    assert int(adj.max()) < 1 << 32
    q = (adj * magic) >> np.uint64(32)
    neg = (z & np.uint64(1)) ^ np.uint64(1)
    t = (q << np.uint64(1)) + neg
    t = np.where(t > 0, t - np.uint64(1), np.uint64(0))
    return (np.minimum(t, np.uint64(65535)) if wide else (t & np.uint64(0xFF))).astype(np.int64)


def test_map_properties_for_every_step_pair():
    q1_u8, q1_z = np.abs(T.coefficient(U8)), np.abs(T.coefficient(Z))
    for s1 in range(1, 65):
        for s2 in range(1, 65):
            n8 = T.requant(U8, s1, s2, False).astype(np.int64)
            nz = T.requant(Z, s1, s2, True).astype(np.int64)
            if s2 <= s1:                                   # untouched, and mapping at s2 == s1 would be the identity too
                assert np.array_equal(n8, U8) and np.array_equal(nz, Z)
            assert (np.abs(T.coefficient(n8)) <= q1_u8).all(), (s1, s2)     # no new escape, no residual guard
            assert (np.abs(T.coefficient(nz)) <= q1_z).all(), (s1, s2)
            # the 256-entry table of the version 2 kernel is filled by the arithmetic of the wide one
            assert np.array_equal(kernel_map(U8, s1, s2, False), n8), (s1, s2)
            assert np.array_equal(kernel_map(Z, s1, s2, True), nz), (s1, s2)
            # ... and up to the largest u16, which the stage call accepts
            big = np.arange(65536 - 4096, 65536, dtype=np.int64)
            assert np.array_equal(kernel_map(big, s1, s2, True), T.requant(big, s1, s2, True)), (s1, s2)


def test_mapping_at_the_same_step_would_be_the_identity():
    for s in range(1, 65):
        for sym, wide in ((U8, False), (Z, True)):
            q = o.quantize(T.centre(sym, s), s, s)
            assert np.array_equal(W3.wide_symbols(q) if wide else o.to_symbols(q), sym), s


def test_a_step_one_source_maps_to_the_direct_encodes_symbols():
    v = np.arange(-2048, 2048, dtype=np.int64)
    for s2 in range(1, 65):
        direct = o.quantize(v, s2, s2)
        assert np.array_equal(T.requant(W3.wide_symbols(v), 1, s2, True), W3.wide_symbols(direct)), s2
        narrow = v[(v >= -127) & (v <= 128)]                # the coefficients a u8 symbol holds without wrapping
        assert np.array_equal(T.requant(o.to_symbols(narrow), 1, s2, False), o.to_symbols(o.quantize(narrow, s2, s2))), s2


@pytest.mark.parametrize("version", [2, 3, 4])
def test_unchanged_step_and_lanes_return_the_input(version):
    w, h, f = TC.SHAPES["padding_on_every_axis"]
    for kind in (0, 1, 2):
        src = TC.source(version, w, h, f, kind, 80)
        assert T.transcode(src, 80) == src
        assert T.transcode(src, 81) == src and SR.quality_to_step(81) == SR.quality_to_step(80) - 1   # a finer target
        assert T.transcode(src, 100, 64, 0) == src
        again = T.transcode(src, 80, 128)
        assert again != src and T.transcode(again, 80, 64) == src           # laned again, and back
    empty = TC.source(version, 0, 5, 3, 0, 80)
    assert len(empty) == T.HEADER and T.transcode(empty, 80) == empty
    assert T.transcode(empty, 50)[:4] == b"ALCC" and len(T.transcode(empty, 50)) == T.HEADER


@pytest.mark.parametrize("version", [2, 3, 4])
def test_kept_rows_of_the_prediction_and_per_channel_steps(version):
    src = TC.mixed_source(version)
    _, info, syms = T._decoded(src)
    assert info["step"] == [4, 9, 20]
    rows = T.step_histograms(src)
    own = [W3.histogram(s) if version >= 3 else np.bincount(s, minlength=256) for s in syms]
    for c, s1 in enumerate(info["step"]):
        for step in range(1, 65):
            if step <= s1:
                assert np.array_equal(rows[step - 1, c], own[c]), (c, step)     # the channel would be left untouched
        assert not np.array_equal(rows[63, c], own[c]), c                         # a coarser step maps it
    # target step 9 (quality 88): one channel mapped, one at the boundary, one kept at 20
    q9 = next(q for q in range(101) if SR.quality_to_step(q) == 9)
    out = T.transcode(src, q9)
    _, got, new = T._decoded(out)
    assert got["step"] == [9, 9, 20] and got["dead_zone"] == [9, 9, 20]
    assert not np.array_equal(new[0], syms[0]) and np.array_equal(new[1], syms[1]) and np.array_equal(new[2], syms[2])
    lo, hi = T.predict(src)
    for q in (0, 30, q9, 100):
        assert int(lo[q]) <= len(T.transcode(src, q)) <= int(hi[q]), q
    assert T.transcode(src, 100) == src


def test_reference_budget_rule_stays_within_the_trial_limit():
    """the budget cases of tests/test_gpu_transcode.py: the reference alone needs at most ALICE_SPLIT_REFINE_TRIALS"""
    w, h, f = TC.SHAPES[TC.BUDGET_SHAPE]
    lo_q, hi_q = TC.BUDGET_RANGE
    for version, quality in ((2, 95), (3, 100)):
        src = TC.source(version, w, h, f, 0, quality)
        for b in TC.budgets(lambda q: len(T.transcode(src, q))):
            q, fits, trials, data = T.choose_transcode(src, b, lo_q, hi_q)
            print(f"v{version} budget {b}: quality {q} fits {fits} trials {trials} size {len(data)}")
            assert trials <= SR.REFINE_TRIALS == 4
            assert (len(data) <= b) == fits
    with pytest.raises(T.InvalidBitstream):
        T.choose_transcode(TC.source(4, w, h, f, 0, 100), 10 ** 6, lo_q, hi_q)
    assert T.choose_transcode(TC.source(4, w, h, f, 0, 100), 10 ** 6, lo_q, hi_q, 0, 3)[3][4] == 3


# ---- the C ABI refuses on the host, in the words of its twins ----

def _refusal(fn, *args, **kw):
    import alice_codec_amd as a
    with pytest.raises(a.CodecError) as e:
        fn(*args, **kw)
    return e.value.code, str(e.value)


def _calls(a):
    return [lambda d, **k: a.transcode(d, 50, **k),
            lambda d, **k: a.transcode_to_size(d, 10 ** 6, 10, 95, **k),
            lambda d, **k: a.predict_transcode_sizes(d, **{x: y for x, y in k.items() if x == "lane_symbols"})]


def test_c_abi_refusals_without_a_device(codec):
    a = codec
    w, h, f = TC.SHAPES["short_block_empty_lanes"]
    good = {v: TC.source(v, w, h, f, 0, 90) for v in (2, 3, 4)}
    v1 = o.encode(TC.clip(w, h, f), w, h, f, 90, 0)
    bad_wavelet = bytearray(good[2]); bad_wavelet[5] = 3
    damaged = {"version 1": v1, "truncated": good[3][:T.HEADER - 1], "fixed fields": good[3][:10], "wavelet": bytes(bad_wavelet),
               "magic": b"ALCD" + good[2][4:]}
    for name, data in damaged.items():
        twin = _refusal(a.decode_frames, data, 0, 1)       # the partial decodes refuse the same container in the same words
        assert twin[0] == 4, name
        for call in _calls(a):
            assert _refusal(call, data) == twin, name
    assert "version 1 has no random access" in _refusal(a.transcode, v1, 50)[1]
    # lane_symbols outside the version's range: the encoders' words
    rgb = TC.clip(w, h, f)
    enc = a.FrameEncoder.with_wavelet(90, a.WaveletType.Cdf53)
    for v, encode, bad in ((2, a.encode_split, (63, 100, 32768)), (3, a.encode_wide, (32, 16384)), (4, a.encode_reversible, (16384,))):
        for L in bad:
            twin = _refusal(encode, enc, rgb, w, h, f, L)
            assert twin[0] == 2
            for call in _calls(a):
                assert _refusal(call, good[v], lane_symbols=L) == twin, (v, L)
    # out_version: 0 keeps, 3 and 4 for a wide source, nothing else
    for v, ov in ((2, 2), (2, 3), (2, 4), (2, 1), (3, 2), (3, 5), (4, 2), (4, 1), (3, 255)):
        for call in _calls(a)[:2]:
            code, msg = _refusal(call, good[v], out_version=ov)
            assert code == 2 and f"out_version {ov}" in msg, (v, ov)
    # the budget call: the quality range in the encoders' words, then a version 4 result
    twin = _refusal(a.encode_split_to_size, rgb, w, h, f, 10 ** 6, a.WaveletType.Cdf53, 50, 40)
    assert twin[0] == 2 and _refusal(a.transcode_to_size, good[3], 10 ** 6, 50, 40) == twin
    for data, k in ((good[4], {}), (good[3], {"out_version": 4})):
        code, msg = _refusal(a.transcode_to_size, data, 10 ** 6, 10, 95, **k)
        assert code == 4 and "version 4" in msg and "out_version = 3" in msg
    # damage the host sees: a block table that does not add up
    broken = bytearray(good[3]); broken[T.HEADER] ^= 1
    assert _refusal(a.transcode, bytes(broken), 50) == _refusal(a.decode_wide, bytes(broken))
    # null and range checks of the stage call
    assert _refusal(a.requant_symbols_device, 0, 0, 4, False, 1, 2)[0] == 9
    assert _refusal(a.requant_symbols_device, 4096, 4096, 4, False, 0, 2)[0] == 5
    assert _refusal(a.requant_symbols_device, 4096, 4096, 4, False, 2, 65)[0] == 5
    assert _refusal(a.requant_symbols_device, 4097, 4097, 4, True, 1, 2)[0] == 2          # u16 at an odd address
    assert _refusal(a.requant_symbols_device, 4096, 4098, 4, False, 1, 2)[0] == 2         # overlap that is not in place
    assert _refusal(a.transcode_device, 0, 0, [1630], 50, 4096, 4096)[0] == 9


def test_psnr_of_a_transcode_next_to_the_direct_encode():
    """48 x 32 x 8 smooth-plus-noise clip, version 3: the exact facts are asserted, the dB values printed."""
    w, h, f = 48, 32, 8
    rgb = WO.smooth_plus_noise(w, h, f)
    print()
    print("wavelet  source -> target   direct dB   transcode dB   direct bytes   transcode bytes")
    for kind, name in ((0, "CDF 5/3"), (1, "CDF 9/7")):
        for qs, qt in ((95, 60), (80, 50), (100, 80), (90, 89)):
            def pixels(blob):
                _, info, syms = T._decoded(blob)
                assert info["step"][0] == info["step"][1] == info["step"][2]
                return WO.inverse_quantised(o, [W3.from_wide_symbols(s) for s in syms], info["step"][0], W3.padded_dims(w, h, f), w, h, f, kind)
            step_s, _, q_s = WO.forward_quantised(o, rgb, w, h, f, qs, kind)
            step_t, _, q_t = WO.forward_quantised(o, rgb, w, h, f, qt, kind)
            src = W3.write_container(kind, w, h, f, 64, (step_s,) * 3, [W3.wide_symbols(q) for q in q_s])
            direct = W3.write_container(kind, w, h, f, 64, (step_t,) * 3, [W3.wide_symbols(q) for q in q_t])
            got = T.transcode(src, qt)
            p_direct, p_got = pixels(direct), pixels(got)
            print(f"{name}   {qs:3d} -> {qt:3d}        {WO.psnr(rgb, p_direct):8.3f}   {WO.psnr(rgb, p_got):8.3f}       "
                  f"{len(direct):8d}   {len(got):8d}")
            if (qs, qt) in ((100, 80), (90, 89)):
                assert got == direct and np.array_equal(p_got, p_direct)
