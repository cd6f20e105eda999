"""PSNR-floor encodes (alice_codec_encode_to_psnr, alice_codec_dev_encode_to_psnr) against the rule of tests/quality_ref.py fed
with squared errors computed on the CPU oracle: the chosen quality, whether the floor was reached, the number of trials
(through the test hook), the bytes and the reported dB."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quality_ref as Q  # noqa: E402
import wide_oracle as WO  # noqa: E402
import wide_ref as R  # noqa: E402

import torch  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
W, H, F = 64, 48, 8
N = W * H * F * 3
L = 128
FORMATS = [(Q.FORMAT_SPLIT, 96), (Q.FORMAT_WIDE, 100)]     # version 2 up to where its symbols do not wrap


def trials_of(codec, n=1):
    t = np.zeros(n, np.uint32)
    assert codec.load_library().alice_codec_test_last_quality_trials(t.ctypes.data_as(C.POINTER(C.c_uint32)), n) == n
    return [int(x) for x in t]


def stride_for(codec, w, h, f):
    return (codec.SPLIT_HEADER_BYTES + 3 * codec.wide_stream_bound(int(np.prod(R.padded_dims(w, h, f))), L) + 255) & ~255


def host_call(codec, version):
    return codec.encode_split_to_psnr if version == Q.FORMAT_SPLIT else codec.encode_wide_to_psnr


def dev_call(codec, version):
    return codec.split_encode_to_psnr_device if version == Q.FORMAT_SPLIT else codec.wide_encode_to_psnr_device


def plain_encode(codec, version, rgb, w, h, f, k, q):
    enc = codec.FrameEncoder.with_wavelet(q, codec.WaveletType(k))
    return (codec.encode_split if version == Q.FORMAT_SPLIT else codec.encode_wide)(enc, rgb, w, h, f, L)


@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("version,max_q", FORMATS)
def test_choices_equal_the_rule_on_oracle_numbers(gpu_codec, version, max_q, k):
    a = gpu_codec
    rgb = WO.smooth_plus_noise(W, H, F)
    table = Q.step_table(version, rgb, W, H, F, k, max_q)
    targets = Q.midway_targets(table, N)
    d_rgb = torch.from_numpy(rgb).to(DEV)
    stride = stride_for(a, W, H, F)
    d_out = torch.zeros(stride, dtype=torch.uint8, device=DEV)
    seen_trials = set()
    for j, t in enumerate(targets):
        q, reached, trials = Q.choose(table, N, t, 0, max_q)
        want_db = Q.psnr_from_sse(table[Q.step_of(q)], N)
        # every target goes through the device call
        chosen, ok, db, sizes = dev_call(a, version)(d_rgb.data_ptr(), W, H, F, 1, a.WaveletType(k), t, d_out.data_ptr(), stride,
                                                     min_quality=0, max_quality=max_q, lane_symbols=L)
        assert (int(chosen[0]), bool(ok[0]), trials_of(a)[0]) == (q, reached, trials), (version, k, t)
        assert float(db[0]) == want_db and want_db >= t
        assert d_out[:int(sizes[0])].cpu().numpy().tobytes() == plain_encode(a, version, rgb, W, H, F, k, q)
        seen_trials.add(trials)
        if j % 3 == 0:        # and every third through the host call as well
            data, hq, hok, hdb = host_call(a, version)(rgb, W, H, F, t, a.WaveletType(k), 0, max_q, L)
            assert (hq, hok, trials_of(a)[0]) == (q, reached, trials), (version, k, t)
            assert hdb == want_db and data == plain_encode(a, version, rgb, W, H, F, k, q)
    assert Q.MAX_TRIALS in seen_trials


@pytest.mark.parametrize("version,max_q", FORMATS)
def test_special_targets(gpu_codec, version, max_q):
    a = gpu_codec
    k = 1
    rgb = WO.smooth_plus_noise(W, H, F)
    table = Q.step_table(version, rgb, W, H, F, k, 100)
    finest = Q.step_of(max_q)
    best, worst = Q.psnr_from_sse(table[finest], N), Q.psnr_from_sse(table[64], N)
    call = host_call(a, version)
    # unreachable: max_q, not reached, the measured value of max_q's step, one trial
    data, q, ok, db = call(rgb, W, H, F, best + 0.5, a.WaveletType(k), 0, max_q, L)
    assert (q, ok, db, trials_of(a)) == (max_q, False, best, [1]) and data == plain_encode(a, version, rgb, W, H, F, k, max_q)
    # already met at min_q: exactly two trials
    data, q, ok, db = call(rgb, W, H, F, worst - 0.5, a.WaveletType(k), 0, max_q, L)
    assert (q, ok, db, trials_of(a)) == (0, True, worst, [2]) and data == plain_encode(a, version, rgb, W, H, F, k, 0)
    # a range of one step: one trial, and the lowest quality that has the step
    data, q, ok, db = call(rgb, W, H, F, 10.0, a.WaveletType(k), 97, 98, L)
    assert (q, ok, trials_of(a)) == Q.choose(table, N, 10.0, 97, 98)[:2] + ([1],)
    # qualities above 100 act as 100
    assert call(rgb, W, H, F, 10.0, a.WaveletType(k), 200, 255, L)[1] == 100
    if version == Q.FORMAT_WIDE:
        # exact: the reference's inverse is off by one somewhere at step 1, so +inf is not reached
        assert table[1] > 0
        data, q, ok, db = call(rgb, W, H, F, math.inf, a.WaveletType(k), 0, 100, L)
        assert (q, ok, db, trials_of(a)) == (100, False, Q.psnr_from_sse(table[1], N), [1])
    else:
        # version 2 wraps at the top: with max_q = 100 the finest step fails a target that q = 96 meets
        t = 0.5 * (Q.psnr_from_sse(table[4], N) + Q.psnr_from_sse(table[5], N))
        assert Q.choose(table, N, t, 0, 100) == (100, False, 1)
        data, q, ok, db = call(rgb, W, H, F, t, a.WaveletType(k), 0, 100, L)
        assert (q, ok, db, trials_of(a)) == (100, False, Q.psnr_from_sse(table[1], N), [1])
        assert call(rgb, W, H, F, t, a.WaveletType(k), 0, 96, L)[1:3] == (96, True)


@pytest.mark.parametrize("version,max_q", FORMATS)
def test_several_chunks_choose_for_themselves(gpu_codec, version, max_q):
    a = gpu_codec
    k = 0
    rng = np.random.default_rng(4)
    noisy = np.clip(WO.smooth_plus_noise(W, H, F, seed=9).astype(np.int16) + rng.integers(-60, 61, N), 0, 255).astype(np.uint8)
    chunks = [WO.smooth_plus_noise(W, H, F, seed=5), np.full(N, 77, np.uint8), noisy,
              (np.arange(N) % 251).astype(np.uint8)]
    t = 20.0
    want = [Q.choose(Q.step_table(version, c, W, H, F, k, max_q), N, t, 5, max_q) for c in chunks]
    assert len({q for q, _, _ in want}) == 4
    d_rgb = torch.from_numpy(np.concatenate(chunks)).to(DEV)
    stride = stride_for(a, W, H, F)
    d_out = torch.zeros(4 * stride, dtype=torch.uint8, device=DEV)
    st = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(st):
        chosen, ok, db, sizes = dev_call(a, version)(d_rgb.data_ptr(), W, H, F, 4, a.WaveletType(k), t, d_out.data_ptr(), stride,
                                                     min_quality=5, max_quality=max_q, lane_symbols=L, stream=st.cuda_stream)
    st.synchronize()
    assert [(int(chosen[i]), bool(ok[i])) for i in range(4)] == [w[:2] for w in want]
    assert trials_of(a, 4) == [w[2] for w in want]
    out = d_out.cpu().numpy()
    for i in range(4):
        table = Q.step_table(version, chunks[i], W, H, F, k, max_q)
        assert float(db[i]) == Q.psnr_from_sse(table[Q.step_of(want[i][0])], N)
        assert out[i * stride:i * stride + int(sizes[i])].tobytes() == plain_encode(a, version, chunks[i], W, H, F, k, want[i][0])
    # a stride too short for a chunk fails before the outputs change hands
    with pytest.raises(a.CodecError) as e:
        dev_call(a, version)(d_rgb.data_ptr(), W, H, F, 4, a.WaveletType(k), t, d_out.data_ptr(), 2000, min_quality=5, max_quality=max_q)
    assert e.value.code == 1


@pytest.mark.parametrize("version,max_q", FORMATS)
def test_regions(gpu_codec, version, max_q):
    a = gpu_codec
    FW, FH, w, h, f, k = 640, 360, 97, 51, 4, 1
    origins = [(3, 5), (541, 307)]
    rng = np.random.default_rng(22)
    frames = rng.integers(0, 256, (2 * f, FH, FW, 3), dtype=np.uint8)
    crops = []
    for i, (x0, y0) in enumerate(origins):
        crop = WO.smooth_plus_noise(w, h, f, seed=70 + 5 * i).reshape(f, h, w, 3)
        frames[i * f:(i + 1) * f, y0:y0 + h, x0:x0 + w] = crop
        crops.append(crop.reshape(-1))
    n_bytes = w * h * f * 3
    t = 33.0
    d_frames = torch.from_numpy(frames.reshape(-1)).to(DEV)
    stride = stride_for(a, w, h, f)
    d_out = torch.zeros(2 * stride, dtype=torch.uint8, device=DEV)
    chosen, ok, db, sizes = dev_call(a, version)(d_frames.data_ptr(), w, h, f, 2, a.WaveletType(k), t, d_out.data_ptr(), stride,
                                                 min_quality=10, max_quality=max_q, lane_symbols=L, frame_width=FW, frame_height=FH,
                                                 origins=origins)
    got_trials = trials_of(a, 2)
    out = d_out.cpu().numpy()
    for i in range(2):
        table = Q.step_table(version, crops[i], w, h, f, k, max_q)
        q, reached, trials = Q.choose(table, n_bytes, t, 10, max_q)
        assert (int(chosen[i]), bool(ok[i]), got_trials[i]) == (q, reached, trials), i
        assert float(db[i]) == Q.psnr_from_sse(table[Q.step_of(q)], n_bytes)
        assert out[i * stride:i * stride + int(sizes[i])].tobytes() == plain_encode(a, version, crops[i], w, h, f, k, q)


def _person_frames():
    """a textured box walking over a flat background; chunk 2 stands empty"""
    rng = np.random.default_rng(21)
    W_, H_, f, n = 96, 64, 4, 4
    bg = np.empty((H_, W_, 3), np.uint8)
    bg[:] = (40, 90, 160)
    texture = rng.integers(0, 256, (24, 18, 3), dtype=np.uint8)
    texture[(np.abs(texture.astype(np.int16) - bg[0, 0]) < 40).any(axis=2)] = (250, 5, 20)     # every box pixel is foreground
    frames = np.repeat(bg[None], n * f, axis=0)
    for t in range(n * f):
        if t // f == 2:
            continue
        x = 6 + 3 * t
        frames[t, 20:44, x:x + 18] = texture
    return W_, H_, f, n, bg, frames


@pytest.mark.parametrize("fmt", ["split", "wide"])
def test_person_chunks_with_a_floor(gpu_codec, fmt):
    a = gpu_codec
    W_, H_, f, n, bg, frames = _person_frames()
    hi = 96
    d_frames = torch.from_numpy(np.ascontiguousarray(frames).reshape(-1)).to(DEV)
    d_bg = torch.from_numpy(np.ascontiguousarray(bg).reshape(-1)).to(DEV)
    plain = a.encode_person_chunks(d_frames, d_bg, W_, H_, f, n, hi, format=fmt, lane_symbols=L)
    t = 30.0
    got = a.encode_person_chunks(d_frames, d_bg, W_, H_, f, n, hi, format=fmt, lane_symbols=L, min_psnr=t)
    assert [b for b, _ in got] == [b for b, _ in plain]
    one = host_call(a, Q.FORMAT_SPLIT if fmt == "split" else Q.FORMAT_WIDE)
    qualities = []
    for c, (bbox, alc) in enumerate(got):
        if c == 2:
            assert bbox == [0, 0, 0, 0] and alc == plain[2][1]
            continue
        bx, by, bw, bh = bbox
        crop = np.ascontiguousarray(frames[c * f:(c + 1) * f, by:by + bh, bx:bx + bw]).reshape(-1)
        data, q, ok, db = one(crop, bw, bh, f, t, a.WaveletType.Cdf53, 10, hi, L)       # the same call, box by box
        assert alc == data, c
        version = Q.FORMAT_SPLIT if fmt == "split" else Q.FORMAT_WIDE
        assert (q, ok) == Q.choose(Q.step_table(version, crop, bw, bh, f, 0, hi), crop.size, t, 10, hi)[:2]
        if ok:
            dec = (a.decode_split if fmt == "split" else a.decode_wide)(alc)
            assert Q.psnr_from_sse(Q.sse_of(crop, dec), crop.size) >= t
        qualities.append(q)
    assert qualities and min(qualities) < hi
