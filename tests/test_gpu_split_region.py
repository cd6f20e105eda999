"""Version 2 on regions of device frames: the region encode must give encode_split's bytes of the numpy crop, the region
decode must paste decode_split's pixels and touch nothing else, and the hybrid person helpers must do both per chunk."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F, N, BW, BH = 6, 3, 32, 24
SENTINEL = 0xA5


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _source(seed, n_frames, H, W):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = ((x[None] * 3 + y[None] * 2 + np.arange(n_frames)[:, None, None] * 5) % 256).astype(np.int16)
    rgb = np.stack([base, 255 - base, (base * 7) % 256], axis=3) + rng.integers(-8, 9, (n_frames, H, W, 3))
    return np.clip(rgb, 0, 255).astype(np.uint8)


def _crop(frames, x0, y0):
    return np.ascontiguousarray(frames[:, y0:y0 + BH, x0:x0 + BW]).reshape(-1)


def _stride(a, L=0):
    return (a.SPLIT_HEADER_BYTES + 3 * a.split_stream_bound(BW * BH * F, L or 512) + 255) & ~255


def _blobs(out, stride, sizes):
    host = out.cpu().numpy().reshape(-1, stride)
    return [host[i, :int(s)].tobytes() for i, s in enumerate(sizes)]


# frames 70 x 50 (W % 4 != 0) and 96 x 64; origins with x0 % 4 == 0, x0 % 4 != 0, and the right / bottom edge
CASES = [(70, 50, [(0, 0), (13, 7), (70 - BW, 50 - BH)], 1), (96, 64, [(8, 4), (37, 11), (96 - BW, 64 - BH)], 0),
         (96, 64, [(64, 40), (3, 0), (0, 39)], 2)]


@pytest.mark.parametrize("W,H,origins,k", CASES)
def test_region_encode_and_decode(gpu_codec, W, H, origins, k):
    a = gpu_codec
    wt = a.WaveletType(k)
    src = _source(W + k, N * F, H, W)
    d = _dev(src)
    stride = _stride(a)
    qs = [80, 35, 97]
    for qualities in (None, qs):
        out = torch.full((N * stride,), 0xCD, dtype=torch.uint8, device="cuda:0")
        sizes = a.split_encode_regions_device(d.data_ptr(), W, H, origins, BW, BH, F, wt, 80, out.data_ptr(), stride, qualities, 64)
        got = _blobs(out, stride, sizes)
        for i, (x0, y0) in enumerate(origins):
            q = 80 if qualities is None else qs[i]
            want = a.encode_split(a.FrameEncoder.with_wavelet(q, wt), _crop(src[i * F:(i + 1) * F], x0, y0), BW, BH, F, 64)
            assert got[i] == want, (W, H, (x0, y0), q)
    # decode of the per-chunk-quality containers into a sentinel-filled frame buffer
    frames_out = torch.full((N * F * H * W * 3,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    a.split_decode_regions_device(out.data_ptr(), stride, sizes, frames_out.data_ptr(), W, H, origins)
    want = np.full((N * F, H, 3 * W), SENTINEL, np.uint8)
    for i, (x0, y0) in enumerate(origins):
        dec = a.decode_split(got[i]).reshape(F, -1)
        for t in range(F):
            a.paste_bbox_numpy(want[i * F + t], dec[t], [3 * x0, y0, 3 * BW, BH])
    assert np.array_equal(frames_out.cpu().numpy().reshape(N * F, H, 3 * W), want)


def test_rectangle_outside_the_frame(gpu_codec):
    a = gpu_codec
    W, H = 70, 50
    d = _dev(_source(1, N * F, H, W))
    stride = _stride(a)
    out = torch.full((N * stride,), 0xCD, dtype=torch.uint8, device="cuda:0")
    for origins in ([(0, 0), (39, 0), (0, 0)], [(0, 0), (0, 0), (0, 27)]):
        with pytest.raises(a.CodecError) as e:
            a.split_encode_regions_device(d.data_ptr(), W, H, origins, BW, BH, F, 0, 80, out.data_ptr(), stride)
        assert e.value.code == 2
        with pytest.raises(a.CodecError) as e:
            a.split_encode_to_budget_device(d.data_ptr(), BW, BH, F, N, 0, [10**6] * N, out.data_ptr(), stride, frame_width=W,
                                            frame_height=H, origins=origins)
        assert e.value.code == 2
    # the raw call leaves its sizes alone as well
    sizes = np.full(N, 77, np.uint64)
    o = np.array([(0, 0), (39, 0), (0, 0)], np.uint32).reshape(-1)
    rc = a.load_library().alice_codec_dev_encode_split_regions(d.data_ptr(), W, H, o.ctypes.data_as(C.POINTER(C.c_uint32)), BW, BH, F, N,
                                                               0, 80, None, 0, out.data_ptr(), stride,
                                                               sizes.ctypes.data_as(C.POINTER(C.c_uint64)), None)
    assert rc == 2 and (sizes == 77).all()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xCD).all()
    # a decode whose rectangle leaves the frame writes nothing either
    good = a.split_encode_regions_device(d.data_ptr(), W, H, [(0, 0)] * N, BW, BH, F, 0, 80, out.data_ptr(), stride)
    frames_out = torch.full((N * F * H * W * 3,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(a.CodecError) as e:
        a.split_decode_regions_device(out.data_ptr(), stride, good, frames_out.data_ptr(), W, H, [(0, 0), (39, 26), (0, 0)])
    assert e.value.code == 2
    assert (frames_out.cpu().numpy() == SENTINEL).all()


def test_budget_call_with_origins(gpu_codec):
    a = gpu_codec
    W, H, k = 96, 64, 1
    origins = [(8, 4), (37, 11), (96 - BW, 64 - BH)]
    src = _source(5, N * F, H, W)
    d = _dev(src)
    stride = _stride(a)
    crops = [_crop(src[i * F:(i + 1) * F], x0, y0) for i, (x0, y0) in enumerate(origins)]
    preds = [a.predict_split_sizes(c, BW, BH, F, k, 64) for c in crops]
    budgets = [int(preds[0].lo.min()) - 1, int(preds[1].hi[70]), 10**9]
    out = torch.full((N * stride,), 0xCD, dtype=torch.uint8, device="cuda:0")
    chosen, fits, sizes = a.split_encode_to_budget_device(d.data_ptr(), BW, BH, F, N, k, budgets, out.data_ptr(), stride, 10, 95, 64,
                                                          frame_width=W, frame_height=H, origins=origins)
    got = _blobs(out, stride, sizes)
    assert list(fits) == [False, True, True] and int(chosen[0]) == 10 and int(chosen[2]) == 95 and int(chosen[1]) >= 70
    for i in range(N):
        one, q, fit = a.encode_split_to_size(crops[i], BW, BH, F, budgets[i], k, 10, 95, 64)   # the host call of the crop agrees
        assert (q, fit) == (int(chosen[i]), bool(fits[i])) and got[i] == one
        assert got[i] == a.encode_split(a.FrameEncoder.with_wavelet(q, a.WaveletType(k)), crops[i], BW, BH, F, 64)
        if fit:
            assert len(got[i]) <= budgets[i]


def test_person_chunks_in_v2(gpu_codec):
    a = gpu_codec
    rng = np.random.default_rng(21)
    W, H, f, n, q = 96, 64, 4, 4, 90
    bg = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    frames = np.repeat(bg[None], n * f, axis=0)
    for t in range(n * f):                                    # a square walking across; chunk 2 stands empty
        if t // f == 2:
            continue
        x = 6 + 3 * t
        frames[t, 20:44, x:x + 18] = [200, 120, 90]
    d_frames, d_bg = _dev(frames), _dev(bg)
    v1 = a.encode_person_chunks(d_frames, d_bg, W, H, f, n, q)
    got = a.encode_person_chunks(d_frames, d_bg, W, H, f, n, q, format="split", lane_symbols=64)
    assert [b for b, _ in got] == [b for b, _ in v1]          # the same boxes as the v1 call
    enc = a.FrameEncoder(q, a.WaveletType.Cdf53)

    def crop_of(c, bbox):
        bx, by, bw, bh = bbox
        return np.ascontiguousarray(frames[c * f:(c + 1) * f, by:by + bh, bx:bx + bw]).reshape(-1)

    for c, (bbox, alc) in enumerate(got):
        assert a.alc_version(alc) == 2
        if c == 2:
            assert bbox == [0, 0, 0, 0] and alc == a.encode_split(enc, b"", 0, 0, f, 64)
            continue
        assert alc == a.encode_split(enc, crop_of(c, bbox), bbox[2], bbox[3], f, 64), c

    def decoded(chunks):
        out = _dev(np.repeat(bg[None], n * f, axis=0))
        a.decode_person_chunks(chunks, out, W, H, f)
        return out.cpu().numpy().reshape(n * f, H, 3 * W)

    def pasted(chunks):
        want = np.repeat(bg[None], n * f, axis=0).reshape(n * f, H, 3 * W)
        for c, (bbox, alc) in enumerate(chunks):
            bx, by, bw, bh = bbox
            if bw * bh == 0:
                continue
            dec = (a.decode_split(alc) if a.alc_version(alc) == 2 else a.FrameDecoder().decode(a.EncodedChunk.from_bytes(alc)))
            dec = dec.reshape(f, -1)
            for t in range(f):
                a.paste_bbox_numpy(want[c * f + t], dec[t], [3 * bx, by, 3 * bw, bh])
        return want

    assert np.array_equal(decoded(got), pasted(got))
    mixed = [v1[0], got[1], got[2], v1[3]]                    # version 1 and version 2 chunks in one list
    assert np.array_equal(decoded(mixed), pasted(mixed))
    # a byte budget per chunk
    box = got[0][0]
    p = a.predict_split_sizes(crop_of(0, box), box[2], box[3], f, 0, 64)
    budget = int(p.hi[40])
    small = a.encode_person_chunks(d_frames, d_bg, W, H, f, n, q, format="split", lane_symbols=64, max_bytes=budget)
    assert [b for b, _ in small] == [b for b, _ in got]
    for c, (bbox, alc) in enumerate(small):
        if c == 2:
            continue
        data, qq, fits = a.encode_split_to_size(crop_of(c, bbox), bbox[2], bbox[3], f, budget, 0, 10, q, 64)
        assert alc == data
        if fits:
            assert len(alc) <= budget
    assert len(small[0][1]) <= budget
    with pytest.raises(a.CodecError):
        a.encode_person_chunks(d_frames, d_bg, W, H, f, n, q, max_bytes=budget)
