"""Version 3 on regions of device frames: the region encode must give encode_wide's bytes of the numpy crop, the region
decode must paste decode_wide's pixels and touch nothing else, the budget call must agree with the host call of the crop,
and the hybrid person helpers must do all of it per chunk -- on crops that have escapes, where version 3 differs from
version 2."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_oracle as WO  # noqa: E402
import wide_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

N = 3
SENTINEL = 0xA5


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _source(seed, w, h, f, noise=8):
    """the sawtooth of tests/test_gpu_split_rate.py: smooth content gave crops without escapes"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = ((x[None] * 3 + y[None] * 2 + np.arange(f)[:, None, None] * 5) % 256).astype(np.int16)
    rgb = np.stack([base, 255 - base, (base * 7) % 256], axis=3) + rng.integers(-noise, noise + 1, (f, h, w, 3))
    return np.clip(rgb, 0, 255).astype(np.uint8).reshape(-1)


# (frame W, H, box w, h, f, origins, wavelet): 70 x 50 frames (W % 4 != 0) with an odd box; 96 x 64 with one dword-aligned
# origin and two byte-path origins
CASES = [(70, 50, 33, 17, 5, [(0, 0), (13, 7), (37, 33)], 0), (96, 64, 48, 32, 4, [(8, 4), (37, 11), (48, 32)], 1)]
L = 64


def _frames(W, H, f, k):
    return _source(W + H + k, W, H, N * f).reshape(N * f, H, W, 3)


def _crop(frames, i, f, x0, y0, bw, bh):
    return np.ascontiguousarray(frames[i * f:(i + 1) * f, y0:y0 + bh, x0:x0 + bw]).reshape(-1)


def _stride(a, bw, bh, f):
    pw, ph, pf = R.padded_dims(bw, bh, f)
    return (a.SPLIT_HEADER_BYTES + 3 * a.wide_stream_bound(pw * ph * pf, L) + 255) & ~255


def _blobs(out, stride, sizes):
    host = out.cpu().numpy().reshape(-1, stride)
    return [host[i, :int(s)].tobytes() for i, s in enumerate(sizes)]


def _escapes(crop, bw, bh, f, k, q=100):
    import oracle.alice_oracle_np as o
    _, _, qs = WO.forward_quantised(o, crop, bw, bh, f, q, k)
    return sum(int((R.wide_symbols(v) >= R.ESCAPE).sum()) for v in qs)


@pytest.mark.parametrize("W,H,bw,bh,f,origins,k", CASES)
def test_region_encode_and_decode(gpu_codec, W, H, bw, bh, f, origins, k):
    a = gpu_codec
    wt = a.WaveletType(k)
    src = _frames(W, H, f, k)
    crops = [_crop(src, i, f, x0, y0, bw, bh) for i, (x0, y0) in enumerate(origins)]
    for i, c in enumerate(crops):
        esc = _escapes(c, bw, bh, f, k)
        print(f"{W}x{H} crop {i} at {origins[i]}: {esc} escapes at q = 100")
        assert esc > 0                                   # a condition of the test: otherwise it repeats version 2's
    d = _dev(src)
    stride = _stride(a, bw, bh, f)
    qs = [100, 80, 100]
    for q_all, qualities in ((100, None), (80, None), (55, qs)):
        out = torch.full((N * stride,), 0xCD, dtype=torch.uint8, device="cuda:0")
        sizes = a.wide_encode_regions_device(d.data_ptr(), W, H, origins, bw, bh, f, wt, q_all, out.data_ptr(), stride, qualities, L)
        got = _blobs(out, stride, sizes)
        host = out.cpu().numpy().reshape(N, stride)
        for i in range(N):
            q = q_all if qualities is None else qs[i]
            want = a.encode_wide(a.FrameEncoder.with_wavelet(q, wt), crops[i], bw, bh, f, L)
            assert a.alc_version(got[i]) == 3 and got[i] == want, (W, H, origins[i], q)
            assert (host[i, int(sizes[i]):] == 0xCD).all()
    # decode of the per-chunk-quality containers into a sentinel-filled frame buffer
    frames_out = torch.full((N * f * H * W * 3,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    a.wide_decode_regions_device(out.data_ptr(), stride, sizes, frames_out.data_ptr(), W, H, origins)
    want = np.full((N * f, H, 3 * W), SENTINEL, np.uint8)
    for i, (x0, y0) in enumerate(origins):
        dec = a.decode_wide(got[i]).reshape(f, -1)
        for t in range(f):
            a.paste_bbox_numpy(want[i * f + t], dec[t], [3 * x0, y0, 3 * bw, bh])
    assert np.array_equal(frames_out.cpu().numpy().reshape(N * f, H, 3 * W), want)
    assert WO.psnr(crops[0], a.decode_wide(got[0])) > 35          # q = 100 comes back


def test_rectangle_outside_the_frame(gpu_codec):
    a = gpu_codec
    W, H, bw, bh, f, _, k = CASES[0]
    d = _dev(_frames(W, H, f, k))
    stride = _stride(a, bw, bh, f)
    out = torch.full((N * stride,), 0xCD, dtype=torch.uint8, device="cuda:0")
    one_right, one_down = [(0, 0), (W - bw + 1, 0), (0, 0)], [(0, 0), (0, 0), (0, H - bh + 1)]
    for origins in (one_right, one_down):
        with pytest.raises(a.CodecError) as e:
            a.wide_encode_regions_device(d.data_ptr(), W, H, origins, bw, bh, f, k, 100, out.data_ptr(), stride, None, L)
        assert e.value.code == 2
        with pytest.raises(a.CodecError) as e:
            a.wide_encode_to_budget_device(d.data_ptr(), bw, bh, f, N, k, [10**6] * N, out.data_ptr(), stride, lane_symbols=L,
                                           frame_width=W, frame_height=H, origins=origins)
        assert e.value.code == 2
    # the raw call leaves its sizes alone as well
    sizes = np.full(N, 77, np.uint64)
    o = np.array(one_right, np.uint32).reshape(-1)
    rc = a.load_library().alice_codec_dev_encode_wide_regions(d.data_ptr(), W, H, o.ctypes.data_as(C.POINTER(C.c_uint32)), bw, bh, f, N,
                                                              k, 100, None, L, out.data_ptr(), stride,
                                                              sizes.ctypes.data_as(C.POINTER(C.c_uint64)), None)
    assert rc == 2 and (sizes == 77).all()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xCD).all()
    # a decode whose rectangle leaves the frame writes nothing either
    good = a.wide_encode_regions_device(d.data_ptr(), W, H, [(0, 0)] * N, bw, bh, f, k, 100, out.data_ptr(), stride, None, L)
    frames_out = torch.full((N * f * H * W * 3,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(a.CodecError) as e:
        a.wide_decode_regions_device(out.data_ptr(), stride, good, frames_out.data_ptr(), W, H, [(0, 0), (W - bw + 1, H - bh), (0, 0)])
    assert e.value.code == 2
    assert (frames_out.cpu().numpy() == SENTINEL).all()
    # and the version 2 region decode refuses version 3 bytes without writing
    with pytest.raises(a.CodecError):
        a.split_decode_regions_device(out.data_ptr(), stride, good, frames_out.data_ptr(), W, H, [(0, 0)] * N)
    assert (frames_out.cpu().numpy() == SENTINEL).all()


def test_budget_call_with_origins(gpu_codec):
    a = gpu_codec
    W, H, bw, bh, f, origins, k = CASES[1]
    src = _frames(W, H, f, k)
    d = _dev(src)
    stride = _stride(a, bw, bh, f)
    crops = [_crop(src, i, f, x0, y0, bw, bh) for i, (x0, y0) in enumerate(origins)]
    preds = [a.predict_wide_sizes(c, bw, bh, f, k, L) for c in crops]
    budgets = [int(preds[0].lo.min()) - 1, int(preds[1].hi[96]), 10**9]
    out = torch.full((N * stride,), 0xCD, dtype=torch.uint8, device="cuda:0")
    chosen, fits, sizes = a.wide_encode_to_budget_device(d.data_ptr(), bw, bh, f, N, k, budgets, out.data_ptr(), stride, 10, 100, L,
                                                         frame_width=W, frame_height=H, origins=origins)
    got = _blobs(out, stride, sizes)
    print("chosen", list(chosen), "fits", list(fits), "sizes", list(sizes), "budgets", budgets)
    assert list(fits) == [False, True, True] and int(chosen[0]) == 10 and int(chosen[2]) == 100 and int(chosen[1]) >= 96
    for i in range(N):
        one, q, fit = a.encode_wide_to_size(crops[i], bw, bh, f, budgets[i], k, 10, 100, L)   # the host call of the crop agrees
        assert (q, fit) == (int(chosen[i]), bool(fits[i])) and got[i] == one
        assert got[i] == a.encode_wide(a.FrameEncoder.with_wavelet(q, a.WaveletType(k)), crops[i], bw, bh, f, L)
        if fit:
            assert len(got[i]) <= budgets[i]


def _person_frames():
    """a textured box walking over a flat background; chunk 2 stands empty"""
    rng = np.random.default_rng(21)
    W, H, f, n = 96, 64, 4, 4
    bg = np.empty((H, W, 3), np.uint8)
    bg[:] = (40, 90, 160)
    texture = rng.integers(0, 256, (24, 18, 3), dtype=np.uint8)
    texture[(np.abs(texture.astype(np.int16) - bg[0, 0]) < 40).any(axis=2)] = (250, 5, 20)     # every box pixel is foreground
    frames = np.repeat(bg[None], n * f, axis=0)
    for t in range(n * f):
        if t // f == 2:
            continue
        x = 6 + 3 * t
        frames[t, 20:44, x:x + 18] = texture
    return W, H, f, n, bg, frames


def test_person_chunks_in_v3(gpu_codec):
    a = gpu_codec
    W, H, f, n, bg, frames = _person_frames()
    q = 100
    d_frames, d_bg = _dev(frames), _dev(bg)
    v1 = a.encode_person_chunks(d_frames, d_bg, W, H, f, n, q)
    v2 = a.encode_person_chunks(d_frames, d_bg, W, H, f, n, q, format="split", lane_symbols=L)
    got = a.encode_person_chunks(d_frames, d_bg, W, H, f, n, q, format="wide", lane_symbols=L)
    assert [b for b, _ in got] == [b for b, _ in v1] == [b for b, _ in v2]       # the same boxes as the other calls
    enc = a.FrameEncoder(q, a.WaveletType.Cdf53)

    def crop_of(c, bbox):
        bx, by, bw, bh = bbox
        return np.ascontiguousarray(frames[c * f:(c + 1) * f, by:by + bh, bx:bx + bw]).reshape(-1)

    for c, (bbox, alc) in enumerate(got):
        assert a.alc_version(alc) == 3
        if c == 2:
            assert bbox == [0, 0, 0, 0] and alc == a.encode_wide(enc, b"", 0, 0, f, L)
            continue
        assert bbox[2] >= 18 and bbox[3] >= 24
        assert _escapes(crop_of(c, bbox), bbox[2], bbox[3], f, 0) > 0
        assert alc == a.encode_wide(enc, crop_of(c, bbox), bbox[2], bbox[3], f, L), c

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
            dec = a.decode_alc(alc).reshape(f, -1)
            for t in range(f):
                a.paste_bbox_numpy(want[c * f + t], dec[t], [3 * bx, by, 3 * bw, bh])
        return want

    def psnr_inside(pixels):
        pix = pixels.reshape(n * f, H, W, 3)
        inside = [(pix[c * f:(c + 1) * f, b[1]:b[1] + b[3], b[0]:b[0] + b[2]], frames[c * f:(c + 1) * f, b[1]:b[1] + b[3], b[0]:b[0] + b[2]])
                  for c, (b, _) in enumerate(got) if b[2] * b[3]]
        return WO.psnr(np.concatenate([x.reshape(-1) for x, _ in inside]), np.concatenate([y.reshape(-1) for _, y in inside]))

    back = decoded(got)
    assert np.array_equal(back, pasted(got))                  # decode_wide's pixels, pasted; nothing else touched
    p3, p2 = psnr_inside(back), psnr_inside(decoded(v2))
    print(f"PSNR inside the boxes at q = {q}: version 3 {p3:.2f} dB, version 2 {p2:.2f} dB")
    assert p3 > p2 and p3 > 35
    mixed = [v1[0], v2[1], got[2], got[3]]                    # versions 1, 2 and 3 in one list
    assert [a.alc_version(x) for _, x in mixed] == [1, 2, 3, 3]
    assert np.array_equal(decoded(mixed), pasted(mixed))
    mixed = [got[0], v2[1], v1[2], v1[3]]
    assert np.array_equal(decoded(mixed), pasted(mixed))
    # a byte budget per chunk
    box = got[0][0]
    p = a.predict_wide_sizes(crop_of(0, box), box[2], box[3], f, 0, L)
    budget = int(p.hi[95])
    small = a.encode_person_chunks(d_frames, d_bg, W, H, f, n, q, format="wide", lane_symbols=L, max_bytes=budget)
    assert [b for b, _ in small] == [b for b, _ in got]
    for c, (bbox, alc) in enumerate(small):
        if c == 2:
            assert alc == got[2][1]
            continue
        data, qq, fits = a.encode_wide_to_size(crop_of(c, bbox), bbox[2], bbox[3], f, budget, 0, 10, q, L)
        assert alc == data and a.alc_version(alc) == 3
        if fits:
            assert len(alc) <= budget
    assert len(small[0][1]) <= budget
    with pytest.raises(a.CodecError):
        a.encode_person_chunks(d_frames, d_bg, W, H, f, n, q, max_bytes=budget)
