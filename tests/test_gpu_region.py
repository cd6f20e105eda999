"""Region encode / decode of device frames (Batch.encode_regions / decode_regions) and the hybrid helpers on the MI355X.
The yardstick is always the oracle: a region's .alc must equal oracle.encode of the numpy crop of the same rectangle, and a
region decode must equal oracle.decode inside the rectangle and leave every other byte of the frames as it was."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segment_ref as R  # noqa: E402

import torch  # noqa: E402

pytestmark = pytest.mark.gpu
WT = {"Cdf53": 0, "Cdf97": 1, "Haar": 2}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _source(seed, n_frames, H, W):
    """smooth-ish frames (so the entropy coder has something to do) with noise; [n, H, W, 3] uint8"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = ((x[None] * 3 + y[None] * 2 + np.arange(n_frames)[:, None, None] * 5) % 256).astype(np.int16)
    rgb = np.stack([base, 255 - base, (base * 7) % 256], axis=3) + rng.integers(-8, 9, (n_frames, H, W, 3))
    return np.clip(rgb, 0, 255).astype(np.uint8)


def _crop(frames, x0, y0, w, h):
    return np.ascontiguousarray(frames[:, y0:y0 + h, x0:x0 + w]).reshape(-1)


def _alcs(bt, sizes):
    packed = torch.empty(int(sizes.sum()), dtype=torch.uint8, device="cuda:0")
    bt.pack_alc(sizes, packed.data_ptr(), packed.numel())
    torch.cuda.synchronize()
    host = packed.cpu().numpy()
    ends = np.cumsum(sizes.astype(np.int64))
    return [host[e - int(s):e].tobytes() for e, s in zip(ends, sizes)]


def _region_case(a, o, W, H, w, h, f, origins, q, wname, seed):
    n = len(origins)
    src = _source(seed, n * f, H, W)
    d = _dev(src)
    bt = a.Batch(w, h, f, n, q, a.WaveletType[wname])
    bt.encode_regions(d.data_ptr(), W, H, origins)
    got = _alcs(bt, bt.encode_finish())
    for i, (x0, y0) in enumerate(origins):
        crop = _crop(src[i * f:(i + 1) * f], x0, y0, w, h)
        assert got[i] == o.encode(crop, w, h, f, q, WT[wname]), (W, H, w, h, f, (x0, y0), wname, i)
    return bt, src, got


# ---- encode parity ----

@pytest.mark.parametrize("x0", [0, 1, 2, 3, 5, 6, 7, 8])
def test_encode_origin_alignment(gpu_codec, oracle_mod, x0):
    """x0 % 4 of 0..3 on a W % 4 == 0 source: only x0 % 4 == 0 takes the dword loads, the rest the byte path"""
    _region_case(gpu_codec, oracle_mod, 200, 120, 150, 90, 6, [(x0, 11)], 90, "Cdf53", 100 + x0)


@pytest.mark.parametrize("wname", ["Cdf53", "Cdf97", "Haar"])
def test_encode_edges_and_wavelets(gpu_codec, oracle_mod, wname):
    """five chunks at different origins, each box touching one frame edge (left, top, right, bottom, all four corners)"""
    W, H, w, h = 260, 150, 131, 77                                     # odd region width and height
    origins = [(0, 40), (60, 0), (W - w, 33), (17, H - h), (W - w, H - h)]
    _region_case(gpu_codec, oracle_mod, W, H, w, h, 5, origins, 80, wname, 7)


def test_encode_unaligned_source_width(gpu_codec, oracle_mod):
    """W % 4 != 0: no origin is dword aligned"""
    _region_case(gpu_codec, oracle_mod, 203, 97, 140, 64, 4, [(0, 0), (4, 9), (63, 33)], 90, "Cdf97", 3)


def test_encode_generic_path(gpu_codec, oracle_mod):
    """regions below the tile kernels' 6 x 6 take the generic path, which reads the rectangle in place too"""
    _region_case(gpu_codec, oracle_mod, 40, 30, 5, 3, 4, [(1, 2), (35, 27), (0, 0)], 90, "Cdf53", 5)
    _region_case(gpu_codec, oracle_mod, 40, 30, 37, 4, 3, [(3, 26)], 90, "Haar", 6)


def test_encode_full_size_region(gpu_codec, oracle_mod):
    """1920x1080 source frames, one 640x720x64 region"""
    _region_case(gpu_codec, oracle_mod, 1920, 1080, 640, 720, 64, [(644, 200)], 90, "Cdf53", 11)


def test_whole_frame_region_equals_batch_encode(gpu_codec, oracle_mod):
    a = gpu_codec
    W, H, f, n = 96, 64, 8, 3
    src = _source(41, n * f, H, W)
    d = _dev(src)
    bt = a.Batch(W, H, f, n, 85, a.WaveletType.Cdf97)
    bt.encode(d.data_ptr())
    whole = _alcs(bt, bt.encode_finish())
    bt2 = a.Batch(W, H, f, n, 85, a.WaveletType.Cdf97)
    bt2.encode_regions(d.data_ptr(), W, H, [(0, 0)] * n)
    assert _alcs(bt2, bt2.encode_finish()) == whole


# ---- decode into a region ----

@pytest.mark.parametrize("W,H,w,h,origins", [
    (200, 120, 150, 90, [(0, 0), (4, 30), (48, 17)]),               # aligned origins, left/top edges
    (200, 120, 151, 89, [(1, 31), (49, 0), (26, 7)]),               # unaligned origins, right/bottom edges
    (203, 97, 140, 64, [(63, 33), (0, 0), (5, 1)]),                 # W % 4 != 0
    (40, 30, 5, 3, [(1, 2), (35, 27), (0, 0)]),                     # generic path
])
def test_decode_into_region_leaves_the_rest(gpu_codec, oracle_mod, W, H, w, h, origins):
    a, o = gpu_codec, oracle_mod
    f, q = 6, 80
    bt, src, alcs = _region_case(a, o, W, H, w, h, f, origins, q, "Cdf97", W + h)
    n = len(origins)
    canary = np.random.default_rng(W * 7 + h).integers(0, 256, (n * f, H, W, 3), dtype=np.uint8)
    out = _dev(canary)
    bt.decode_regions(bt.alc_ptr(0), bt.alc_stride, out.data_ptr(), W, H, origins)
    bt.decode_finish()
    got = out.cpu().numpy()
    want = canary.copy()
    for i, (x0, y0) in enumerate(origins):
        want[i * f:(i + 1) * f, y0:y0 + h, x0:x0 + w] = o.decode(alcs[i]).reshape(f, h, w, 3)
    assert np.array_equal(got, want)
    # rgb_ptr names the first pixel of each rectangle
    for i, (x0, y0) in enumerate(origins):
        assert bt.rgb_ptr(i) == out.data_ptr() + ((i * f * H + y0) * W + x0) * 3


def test_decode_regions_of_packed_alc(gpu_codec, oracle_mod):
    """decode_regions takes any .alc of the batch's shape, e.g. chunks encoded by FrameEncoder and packed by hand"""
    a, o = gpu_codec, oracle_mod
    W, H, w, h, f = 64, 48, 30, 20, 4
    chunks = [_crop(_source(60 + i, f, H, W), 3 * i, i, w, h) for i in range(2)]
    alcs = [o.encode(c, w, h, f, 90, 0) for c in chunks]
    stride = (max(map(len, alcs)) + 255) & ~255
    host = np.zeros((2, stride), np.uint8)
    for i, b in enumerate(alcs):
        host[i, :len(b)] = np.frombuffer(b, np.uint8)
    d_alc = _dev(host)
    out = torch.zeros(2 * f * H * W * 3, dtype=torch.uint8, device="cuda:0")
    bt = a.Batch(w, h, f, 2, 90)
    bt.decode_regions(d_alc.data_ptr(), stride, out.data_ptr(), W, H, [(0, 28), (34, 0)])
    bt.decode_finish()
    got = out.cpu().numpy().reshape(2 * f, H, W, 3)
    for i, (x0, y0) in enumerate([(0, 28), (34, 0)]):
        blk = got[i * f:(i + 1) * f]
        assert np.array_equal(blk[:, y0:y0 + h, x0:x0 + w].reshape(-1), o.decode(alcs[i]).reshape(-1))
        blk[:, y0:y0 + h, x0:x0 + w] = 0
    assert not got.any()


# ---- retry, mixed calls, errors ----

def test_capacity_retry_rereads_the_regions(gpu_codec, oracle_mod):
    """the forced 4352-byte first capacity overflows every chain: encode_finish re-runs the encode, which must read the
    rectangles again (not a contiguous buffer at the frames' base)"""
    a, o = gpu_codec, oracle_mod
    W, H, w, h, f, n = 160, 100, 96, 64, 16, 2
    src = np.random.default_rng(77).integers(0, 256, (n * f, H, W, 3), dtype=np.uint8)
    origins = [(33, 21), (64, 36)]
    refs = [o.encode(_crop(src[i * f:(i + 1) * f], x, y, w, h), w, h, f, 90, 1) for i, (x, y) in enumerate(origins)]
    assert all(len(r) > 3138 + 3 * 4352 for r in refs)
    d = _dev(src)
    lib = a.load_library()
    lib.alice_codec_test_force_first_cap(4352)
    try:
        bt = a.Batch(w, h, f, n, 90, a.WaveletType.Cdf97)
        bt.encode_regions(d.data_ptr(), W, H, origins)
        sizes = bt.encode_finish()
    finally:
        lib.alice_codec_test_force_first_cap(0)
    assert _alcs(bt, sizes) == refs


def test_mixed_region_and_contiguous_calls(gpu_codec, oracle_mod):
    a, o = gpu_codec, oracle_mod
    W, H, w, h, f, n = 120, 80, 70, 50, 4, 2
    big = _source(91, n * f, H, W)
    small = _source(92, n * f, h, w)
    d_big, d_small = _dev(big), _dev(small)
    origins = [(9, 30), (48, 3)]
    want_region = [o.encode(_crop(big[i * f:(i + 1) * f], x, y, w, h), w, h, f, 90, 0) for i, (x, y) in enumerate(origins)]
    want_packed = [o.encode(small[i * f:(i + 1) * f].reshape(-1), w, h, f, 90, 0) for i in range(n)]
    bt = a.Batch(w, h, f, n, 90)
    for _ in range(2):
        bt.encode_regions(d_big.data_ptr(), W, H, origins)
        assert _alcs(bt, bt.encode_finish()) == want_region
        bt.encode(d_small.data_ptr())
        assert _alcs(bt, bt.encode_finish()) == want_packed
    # decode both ways from the same .alc
    out = torch.zeros(n * f * h * w * 3, dtype=torch.uint8, device="cuda:0")
    bt.decode(bt.alc_ptr(0), bt.alc_stride, out.data_ptr())
    bt.decode_finish()
    frames = torch.zeros(n * f * H * W * 3, dtype=torch.uint8, device="cuda:0")
    bt.decode_regions(bt.alc_ptr(0), bt.alc_stride, frames.data_ptr(), W, H, origins)
    bt.decode_finish()
    fr = frames.cpu().numpy().reshape(n * f, H, W, 3)
    flat = out.cpu().numpy().reshape(n, -1)
    for i, (x, y) in enumerate(origins):
        assert np.array_equal(flat[i], o.decode(want_packed[i]).reshape(-1))
        assert np.array_equal(_crop(fr[i * f:(i + 1) * f], x, y, w, h), o.decode(want_packed[i]).reshape(-1))


def test_region_errors(gpu_codec):
    a = gpu_codec
    W, H, w, h, f = 64, 48, 30, 20, 2
    src = _source(5, 2 * f, H, W)
    d = _dev(src)
    bt = a.Batch(w, h, f, 2, 90)
    for bad in ([(0, 0), (W - w + 1, 0)], [(0, H - h + 1), (0, 0)], [(2 ** 32 - 1, 0), (0, 0)]):
        with pytest.raises(a.CodecError) as e:
            bt.encode_regions(d.data_ptr(), W, H, bad)
        assert e.value.kind == "InvalidDimensions"
    with pytest.raises(a.CodecError) as e:
        bt.encode_regions(d.data_ptr(), W, H, [(0, 0)])
    assert e.value.kind == "InvalidBufferSize"
    bt.encode_regions(d.data_ptr(), W, H, [(0, 0), (34, 28)])
    sizes = bt.encode_finish()
    canary = np.random.default_rng(9).integers(0, 256, src.shape, dtype=np.uint8)
    out = _dev(canary)
    with pytest.raises(a.CodecError) as e:
        bt.decode_regions(bt.alc_ptr(0), bt.alc_stride, out.data_ptr(), W, H, [(0, 0), (35, 28)])
    assert e.value.kind == "InvalidDimensions"
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), canary)
    lib = a.load_library()
    o = np.zeros(4, np.uint32)
    op = o.ctypes.data_as(a._u32p)
    assert lib.alice_codec_batch_encode_regions(bt._h, None, W, H, op, None) == 9
    assert lib.alice_codec_batch_encode_regions(bt._h, d.data_ptr(), W, H, None, None) == 9
    assert lib.alice_codec_batch_encode_regions(None, d.data_ptr(), W, H, op, None) == 9
    assert lib.alice_codec_batch_decode_regions(bt._h, None, bt.alc_stride, out.data_ptr(), W, H, op, None) == 9
    assert lib.alice_codec_batch_decode_regions(bt._h, bt.alc_ptr(0), bt.alc_stride, None, W, H, op, None) == 9
    assert lib.alice_codec_batch_decode_regions(None, bt.alc_ptr(0), bt.alc_stride, out.data_ptr(), W, H, op, None) == 9
    # the batch still works after the refused calls
    assert np.array_equal(bt.encode_finish(), sizes)


# ---- the hybrid helpers ----

def test_hybrid_end_to_end(gpu_codec, oracle_mod):
    a, o = gpu_codec, oracle_mod
    rng = np.random.default_rng(21)
    W, H, f, n, q = 160, 96, 4, 4, 90
    bg = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    frames = np.repeat(bg[None], n * f, axis=0)
    for k in range(n * f):                                    # a "person" walking across; chunk 2 stands empty
        if k // f == 2:
            continue
        x = 10 + 7 * k
        frames[k, 30:70, x:x + 25] = [200, 120, 90]
    d_frames, d_bg = _dev(frames), _dev(bg)
    got = a.encode_person_chunks(d_frames, d_bg, W, H, f, n, q)
    # the boxes follow from the segmentation stats of the byte view and person_chunk_boxes
    st = R.vec_motion(frames.reshape(n * f, H, 3 * W), bg.reshape(1, H, 3 * W), 25, 2, 1)[1]
    x0, x1 = st[:, 0] // 3, -(-(st[:, 0] + st[:, 2]) // 3)
    st[:, 0], st[:, 2] = x0, x1 - x0
    assert [b for b, _ in got] == a.person_chunk_boxes(st, W, H, f)
    empty = o.encode(np.zeros(0, np.uint8), 0, 0, f, q, 0)
    for c, (bbox, alc) in enumerate(got):
        if c == 2:
            assert bbox == [0, 0, 0, 0] and alc == empty
            continue
        bx, by, bw, bh = bbox
        assert bw * bh > 0 and bx % 4 == 0
        crop = b"".join(a.crop_to_bbox(frames[k].reshape(-1), W * 3, [bx * 3, by, bw * 3, bh]) for k in range(c * f, (c + 1) * f))
        assert alc == o.encode(np.frombuffer(crop, np.uint8), bw, bh, f, q, 0), c
    # decode onto the background: the numpy paste of the oracle's decode
    out = _dev(np.repeat(bg[None], n * f, axis=0))
    a.decode_person_chunks(got, out, W, H, f)
    want = np.repeat(bg[None], n * f, axis=0)
    for c, (bbox, alc) in enumerate(got):
        if c == 2:
            continue
        bx, by, bw, bh = bbox
        dec = o.decode(alc).reshape(f, -1)
        for k in range(f):
            a.paste_from_bbox(want[c * f + k], W * 3, dec[k], [bx * 3, by, bw * 3, bh])
    assert np.array_equal(out.cpu().numpy(), want)


def test_hybrid_chroma_switch(gpu_codec, oracle_mod):
    a, o = gpu_codec, oracle_mod
    W, H, f, n = 64, 48, 2, 2
    frames = np.zeros((n * f, H, W, 3), np.uint8)
    frames[..., 1] = 255                                       # a green screen
    frames[:f, 10:30, 8:20] = [180, 90, 60]
    frames[f:, 20:40, 30:50] = [180, 90, 60]
    got = a.encode_person_chunks(_dev(frames), None, W, H, f, n, 90, green_threshold=30)
    st = R.vec_chroma(R.vec_cg_of_rgb(frames), 30)[1]
    assert [b for b, _ in got] == a.person_chunk_boxes(st, W, H, f)
    for c, (bbox, alc) in enumerate(got):
        bx, by, bw, bh = bbox
        assert bw * bh > 0
        assert alc == o.encode(_crop(frames[c * f:(c + 1) * f], bx, by, bw, bh), bw, bh, f, 90, 0), c
