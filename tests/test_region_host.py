"""The host side of region coding, without a GPU: the hybrid helper's box policy (person_chunk_boxes) against a brute-force
restatement on random stats, and argument validation of the region calls and hybrid helpers, which must refuse bad input
before any device work."""
import numpy as np
import pytest


def _unions(st, f):
    out = []
    for c in range(len(st) // f):
        s = st[c * f:(c + 1) * f]
        s = s[s[:, 4] > 0]
        out.append(None if not len(s) else (s[:, 0].min(), s[:, 1].min(), (s[:, 0] + s[:, 2]).max(), (s[:, 1] + s[:, 3]).max()))
    return out


def _brute_force(st, W, H, f):
    """the smallest common width (a multiple of 4 where W % 4 == 0) for which every chunk has an admissible x, the largest
    union height; boxes: the largest admissible x / y not past the union's left / top edge"""
    us = _unions(st, f)
    fg = [u for u in us if u is not None]
    if not fg:
        return [[0, 0, 0, 0]] * len(us)
    align = W % 4 == 0
    ch = max(u[3] - u[1] for u in fg)

    def xs(u, cw):
        return [x for x in range(0, W - cw + 1) if x <= u[0] and x + cw >= u[2] and (not align or x % 4 == 0)]

    cw = next(c for c in range(1, W + 1) if (not align or c % 4 == 0 or c == W) and all(xs(u, c) for u in fg))
    return [[0, 0, 0, 0] if u is None else [max(xs(u, cw)), min(u[1], H - ch), cw, ch] for u in us]


def _random_stats(rng, W, H, f, n):
    st = np.zeros((n * f, 5), np.int64)
    for k in range(n * f):
        if rng.random() < 0.25:
            continue                                           # a frame without foreground
        x0, y0 = rng.integers(0, W), rng.integers(0, H)
        st[k] = [x0, y0, rng.integers(1, W - x0 + 1), rng.integers(1, H - y0 + 1), rng.integers(1, 1000)]
    for c in range(n):                                         # and some chunks without any
        if rng.random() < 0.15:
            st[c * f:(c + 1) * f] = 0
    return st


def test_person_chunk_boxes_random(codec):
    rng = np.random.default_rng(2024)
    for trial in range(400):
        W = int(rng.choice([int(rng.integers(1, 80)), 4 * int(rng.integers(1, 20))]))
        H, f, n = int(rng.integers(1, 50)), int(rng.integers(1, 5)), int(rng.integers(1, 6))
        st = _random_stats(rng, W, H, f, n)
        got = codec.person_chunk_boxes(st, W, H, f)
        assert got == _brute_force(st, W, H, f), (trial, W, H, f, n)
        sizes = {tuple(b[2:]) for b in got if b[2] * b[3]}
        assert len(sizes) <= 1
        for b, u in zip(got, _unions(st, f)):
            if u is None:
                assert b == [0, 0, 0, 0]
                continue
            x, y, w, h = b
            assert 0 <= x and x + w <= W and 0 <= y and y + h <= H
            assert x <= u[0] and y <= u[1] and x + w >= u[2] and y + h >= u[3]
            if W % 4 == 0:
                assert x % 4 == 0
            # the width never needs more than 6 pixels beyond the widest union box
            assert w <= max(uu[2] - uu[0] for uu in _unions(st, f) if uu is not None) + 6


def test_person_chunk_boxes_cases(codec):
    st = np.array([[1, 2, 3, 4, 5], [10, 2, 5, 4, 1]])
    assert codec.person_chunk_boxes(st, 16, 8, 1) == [[0, 2, 8, 4], [8, 2, 8, 4]]
    assert codec.person_chunk_boxes(st, 15, 8, 1) == [[1, 2, 5, 4], [10, 2, 5, 4]]
    assert codec.person_chunk_boxes(np.zeros((4, 5)), 16, 8, 2) == [[0, 0, 0, 0], [0, 0, 0, 0]]
    with pytest.raises(codec.CodecError):
        codec.person_chunk_boxes(np.zeros((3, 5)), 16, 8, 2)     # not a whole number of chunks
    with pytest.raises(codec.CodecError):
        codec.person_chunk_boxes(np.array([[10, 0, 7, 1, 1]]), 16, 8, 1)   # box past the frame
    with pytest.raises(codec.CodecError):
        codec.person_chunk_boxes(np.zeros((1, 5)), 0, 8, 1)


def test_hybrid_argument_validation(codec):
    """every one of these raises before a device is touched (this machine may have none)"""
    bad_encode = [
        dict(width=0), dict(height=0), dict(frames=0), dict(n_chunks=0), dict(quality=256), dict(width=2 ** 32),
        dict(d_background=None),
    ]
    for kw in bad_encode:
        args = dict(d_frames=1 << 20, d_background=1 << 20, width=64, height=48, frames=2, n_chunks=2, quality=90)
        args.update(kw)
        with pytest.raises(codec.CodecError):
            codec.encode_person_chunks(**args)
    empty = codec.FrameEncoder(90).encode(b"", 0, 0, 2).to_bytes()
    with pytest.raises(codec.CodecError):                          # box past the frame
        codec.decode_person_chunks([([60, 0, 8, 8], b"")], 1 << 20, 64, 48, 2)
    with pytest.raises(codec.CodecError):                          # .alc of another shape than the box
        codec.decode_person_chunks([([0, 0, 8, 8], empty)], 1 << 20, 64, 48, 2)
    with pytest.raises(codec.CodecError):
        codec.decode_person_chunks([([0, 0, 8, 8], b"not an alc")], 1 << 20, 64, 48, 2)
    with pytest.raises(codec.CodecError):
        codec.decode_person_chunks([], 1 << 20, 64, 0, 2)
    # only empty chunks: nothing to do, no device needed
    assert codec.decode_person_chunks([([0, 0, 0, 0], empty)] * 3, 1 << 20, 64, 48, 2) is None


def test_region_abi_null_arguments(codec):
    lib = codec.load_library()
    o = np.zeros(2, np.uint32)
    op = o.ctypes.data_as(codec._u32p)
    assert lib.alice_codec_batch_encode_regions(None, 1 << 20, 64, 48, op, None) == 9
    assert lib.alice_codec_batch_decode_regions(None, 1 << 20, 4096, 1 << 20, 64, 48, op, None) == 9
    assert lib.alice_codec_batch_decode_regions(None, None, 4096, 1 << 20, 64, 48, op, None) == 9
