"""A frame range is the rectangle of the whole frame (DESIGN.md sections 14 and 16) on the MI355X: alice_codec_decode_frames
and alice_codec_dev_decode_frames against alice_codec_decode_rect and alice_codec_dev_decode_rect at (0, 0, w, h) and against
the same frames of the library's full decode, byte for byte, and what the frame hook reports against what the rectangle hook
reports.  The frame calls run the rectangle body; this file pins that the fold changes nothing the caller can see.  Versions
2, 3 and 4, the three wavelets, lane length 64: (33, 17, 5) and (5, 3, 7) are odd on every axis (pad column, row and frame),
(50, 38, 13) has blocks that straddle plane and band edges; the first frame, the last one and an interior range."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frames_ref as FR  # noqa: E402
import wide_oracle as WO  # noqa: E402
from test_gpu_frames import DEV, L, QUALITIES, _encode, _full_decode  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(33, 17, 5), (50, 38, 13), (5, 3, 7)]
WAVELETS = (0, 1, 2)


def _ranges(f):
    return [(0, 1), (f - 1, f), (f // 2 - 1, f // 2 + 2)]


def _frame_columns(st):
    """(a, b, blocks, uploaded, frames) of the frame hook"""
    return tuple(st)


def _rect_columns(st):
    """(ta, tb, blocks, uploaded, frames) of the rectangle hook"""
    return (st[0], st[1], st[6], st[7], st[8])


@pytest.mark.parametrize("version", [2, 3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_frame_calls_equal_whole_frame_rectangles(gpu_codec, shape, version):
    a = gpu_codec
    assert L == 64
    w, h, f = shape
    fb = w * h * 3
    rgb = WO.smooth_plus_noise(w, h, f, seed=w * 7 + f)
    d_frames = torch.empty(f * fb, dtype=torch.uint8, device=DEV)
    d_rect = torch.empty(f * fb, dtype=torch.uint8, device=DEV)
    for kind in WAVELETS:
        q = QUALITIES[version][(SHAPES.index(shape) + kind) % len(QUALITIES[version])]
        blob = _encode(a, version, rgb, w, h, f, q, kind)
        full = np.asarray(_full_decode(a, version, blob)).reshape(f, fb)
        raw = np.frombuffer(blob, np.uint8)
        d_alc = torch.from_numpy(raw.copy()).to(DEV)
        for t0, t1 in _ranges(f):
            where = (shape, version, kind, (t0, t1))
            n = (t1 - t0) * fb
            want = full[t0:t1].reshape(-1)
            # the host pair
            host_frames = np.asarray(a.decode_frames(blob, t0, t1 - t0))
            fst = a._test_last_frames_stats()
            host_rect = np.asarray(a.decode_rect(blob, t0, t1 - t0, 0, 0, w, h))
            rst = a._test_last_rect_stats()
            assert np.array_equal(host_frames, host_rect), where
            assert np.array_equal(host_frames, want), where
            assert _frame_columns(fst) == _rect_columns(rst), (where, fst, rst)
            assert fst[:2] == FR.frame_window(kind, f, t0, t1) and fst[3] > 0 and fst[4] == t1 - t0, (where, fst)
            # the device pair
            d_frames.fill_(0x5A)
            d_rect.fill_(0xA5)
            a.frames_decode_device(d_alc.data_ptr(), raw.size, t0, t1 - t0, d_frames.data_ptr())
            fsd = a._test_last_frames_stats()
            a.rect_decode_device(d_alc.data_ptr(), raw.size, t0, t1 - t0, 0, 0, w, h, d_rect.data_ptr())
            rsd = a._test_last_rect_stats()
            torch.cuda.synchronize()
            assert torch.equal(d_frames[:n], d_rect[:n]), where
            assert np.array_equal(d_frames[:n].cpu().numpy(), host_frames), where
            assert bool((d_frames[n:] == 0x5A).all()) and bool((d_rect[n:] == 0xA5).all()), where
            assert _frame_columns(fsd) == _rect_columns(rsd), (where, fsd, rsd)
            assert fsd == fst[:3] + (0,) + fst[4:], (where, fsd, fst)
