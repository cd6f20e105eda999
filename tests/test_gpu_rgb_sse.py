"""The squared-error kernel alone (csrc/quality.hip through alice_codec_dev_rgb_sse) against numpy in int64, over the case
table of tests/quality_cases.py.  Both buffers sit inside guard bytes that hold 0 on side a and 255 on side b, between the
rows and frames of a pitched side too, so a byte read outside the pixels changes the sum by up to 255^2."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quality_cases as QC  # noqa: E402

import torch  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = QC.cases()


def run_case(codec, c, seed=0):
    lib = codec.load_library()
    a, b, ref = c.build(seed)
    d_a = torch.from_numpy(a).to(DEV)
    d_b = torch.from_numpy(b).to(DEV)
    assert d_a.data_ptr() % 256 == 0 and d_b.data_ptr() % 256 == 0
    d_out = torch.full((c.n + 2,), 0x5A5A5A5A, dtype=torch.int64, device=DEV)
    try:
        if c.cap:
            lib.alice_codec_test_set_grid_cap(c.cap)
        codec.rgb_sse_device(d_a.data_ptr() + QC.GUARD + c.off[0], d_b.data_ptr() + QC.GUARD + c.off[1], c.w, c.h, c.n,
                             a_pitches=(c.row_pitch(0), c.frame_pitch(0)), b_pitches=(c.row_pitch(1), c.frame_pitch(1)),
                             d_frame_sse_ptr=d_out.data_ptr() + 8)
    finally:
        lib.alice_codec_test_set_grid_cap(0)
    out = d_out.cpu().numpy()
    assert out[0] == 0x5A5A5A5A and out[-1] == 0x5A5A5A5A                       # exactly n results are written
    got = out[1:-1].view(np.uint64)
    assert np.array_equal(got, ref), (c.name, got[:4], ref[:4], int(np.flatnonzero(got != ref)[0]))
    assert torch.equal(d_a.cpu(), torch.from_numpy(a)) and torch.equal(d_b.cpu(), torch.from_numpy(b))   # the inputs are only read


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_equals_numpy(gpu_codec, case):
    run_case(gpu_codec, case)


def test_result_does_not_depend_on_the_grid(gpu_codec):
    c = next(x for x in CASES if x.name == "multi-vb-rows")
    for cap in (1, 2, 3, 5, 64, 0):
        c2 = QC.Case(f"{c.name}-cap{cap}", c.w, c.h, c.n, c.off, c.row_pad, c.frame_pad, c.content, cap)
        run_case(gpu_codec, c2, seed=3)


def test_returned_array_and_identical_volumes(gpu_codec):
    w, h, n = 19, 7, 4
    rgb = np.random.default_rng(8).integers(0, 256, n * h * w * 3, dtype=np.uint8)
    d = torch.from_numpy(rgb).to(DEV)
    got = gpu_codec.rgb_sse_device(d.data_ptr(), d.data_ptr(), w, h, n)
    assert got.dtype == np.uint64 and list(got) == [0] * n
    other = rgb.copy()
    other[5] ^= 0x80
    d2 = torch.from_numpy(other).to(DEV)
    assert list(gpu_codec.rgb_sse_device(d.data_ptr(), d2.data_ptr(), w, h, n)) == [128 * 128, 0, 0, 0]
