"""Every mirrored instance of the inverse transform (.alc version 4, DESIGN.md section 12.3: six inv_t_wide_kernel, eight
inv_xy_kernel, two axis_lift_kernel) at the magnitudes its class is about.  The plan -- volumes with |q| = 2175 in every
sample, the first and last quantiser step of every class, five shapes (interior tile, pad row and column, a single frame,
the generic path, one tile row per band) -- and the numpy references are tests/reversible_extreme_cases.py's;
tests/test_reversible_extremes_host.py shows without a device that the plan reaches what it claims and that every class has
a case on which the mirrored and the reference inverse differ.  Every comparison is bit-exact."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reversible_extreme_cases as P  # noqa: E402
import reversible_ref as RR  # noqa: E402
import wide_oracle as WO  # noqa: E402
import wide_ref as R3  # noqa: E402

import torch  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 256
SENTINEL = 0xA5
_ran = {k: set() for k in P.KINDS}      # classes the mirrored tile kernels ran in this process


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class band_target:
    """alice_codec_test_set_tuning for the shapes that ask for it, restored on the way out"""

    def __init__(self, lib, kb):
        self.lib, self.kb = lib, kb

    def __enter__(self):
        if self.kb is not None:
            self.lib.alice_codec_test_set_tuning(self.kb)

    def __exit__(self, *exc):
        if self.kb is not None:
            self.lib.alice_codec_test_set_tuning(1024 * 1024)


# ---- a. every class edge, version 4 ----
@pytest.mark.parametrize("shape", list(P.SHAPES))
@pytest.mark.parametrize("kind", P.KINDS)
def test_version_4_containers_at_every_class_edge(gpu_codec, kind, shape):
    a = gpu_codec
    lib = a.load_library()
    told_apart = set()
    with band_target(lib, P.SHAPES[shape][0]):
        for name, steps, v in P.cases(lib, kind, shape):
            assert P.variant(lib, kind, steps) == v, (kind, steps)
            blob = P.container(kind, shape, name, steps, 4)
            want = P.reference(kind, shape, name, steps)
            got = a.decode_reversible(blob)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (kind, shape, steps, v, name, bad.size, bad[:4].tolist())
            assert np.array_equal(a.decode_alc(blob), want), (kind, shape, steps, v, name)
            if P.differing_pixels(kind, shape, name, steps):       # the mirrored instance ran, not its twin
                assert not np.array_equal(got, P.reference(kind, shape, name, steps, mirrored=False))
                told_apart.add(v)
            if P.tile_eligible(shape):
                _ran[kind].add(v)
    assert told_apart == P.EXPECTED_CLASSES[kind], (kind, shape, told_apart)


# ---- b. the version 3 twin on the shapes the wide extremes never used ----
@pytest.mark.parametrize("shape", [(256, 250, 6), (104, 40, 1), (3, 40, 4)])
@pytest.mark.parametrize("kind", P.KINDS)
def test_version_3_twin_on_the_banded_single_frame_and_generic_shapes(gpu_codec, kind, shape):
    a = gpu_codec
    lib = a.load_library()
    with band_target(lib, P.SHAPES[shape][0]):
        for name, steps, v in P.cases(lib, kind, shape):
            blob = P.container(kind, shape, name, steps, 3)
            want = P.reference(kind, shape, name, steps, mirrored=False)
            got = a.decode_wide(blob)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (kind, shape, steps, v, name, bad.size, bad[:4].tolist())


# ---- d. the device and region paths at saturation ----
@pytest.mark.parametrize("kind", P.KINDS)
def test_device_and_region_decodes_of_the_loud_volume(gpu_codec, kind):
    """The 200x70x4 loud container at the last step of the last fast class: reversible_decode_device inside guard bytes, and
    reversible_decode_regions_device into 212x76 frames at x0 % 4 != 0 and == 0 -- the saturated pixels through the unaligned
    store path, nothing outside the rectangles written."""
    a = gpu_codec
    lib = a.load_library()
    shape = P.DEVICE_SHAPE
    w, h, f = shape
    v, _, top = P.classes(lib, kind)[-2]
    steps = (top, top, top)
    name = f"loud{P.SHAPES[shape][2][0]}"
    assert (name, steps, v) in P.cases(lib, kind, shape)
    blob = P.container(kind, shape, name, steps, 4)
    want = P.reference(kind, shape, name, steps)
    assert P.differing_pixels(kind, shape, name, steps) > 0
    assert int(want.min()) == 0 and int(want.max()) == 255          # pixels at both ends of the u8 range
    stride = (len(blob) + 255) & ~255
    origins = [(5, 3), (8, 4)]
    n = len(origins)
    alc = np.zeros(n * stride, np.uint8)
    for i in range(n):
        alc[i * stride:i * stride + len(blob)] = np.frombuffer(blob, np.uint8)
    d_alc = _dev(alc)
    sizes = [len(blob)] * n
    # packed output
    n_out = w * h * f * 3
    d_rgb = torch.full((GUARD + n * n_out + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    a.reversible_decode_device(d_alc.data_ptr(), stride, sizes, d_rgb.data_ptr() + GUARD)
    torch.cuda.synchronize()
    host = d_rgb.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[-GUARD:] == SENTINEL).all(), "guard bytes were written"
    for i in range(n):
        assert np.array_equal(host[GUARD + i * n_out:GUARD + (i + 1) * n_out], want), (kind, i)
    # regions of larger frames
    W, H = 212, 76
    d_frames = torch.full((GUARD + n * f * H * W * 3 + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    a.reversible_decode_regions_device(d_alc.data_ptr(), stride, sizes, d_frames.data_ptr() + GUARD, W, H, origins)
    torch.cuda.synchronize()
    got = d_frames.cpu().numpy()
    assert (got[:GUARD] == SENTINEL).all() and (got[-GUARD:] == SENTINEL).all(), "guard bytes were written"
    expect = np.full((n * f, H, W, 3), SENTINEL, np.uint8)
    for i, (x0, y0) in enumerate(origins):
        expect[i * f:(i + 1) * f, y0:y0 + h, x0:x0 + w] = want.reshape(f, h, w, 3)
    assert np.array_equal(got[GUARD:-GUARD].reshape(expect.shape), expect)      # exact inside the boxes, untouched outside
    assert np.array_equal(d_alc.cpu().numpy(), alc)


# ---- e. lossless at the top of the forward range ----
@pytest.mark.parametrize("pair", list(P.PAIRS))
@pytest.mark.parametrize("kind", P.KINDS)
def test_lossless_at_the_top_of_the_forward_range(gpu_codec, kind, pair):
    """Co (Cg) = +-255 with the signs that drive the forward transform highest: |coefficient| 2040 (1177 for CDF 9/7), at
    quality 100 z = 4079 / 4080, a residual of 3825 of the format's 4095 -- and the input comes back."""
    a = gpu_codec
    w, h, f = P.DEVICE_SHAPE
    rgb = P.top_of_range_content(kind, pair)
    step, _, qs = WO.forward_quantised(RR.o, rgb, w, h, f, 100, kind)
    ch = P.PAIRS[pair][2]
    top = int(np.abs(qs[ch]).max())
    assert step == 1 and top == P.FORWARD_TOP[kind]
    blob = a.encode_lossless(rgb, w, h, f, a.WaveletType(kind), P.LANE_SYMBOLS)
    assert blob == RR.encode(rgb, w, h, f, 100, kind, P.LANE_SYMBOLS), (kind, pair)
    assert int(R3.wide_symbols(qs[ch]).max()) in (2 * top - 1, 2 * top)      # the symbols those bytes hold
    assert np.array_equal(a.decode_reversible(blob), rgb), (kind, pair)
    assert np.array_equal(a.decode_alc(blob), rgb)


# ---- c. after the module: every mirrored instance class ran ----
def test_every_mirrored_class_is_covered(gpu_codec):
    """The plan covers every class of every wavelet; and what ran in this process (when the tests above ran) is the plan."""
    lib = gpu_codec.load_library()
    for kind in P.KINDS:
        assert {v for _, v in P.step_cases(lib, kind)} == P.EXPECTED_CLASSES[kind]
        if _ran[kind]:
            assert _ran[kind] == P.EXPECTED_CLASSES[kind], (kind, _ran[kind])
        print(f"{P.NAMES[kind]}: the plan covers classes {sorted(P.EXPECTED_CLASSES[kind])}, ran {sorted(_ran[kind])}")
