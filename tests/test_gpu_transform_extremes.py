"""Every instance of the inverse transform (exact, fast i32, i16 band slot, packed i16 tile) at the magnitudes its proof
is about, and the wide forward at the top of the 8-bit range.  The symbol volumes are the worst-sign volumes and the
loud-random volumes of tests/transform_extremes.py; the quantiser steps are the first and last of each class, read from
alice_codec_test_inverse_variant; every comparison with the CPU oracle is bit-exact.  tests/test_inverse_bounds_host.py
pins the class table and shows that these volumes reach what they claim."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_ref as R2  # noqa: E402
import transform_extremes as X  # noqa: E402
from transform_extremes import EXPECTED_VARIANTS, byte_step_cases, classes, edge_steps, variant  # noqa: E402
import wide_oracle as WO  # noqa: E402
import wide_ref as R3  # noqa: E402
from slab_oracle_stages import OracleStages  # noqa: E402

import torch  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
CDF53, CDF97, HAAR = 0, 1, 2
KINDS = (CDF53, CDF97, HAAR)
_ran = {(k, wide): set() for k in KINDS for wide in (0, 1)}      # variants the tile kernels ran in this process


# (w, h, f) -> band target in KiB (None: the default) and the centres (t, y, x) of the two worst volumes.  Inverse tiles
# are 96 x 32: tile (1, 1) is interior from w >= 196, h >= 68 on.
SHAPES = {
    (200, 70, 4): (None, {"border": (1, 3, 5), "interior": (1, 47, 143)}),
    (199, 69, 3): (None, {"border": (1, 67, 197), "interior": (1, 49, 141)}),       # border: the tile with the pad row and column
    (104, 40, 1): (None, {"border": (1, 3, 5), "seam": (1, 31, 95)}),               # pf = 2; no interior tile: the tile seam
    (3, 40, 4): (None, {"border": (1, 3, 1), "middle": (1, 21, 3)}),                # generic path: parity only
    (256, 250, 6): (96, {"border": (1, 3, 5), "halo": (3, 63, 143)}),               # one tile row per band: row 63 reads band 2's rows
}
_volumes = {}


def byte_volumes(kind, shape):
    """{pattern: (3, pf, ph, pw) u8 symbols}, built once per (wavelet, shape) and never written"""
    if (kind, shape) not in _volumes:
        w, h, f = shape
        pw, ph, pf = R2.padded_dims(w, h, f)
        vols = {}
        for name, centre in SHAPES[shape][1].items():
            s = X.worst_volume(kind, (pf, ph, pw), centre)
            vols[name] = np.stack([X.byte_symbols(s), X.byte_symbols(-s), X.byte_symbols(s)])
        vols["loud"] = np.stack([X.loud_random_bytes((pf, ph, pw), 100 * kind + c) for c in range(3)])
        for v in vols.values():
            v.setflags(write=False)
        _volumes[(kind, shape)] = vols
    return _volumes[(kind, shape)]


def gpu_inverse(codec, sym, w, h, f, kind, steps, align):
    """alice_codec_dev_inverse_symbols into a guarded buffer, `align` bytes off a dword"""
    lib = codec.load_library()
    n = w * h * f * 3
    d_sym = torch.from_numpy(np.array(sym)).to(DEV)
    d_rgb = torch.full((GUARD + align + n + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    rc = lib.alice_codec_dev_inverse_symbols(d_sym.data_ptr(), w, h, f, kind, (C.c_int32 * 3)(*[int(s) for s in steps]),
                                             d_rgb.data_ptr() + GUARD + align, None)
    torch.cuda.synchronize()
    assert rc == 0, lib.alice_codec_last_error_message()
    host = d_rgb.cpu().numpy()
    lo = GUARD + align
    assert (host[:lo] == 0xA5).all() and (host[lo + n:] == 0xA5).all(), "bytes beside the pixels were written"
    assert np.array_equal(d_sym.cpu().numpy(), sym), "the symbols were modified"
    return host[lo:lo + n]


def oracle_inverse(sym, w, h, f, kind, steps):
    return OracleStages().inverse_symbols(torch.from_numpy(np.array(sym)), w, h, f, kind, list(steps)).numpy().reshape(-1)


# ---- a. u8 symbols through the inverse_chunk of the version 1 and 2 decodes ----
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("kind", KINDS)
def test_byte_symbols_at_every_class_edge(gpu_codec, oracle_mod, kind, shape):
    lib = gpu_codec.load_library()
    w, h, f = shape
    band_kb, _ = SHAPES[shape]
    tiles = min(R2.padded_dims(w, h, f)[:2]) >= 6
    try:
        if band_kb is not None:
            lib.alice_codec_test_set_tuning(band_kb)
        for steps, v in byte_step_cases(lib, kind):
            for i, (name, sym) in enumerate(byte_volumes(kind, shape).items()):
                assert variant(lib, kind, steps) == v, (kind, steps)
                got = gpu_inverse(gpu_codec, sym, w, h, f, kind, steps, align=i)
                want = oracle_inverse(sym, w, h, f, kind, steps)
                bad = np.flatnonzero(got != want)
                assert bad.size == 0, (kind, shape, steps, v, name, bad.size, bad[:4].tolist())
                if tiles:
                    _ran[(kind, 0)].add(v)
    finally:
        if band_kb is not None:
            lib.alice_codec_test_set_tuning(1024 * 1024)


# ---- b. the same volumes as containers ----
CONTAINER_SHAPE = (200, 70, 4)


@pytest.mark.parametrize("kind", KINDS)
def test_version_2_containers_of_extreme_symbols(gpu_codec, oracle_mod, kind):
    lib = gpu_codec.load_library()
    w, h, f = CONTAINER_SHAPE
    vols = byte_volumes(kind, CONTAINER_SHAPE)
    seen = set()
    for v, first, last in classes(lib, kind, 0):
        s = last if v else first        # the last step of each fast class, the first of the exact one
        for name in ("interior", "loud"):
            sym = vols[name]
            steps = (s, s, s) if name == "interior" else (s, 1, max(s // 2, 1))
            blob = R2.write_container(kind, w, h, f, 64, steps, sym.reshape(3, -1))
            got = gpu_codec.decode_split(blob)
            assert np.array_equal(got, oracle_inverse(sym, w, h, f, kind, steps)), (kind, steps, name)
            assert np.array_equal(gpu_codec.decode_alc(blob), got)
            assert variant(lib, kind, steps) == v
            _ran[(kind, 0)].add(v)
        seen.add(v)
    assert seen == EXPECTED_VARIANTS[kind]


_wide_volumes = {}


def wide_volumes(kind, shape):
    if (kind, shape) not in _wide_volumes:
        w, h, f = shape
        pw, ph, pf = R3.padded_dims(w, h, f)
        s = X.worst_volume(kind, (pf, ph, pw), SHAPES[CONTAINER_SHAPE][1]["interior"])
        vols = {"interior": [X.wide_symbols_extreme(s), X.wide_symbols_extreme(-s), X.wide_symbols_extreme(s)],
                "loud": [X.loud_random_wide((pf, ph, pw), 200 + 10 * kind + c) for c in range(3)]}
        _wide_volumes[(kind, shape)] = {k: [z.reshape(-1) for z in v] for k, v in vols.items()}
    return _wide_volumes[(kind, shape)]


@pytest.mark.parametrize("shape", [(200, 70, 4), (199, 69, 3)])
@pytest.mark.parametrize("kind", KINDS)
def test_version_3_containers_of_extreme_symbols(gpu_codec, oracle_mod, kind, shape):
    """z = 4349 / 4350 (q = +-2175) in every sample: each coded symbol is an escape with a residual of 4094 / 4095."""
    lib = gpu_codec.load_library()
    w, h, f = shape
    dims = R3.padded_dims(w, h, f)
    vols = wide_volumes(kind, shape)
    payloads = {}
    cases = edge_steps(lib, kind, 1)
    assert [s[0] for s, _ in cases] == {CDF53: [1, 2, 3, 6, 7, 19, 20], CDF97: [1, 2, 3], HAAR: [1, 2, 3, 6, 7, 12, 13]}[kind]
    for edge, v in cases:
        for name, z in vols.items():
            steps = (edge[0], 1, edge[0]) if name == "loud" else edge
            assert variant(lib, kind, steps, 1) == v
            if name not in payloads:       # the payloads do not depend on the steps: code them once, patch the headers
                payloads[name] = bytearray(R3.write_container(kind, w, h, f, 64, steps, z))
            blob = payloads[name]
            for c in range(3):
                o = R3.FIXED + c * R3.CHANNEL
                blob[o:o + 8] = int(steps[c]).to_bytes(4, "little", signed=True) * 2
            assert R3.parse_container(bytes(blob))["step"] == list(steps)
            want = X.inverse_quantised_steps([R3.from_wide_symbols(zz) for zz in z], steps, dims, w, h, f, kind)
            got = gpu_codec.decode_wide(bytes(blob))
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (kind, shape, steps, v, name, bad.size, bad[:4].tolist())
            assert np.array_equal(gpu_codec.decode_alc(bytes(blob)), want)
            _ran[(kind, 1)].add(v)


# ---- c. the wide forward at the top of the 8-bit range ----
PAIRS = {"red/blue": ((255, 0, 0), (0, 0, 255), 1), "green/magenta": ((0, 255, 0), (255, 0, 255), 2)}   # -> the channel at +-255


@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("kind", KINDS)
def test_wide_forward_at_the_top_of_the_range(gpu_codec, oracle_mod, kind, pair):
    """Co (Cg) = +-255 with the signs that drive the forward transform highest: |coefficient| 2040 (1177 for CDF 9/7), 8
    below the value table's radius; at quality 100 z = 4079 / 4080, a residual of 3825 of the format's 4095."""
    from test_gpu_wide import forward_symbols_wide
    import oracle.alice_oracle_np as o
    w, h, f = 200, 70, 4
    plus, minus, ch = PAIRS[pair]
    signs = X.worst_volume(kind, (f, h, w), (1, 47, 143), inverse=False)
    rgb = np.where(signs[..., None] > 0, np.array(plus, np.uint8), np.array(minus, np.uint8)).astype(np.uint8).reshape(-1)
    step, dims, qs = WO.forward_quantised(o, rgb, w, h, f, 100, kind)
    assert step == 1
    top = int(np.abs(qs[ch]).max())
    assert top == (1177 if kind == CDF97 else 2040)
    z = [R3.wide_symbols(q) for q in qs]
    assert int(z[ch].max()) in (2 * top - 1, 2 * top)      # 4079 / 4080: an escape with a residual of 3824 / 3825
    got_z, got_hist = forward_symbols_wide(gpu_codec, rgb, w, h, f, kind, 100)
    for c in range(3):
        assert np.array_equal(got_z[c], z[c]), (kind, pair, c)
        assert np.array_equal(got_hist[c], R3.histogram(z[c])), (kind, pair, c)
    enc = gpu_codec.FrameEncoder.with_wavelet(100, gpu_codec.WaveletType(kind))
    blob = gpu_codec.encode_wide(enc, rgb, w, h, f, 64)
    assert blob == R3.write_container(kind, w, h, f, 64, [1] * 3, z), (kind, pair)
    want = WO.inverse_quantised(o, [R3.from_wide_symbols(zz) for zz in z], 1, dims, w, h, f, kind)
    assert np.array_equal(gpu_codec.decode_wide(blob), want), (kind, pair)
    assert WO.psnr(want, rgb) > 45        # step 1: the pixels come back but for the ties of the lifting's rounding


# ---- after the module: every instance ran ----
def test_every_variant_is_covered(gpu_codec):
    """The plan covers every class of every wavelet; and what ran in this process (when the tests above ran) is the plan."""
    lib = gpu_codec.load_library()
    wide_expected = {CDF53: {0, 1, 2, 3}, CDF97: {0, 2}, HAAR: {0, 1, 2, 3}}
    for kind in KINDS:
        assert {v for _, v in byte_step_cases(lib, kind)} == EXPECTED_VARIANTS[kind]
        assert {v for _, v in edge_steps(lib, kind, 1)} == wide_expected[kind]
        if _ran[(kind, 0)]:
            assert _ran[(kind, 0)] == EXPECTED_VARIANTS[kind], (kind, _ran[(kind, 0)])
        if _ran[(kind, 1)]:
            assert _ran[(kind, 1)] == wide_expected[kind], (kind, _ran[(kind, 1)])
