"""The launch geometry of the generic stage kernels (csrc/generic.hip, and coef_hist_kernel of csrc/rate.hip) on the MI355X.
Every one of them is a grid-stride loop under a host-side cap on the grid; the sizes here make each loop take one trip,
exactly one, exactly two, and two-and-a-bit (tests/generic_cases.py holds the tables, tests/test_generic_cases_host.py holds
them to the caps).  The cap of grid_for() -- 262 140 workgroups, 67 million items a trip -- is lowered by the test hook
alice_codec_test_set_grid_cap to 1 and to 3 workgroups; the caps of 2048 and 1024 workgroups and of 65 536 rows are crossed
at their real values.  Every comparison is exact, against the oracle (tests/wide_ref.py for the wide symbol map): these
kernels are bit-exact by design, and results must not depend on the cap.

With the hook compiled in and downsample2_kernel / ssim_blocks_kernel as they were before they got their loops (one item
per thread, `return` past the end), test_ssim_and_ms_ssim fails at the 8 of its 10 images whose capped launches need a
second trip (run once on the MI355X); the two whose capped launches are exactly one trip pass, as does every uncapped call."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import generic_cases as G  # noqa: E402
import rate_ref as RR  # noqa: E402
import split_rate_ref as SR  # noqa: E402
import split_ref as R2  # noqa: E402
from slab_oracle_stages import OracleStages  # noqa: E402
import wide_oracle as WO  # noqa: E402
import wide_rate_ref as WR  # noqa: E402
import wide_ref as R3  # noqa: E402

import torch  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


@pytest.fixture
def grid_cap(gpu_codec):
    lib = gpu_codec.load_library()
    yield lambda max_blocks: lib.alice_codec_test_set_grid_cap(max_blocks)
    lib.alice_codec_test_set_grid_cap(0)


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True)).to(DEV)     # a copy: the shared references are read-only


# ---------------------------------------------------------------------------------------------------------------------
# under the hook: element-wise kernels
# ---------------------------------------------------------------------------------------------------------------------

def _coeffs(n, seed, spread=5000):
    """random i32 with the values that matter at BOTH ends: the last trip is the one a wrong loop loses"""
    v = np.random.default_rng(seed).integers(-spread, spread + 1, n).astype(np.int32)
    special = np.array([0, I32_MAX, I32_MIN, -1, 1, 7, -7, 8, -8, 20, -21, 127, -128, 128, 32767, -32768, 32768], np.int32)
    k = min(len(special), n // 2)
    if k:
        v[:k] = special[:k]
        v[n - k:] = special[:k][::-1]
    return v


def _wide_z(c):
    """DESIGN.md section 11.2 with the clamp of the generic path: the untruncated zigzag, 65535 where it does not fit"""
    c = np.asarray(c, np.int64)
    return np.minimum(np.where(c > 0, 2 * c - 1, -2 * c), 65535).astype(np.uint16)


def _wide_call(codec, c):
    n = c.size
    out = np.zeros(1024 + 6 * n, np.uint8)
    rc = codec.load_library().alice_codec_test_wide_symbols(c.ctypes.data_as(C.POINTER(C.c_int32)), n,
                                                            out.ctypes.data_as(C.POINTER(C.c_uint8)))
    assert rc == 0
    return out[:1024].view(np.uint32), out[1024:1024 + 4 * n].view(np.int32), out[1024 + 4 * n:].view(np.uint16)


def _elementwise(codec, o, name, n):
    """-> list of (what, got, want) of one kernel at n items; the reference is computed here, once per call"""
    rng = np.random.default_rng(n)
    v = _coeffs(n, n)
    if name == "quantize":
        # true division, the negation of step -1, dead zones below / at / above the step, no dead zone
        return [((s, dz), codec.Quantizer.with_dead_zone(s, dz).quantize_buffer(v), o.quantize_buffer(s, v, dz))
                for s, dz in ((8, 8), (14, 21), (1, 1), (3, 0), (-5, 4), (-1, 0), (-1, 7), (I32_MAX, 1))]
    if name == "fast_quantize":
        out = []
        for s, dz in ((8, None), (14, 21), (1, 1), (3, 0), (64, 64), (I32_MAX, 5)):
            want = o.fast_quantize_buffer(o.fast_quantizer(s, dz), v)
            out.append(((s, dz), codec.FastQuantizer(s, dz).quantize_buffer(v), want))
        return out
    if name == "dequantize":
        return [(s, codec.Quantizer(s).dequantize_buffer(v), o.dequantize_buffer(s, v)) for s in (8, -5, 1, I32_MAX, 65536)]
    if name == "to_symbols":
        return [("u8", codec.to_symbols(v), o.to_symbols(v))]
    if name == "from_symbols":
        s = rng.integers(0, 256, n).astype(np.uint8)
        s[:min(n, 4)] = [0, 1, 2, 255][:min(n, 4)]
        s[n - min(n, 4):] = [255, 254, 1, 0][:min(n, 4)]
        return [("u8", codec.from_symbols(s), o.from_symbols(s))]
    if name == "wide_symbols":
        hist, back, z = _wide_call(codec, v)
        want_z = _wide_z(v)
        return [("z", z, want_z), ("back", back, R3.from_wide_symbols(want_z)), ("hist", hist, R3.histogram(want_z))]
    if name == "rgb_to_ycocg":
        rgb = rng.integers(0, 256, 3 * n).astype(np.uint8)
        rgb[:6] = [0, 0, 0, 255, 0, 255][:min(6, 3 * n)]
        rgb[3 * n - 3:] = [0, 255, 0]
        return [(ch, a, b) for ch, a, b in zip("y co cg".split(), codec.rgb_bytes_to_ycocg_r(rgb), o.rgb_to_ycocg_r(rgb))]
    if name == "ycocg_to_rgb":
        # the whole i16 range: the sums wrap, then clamp to a byte
        y, co, cg = (rng.integers(-32768, 32768, n).astype(np.int16) for _ in range(3))
        y[n - 1], co[n - 1], cg[n - 1] = 32767, -32768, 32767
        y[0], co[0], cg[0] = -32768, 32767, -32768
        small = [rng.integers(-300, 300, n).astype(np.int16) for _ in range(3)]
        return [("wrap", codec.ycocg_r_to_rgb_bytes(y, co, cg), o.ycocg_r_to_rgb(y, co, cg)),
                ("clamp", codec.ycocg_r_to_rgb_bytes(*small), o.ycocg_r_to_rgb(*small))]
    raise KeyError(name)


@pytest.mark.parametrize("name", ["quantize", "fast_quantize", "dequantize", "to_symbols", "from_symbols", "wide_symbols",
                                  "rgb_to_ycocg", "ycocg_to_rgb"])
def test_elementwise_kernels_wrap_the_grid(gpu_codec, oracle_mod, grid_cap, name):
    for cap in G.HOOK_CAPS:
        for n in G.elementwise_sizes(cap):
            for c in (cap, 0):
                grid_cap(c)
                for what, got, want in _elementwise(gpu_codec, oracle_mod, name, n):
                    assert got.dtype == want.dtype and np.array_equal(got, want), (name, what, n, c)


# ---------------------------------------------------------------------------------------------------------------------
# under the hook: launch_wavelet_axis through Wavelet1D / 2D / 3D
# ---------------------------------------------------------------------------------------------------------------------

def _wavelet_pair(codec, o, k, shape):
    """(gpu, oracle) callables f(data, inverse) for this shape"""
    if len(shape) == 1:
        w1 = codec.Wavelet1D(codec.WaveletType(k))
        return (lambda d, inv: w1.inverse(d) if inv else w1.forward(d)), (lambda d, inv: o.wavelet1d(k, d, inv))
    if len(shape) == 2:
        w2 = codec.Wavelet2D(codec.WaveletType(k))
        return ((lambda d, inv: w2.inverse(d, *shape) if inv else w2.forward(d, *shape)),
                (lambda d, inv: o.wavelet2d(k, d, *shape, inverse=inv)))
    w3 = codec.Wavelet3D(codec.WaveletType(k))
    return ((lambda d, inv: w3.inverse(d, *shape) if inv else w3.forward(d, *shape)),
            (lambda d, inv: o.wavelet3d(k, d, *shape, inverse=inv)))


@pytest.mark.parametrize("k", [0, 1, 2])
def test_wavelet_axis_launches_wrap_the_grid(gpu_codec, oracle_mod, grid_cap, k):
    for shape in G.wavelet_shapes():
        assert not G.tile_eligible(shape), shape
        n = int(np.prod(shape))
        rng = np.random.default_rng(n + k)
        # pixel-sized values and the whole i32 range (the lifting sums wrap like the reference's)
        for data in (rng.integers(-300, 300, n).astype(np.int32), rng.integers(I32_MIN, I32_MAX + 1, n).astype(np.int32)):
            gpu, ref = _wavelet_pair(gpu_codec, oracle_mod, k, shape)
            want = {inv: ref(data, inv) for inv in (False, True)}
            for cap in G.HOOK_CAPS + (0,):
                grid_cap(cap)
                for inv in (False, True):
                    assert np.array_equal(gpu(data, inv), want[inv]), (shape, k, cap, inv)


# ---------------------------------------------------------------------------------------------------------------------
# under the hook: pad / strip and the whole generic pipeline, containers v1, v2 and v3
# ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _pipeline_reference(shape, k):
    """rgb and, per container version, (quality, the container's bytes, the decoded pixels): computed once, never modified"""
    import oracle
    import oracle.alice_oracle_np as onp
    w, h, f = shape
    rgb = WO.smooth_plus_noise(w, h, f, seed=w + 3 * h + 7 * f)
    rgb.setflags(write=False)
    out = {}
    v1 = oracle.encode(rgb, w, h, f, 80, k)
    out[1] = (80, v1, oracle.decode(v1))
    sym = oracle.encode_symbols(rgb, w, h, f, 90, k).reshape(3, -1)
    step = RR.quality_to_step(90)
    # version 2 decodes to the inverse of exactly these symbols (a version 1 stream of so few symbols need not: its table gives
    # every absent symbol a slot and the last frequency absorbs the excess)
    pw, ph, pf = G.padded_dims(w, h, f)
    pixels = OracleStages().inverse_symbols(torch.from_numpy(sym.reshape(3, pf, ph, pw)), w, h, f, k, [step] * 3).numpy().reshape(-1)
    out[2] = (90, R2.write_container(k, w, h, f, 64, [step] * 3, sym), pixels)
    step, dims, qs = WO.forward_quantised(onp, rgb, w, h, f, 100, k)
    z = [R3.wide_symbols(q) for q in qs]
    pixels = WO.inverse_quantised(onp, [R3.from_wide_symbols(zz) for zz in z], step, dims, w, h, f, k)
    out[3] = (100, R3.write_container(k, w, h, f, 64, [step] * 3, z), pixels)
    return rgb, out


def _pipeline_run(codec, version, rgb, w, h, f, k, q):
    enc = codec.FrameEncoder.with_wavelet(q, codec.WaveletType(k))
    if version == 1:
        chunk = enc.encode(rgb, w, h, f)
        return chunk.to_bytes(), codec.FrameDecoder().decode(chunk)
    if version == 2:
        got = codec.encode_split(enc, rgb, w, h, f, 64)
        return got, codec.decode_split(got)
    got = codec.encode_wide(enc, rgb, w, h, f, 64)
    return got, codec.decode_wide(got)


@pytest.mark.parametrize("version", [1, 2, 3])
def test_generic_pipeline_wraps_the_grid(gpu_codec, grid_cap, version):
    for i, shape in enumerate(G.PIPELINE_SHAPES):
        w, h, f = shape
        k = i % 3
        rgb, ref = _pipeline_reference(shape, k)
        q, want_bytes, want_pixels = ref[version]
        for cap in G.HOOK_CAPS + (0,):
            grid_cap(cap)
            got, pixels = _pipeline_run(gpu_codec, version, rgb, w, h, f, k, q)
            assert got == want_bytes, (shape, k, version, cap)
            assert np.array_equal(pixels, want_pixels), (shape, k, version, cap)


# ---------------------------------------------------------------------------------------------------------------------
# under the hook: ssim / ms_ssim (ssim_blocks_kernel, downsample2_kernel)
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,caps", G.SSIM_CASES)
def test_ssim_and_ms_ssim(gpu_codec, oracle_mod, grid_cap, w, h, caps):
    rng = np.random.default_rng(w * 1000 + h)
    y, x = np.mgrid[0:h, 0:w]
    a = np.clip(128 + 90 * np.sin(x / 11.0) * np.cos(y / 7.0) + rng.integers(-10, 11, (h, w)), 0, 255).astype(np.uint8).reshape(-1)
    b = np.clip(a.astype(np.int16) + rng.integers(-25, 26, a.size), 0, 255).astype(np.uint8)
    b[-w * (h % 8 + 8):] = rng.integers(0, 256, w * (h % 8 + 8))       # the last block row differs most: the last trip counts
    want = oracle_mod.ssim(a, b, w, h), oracle_mod.ssim(a, b, w, h, multi_scale=True)
    for cap in caps:
        grid_cap(cap)
        got = gpu_codec.ssim(a, b, w, h), gpu_codec.ms_ssim(a, b, w, h)
        print(f"{w}x{h} cap {cap}: ssim {got[0]!r} (oracle {want[0]!r}), ms_ssim {got[1]!r} (oracle {want[1]!r})")
        assert got[0] == want[0], (w, h, cap)
        assert got[1] == want[1], (w, h, cap)


# ---------------------------------------------------------------------------------------------------------------------
# at the real caps: the histograms
# ---------------------------------------------------------------------------------------------------------------------

GUARD = 64   # u32 words on either side of the 256 bins


def _dev_histogram(codec, d_base, off, n):
    out = torch.full((GUARD + 256 + GUARD,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    rc = codec.load_library().alice_codec_dev_histogram(d_base.data_ptr() + off, n, out.data_ptr() + 4 * GUARD, None)
    torch.cuda.synchronize()
    assert rc == 0
    host = out.cpu().numpy().view(np.uint32)
    assert (host[:GUARD] == 0x5A5A5A5A).all() and (host[GUARD + 256:] == 0x5A5A5A5A).all(), "words outside the bins were written"
    return host[GUARD:GUARD + 256]


def _hist_contents(n, seed):
    """name -> n bytes (built at the largest size once and cut)"""
    rng = np.random.default_rng(seed)
    skew = rng.choice(256, size=n, p=(lambda p: p / p.sum())(1.0 / (1.0 + np.arange(256)) ** 1.2)).astype(np.uint8)
    one = np.zeros(n, np.uint8)
    return {"random": skew, "one_nonzero": one, "zeros": np.zeros(n, np.uint8), "all_255": np.full(n, 255, np.uint8)}


def test_dev_histogram_alignment_and_trips(gpu_codec):
    top = max(G.HIST_SIZES)
    contents = _hist_contents(top, 17)
    d_base = torch.zeros(top + 16, dtype=torch.uint8, device=DEV)
    assert d_base.data_ptr() % 16 == 0
    for name, full in contents.items():
        for n in G.HIST_SIZES:
            if n > G.HIST_ALL_CONTENTS and name not in ("random", "one_nonzero"):
                continue
            data = full[:n].copy()
            if name == "one_nonzero" and n:
                data[n - 1] = 7                     # the very last byte: the tail of the last trip
            want = np.bincount(data, minlength=256).astype(np.uint32)
            d_data = torch.from_numpy(data).to(DEV)
            for off in G.hist_offsets(n):
                d_base.zero_()
                d_base[off:off + n] = d_data
                assert np.array_equal(_dev_histogram(gpu_codec, d_base, off, n), want), (name, off, n)
    # the host entry point reaches the same kernel
    data = contents["random"][:G.HIST_VEC * G.REDUCE_TRIP + 4805]
    assert np.array_equal(gpu_codec.build_histogram(data), np.bincount(data, minlength=256).astype(np.uint32))


@pytest.mark.parametrize("n", G.WIDE_HIST_SIZES)
def test_wide_histogram_trips_and_escape_boundary(gpu_codec, n):
    rng = np.random.default_rng(n)
    c = rng.integers(-40, 41, n).astype(np.int32)
    # z = 253 .. 257 around the escape, the top of the u16 range and beyond it, at the start, at the trip edge, at the very end
    special = np.array([127, -127, 128, -128, 129, 32768, -32767, -32768, 32769, 40000, I32_MAX, I32_MIN], np.int32)
    for at in (0, min(n, G.REDUCE_TRIP) - len(special), n - len(special)):
        c[at:at + len(special)] = special
    hist, back, z = _wide_call(gpu_codec, c)
    want_z = _wide_z(c)
    assert {253, 254, 255, 256, 257, 65534, 65535} <= set(int(v) for v in want_z[n - len(special):])
    assert np.array_equal(z, want_z)
    assert np.array_equal(back, R3.from_wide_symbols(want_z))
    assert np.array_equal(hist, R3.histogram(want_z))


def test_wide_stage_encode_counts_the_second_trip(gpu_codec):
    """alice_codec_dev_wide_encode counts the symbols with histogram_wide_kernel before it trusts the caller's histogram:
    a symbol that only the second trip sees, and that the histogram denies, must be refused."""
    lib = gpu_codec.load_library()
    n, L = 600_001, 8192
    z = np.random.default_rng(5).integers(0, 20, n).astype(np.uint16)
    for last, sym in ((255 + 9, 255), (254, 254), (65535, 255)):
        zz = z.copy()
        zz[n - 1] = last
        d_sym = torch.from_numpy(zz.view(np.int16).copy()).to(DEV)
        cap = gpu_codec.wide_stream_bound(n, L)
        out = torch.zeros(cap, dtype=torch.uint8, device=DEV)
        true = R3.histogram(zz)
        assert true[sym] == 1
        denied = true.copy()
        denied[sym] = 0
        denied[0] += 1
        got = C.c_uint64(0)
        for hist, rc_want in ((denied, 1), (true, 0 if last < 65535 else None)):
            if rc_want is None:      # a residual above 4095 has no code: refused later, for another reason
                continue
            rc = lib.alice_codec_dev_wide_encode(d_sym.data_ptr(), n, hist.ctypes.data_as(C.POINTER(C.c_uint32)), L, out.data_ptr(),
                                                 cap, C.byref(got), None)
            torch.cuda.synchronize()
            assert rc == rc_want, (last, rc, rc_want)


# ---------------------------------------------------------------------------------------------------------------------
# at the real caps: psnr (sq_diff_sum_kernel) and AnalyticalRDO (sum_i32_kernel)
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", G.PSNR_SIZES)
def test_psnr_trips(gpu_codec, oracle_mod, n):
    rng = np.random.default_rng(n)
    a = rng.integers(0, 256, n).astype(np.uint8)
    b = np.clip(a.astype(np.int16) + rng.integers(-3, 4, n), 0, 255).astype(np.uint8)
    b[n - 1] = a[n - 1] ^ 0xFF                      # the last item carries a large share of the sum
    got, want = gpu_codec.psnr(a, b), oracle_mod.psnr(a, b)
    print(f"n {n}: psnr {got!r} (oracle {want!r})")
    assert got == want
    assert gpu_codec.psnr(a, a) == oracle_mod.psnr(a, a)


@pytest.mark.parametrize("n", G.RDO_SIZES)
def test_rdo_quantizer_trips_and_signed_sum(gpu_codec, oracle_mod, n):
    rng = np.random.default_rng(n)
    noise = rng.integers(-100, 101, n).astype(np.int32)
    contents = {
        # a small variance around a large negative mean: the step follows the mean, and every partial sum is negative, so
        # the u64 atomic adds have to wrap into the signed sum
        "negative_mean": (noise - 2 ** 30).astype(np.int32),
        "positive_mean": (noise + 2 ** 30).astype(np.int32),
        # the two halves cancel: the sum passes through large values of both signs
        "cancelling": np.where(np.arange(n) % 2 == 0, 2 ** 30, -2 ** 30).astype(np.int32) + noise,
        "full_range": rng.integers(-2 ** 30, 2 ** 30 + 1, n).astype(np.int32),
    }
    for q in (75, 20):
        rdo = gpu_codec.AnalyticalRDO.with_quality(q)
        for name, c in contents.items():
            for sb in (0, 7):
                got = rdo.compute_quantizer(c, gpu_codec.SubBand3D(sb))
                want = oracle_mod.rdo_compute_quantizer(rdo.target_bpp(), c, sb)
                assert (got.step, got.dead_zone) == want, (n, q, name, sb)
    # a condition of the test: the step depends on the mean (it is not clamped), so a lost trip would show
    step, _ = oracle_mod.rdo_compute_quantizer(gpu_codec.AnalyticalRDO.with_quality(75).target_bpp(), contents["negative_mean"], 0)
    assert 10 < step < 1000, step


# ---------------------------------------------------------------------------------------------------------------------
# at the real caps: size prediction on the generic path (coef_hist_kernel: 1024 workgroups, 262 144 coefficients a trip)
# ---------------------------------------------------------------------------------------------------------------------

def _late_frames(w, h, f):
    """black, but the odd frames from 57 on are grey 40: every coefficient outside [-24, 24) is a temporal high-pass one of
    the last frames, beyond the first 262 144 coefficients of the Y volume"""
    fr = np.zeros((f, h, w, 3), np.uint8)
    fr[57::2] = 40
    return fr.reshape(-1)


@functools.lru_cache(maxsize=None)
def _rate_reference(shape, k, content="noise"):
    """(rgb, coefficient volumes [3], u8 step histograms (64, 3, 256), wide step histograms): the oracle's forward transform
    once, then rate_ref's fold (the oracle's quantiser and symbol map on the distinct values) at each of the 64 steps"""
    import oracle
    import oracle.alice_oracle_np as onp
    w, h, f = shape
    rgb = WO.smooth_plus_noise(w, h, f, seed=w + h + f + k) if content == "noise" else _late_frames(w, h, f)
    rgb.setflags(write=False)
    coefs = []
    for ch in oracle.rgb_to_ycocg_r(rgb):
        v, pw, ph, pf = onp._pad(ch, w, h, f)
        coefs.append(oracle.wavelet3d(k, v.reshape(-1), pw, ph, pf))
    u8 = np.zeros((64, 3, 256), np.uint64)
    wide = np.zeros((64, 3, 256), np.uint32)
    for c in range(3):
        vals, counts = np.unique(coefs[c], return_counts=True)
        for step in range(1, 65):
            u8[step - 1, c] = RR.fold(oracle, vals, counts, step)
            z = R3.wide_symbols(onp.quantize(vals, step, step))
            wide[step - 1, c] = np.bincount(R3.coded(z), weights=counts, minlength=256).astype(np.uint32)
    # the fold is the oracle's encode: the header histograms at the two ends of the quality scale
    for q in (0, 100):
        assert np.array_equal(RR.header_hists(oracle.encode(rgb, w, h, f, q, k)), u8[RR.quality_to_step(q) - 1])
    return rgb, coefs, u8, wide


def _check_rate(codec, oracle_mod, shape, k, content, containers):
    w, h, f = shape
    rgb, _, u8, wide = _rate_reference(shape, k, content)
    d = _dev(rgb)
    if 1 in containers:
        d_hist = torch.zeros(64 * 3 * 256, dtype=torch.int32, device=DEV)
        p = codec.predict_sizes_device(d.data_ptr(), w, h, f, 1, k, d_hist.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d_hist.cpu().numpy().view(np.uint32).reshape(64, 3, 256), u8), (shape, k, content)
        lo, hi, st = RR.chunk_prediction(oracle_mod, u8, RR.log_table(codec))
        assert np.array_equal(p.lo[0], lo) and np.array_equal(p.hi[0], hi) and np.array_equal(p.status[0], st), (shape, k, content)
    if 2 in containers:
        lo, hi = SR.chunk_prediction(u8, 512)
        p = codec.predict_split_sizes(rgb, w, h, f, k)
        assert np.array_equal(p.lo, lo) and np.array_equal(p.hi, hi), (shape, k, content)
    if 3 in containers:
        lo, hi = WR.chunk_prediction(wide, 64)
        d_hist = torch.zeros(64 * 3 * 256, dtype=torch.int32, device=DEV)
        p = codec.predict_wide_sizes_device(d.data_ptr(), w, h, f, 1, k, 64, d_step_hist=d_hist.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d_hist.cpu().numpy().view(np.uint32).reshape(64, 3, 256), wide), (shape, k, content)
        assert np.array_equal(p.lo[0], lo) and np.array_equal(p.hi[0], hi), (shape, k, content)


@pytest.mark.parametrize("shape", G.RATE_SHAPES)
def test_generic_size_prediction_trips(gpu_codec, oracle_mod, shape):
    full = shape == G.RATE_FULL
    _check_rate(gpu_codec, oracle_mod, shape, 1 if full else sum(shape) % 3, "noise", (1, 2, 3) if full else (1,))
    if full:
        assert int(_rate_reference(shape, 1)[3][0, :, 255].sum()) > 0        # escapes at step 1: version 3 differs from 2


def test_out_of_range_counter_fires_on_the_second_trip(gpu_codec, oracle_mod):
    lib = gpu_codec.load_library()
    shape, r = G.RATE_FULL, 24
    for k in (0, 2):
        coefs = _rate_reference(shape, k, "late")[1]
        out = [np.nonzero((c < -r) | (c >= r))[0] for c in coefs]
        assert out[0].size and out[0].min() >= G.COEF_TRIP and not out[1].size and not out[2].size    # a condition of the test
    try:
        lib.alice_codec_test_set_value_table_radius(r)
        for k in (0, 2):
            _check_rate(gpu_codec, oracle_mod, shape, k, "late", (1, 2, 3))
    finally:
        lib.alice_codec_test_set_value_table_radius(2048)


# ---------------------------------------------------------------------------------------------------------------------
# at the real caps: region encode and decode on the generic path (65 536 rows a trip, 256 pixels a trip across a row)
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H,w,h,f,origins", G.REGION_CASES)
def test_generic_regions_rows_and_width(gpu_codec, oracle_mod, W, H, w, h, f, origins):
    from test_gpu_region import _alcs, _crop, _source
    a, o = gpu_codec, oracle_mod
    n, q, k = len(origins), 90, (w + h) % 3
    assert {x0 % 4 for x0, _ in origins} >= ({0, 1} if n > 1 else set())
    src = _source(W + h, n * f, H, W)
    d = _dev(src)
    bt = a.Batch(w, h, f, n, q, a.WaveletType(k))
    bt.encode_regions(d.data_ptr(), W, H, origins)
    alcs = _alcs(bt, bt.encode_finish())
    for i, (x0, y0) in enumerate(origins):
        assert alcs[i] == o.encode(_crop(src[i * f:(i + 1) * f], x0, y0, w, h), w, h, f, q, k), (W, H, w, h, f, (x0, y0))
    canary = np.random.default_rng(W * 7 + h).integers(0, 256, (n * f, H, W, 3), dtype=np.uint8)
    out = _dev(canary)
    bt.decode_regions(bt.alc_ptr(0), bt.alc_stride, out.data_ptr(), W, H, origins)
    bt.decode_finish()
    want = canary.copy()
    for i, (x0, y0) in enumerate(origins):
        want[i * f:(i + 1) * f, y0:y0 + h, x0:x0 + w] = o.decode(alcs[i]).reshape(f, h, w, 3)
    assert np.array_equal(out.cpu().numpy(), want)           # the rectangles, and every byte outside them unchanged
