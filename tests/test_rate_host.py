"""Rate control without a device: the size bracket against the oracle's own rANS, the fixed-point log table, the fold
through the oracle's quantiser, the restated RateController / estimate_quality of src/rate_control.rs, and the argument
checks of the new C entry points."""
import math
import os
import sys
from decimal import Decimal, getcontext

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rate_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def table(codec):
    return R.log_table(codec)


# ---- the fixed-point log table ----

def test_log_table_rounding_directions(table):
    lo, hi, (g_up, g_dn) = table
    getcontext().prec = 50
    scale = Decimal(1 << R.FRAC)
    ln2 = Decimal(2).ln()
    for f in range(1, 4097):
        if f & (f - 1) == 0:      # exact: 12 - log2(f) bits
            assert lo[f] == hi[f] == (12 - f.bit_length() + 1) << R.FRAC, f
            continue
        v = (Decimal(4096) / Decimal(f)).ln() / ln2 * scale
        assert Decimal(int(lo[f])) < v < Decimal(int(lo[f]) + 1), f
        assert hi[f] == lo[f] + 1, f
    up = (Decimal(1) + Decimal(2) ** -11).ln() / ln2 * scale
    dn = -(Decimal(1) - Decimal(2) ** -11).ln() / ln2 * scale
    assert g_up - 1 < up <= g_up and g_dn - 1 < dn <= g_dn


# ---- the bracket against the oracle's encoder ----

def _symbol_arrays(rng):
    lengths = [1, 2, 3, 7, 64, 255, 256, 1000, 4096, 10_000]
    for i in range(2400):
        n = int(lengths[i % len(lengths)]) if i % 3 else int(rng.integers(1, 3000))
        kind = i % 6
        if kind == 0:     # skewed (geometric)
            s = np.minimum(rng.geometric(rng.uniform(0.05, 0.9), n) - 1, 255)
        elif kind == 1:   # near-uniform over all symbols
            s = rng.integers(0, 256, n)
        elif kind == 2:   # one symbol
            s = np.full(n, int(rng.integers(0, 256)))
        elif kind == 3:   # two symbols
            a, b = rng.choice(256, 2, replace=False)
            s = np.where(rng.random(n) < rng.uniform(0.01, 0.99), a, b)
        elif kind == 4:   # many rare symbols + symbol 255 (the wrapping correction on the last bin)
            s = np.concatenate([rng.integers(0, 256, max(n // 8, 1)), np.full(max(n // 50, 1), 255), np.zeros(n, int)])
        else:             # few symbols at the top of the alphabet
            s = rng.integers(250, 256, n)
        yield rng.permutation(s).astype(np.uint8)
    for n in (30_000, 100_000):
        yield np.minimum(rng.geometric(0.3, n) - 1, 255).astype(np.uint8)
        yield rng.integers(0, 256, n).astype(np.uint8)


def test_bracket_holds_on_oracle_rans(oracle_mod, table):
    rng = np.random.default_rng(2024)
    seen = {R.BOUNDED: 0, R.UNBOUNDED: 0, R.DIVERGES: 0}
    for sym in _symbol_arrays(rng):
        hist = np.bincount(sym, minlength=256).astype(np.uint64)
        status, lo, hi = R.channel_cost(oracle_mod, hist, table)
        seen[status] += 1
        if status != R.BOUNDED:
            ft = oracle_mod.FrequencyTable(hist.astype(np.uint32))
            f = ft.freq.astype(int); c = ft.cum_freq.astype(int)
            present = hist > 0
            assert np.any(present & ((f == 0) | (f > 4096)))
            continue
        n = len(oracle_mod.rans_encode(sym, oracle_mod.FrequencyTable(hist.astype(np.uint32))))
        assert lo <= n <= hi, (len(sym), lo, n, hi)
    assert seen[R.BOUNDED] > 2000


def test_unbounded_and_diverging_tables_are_classified(oracle_mod, table):
    # 256 present symbols, one of them dominant: the freq-1 floors push the sum past 4096, later cums pass 4096 (bounded,
    # with the excess in the bracket), and the correction on symbol 255 wraps its frequency to a u16 above 4096
    h = np.ones(256, np.uint64); h[0] = 10_000_000
    ft = oracle_mod.FrequencyTable(h.astype(np.uint32))
    assert int(ft.freq[255]) > 4096 and R.channel_cost(oracle_mod, h, table)[0] == R.UNBOUNDED
    sym = np.concatenate([np.zeros(100_000, np.uint8), np.arange(1, 255, dtype=np.uint8)])
    hh = np.bincount(sym, minlength=256).astype(np.uint64)
    ft = oracle_mod.FrequencyTable(hh.astype(np.uint32))
    assert int(ft.cum_freq[254]) + int(ft.freq[254]) > 4096
    status, lo, hi = R.channel_cost(oracle_mod, hh, table)
    assert status == R.BOUNDED and lo <= len(oracle_mod.rans_encode(sym, ft)) <= hi
    # the wrapping correction takes symbol 255 to frequency 0 while it is present
    h = np.zeros(256, np.uint64); h[0] = 4096 * 255; h[1:] = 1
    ft = oracle_mod.FrequencyTable(h.astype(np.uint32))
    status = R.channel_cost(oracle_mod, h, table)[0]
    assert status == (R.DIVERGES if int(ft.freq[255]) == 0 else R.UNBOUNDED)


# ---- the fold: one coefficient histogram gives the header histogram at every step ----

def test_fold_of_coefficient_histogram_equals_header_histograms(oracle_mod):
    import oracle.alice_oracle_np as onp
    rng = np.random.default_rng(5)
    w, h, f = 13, 9, 3
    rgb = rng.integers(0, 256, w * h * f * 3, dtype=np.uint8)
    for wavelet in (0, 1, 2):
        coefs = []
        for ch in onp.rgb_to_ycocg_r(rgb):
            v, pw, ph, pf = onp._pad(ch, w, h, f)
            coefs.append(np.asarray(onp.wavelet3d(wavelet, v, pw, ph, pf)).reshape(-1))
        for q in (0, 37, 80, 99, 100):
            step = R.quality_to_step(q)
            want = R.header_hists(oracle_mod.encode(rgb, w, h, f, q, wavelet))
            for c in range(3):
                vals, counts = np.unique(coefs[c], return_counts=True)
                assert np.array_equal(R.fold(oracle_mod, vals, counts, step), want[c]), (wavelet, q, c)


# ---- src/rate_control.rs restated (assertions of :213-343) ----

def test_rate_control_reference_tests(codec):
    RC, Cfg = codec.RateController, codec.RateControlConfig
    # :214-218 default_config
    cfg = Cfg()
    assert cfg.target_bitrate_kbps == 5_000 and abs(cfg.framerate - 30.0) < 1e-10
    assert (cfg.min_quality, cfg.max_quality, cfg.buffer_size_bits) == (10, 95, 10_000_000)
    # :221-226 target_bits_per_frame
    t = RC.with_defaults().target_bits_per_frame()
    assert 150_000 < t < 180_000 and t == 166_666
    # :229-233 initial_quality (u32::midpoint(10, 95) = 52)
    q = RC.with_defaults().recommended_quality()
    assert 10 <= q <= 95 and q == 52
    # :236-248 quality_decreases_on_overshoot
    c = RC.with_defaults(); t = c.target_bits_per_frame()
    for _ in range(30):
        c.update(t * 3)
    assert c.current_quality() < 52
    # :251-263 quality_increases_on_undershoot
    c = RC.with_defaults()
    for _ in range(30):
        c.update(t // 3)
    assert c.current_quality() > 52
    # :266-284 quality_clamped
    c = RC(Cfg(min_quality=20, max_quality=80))
    for _ in range(1000):
        c.update(10_000_000)
    assert c.current_quality() >= 20
    for _ in range(1000):
        c.update(1)
    assert c.current_quality() <= 80
    # :287-295 buffer_ratio_range
    c = RC.with_defaults(); c.update(0)
    assert -1.0 <= c.buffer_ratio() <= 1.0
    # :298-304 average_frame_size
    c = RC.with_defaults()
    for s in (1000, 2000, 3000):
        c.update(s)
    assert c.average_frame_size() == 2000
    # :307-313 frame_count
    c = RC.with_defaults()
    assert c.frame_count() == 0
    c.update(1000); c.update(2000)
    assert c.frame_count() == 2
    # :316-325 actual_to_target_ratio
    c = RC.with_defaults(); c.update(c.target_bits_per_frame())
    assert abs(c.actual_to_target_ratio() - 1.0) < 0.01
    # :328-331, :334-337, :340-343 estimate_quality
    assert codec.estimate_quality(50_000, 1920, 1080, 30.0) > 50
    assert codec.estimate_quality(100, 1920, 1080, 30.0) < 30
    assert codec.estimate_quality(5000, 0, 0, 30.0) == 50


def test_rate_control_integer_behaviour(codec):
    RC, Cfg = codec.RateController, codec.RateControlConfig
    # thresholds: +1 above 0.3, -2 below -0.3, a 30-entry history, the buffer starts half full
    c = RC.with_defaults()
    assert c.buffer_ratio() == 0.5
    c.update(c.target_bits_per_frame())
    assert c.current_quality() == 53                    # ratio 0.5 > 0.3
    c = RC(Cfg(buffer_size_bits=1000))
    c.update(c.target_bits_per_frame() + 1000)          # 500 - 1000: ratio -0.5 < -0.3
    assert c.current_quality() == 50 and c.buffer_ratio() == -0.5
    c.update(c.target_bits_per_frame() + 10**9)          # clamped to -buffer
    assert c.current_quality() == 48 and c.buffer_ratio() == -1.0
    c = RC.with_defaults()
    for i in range(40):
        c.update(i)
    assert c.average_frame_size() == sum(range(10, 40)) // 30 and c.frame_count() == 40
    # f64 -> u64 casts saturate, NaN -> 0; framerate <= 0 -> 0
    assert RC(Cfg(framerate=0.0)).target_bits_per_frame() == 0
    assert RC(Cfg(framerate=-5.0)).target_bits_per_frame() == 0
    assert RC(Cfg(framerate=math.nan)).target_bits_per_frame() == 0
    assert RC(Cfg(framerate=1e-300)).target_bits_per_frame() == (1 << 64) - 1
    assert RC(Cfg(framerate=math.inf)).target_bits_per_frame() == 0
    assert RC(Cfg(framerate=0.0)).actual_to_target_ratio() == 0.0
    assert RC(Cfg(buffer_size_bits=0)).buffer_ratio() == 0.0
    # u32::midpoint does not overflow
    assert RC(Cfg(min_quality=0xFFFFFFFF, max_quality=0xFFFFFFFF)).recommended_quality() == 0xFFFFFFFF
    assert RC(Cfg(min_quality=3, max_quality=6)).recommended_quality() == 4
    # estimate_quality: clamp(5, 100), NaN fps -> 0 -> 5, mul_add branches
    assert codec.estimate_quality(1, 1920, 1080, 30.0) == 5
    assert codec.estimate_quality(5000, 1920, 1080, math.nan) == 5
    assert codec.estimate_quality(5000, 1920, 1080, -1.0) == 50
    assert codec.estimate_quality(10**9, 16, 16, 1.0) == 95
    assert codec.estimate_quality(3000, 1000, 1000, 3.0) == 65     # bpp 1.0 -> 1.0 * 30 + 35
    assert codec.estimate_quality(300, 1000, 1000, 1.0) == 35       # bpp 0.3 -> 0.3 * 75 + 12.5 = 35.0
    assert codec.budget_bytes_per_chunk(5000, 30.0, 64) == 166_666 * 64 // 8


# ---- the new C entry points without a device ----

def test_c_entry_points_validate_without_device(codec):
    with pytest.raises(codec.CodecError) as e:        # no pixels, but bytes: buffer size (src/pipeline.rs:391-412)
        codec.predict_sizes(np.zeros(3, np.uint8), 0, 4, 4)
    assert e.value.code == 1
    with pytest.raises(codec.CodecError) as e:        # w*h*f overflows: dimensions first, whatever the buffer
        codec.predict_sizes(np.zeros(3, np.uint8), 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)
    assert e.value.code == 3
    p = codec.predict_sizes(np.zeros(0, np.uint8), 0, 7, 3)   # the empty chunk: its header at every quality
    assert np.all(p.lo == R.HEADER) and np.all(p.hi == R.HEADER) and np.all(p.status == 0)
    chunk, q, fits = codec.encode_to_size(np.zeros(0, np.uint8), 5, 0, 2, 10_000, min_quality=20, max_quality=150)
    assert (q, fits) == (100, True) and chunk.compressed_size() == 0 and len(chunk.to_bytes()) == R.HEADER
    chunk, q, fits = codec.encode_to_size(np.zeros(0, np.uint8), 5, 0, 2, 100, min_quality=20, max_quality=30)
    assert (q, fits) == (20, False)
    with pytest.raises(codec.CodecError) as e:        # min > max after qualities above 100 became 100
        codec.encode_to_size(np.zeros(0, np.uint8), 5, 0, 2, 10_000, min_quality=60, max_quality=50)
    assert e.value.code == 2
    codec.encode_to_size(np.zeros(0, np.uint8), 5, 0, 2, 10_000, min_quality=200, max_quality=120)
    with pytest.raises(codec.CodecError) as e:        # buffer size before the quality range
        codec.encode_to_size(np.zeros(5, np.uint8), 5, 0, 2, 10_000, min_quality=60, max_quality=50)
    assert e.value.code == 1
    with pytest.raises(codec.CodecError) as e:
        codec.predict_sizes(np.zeros(12, np.uint8), 2, 2, 1, wavelet_type=7)
    assert e.value.code == 4
    lib = codec.load_library()
    assert lib.alice_codec_predict_sizes(0, None, 0, 0, 0, 0, None, None, None) == 9
    assert lib.alice_codec_dev_predict_sizes(None, 4, 4, 2, 1, 0, None, None, None, None, None) == 9


def test_budgets_out_of_u64_range_are_refused(codec):
    for bad in (-1, 1 << 64):
        with pytest.raises(ValueError):
            codec.encode_to_size(np.zeros(0, np.uint8), 5, 0, 2, bad)
