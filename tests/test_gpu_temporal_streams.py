"""Every instance of the two streaming temporal bodies (FwdT::run and InvT::run of csrc/transform.hip: the u8, wide and
bins forwards, the u8, wide and mirrored inverses and their window twins) at every frame-count class of its peeled loop --
first block only, tail only, one and two steady blocks with every tail length -- on the MI355X.  The plan (frame counts 1 ..
26, 33, 34, 39, 40 on 12x10, the steady-loop counts again on 70x34, the contents, one quantiser step from the middle of
every instance class, the frame ranges) is tests/temporal_cases.py's, and tests/test_temporal_cases_host.py shows without
a device that it reaches what it claims.  Every expected value comes from the CPU oracle or from the numpy restatements
(wide_oracle / wide_ref, rate_ref, transform_extremes, reversible_ref), never from another call of the library, and every
comparison is bit-exact.  The last test holds what ran in the process against the class tables."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frames_ref as FR  # noqa: E402
import rate_ref as RATE  # noqa: E402
import temporal_cases as T  # noqa: E402
import transform_extremes as X  # noqa: E402
import wide_oracle as WO  # noqa: E402
import wide_ref as R3  # noqa: E402
from test_gpu_frames import Chunk, _check_stats  # noqa: E402
from test_gpu_transform_extremes import gpu_inverse  # noqa: E402
from test_gpu_value_table import loud_and_quiet  # noqa: E402
from test_gpu_wide import forward_symbols_wide  # noqa: E402

import torch  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
SENTINEL = 0xA5
QUALITIES = (100, 80)        # step 1 (the STEP1 instances) and step 14
_ran = set()                 # (family, wavelet, variant) that ran at a frame count inside the steady loop
_done = set()                # the cases of the tests below that ran to their end in this process
N_CASES = 6 + 6 + 3 + 3 + 6 + 9


def _mismatch(got, want):
    bad = np.flatnonzero(np.asarray(got).reshape(-1) != np.asarray(want).reshape(-1))
    return bad.size, bad[:4].tolist()


# ---- a. the u8 forward: fwd_t_kernel<NS, STEP1>, table and arithmetic ----
def gpu_forward(codec, rgb, w, h, f, kind, q):
    """alice_codec_dev_forward_symbols into guarded symbol and histogram buffers -> ((3, n) u8, (3, 256) u32)"""
    lib = codec.load_library()
    n = int(np.prod(T.dims(w, h, f)))
    d_rgb = torch.from_numpy(np.array(rgb)).to(DEV)
    d_sym = torch.full((GUARD + 3 * n + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    d_hist = torch.full((GUARD + 3 * 256 + GUARD,), -1, dtype=torch.int32, device=DEV)
    d_hist[GUARD:GUARD + 768] = 0
    rc = lib.alice_codec_dev_forward_symbols(d_rgb.data_ptr(), w, h, f, kind, q, d_sym.data_ptr() + GUARD,
                                             d_hist.data_ptr() + 4 * GUARD, None)
    torch.cuda.synchronize()
    assert rc == 0, lib.alice_codec_last_error_message()
    sym, hist = d_sym.cpu().numpy(), d_hist.cpu().numpy()
    assert (sym[:GUARD] == SENTINEL).all() and (sym[GUARD + 3 * n:] == SENTINEL).all(), "bytes beside the symbols were written"
    assert (hist[:GUARD] == -1).all() and (hist[GUARD + 768:] == -1).all(), "words beside the histograms were written"
    assert np.array_equal(d_rgb.cpu().numpy(), rgb), "the pixels were modified"
    return sym[GUARD:GUARD + 3 * n].reshape(3, n), hist[GUARD:GUARD + 768].view(np.uint32).reshape(3, 256)


@pytest.mark.parametrize("q", QUALITIES)
@pytest.mark.parametrize("kind", T.KINDS)
def test_u8_forward_at_every_frame_count(gpu_codec, oracle_mod, kind, q):
    """Radius 2048: every value goes through the value table; radius 48: the left half of the frames (Co = +-255
    checkerboards) sends its wavefronts through the arithmetic, on 70x34 beside wavefronts that stay in the table."""
    lib = gpu_codec.load_library()
    try:
        for w, h, f in T.shapes():
            rgb = loud_and_quiet(w, h, f, seed=w + f)
            want = oracle_mod.encode_symbols(rgb, w, h, f, q, kind).reshape(3, -1)
            hists = [oracle_mod.build_histogram(want[c]) for c in range(3)]
            for r in (2048, 48):
                lib.alice_codec_test_set_value_table_radius(r)
                sym, hist = gpu_forward(gpu_codec, rgb, w, h, f, kind, q)
                for c in range(3):
                    assert np.array_equal(sym[c], want[c]), (kind, q, (w, h, f), r, c, _mismatch(sym[c], want[c]))
                    assert np.array_equal(hist[c], hists[c]), (kind, q, (w, h, f), r, c)
            if T.half_of(f) >= 9:
                _ran.add(("fwd_u8", kind, q == 100))
    finally:
        lib.alice_codec_test_set_value_table_radius(2048)
    _done.add(("a", kind, q))


# ---- b. the wide forward: fwd_t_wide_kernel<NS, STEP1> ----
@pytest.mark.parametrize("q", QUALITIES)
@pytest.mark.parametrize("kind", T.KINDS)
def test_wide_forward_at_every_frame_count(gpu_codec, kind, q):
    import oracle.alice_oracle_np as o
    for w, h, f in T.shapes():
        rgb = T.random_rgb(w, h, f)
        step, _, qs = WO.forward_quantised(o, rgb, w, h, f, q, kind)
        assert step == {100: 1, 80: 14}[q]
        z = [R3.wide_symbols(v) for v in qs]
        got_z, got_hist = forward_symbols_wide(gpu_codec, np.array(rgb), w, h, f, kind, q)
        for c in range(3):
            assert np.array_equal(got_z[c], z[c]), (kind, q, (w, h, f), c, _mismatch(got_z[c], z[c]))
            assert np.array_equal(got_hist[c], R3.histogram(z[c])), (kind, q, (w, h, f), c)
        if T.half_of(f) >= 9:
            _ran.add(("fwd_wide", kind, q == 100))
    _done.add(("b", kind, q))


# ---- c. the bins of the rate prediction: fwd_t_bins_kernel<NS> ----
_step_hists = {}


def _bins_case(oracle_mod, w, h, f, kind):
    """(rgb, the (64, 3, 256) header histograms of oracle.encode at every step), once per case.  The reference's entropy
    coder has no encoding for a few histograms (ReferenceDiverges: a symbol whose table frequency is 0), and then there is
    no header to read: such content is left for the next seed."""
    key = (w, h, f, kind)
    for seed in range(3 * w + f, 3 * w + f + 4000, 1000):
        if key in _step_hists:
            break
        rgb = WO.smooth_plus_noise(w, h, f, seed=seed)
        try:
            _step_hists[key] = (rgb, RATE.oracle_step_hists(oracle_mod, rgb, w, h, f, kind))
        except oracle_mod.OracleError as e:
            if e.code != oracle_mod.ERR_REFERENCE_DIVERGES:
                raise
    return _step_hists[key]


def _device_step_hists(codec, rgb, w, h, f, kind):
    d = torch.from_numpy(np.array(rgb)).to(DEV)
    hist = torch.full((GUARD + 64 * 3 * 256 + GUARD,), -1, dtype=torch.int32, device=DEV)
    hist[GUARD:GUARD + 64 * 768] = 0
    codec.predict_sizes_device(d.data_ptr(), w, h, f, 1, kind, hist.data_ptr() + 4 * GUARD)
    torch.cuda.synchronize()
    host = hist.cpu().numpy()
    assert (host[:GUARD] == -1).all() and (host[GUARD + 64 * 768:] == -1).all(), "words beside the histograms were written"
    assert np.array_equal(d.cpu().numpy(), rgb), "the pixels were modified"
    return host[GUARD:GUARD + 64 * 768].view(np.uint32).reshape(64, 3, 256)


@pytest.mark.parametrize("kind", T.KINDS)
def test_bins_at_every_frame_count(gpu_codec, oracle_mod, kind):
    """The step histograms folded from the coefficient bins; then radius 24 on three steady-loop counts and on 70x34:
    the coefficients outside [-24, 24) go to the out-of-range counter, whose fallback must give the same histograms."""
    lib = gpu_codec.load_library()
    try:
        for w, h, f in T.shapes():
            rgb, want = _bins_case(oracle_mod, w, h, f, kind)
            got = _device_step_hists(gpu_codec, rgb, w, h, f, kind)
            assert np.array_equal(got, want), (kind, (w, h, f), _mismatch(got, want))
            if T.half_of(f) >= 9:
                _ran.add(("bins", kind, None))
        lib.alice_codec_test_set_value_table_radius(24)
        for w, h, f in (T.SHAPE + (17,), T.SHAPE + (26,), T.SHAPE + (40,), T.SHAPE_WIDE + (18,)):
            rgb, want = _bins_case(oracle_mod, w, h, f, kind)
            got = _device_step_hists(gpu_codec, rgb, w, h, f, kind)
            assert np.array_equal(got, want), (kind, (w, h, f), "radius 24", _mismatch(got, want))
    finally:
        lib.alice_codec_test_set_value_table_radius(2048)
    _done.add(("c", kind))


# ---- d. the u8 inverse: inv_t_kernel<NS, EXACT, MidT> ----
@pytest.mark.parametrize("kind", T.KINDS)
def test_u8_inverse_at_every_frame_count(gpu_codec, oracle_mod, kind):
    lib = gpu_codec.load_library()
    cases = T.step_cases(lib, kind, 0)
    assert {v for _, v in cases} == T.expected_classes(kind, 0)
    for i, (w, h, f) in enumerate(T.shapes()):
        sym = T.byte_symbols(kind, w, h, f)
        for j, (steps, v) in enumerate(cases):
            assert X.variant(lib, kind, steps) == v
            got = gpu_inverse(gpu_codec, sym, w, h, f, kind, steps, align=(i + j) & 3)
            want = T.byte_reference(kind, w, h, f, steps)
            assert np.array_equal(got, want), (kind, (w, h, f), steps, v, _mismatch(got, want))
            if T.half_of(f) >= 8:
                _ran.add(("inv_u8", kind, v))
    _done.add(("d", kind))


# ---- e. the wide and the mirrored inverse: inv_t_wide_kernel<NS, EXACT, MidT, MIRROR> ----
@pytest.mark.parametrize("version", [3, 4])
@pytest.mark.parametrize("kind", T.KINDS)
def test_wide_inverse_at_every_frame_count(gpu_codec, kind, version):
    a = gpu_codec
    lib = a.load_library()
    cases = T.step_cases(lib, kind, 1)
    assert {v for _, v in cases} == T.expected_classes(kind, 1)
    decode = {3: a.decode_wide, 4: a.decode_reversible}[version]
    told_apart = False
    for w, h, f in T.shapes():
        for steps, v in cases:
            blob = T.container(kind, w, h, f, version, steps)
            want = T.reference(kind, w, h, f, version, steps)
            got = np.asarray(decode(blob))
            assert np.array_equal(got, want), (kind, version, (w, h, f), steps, v, _mismatch(got, want))
            told_apart |= not np.array_equal(want, T.reference(kind, w, h, f, 7 - version, steps))
            if T.half_of(f) >= 8:
                _ran.add(("inv_wide" if version == 3 else "inv_mirror", kind, v))
    assert told_apart        # this inverse ran, not its twin
    _done.add(("e", kind, version))


# ---- f. the windows: inv_t_win_kernel and inv_t_wide_win_kernel ----
@pytest.mark.parametrize("version", T.VERSIONS)
@pytest.mark.parametrize("kind", T.KINDS)
def test_windows_at_every_frame_count_class(gpu_codec, oracle_mod, kind, version):
    """The window instances lift the virtual chunk of the window: its half is (b - a) / 2, and the plan's ranges give it
    every class.  Both calls, every range, one step per instance class; the calls must report the plan's window."""
    a = gpu_codec
    lib = a.load_library()
    w, h = T.SHAPE
    wide = int(version != 2)
    cases = T.step_cases(lib, kind, wide)
    n = w * h * 3
    reached = set()
    for f in T.WINDOW_FRAMES:
        ch = None
        for steps, v in cases:
            blob = T.container(kind, w, h, f, version, steps)
            full = T.reference(kind, w, h, f, version, steps)
            if ch is None:
                ch = Chunk(a, version, (w, h, f), kind, blob=blob)
            else:
                ch.blob = blob
                ch.set_container(blob)
            for t0, t1 in T.window_ranges(kind, f):
                where = (kind, version, f, steps, v, (t0, t1))
                plan = FR.frame_plan(kind, w, h, f, T.LANE_SYMBOLS, t0, t1)
                assert (plan["a"], plan["b"]) == FR.frame_window(kind, f, t0, t1)
                got = ch.dev_frames(t0, t1).cpu().numpy()
                assert np.array_equal(got, full[t0 * n:t1 * n]), (where, _mismatch(got, full[t0 * n:t1 * n]))
                _check_stats(a, plan, t1 - t0, 0)
                host = np.asarray(a.decode_frames(blob, t0, t1 - t0))
                assert np.array_equal(host, full[t0 * n:t1 * n]), (where, _mismatch(host, full[t0 * n:t1 * n]))
                _check_stats(a, plan, t1 - t0, ch.planned_bytes(plan))
                reached.add(T.window_class(kind, f, t0, t1))
                if (plan["b"] - plan["a"]) // 2 >= 8:
                    _ran.add((f"win{version}", kind, v))
            assert np.array_equal(ch.alc_view.cpu().numpy(), np.frombuffer(blob, np.uint8)), "the container was modified"
    assert reached == set(T.INVERSE_CLASSES)
    _done.add(("f", kind, version))


# ---- after the module: every instance ran inside its steady loop ----
def expected_instances():
    """Forward: NS x STEP1 of the u8 and of the wide kernel (CDF 5/3 and Haar share NS = 2, with coefficients of their own),
    NS of the bins.  Inverse: the instance classes of every wavelet for the u8, the wide and the mirrored kernel and for the
    window twin of each."""
    out = set()
    for kind in T.KINDS:
        out |= {(fam, kind, step1) for fam in ("fwd_u8", "fwd_wide") for step1 in (True, False)}
        out.add(("bins", kind, None))
        out |= {(fam, kind, v) for fam in ("inv_u8", "win2") for v in T.expected_classes(kind, 0)}
        out |= {(fam, kind, v) for fam in ("inv_wide", "inv_mirror", "win3", "win4") for v in T.expected_classes(kind, 1)}
    return out


def test_every_instance_ran_inside_its_steady_loop(gpu_codec):
    """The class tables: 4 + 4 + 2 forward instances and 11 + 10 + 10 inverse classes, the latter once more through a
    window; and what ran in this process at a steady-loop frame count (when the tests above ran) is all of them."""
    lib = gpu_codec.load_library()
    want = expected_instances()
    ns = {T.CDF53: 2, T.CDF97: 4, T.HAAR: 2}
    assert len({(fam, ns[k], s) for fam, k, s in want if fam in ("fwd_u8", "fwd_wide")}) == 4 + 4
    assert len({ns[k] for fam, k, _ in want if fam == "bins"}) == 2
    for fam, n in (("inv_u8", 11), ("win2", 11), ("inv_wide", 10), ("inv_mirror", 10), ("win3", 10), ("win4", 10)):
        assert len({x for x in want if x[0] == fam}) == n, fam
    for kind in T.KINDS:
        for wide in (0, 1):
            assert {v for _, v in T.step_cases(lib, kind, wide)} == T.expected_classes(kind, wide)
    assert _ran <= want, sorted(_ran - want, key=str)
    if len(_done) == N_CASES:
        assert _ran == want, sorted(want - _ran, key=str)
    print(f"{len(want)} (family, wavelet, variant) combinations planned, {len(_ran)} ran inside the steady loop")
