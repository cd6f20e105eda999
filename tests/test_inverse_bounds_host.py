"""Which instance of the inverse transform a decode picks (csrc/codec.hip, inverse_bounds, read through
alice_codec_test_inverse_variant), without a device: the class table, its monotonicity, the worst channel deciding, and the
soundness of every class against the reference arithmetic on the volumes that drive the inverse highest
(tests/transform_extremes.py).  Variants: 0 exact, 1 fast i32, 2 fast with an i16 band slot, 3 that and the packed i16 tile."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import transform_extremes as X  # noqa: E402

CDF53, CDF97, HAAR = 0, 1, 2
NAMES = {CDF53: "CDF 5/3", CDF97: "CDF 9/7", HAAR: "Haar"}
STEPS = np.arange(1, 401)
DIMS = (8, 16, 16)     # (pf, ph, pw): the gains of a pass do not depend on the length from 4 samples on

# First quantiser step of each class, (packed i16 tile, i16 slot, fast i32, exact); None: the wavelet has no such class.
# THIS TABLE IS THE RULE OF THE COMMIT BEFORE THE HOOK EXISTED (a port of its inverse_bounds() evaluated for every step):
# a change of inverse_bounds() that moves a step into another class has to change it here, on purpose.
FIRST_STEP = {
    (0, CDF53): (1, 51, 114, 324), (0, CDF97): (1, 12, None, 37), (0, HAAR): (1, 41, 103, 219),
    (1, CDF53): (1, 3, 7, 20), (1, CDF97): (None, 1, None, 3), (1, HAAR): (1, 3, 7, 13),
}
CASES = [(wide, kind) for wide in (0, 1) for kind in (CDF53, CDF97, HAAR)]


def variant(lib, kind, steps, wide):
    s = (C.c_int32 * 3)(*[int(v) for v in steps])
    return lib.alice_codec_test_inverse_variant(kind, s, wide)


def expected_variants(wide, kind):
    want = np.zeros(STEPS.size, np.int64)
    for v, first in zip((3, 2, 1, 0), FIRST_STEP[(wide, kind)]):
        if first is not None:
            want[STEPS >= first] = v
    return want


@pytest.fixture(scope="module")
def lib(codec):
    return codec.load_library()


@pytest.mark.parametrize("wide,kind", CASES)
def test_class_table_is_the_parent_rule(lib, wide, kind):
    got = np.array([variant(lib, kind, (s, s, s), wide) for s in STEPS])
    want = expected_variants(wide, kind)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (NAMES[kind], wide, [(int(STEPS[i]), int(got[i]), int(want[i])) for i in bad[:8]])
    assert np.all(np.diff(got) <= 0), "a larger step may only move towards the exact instance"


@pytest.mark.parametrize("wide,kind", CASES)
def test_the_worst_channel_decides_and_the_sign_does_not(lib, wide, kind):
    for first in FIRST_STEP[(wide, kind)]:
        if first is None:
            continue
        for s in {max(first - 1, 1), first}:
            v = variant(lib, kind, (s, s, s), wide)
            for triple in ((s, 1, 1), (1, s, 1), (1, 1, s), (-s, s, s), (-s, -s, -s), (1, -s, 1), (1, 1, -s)):
                assert variant(lib, kind, triple, wide) == v, (NAMES[kind], wide, triple)
    assert variant(lib, CDF53, (1, 1, 323), 0) == variant(lib, CDF53, (323, 323, 323), 0) == 1


def test_the_ends_of_the_step_range_are_exact_and_unknown_wavelets_are_refused(lib):
    for kind in (CDF53, CDF97, HAAR):
        for wide in (0, 1):
            for s in (2**31 - 1, -2**31):
                assert variant(lib, kind, (s, s, s), wide) == 0
                assert variant(lib, kind, (1, s, 1), wide) == 0
    assert variant(lib, 3, (1, 1, 1), 0) == -1 and variant(lib, 255, (1, 1, 1), 1) == -1


# ---- soundness against the reference arithmetic ----
I16_MAX = 32767
PAIR_LIMIT = 1 << 22     # a value below 2^22 in magnitude: the sum of two fits the 24-bit multiply's signed operand


def violations(v, maxima):
    """What instance `v` may not do with values this large.  maxima: (input, after temporal, after column, after row)."""
    m_in, m_t, m_c, m_r = maxima
    bad = []
    if v >= 2 and m_t > I16_MAX:
        bad.append(f"i16 band slot holds {m_t}")
    if v == 3 and m_c > I16_MAX:
        bad.append(f"packed i16 tile holds {m_c}")
    if v >= 1 and max(m_in, m_t, m_c, m_r) >= PAIR_LIMIT:
        bad.append(f"a pair sum of values up to {max(m_in, m_t, m_c, m_r)} leaves 24 bits")
    return bad


_maxima = {}


def worst_maxima(wide, kind):
    """Per step 1 .. 400: (input, after temporal, after column, after row) maxima of the inverse of the worst-sign volume
    whose every coefficient is +-max_q * step, the premise of the bound (the u8 symbol volumes stop at -127)."""
    if (wide, kind) not in _maxima:
        max_q = X.WIDE_MAX_Q if wide else X.BYTE_MAX_Q
        signs = X.worst_volume(kind, DIMS)
        coef = signs[..., None] * (max_q * STEPS)[None, None, None, :]
        _maxima[(wide, kind)] = (max_q * STEPS,) + X.per_pass_maxima(kind, coef)
    return _maxima[(wide, kind)]


@pytest.mark.parametrize("wide,kind", CASES)
def test_every_class_is_sound_on_the_worst_volume(lib, wide, kind):
    m = worst_maxima(wide, kind)
    top = {}
    for i, s in enumerate(STEPS):
        v = variant(lib, kind, (s, s, s), wide)
        here = tuple(int(a[i]) for a in m)
        assert not violations(v, here), (NAMES[kind], "wide" if wide else "u8", int(s), v, violations(v, here))
        top[v] = (int(s),) + here[1:]
    for v in sorted(top, reverse=True):    # shown with -s: the largest values each instance is handed
        print(f"{NAMES[kind]} {'wide' if wide else 'u8'} variant {v}: last step {top[v][0]}, maxima after temporal / column / row {top[v][1:]}")


def test_the_soundness_check_bites(lib):
    """Step 323 of CDF 5/3 is the last of the fast i32 class: treated as an i16-slot class it must be reported."""
    m = worst_maxima(0, CDF53)
    here = tuple(int(a[322]) for a in m)
    assert variant(lib, CDF53, (323, 323, 323), 0) == 1 and not violations(1, here)
    assert violations(2, here) and violations(3, here)
    here = tuple(int(a[63]) for a in m)     # step 64: 4 * 128 * 64 = 32768 after the column pass, one past i16
    assert here[2] == 32768 and not violations(2, here) and violations(3, here)
    assert violations(1, (PAIR_LIMIT, 0, 0, 0)) and not violations(0, (1 << 40,) * 4)


# ---- teeth: the inputs are as extreme as claimed ----
# (wavelet, step) -> maxima after the temporal / column / row pass of the reference inverse, every coefficient +-128 * step
TABLE = {
    (CDF53, 50): (12800, 25600, 51200),       # last step of the packed tile
    (CDF53, 113): (28928, 57856, 115712),     # last of the i16 slot
    (CDF53, 323): (82688, 165376, 330752),    # last of fast i32
    (HAAR, 102): (26112, 52224, 104448),
    (HAAR, 218): (55808, 111616, 223232),
}


@pytest.mark.parametrize("kind,step", sorted(TABLE))
def test_the_worst_volumes_reach_the_stated_maxima(kind, step):
    """Guards the pattern generator, not the kernels: if the volumes stop being extreme this fails first."""
    want = TABLE[(kind, step)]
    assert want == (256 * step, 512 * step, 1024 * step)     # gain 2.0 per pass on 128 * step
    for centre in (None, (5, 9, 9)):
        signs = X.worst_volume(kind, DIMS, centre)
        assert X.per_pass_maxima(kind, signs * (128 * step)) == want, centre
        # the u8 symbols of the same signs: 255 -> +128 but 254 -> -127, so between 127/128 of the table and the table
        q = X.o.from_symbols(X.byte_symbols(signs))
        assert int(q.max()) == 128 and int(q.min()) == -127
        got = X.per_pass_maxima(kind, X.dequantised(q, step))
        for g, t in zip(got, want):
            assert t * 127 // 128 - 8 <= g <= t, (got, want)
        # the maximum is where worst_position says
        t, y, x = X.worst_position(kind, DIMS, centre)
        vol = X.o.wavelet3d(kind, X.dequantised(q, step), DIMS[2], DIMS[1], DIMS[0], inverse=True).reshape(DIMS)
        assert abs(int(vol[t, y, x])) == got[2]
    assert got[0] > I16_MAX or step <= 113       # the fast i32 rows leave i16 after the temporal pass already
    assert got[1] > I16_MAX or step <= 50


def test_the_measured_gains():
    """2.0 / 1.666 / 2.0 per inverse pass; CDF 9/7 stays far below the bound's 4.8 per pass (7678 / 12793 / 21317 at step 36)."""
    for n in (4, 8, 16, 70):
        assert X.pass_gain(CDF53, n) == pytest.approx(2.0, abs=1e-4) and X.pass_gain(HAAR, n) == pytest.approx(2.0, abs=1e-4)
    for n in (8, 16, 70):
        assert X.pass_gain(CDF97, n) == pytest.approx(1.666, abs=1e-3)
    assert X.per_pass_maxima(CDF97, X.worst_volume(CDF97, DIMS) * (128 * 36)) == (7678, 12793, 21317)
    for kind in (CDF53, CDF97, HAAR):      # the wide symbols carry +-2175 both ways
        q = X.from_wide(X.wide_symbols_extreme(X.worst_volume(kind, DIMS)))
        assert int(q.max()) == 2175 and int(q.min()) == -2175


def test_the_loud_random_volumes_hold_every_magnitude():
    b = X.o.from_symbols(X.loud_random_bytes((4, 70, 200), 1))
    assert set(np.unique(np.abs(b))) == {0, 1, 64, 127, 128} and int(b.min()) == -127 and int(b.max()) == 128
    w = X.from_wide(X.loud_random_wide((4, 70, 200), 1))
    assert set(np.unique(w)) == {0, 1, -1, 1087, -1087, 2174, -2174, 2175, -2175}
