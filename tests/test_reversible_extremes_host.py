"""CPU-only: the plan of tests/reversible_extreme_cases.py tests what it claims.  Its worst-sign volumes hand every class of
the mirrored inverse the magnitudes the class table is about, at every shape of the plan; every class
of every (wavelet, shape) has a case whose mirrored decode differs from the reference inverse's decode of the same bytes, so
that a device test can tell which inverse ran; and the contents at the top of the forward range come back exactly."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reversible_extreme_cases as P  # noqa: E402
import reversible_ref as RR  # noqa: E402
import transform_extremes as X  # noqa: E402
import wide_oracle as WO  # noqa: E402
import wide_ref as R3  # noqa: E402

I16_MAX = 32767
OPERAND_LIMIT = 1 << 23    # |a + b| < 2^23: the signed 24-bit operand of v_mad_i32_i24
PRODUCT_LIMIT = 1 << 31    # |v| + 4096 < 2^31


@pytest.mark.parametrize("kind", P.KINDS)
def test_the_plan_has_the_class_edges(codec, kind):
    lib = codec.load_library()
    cases = P.step_cases(lib, kind)
    assert [s[0] for s, _ in P.edge_steps(lib, kind)] == P.EDGE_STEPS[kind]
    assert {v for _, v in cases} == P.EXPECTED_CLASSES[kind]
    v, _, top = P.classes(lib, kind)[-2]
    assert top == {P.CDF53: 19, P.CDF97: 2, P.HAAR: 12}[kind] and v == min(P.EXPECTED_CLASSES[kind] - {0})
    for steps in ((top, 1, 2), (2, top, 1), (1, 2, top)):
        assert (steps, v) in cases and P.variant(lib, kind, steps) == v
    for steps, v in cases:
        assert P.variant(lib, kind, steps) == v


@pytest.mark.parametrize("shape", list(P.SHAPES))
@pytest.mark.parametrize("kind", P.KINDS)
def test_worst_volumes_reach_the_class_bounds_and_stay_inside(codec, kind, shape):
    """Each shape's worst volume -- the plan's channels carry it with both signs -- at the last step of each class: the
    mirrored maxima after the temporal, column and row pass are the reference inverse's, and lie inside what the class
    assumes.  Per sign the temporal and column maxima (what the i16 classes store) are equal everywhere; the row-pass maxima
    of the two signs trade places at 104x40x1 with CDF 5/3 (a single padded frame has a temporal gain of 1.75, so the values
    turn odd and the two roundings part: 30448 / 30452 at step 2, 91348 / 91352 at step 6), so the row pass is compared over
    the volume's channels, which hold both signs."""
    lib = codec.load_library()
    last = P.last_steps(lib, kind)
    assert [s for _, s in last] == P.EDGE_STEPS[kind][1:-1:2]
    signs = P.worst_signs(kind, shape)
    coef = np.stack([X.dequantised(sign * signs * X.WIDE_MAX_Q, s) for _, s in last for sign in (1, -1)], axis=-1)
    mirrored, pair, prod = RR.per_pass_mirror(kind, coef)
    ref = X.per_pass_maxima(kind, coef)
    for j, (v, s) in enumerate(last):
        for i in (2 * j, 2 * j + 1):
            m_t, m_c, m_r = (int(m[i]) for m in mirrored)
            print(f"{P.NAMES[kind]} {shape} class {v} step {s} sign {'+-'[i & 1]}: mirrored maxima {m_t} / {m_c} / {m_r}, "
                  f"reference {ref[0][i]} / {ref[1][i]} / {ref[2][i]}, neighbour sum {pair[i]}, |sum * c| + 4096 {prod[i]}")
            assert (m_t, m_c) == (ref[0][i], ref[1][i]), (P.NAMES[kind], shape, v, s)
            assert pair[i] < OPERAND_LIMIT and prod[i] < PRODUCT_LIMIT
            if v >= 2:
                assert m_t <= I16_MAX          # the i16 band slot
            if v == 3:
                assert m_c <= I16_MAX          # the packed i16 tile
            assert m_t > X.WIDE_MAX_Q * s      # the signs are the worst ones: every pass has a gain above 1
        both = slice(2 * j, 2 * j + 2)
        assert [int(m[both].max()) for m in mirrored] == [int(m[both].max()) for m in ref], (P.NAMES[kind], shape, v, s)


@pytest.mark.parametrize("shape", list(P.SHAPES))
@pytest.mark.parametrize("kind", P.KINDS)
def test_every_class_has_a_case_that_tells_the_two_inverses_apart(codec, kind, shape):
    """A condition on the plan, not a tolerance: per class, at least one case whose mirrored decode is not the reference
    inverse's.  A case with a count of 0 stays in the plan as a magnitude case."""
    lib = codec.load_library()
    best = {}
    for name, steps, v in P.cases(lib, kind, shape):
        n = P.differing_pixels(kind, shape, name, steps)
        print(f"{P.NAMES[kind]} {shape} class {v} steps {steps} {name}: {n} pixels differ from the reference inverse")
        best[v] = max(best.get(v, 0), n)
    assert set(best) == P.EXPECTED_CLASSES[kind]
    assert all(n > 0 for n in best.values()), (P.NAMES[kind], shape, best)


def test_the_references_are_the_two_numpy_inverses():
    """the per-channel planes the plan shares assemble to reversible_ref.inverse_quantised / inverse_quantised_steps"""
    kind, shape, steps = P.CDF97, (3, 40, 4), (2, 1, 2)
    w, h, f = shape
    dims = R3.padded_dims(w, h, f)
    for name, z in P.volumes(kind, shape).items():
        qs = [R3.from_wide_symbols(zz) for zz in z]
        assert np.array_equal(P.reference(kind, shape, name, steps), RR.inverse_quantised(qs, steps, dims, w, h, f, kind))
        assert np.array_equal(P.reference(kind, shape, name, steps, False), X.inverse_quantised_steps(qs, steps, dims, w, h, f, kind))
        blob = P.container(kind, shape, name, steps, 4)
        assert blob[4] == 4 and np.array_equal(RR.decode(blob), P.reference(kind, shape, name, steps))
        assert int(max(zz.max() for zz in z)) in (4349, 4350)


@pytest.mark.parametrize("pair", list(P.PAIRS))
@pytest.mark.parametrize("kind", P.KINDS)
def test_lossless_at_the_top_of_the_forward_range(kind, pair):
    """Co (Cg) = +-255 with the forward's worst signs: |coefficient| 2040 (1177 for CDF 9/7), z = 4079 / 4080."""
    w, h, f = P.DEVICE_SHAPE
    rgb = P.top_of_range_content(kind, pair)
    step, _, qs = WO.forward_quantised(RR.o, rgb, w, h, f, 100, kind)
    ch = P.PAIRS[pair][2]
    assert step == 1 and int(np.abs(qs[ch]).max()) == P.FORWARD_TOP[kind]
    assert max(int(np.abs(q).max()) for q in qs) <= X.WIDE_MAX_Q
    assert np.array_equal(RR.roundtrip(rgb, w, h, f, 100, kind), rgb)
