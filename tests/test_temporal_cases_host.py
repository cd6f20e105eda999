"""CPU-only: the plan of tests/temporal_cases.py tests what it claims.  The frame counts reach every frame-count class of the
forward and of the inverse stream, each from an even and from an odd f; the class rule is the peeled loops' own arithmetic;
the window ranges reach every inverse class through the virtual chunk, for every wavelet and through every kind of window;
the step cases name every instance class; and the references the device tests compare with agree with each other where
they must."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frames_ref as FR  # noqa: E402
import oracle.alice_oracle_np as o  # noqa: E402
import reversible_ref as RR  # noqa: E402
import split_ref as R2  # noqa: E402
import temporal_cases as T  # noqa: E402
import transform_extremes as X  # noqa: E402
import wide_ref as R3  # noqa: E402
from slab_oracle_stages import OracleStages  # noqa: E402


# ---- the frame counts ----
def test_frames_reach_every_class_at_both_parities():
    assert T.FRAMES == list(range(1, 27)) + [33, 34, 39, 40] and len(T.FRAMES) == 30
    fwd = {(T.forward_class(T.half_of(f)), f & 1) for f in T.FRAMES}
    inv = {(T.inverse_class(T.half_of(f)), f & 1) for f in T.FRAMES}
    assert len(T.FORWARD_CLASSES) == 14 and len(T.INVERSE_CLASSES) == 13
    assert fwd == {(c, p) for c in T.FORWARD_CLASSES for p in (0, 1)} and len(fwd) == 28
    assert inv == {(c, p) for c in T.INVERSE_CLASSES for p in (0, 1)} and len(inv) == 26
    assert {T.half_of(f) for f in T.FRAMES_WIDE} == {9, 13} and set(T.FRAMES_WIDE) <= set(T.STEADY_FRAMES)
    assert {(T.forward_class(T.half_of(f))[0], T.inverse_class(T.half_of(f))[0]) for f in T.FRAMES_WIDE} == {(1, 1), (2, 2)}
    assert T.STEADY_FRAMES == [17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 33, 34, 39, 40]


def _walk(half, forward):
    """The peeled loop as the kernels write it, counting ticks: (ticks of the first block, steady blocks, tail ticks)"""
    first = sum(1 for u in range(4) if u < half)
    kb, steady = 4, 0
    while kb + 4 <= (half - 1 if forward else half):
        steady += 1
        kb += 4
    tail = 0
    while kb < half:          # the inverse's tail is one block of at most three ticks; the forward's may take two trips
        tail += sum(1 for u in range(4) if kb + u < half)
        kb += 4
    return first, steady, tail


def test_the_class_rule_is_the_loops_arithmetic():
    for half in range(1, 200):
        for forward, rule in ((True, T.forward_class), (False, T.inverse_class)):
            first, steady, tail = _walk(half, forward)
            assert first + 4 * steady + tail == half
            if half <= 4:
                assert rule(half) == ("short", half) and (first, steady, tail) == (half, 0, 0)
            else:
                assert rule(half) == (min(steady, 2), tail), (half, forward)
                assert (1 <= tail <= 4) if forward else (0 <= tail <= 3)
    # the table of DESIGN.md section 4
    assert [T.forward_class(h)[0] for h in range(5, 10)] == [0, 0, 0, 0, 1]
    assert [T.inverse_class(h)[0] for h in range(5, 9)] == [0, 0, 0, 1]
    assert T.half_of(17) == 9 and T.half_of(15) == 8 and T.half_of(64) == 32


def test_the_shapes_are_what_they_are_for():
    w, h = T.SHAPE
    assert min(w, h) >= 6 and w % 2 == 0 and h % 2 == 0 and w * h // 4 == 30 < 64
    w, h = T.SHAPE_WIDE
    groups = w * h // 4
    assert w * h % 4 == 0 and -(-groups // 256) == 3 and groups % 256 != 0     # three workgroups, the last one partial
    assert h > 32 and w < 96                                                   # two inverse tile rows: a seam
    assert len(T.shapes()) == 34


# ---- the steps ----
@pytest.mark.parametrize("kind", T.KINDS)
def test_the_step_cases_name_every_instance_class(codec, kind):
    lib = codec.load_library()
    for wide in (0, 1):
        steps = T.class_steps(lib, kind, wide)
        assert {v for _, v in steps} == T.expected_classes(kind, wide) and len(steps) == len(T.expected_classes(kind, wide))
        for (s, v), (cv, first, last) in zip(steps, X.classes(lib, kind, wide)):
            assert v == cv and first <= s <= last
        cases = T.step_cases(lib, kind, wide)
        assert len(set(cases[-1][0])) == min(3, len(steps))          # a different class step in each channel


# ---- the windows ----
@pytest.mark.parametrize("kind", T.KINDS)
def test_window_ranges_reach_every_inverse_class(kind):
    reached, kinds_long = {}, {}
    for f in T.WINDOW_FRAMES:
        for t0, t1 in T.window_ranges(kind, f):
            assert 0 <= t0 < t1 <= f
            c = T.window_class(kind, f, t0, t1)
            reached.setdefault(c, []).append((f, t0, t1))
            if f >= 26:
                kinds_long.setdefault(c, set()).add(T.window_kind(kind, f, t0, t1))
    assert set(reached) == set(T.INVERSE_CLASSES), set(T.INVERSE_CLASSES) - set(reached)
    for f in (26, 33, 40):
        assert {T.window_kind(kind, f, *r) for r in T.window_ranges(kind, f)} == T.WINDOW_KINDS, f
        assert {(0, 1), (f // 2, f // 2 + 1), (3, 9), (5, 17), (4, 20), (2, f - 3), (f - 20, f), (f - 1, f), (0, f)} <= set(T.window_ranges(kind, f))
    # a window clipped at neither end for every class such a window can have: one kept frame and its halo on both sides
    smallest = FR.LIFT_STEPS[kind] + 1
    for c in T.INVERSE_CLASSES:
        halves = [hf for hf in range(1, 21) if T.inverse_class(hf) == c]
        if max(halves) >= smallest and min(halves) <= 11:
            assert "neither_end" in kinds_long[c], (kind, c, kinds_long[c])
    # the steady loop of the window instances: entered at an even and an odd first kept frame
    steady = [(f, t0, t1) for c, rs in reached.items() if c[0] in (1, 2) for f, t0, t1 in rs]
    assert {(t0 - FR.frame_window(kind, f, t0, t1)[0]) & 1 for f, t0, t1 in steady} == {0, 1}
    print(f"{T.NAMES[kind]}: {sum(len(r) for r in reached.values())} ranges, per class {({c: len(r) for c, r in reached.items()})}")


# ---- the references ----
@pytest.mark.parametrize("kind", T.KINDS)
def test_the_mirrored_round_trip_returns_the_input_at_every_frame_count(kind):
    w, h = T.SHAPE
    for f in T.FRAMES:
        rgb = T.random_rgb(w, h, f)
        assert np.array_equal(RR.roundtrip(rgb, w, h, f, 100, kind), rgb), (kind, f)


@pytest.mark.parametrize("kind", T.KINDS)
def test_the_numpy_inverse_is_the_oracles_on_byte_symbols(kind):
    """transform_extremes.inverse_quantised_steps (the reference of the wide containers) against the CPU oracle's decoder
    (the reference of the u8 symbols), on the plan's u8 volumes above 16 frames"""
    w, h = T.SHAPE
    for f, steps in ((17, (1, 1, 1)), (26, (3, 9, 2)), (33, (20, 1, 7)), (40, (70000, 2, 1))):
        sym = T.byte_symbols(kind, w, h, f)
        qs = [o.from_symbols(sym[c].reshape(-1)) for c in range(3)]
        want = OracleStages().inverse_symbols(torch.from_numpy(np.array(sym)), w, h, f, kind, list(steps)).numpy().reshape(-1)
        assert np.array_equal(X.inverse_quantised_steps(qs, steps, T.dims(w, h, f), w, h, f, kind), want), (kind, f)
        assert np.array_equal(T.byte_reference(kind, w, h, f, steps), want)


def test_the_containers_hold_the_volumes():
    kind, (w, h), f = T.CDF97, T.SHAPE, 33
    for version, steps in ((2, (11, 1, 2)), (3, (2, 1, 2)), (4, (2, 1, 2))):
        blob = T.container(kind, w, h, f, version, steps)
        assert blob[4] == version
        info, syms = R2.decode_container(blob) if version == 2 else R3.decode_container(RR.with_version(blob, 3))
        assert info["step"] == list(steps) and info["lane_symbols"] == T.LANE_SYMBOLS and info["frames"] == f
        want = T.byte_symbols(kind, w, h, f).reshape(3, -1) if version == 2 else T.wide_symbols(kind, w, h, f)
        assert all(np.array_equal(s, z) for s, z in zip(syms, want))
    assert int(max(z.max() for z in T.wide_symbols(kind, w, h, f))) == 4350
    assert int(T.byte_symbols(kind, w, h, f).max()) == 255
    full = T.reference(kind, w, h, f, 4, (2, 1, 2))
    assert not np.array_equal(full, T.reference(kind, w, h, f, 3, (2, 1, 2)))      # the two inverses are told apart
