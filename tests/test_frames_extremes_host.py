"""CPU-only: the plan of tests/frames_extreme_cases.py tests what it claims.  The window rule holds at the
magnitudes where i32 wrapping and the rounding of the lifting steps matter, for both inverses; the virtual chunks -- their halo
frames, which carry the wrong extension at an interior window end, included -- stay inside what each instance class assumes
at the last step of that class; the plan reaches every (format, wavelet, class) triple through every kind of window; and
every class of the wide formats has a planned case on which the mirrored and the reference inverse differ inside the kept
frames, so that a device test can tell which one ran."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frames_extreme_cases as F  # noqa: E402
import frames_ref as FR  # noqa: E402
import reversible_ref as RR  # noqa: E402
import split_ref as R2  # noqa: E402
import transform_extremes as X  # noqa: E402
import wide_ref as R3  # noqa: E402
from test_inverse_bounds_host import violations  # noqa: E402

I16_MAX = 32767
OPERAND_LIMIT = 1 << 23    # |a + b| < 2^23: the signed 24-bit operand of v_mad_i32_i24 (the mirrored instances)
PRODUCT_LIMIT = 1 << 31    # |v| + 4096 < 2^31
IDS = [F.case_id(c) for c in F.CASES]


def _windows(kind, shape):
    """{(a, b): [(t0, t1)]} of the plan's ranges"""
    out = {}
    for t0, t1 in F.ranges(kind, shape):
        out.setdefault(FR.frame_window(kind, shape[2], t0, t1), []).append((t0, t1))
    return out


# ---- B.1 the window rule at the plan's magnitudes ----
@pytest.mark.parametrize("case", F.CASES, ids=IDS)
def test_window_rule_at_the_class_edges(codec, case):
    """Versions 2 and 3 through the reference's inverse (u8 and wide symbols), version 4 through the mirrored one: the
    inverse of the virtual chunk at [t0 - a, t1 - a) is the full inverse's frames [t0, t1), for every volume, every channel
    at every step the step cases give it, and every range."""
    shape, kind, version = case
    lib = codec.load_library()
    mirrored = version == 4
    pf = F.dims(shape)[2]
    windows = _windows(kind, shape)
    steps_of = [sorted({steps[c] for steps, _ in F.step_cases(lib, kind, version)}) for c in range(3)]
    compared = 0
    for name in F.volumes(kind, shape, version):
        for c in range(3):
            if name == "worst" and c == 2:
                continue        # channel 0's symbols; the step sets of the two channels are the same
            for step in sorted(set(steps_of[c]) | set(steps_of[2] if name == "worst" and c == 0 else ())):
                full = F.plane(kind, shape, version, name, c, step, mirrored)
                for (a, b), rs in windows.items():
                    virt = full if (a, b) == (0, pf) else F.window_plane(kind, shape, version, name, c, step, mirrored, a, b)
                    for t0, t1 in rs:
                        assert np.array_equal(virt[t0 - a:t1 - a], full[t0:t1]), (case, name, c, step, (t0, t1), (a, b))
                        compared += 1
    print(f"{F.case_id(case)}: {compared} (volume, channel, step, range) comparisons, {len(windows)} windows")
    assert compared >= 5 * len(steps_of[0]) * len(F.ranges(kind, shape))


# ---- B.2 the virtual chunks stay inside what their class assumes ----
@pytest.mark.parametrize("case", F.CASES, ids=IDS)
def test_virtual_chunks_stay_inside_their_class(codec, case):
    """At the last step of each class that assumes something: the per-pass maxima over ALL frames of the virtual chunk of
    every planned window, for every volume and channel.  Bounds as tests/test_inverse_bounds_host.py (reference inverse) and
    tests/test_reversible_extremes_host.py (mirrored inverse) state them.  A window that leaves a bound the full chunk
    keeps is a finding about the class table, not a case to drop."""
    shape, kind, version = case
    lib = codec.load_library()
    pw, ph, pf = F.dims(shape)
    last = F.last_steps(lib, kind, version)
    vols = F.volumes(kind, shape, version)
    chans = [(name, c) for name in vols for c in range(3) if not (name == "worst" and c == 2)]
    q = np.stack([F.quantised(vols[name][c], version).astype(np.int64) for name, c in chans], axis=-1)     # (n, k)
    max_q = X.WIDE_MAX_Q if version != 2 else X.BYTE_MAX_Q
    assert int(np.abs(q).max()) == max_q
    top = {}
    for a, b in _windows(kind, shape):
        qv = np.stack([FR.window_volume(q[:, i], (pw, ph, pf), a, b) for i in range(len(chans))], axis=-1)
        for v, s in last:
            assert F.variant(lib, kind, (s, s, s), version) == v
            coef = X.dequantised(qv, s)
            if version == 4:
                (m_t, m_c, m_r), pair, prod = RR.per_pass_mirror(kind, coef)
            else:
                m_t, m_c, m_r = X.per_pass_maxima(kind, coef)
            for i, ch in enumerate(chans):
                where = (case, (a, b), v, s, ch)
                if version == 4:
                    assert pair[i] < OPERAND_LIMIT and prod[i] < PRODUCT_LIMIT, where
                    assert v < 2 or m_t[i] <= I16_MAX, (where, int(m_t[i]))
                    assert v < 3 or m_c[i] <= I16_MAX, (where, int(m_c[i]))
                else:
                    bad = violations(v, (max_q * s, int(m_t[i]), int(m_c[i]), int(m_r[i])))
                    assert not bad, (where, bad)
            old = top.get((v, s), (0, 0, 0))
            top[(v, s)] = tuple(max(o_, int(m.max())) for o_, m in zip(old, (m_t, m_c, m_r)))
    for (v, s), m in top.items():
        print(f"{F.case_id(case)} class {v} last step {s}: largest maxima after temporal / column / row over the windows {m}")
        assert m[0] > max_q * s       # the volumes are loud: a pass gains


# ---- B.3 every triple through every kind of window ----
def test_the_plan_reaches_every_triple_through_every_kind_of_window(codec):
    lib = codec.load_library()
    reached, at_edges = {}, {}
    for shape, kind, version in F.CASES:
        if not F.tile_eligible(shape):
            continue
        edges = F.class_edges(lib, kind, version)
        for steps, v in F.step_cases(lib, kind, version):
            assert F.variant(lib, kind, steps, version) == v
            for t0, t1 in F.ranges(kind, shape):
                kinds = F.range_classes(kind, shape, t0, t1)
                reached.setdefault((version, kind, v), set()).update(kinds)
                if steps in edges[v]:
                    at_edges.setdefault((version, kind, v, steps), set()).update(kinds)
    want = {(version, kind, v) for version in F.VERSIONS for kind in F.KINDS for v in F.EXPECTED[version][kind]}
    assert len(want) == 11 + 10 + 10 and set(reached) == want
    for key, kinds in reached.items():
        assert kinds == F.WINDOW_KINDS, (key, F.WINDOW_KINDS - kinds)
    for version in F.VERSIONS:
        for kind in F.KINDS:
            for v, edge in F.class_edges(lib, kind, version).items():
                for steps in edge:      # the first and the last step of the class, each through all four kinds of window
                    assert at_edges.get((version, kind, v, steps)) == F.WINDOW_KINDS, (version, kind, v, steps)


def test_the_shapes_are_what_they_are_for():
    assert [F.tile_eligible(s) for s in F.SHAPES] == [True, True, False, True]
    for shape in F.SHAPES:
        for kind in F.KINDS:
            T, f = F.centre_frame(kind, shape), shape[2]
            assert abs(T - F.dims(shape)[2] // 2) <= 2, (shape, kind, T)
            rs = F.ranges(kind, shape)
            assert {(T, T + 1), (T + 1, T + 2), (T - 1, T + 2)} <= set(rs) and set(FR.named_ranges(kind, f)) <= set(rs)
            firsts = {(t0 - FR.frame_window(kind, f, t0, t1)[0]) & 1 for t0, t1 in ((T, T + 1), (T + 1, T + 2))}
            assert firsts == {0, 1}       # the even and the odd put are each the first frame kept
            t = F.halo_only_frame(kind, shape)
            assert (t, t + 1) in rs
    assert "pad_frame" in FR.frame_plan(F.CDF97, 99, 37, 13, 64, 12, 13)["classes"]


# ---- B.4 the two inverses can be told apart inside the kept frames ----
@pytest.mark.parametrize("shape", [s for s in F.SHAPES if F.tile_eligible(s)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", F.KINDS)
def test_every_class_has_a_window_that_tells_the_two_inverses_apart(codec, kind, shape):
    """A condition on the plan, not a tolerance: per class, the number of planned (volume, steps, range) on which the
    mirrored decode of the kept frames is not the reference inverse's.  A case with a count of 0 stays in the plan."""
    lib = codec.load_library()
    telling, planned = {}, {}
    for name, steps, v in F.cases(lib, kind, shape, 4):
        for t0, t1 in F.ranges(kind, shape):
            n = F.differing_pixels(kind, shape, name, steps, t0, t1)
            planned[v] = planned.get(v, 0) + 1
            telling[v] = telling.get(v, 0) + (n > 0)
    print(f"{F.NAMES[kind]} {shape}: planned (volume, steps, range) per class {planned}, of which tell the inverses apart {telling}")
    assert set(telling) == F.P.EXPECTED_CLASSES[kind]
    assert all(n > 0 for n in telling.values()), (F.NAMES[kind], shape, telling)


# ---- the references and the containers are what they claim ----
def test_the_references_are_the_numpy_inverses_and_the_containers_hold_the_volumes():
    kind, shape = F.CDF97, (3, 40, 16)
    w, h, f = shape
    dims = F.dims(shape)
    for version, steps in ((2, (11, 1, 2)), (3, (2, 1, 2)), (4, (2, 1, 2))):
        for name, z in F.volumes(kind, shape, version).items():
            qs = [F.quantised(zz, version) for zz in z]
            full = (RR.inverse_quantised if version == 4 else X.inverse_quantised_steps)(qs, steps, dims, w, h, f, kind)
            assert np.array_equal(F.reference(kind, shape, version, name, steps, 0, f), full)
            assert np.array_equal(F.reference(kind, shape, version, name, steps, 5, 8), full[5 * w * h * 3:8 * w * h * 3])
            blob = F.container(kind, shape, name, steps, version)
            assert blob[4] == version
            info, syms = (R2.decode_container(blob) if version == 2 else R3.decode_container(RR.with_version(blob, 3)))
            assert info["step"] == list(steps) and info["lane_symbols"] == F.LANE_SYMBOLS
            assert all(np.array_equal(s, zz) for s, zz in zip(syms, z))
    assert int(max(zz.max() for zz in F.volumes(kind, shape, 3)["worst"])) == 4350
    assert set(np.unique(F.volumes(kind, shape, 2)["worst"][0])) == {254, 255}


# ---- C.3 / C.4: the lane-size and damage plans ----
def test_lane_size_plans_reach_the_block_classes_away_from_64():
    w, h, f = F.LANE_SHAPE
    seen = {}
    for version in F.VERSIONS:
        assert F.LANE_SIZES[version][-1] == (16384 if version == 2 else 8192)
        assert {F.lane_kind(version, L) for L in F.LANE_SIZES[version]} == set(F.KINDS)
        for L in F.LANE_SIZES[version]:
            assert L != 64 and (R2.lane_ok(L) if version == 2 else R3.lane_ok(L))
            kind = F.lane_kind(version, L)
            for r in F.lane_ranges(kind, f):
                for c in FR.frame_plan(kind, w, h, f, L, *r)["classes"]:
                    seen.setdefault((version, L), set()).add(c)
    for version in F.VERSIONS:
        sizes = F.LANE_SIZES[version]
        assert F.LANE_CLASSES <= set().union(*[seen[(version, L)] for L in sizes]), version
        assert {"short_last_block", "edge_inside_block", "shared_block"} <= seen[(version, 2048)]     # 3.75 blocks
        assert "one_block_channel" in seen[(version, sizes[-1])] and "blocks_skipped" in seen[(version, 128)]
        assert w * h * f < 64 * sizes[-1]       # the one block is partly filled: its lanes hold fewer than L symbols
    w, h, f = F.ESCAPE_SHAPE
    for L in F.ESCAPE_LANES:
        cls = set().union(*[FR.frame_plan(k, w, h, f, L, *r)["classes"] for k in F.KINDS for r in F.lane_ranges(k, f)])
        assert {"edge_inside_block", "blocks_skipped", "short_last_block"} <= cls, (L, cls)


def test_the_damage_ranges_have_the_classes_they_are_for():
    w, h, f = F.DAMAGE_SHAPE
    every = [FR.frame_plan(F.DAMAGE_KIND, w, h, f, 64, t0, t1)["classes"] for t0 in range(f) for t1 in range(t0 + 1, f + 1)]
    assert not any({"start_clipped", "end_clipped", "shared_block"} <= c for c in every)       # hence two ranges
    clipped = FR.frame_plan(F.DAMAGE_KIND, w, h, f, 64, *F.DAMAGE_CLIPPED)
    shared = FR.frame_plan(F.DAMAGE_KIND, w, h, f, 64, *F.DAMAGE_SHARED)
    skipping = FR.frame_plan(F.DAMAGE_KIND, w, h, f, 64, *F.DAMAGE_SKIPPING)
    assert {"start_clipped", "end_clipped", "edge_inside_block"} <= clipped["classes"]
    assert {"start_clipped", "shared_block", "short_last_block"} <= shared["classes"]
    assert {"start_clipped", "edge_inside_block", "blocks_skipped"} <= skipping["classes"] and skipping["planned"] == [1, 2, 3, 5, 6]
    assert (shared["a"], shared["b"]) == (2, 14) and shared["ranges"][0][1] // 4096 == shared["ranges"][1][0] // 4096 == 3
