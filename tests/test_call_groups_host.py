"""Calls of more than one group, the part that needs no device: the band slot of a decode group (group_scratch_bytes in
codec.hip through its hook), the group-size hook and its getter, and the plan of tests/test_gpu_call_groups.py held to its
claims on the CPU references alone (tests/group_cases.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import banded_ref as B5  # noqa: E402
import group_cases as G  # noqa: E402
import split_rate_ref as SR  # noqa: E402
import split_ref as R2  # noqa: E402
import transcode_ref as T  # noqa: E402
import wide_ref as W3  # noqa: E402

DEFAULT_BAND_KB = 1024 * 1024

# shape, band target in KiB, (bands are not reported) slot bytes of the i16 plan, of the i32 plan: plan_bands evaluated by hand
# (tile rows of 32, halo 4)
SLOTS = [
    ((256, 256, 16), 4096, 6_291_712, 3_539_200),                     # the i32 plan cuts four bands, the i16 plan none
    ((7680, 4320, 64), DEFAULT_BAND_KB, 1_061_683_456, 990_904_576),  # 13 bands against 27
    ((3840, 2160, 64), DEFAULT_BAND_KB, 813_957_376, 967_311_616),    # 4 against 7
    ((1920, 1080, 64), DEFAULT_BAND_KB, 796_262_656, 1_592_525_056),  # neither plan cuts
]


@pytest.fixture
def lib(codec):
    lib = codec.load_library()
    yield lib
    lib.alice_codec_test_set_tuning(DEFAULT_BAND_KB)
    lib.alice_codec_test_set_group_chunks(0)


@pytest.mark.parametrize("shape,band_kb,i16,i32", SLOTS)
def test_group_slot_covers_every_width_in_the_group(lib, shape, band_kb, i16, i32):
    lib.alice_codec_test_set_tuning(band_kb)
    one = {m: int(lib.alice_codec_test_inverse_scratch_bytes(*shape, m)) for m in (1, 0)}
    assert (one[1], one[0]) == (i16, i32)
    # a group of one width allocates exactly that width's slot, as it always has
    assert int(lib.alice_codec_test_group_scratch_bytes(*shape, 1, 0)) == i16
    assert int(lib.alice_codec_test_group_scratch_bytes(*shape, 0, 1)) == i32
    assert int(lib.alice_codec_test_group_scratch_bytes(*shape, 0, 0)) == i16        # an empty group: what all16 gave
    # a group of both holds either chunk's plan, and no more than the larger needs
    mixed = int(lib.alice_codec_test_group_scratch_bytes(*shape, 1, 1))
    assert mixed >= i16 and mixed >= i32 and mixed == max(i16, i32)


def test_the_i32_slot_alone_is_too_small_for_two_of_the_shapes(lib):
    """What the decodes allocated for a mixed group before group_scratch_bytes: inverse_scratch_bytes(d, false).  The i16
    chunk of such a group plans its own bands and needs more: 2 752 512 bytes more at 256x256x16 under a 4 MiB target,
    70 778 880 more at 8K x 64 under the default."""
    short = {}
    for shape, band_kb, i16, i32 in SLOTS:
        lib.alice_codec_test_set_tuning(band_kb)
        was = int(lib.alice_codec_test_inverse_scratch_bytes(*shape, 0))
        need = int(lib.alice_codec_test_inverse_scratch_bytes(*shape, 1))
        short[shape] = need - was
        assert int(lib.alice_codec_test_group_scratch_bytes(*shape, 1, 1)) >= need
    assert short[(256, 256, 16)] == 2_752_512 and short[(7680, 4320, 64)] == 70_778_880
    assert short[(3840, 2160, 64)] < 0 and short[(1920, 1080, 64)] < 0


def test_shapes_without_tiles_have_no_slot(lib):
    assert int(lib.alice_codec_test_group_scratch_bytes(*G.SHAPES["generic"], 1, 1)) == 0
    assert int(lib.alice_codec_test_group_scratch_bytes(0, 4, 4, 1, 1)) == 0


def test_group_sizes_at_the_default_and_under_a_cap(lib):
    hd = (1920, 1080, 64)
    default = [10, 5, 5]
    assert [int(lib.alice_codec_test_group_chunks(*hd, v)) for v in (2, 3, 4)] == default
    for shape in G.SHAPES.values():
        assert [int(lib.alice_codec_test_group_chunks(*shape, v)) for v in (2, 3, 4)] == [21845] * 3
    assert int(lib.alice_codec_test_group_chunks(*hd, 1)) == 0 and int(lib.alice_codec_test_group_chunks(*hd, 5)) == 0
    lib.alice_codec_test_set_group_chunks(3)
    assert [int(lib.alice_codec_test_group_chunks(*hd, v)) for v in (2, 3, 4)] == [3, 3, 3]
    assert int(lib.alice_codec_test_group_chunks(*G.SHAPES["tile"], 2)) == 3
    lib.alice_codec_test_set_group_chunks(1)
    assert int(lib.alice_codec_test_group_chunks(*hd, 3)) == 1
    lib.alice_codec_test_set_group_chunks(50)                       # never above what the call computes
    assert [int(lib.alice_codec_test_group_chunks(*hd, v)) for v in (2, 3, 4)] == default
    assert int(lib.alice_codec_test_group_chunks(*G.SHAPES["tile"], 2)) == 50
    lib.alice_codec_test_set_group_chunks(0xFFFFFFFF)
    assert int(lib.alice_codec_test_group_chunks(*G.SHAPES["tile"], 2)) == 21845
    lib.alice_codec_test_set_group_chunks(0)
    assert [int(lib.alice_codec_test_group_chunks(*hd, v)) for v in (2, 3, 4)] == default
    assert int(lib.alice_codec_test_group_chunks(*G.SHAPES["tile"], 4)) == 21845


# ---- the plan ----

def _distinct(values):
    values = list(values)
    return len(set(values)) == len(values)


def test_caps_cut_seven_chunks_into_ragged_groups():
    for cap in G.CAPS:
        groups = [min(cap, G.N - first) for first in range(0, G.N, cap)]
        assert len(groups) > 1 and groups[-1] == 1 and sum(groups) == G.N, cap
    assert G.BIG // G.VERDICT_CAP == 1 and G.BIG % G.VERDICT_CAP == 1       # inside the second of three groups


@pytest.mark.parametrize("shape", list(G.SHAPES))
def test_contents_and_qualities_differ(shape):
    assert _distinct(G.clip(shape, i).tobytes() for i in range(G.N))
    for version in (2, 3, 4):
        qs = G.QUALITIES[version]
        assert _distinct(SR.quality_to_step(q) for q in qs)
        assert SR.quality_to_step(qs[G.BIG]) == min(SR.quality_to_step(q) for q in qs)
        blobs = G.containers(version, shape)
        assert _distinct(blobs) and _distinct(len(b) for b in blobs), (version, [len(b) for b in blobs])
        assert all(len(blobs[G.BIG]) > len(b) for i, b in enumerate(blobs) if i != G.BIG)
        assert _distinct(G.pixels(version, shape, i, qs[i]).tobytes() for i in range(G.N))
        sse = [G.sse(version, shape, i, qs[i]) for i in range(G.N)]
        assert _distinct(sse), (version, sse)
        f = G.SHAPES[shape][2]
        for i in range(G.N):
            rows = G.frame_sse(version, shape, i, qs[i])
            assert rows.shape == (f,) and int(rows.sum()) == sse[i]
        if version == 2:        # the containers are what the reference decoders read back
            for i, b in enumerate(blobs):
                _, syms = R2.decode_container(b)
                assert all(np.array_equal(s, z) for s, z in zip(syms, G.symbols(2, shape, i, SR.quality_to_step(qs[i]))))


def test_quality_lists_take_inverse_instances_on_both_sides_of_two(codec):
    lib = codec.load_library()
    for version, qs in list(G.QUALITIES.items()) + [(v, G.MIXED_QUALITIES[v]) for v in G.MIXED_QUALITIES]:
        kind = G.KIND[version] if len(qs) == G.N else G.MIXED_KIND
        wide = int(version >= 3)

        def variant(step):
            return int(lib.alice_codec_test_inverse_variant(kind, (C.c_int32 * 3)(step, step, step), wide))

        possible = {variant(s) >= 2 for s in range(1, 65)}
        got = {variant(SR.quality_to_step(q)) >= 2 for q in qs}
        assert got == possible, (version, kind, qs)
        assert len(possible) == 2, (version, kind)                # every (version, wavelet) of the plan has both
    for version, (q16, q32) in G.MIXED_QUALITIES.items():         # and the mixed pairs are (i16, i32) in this order
        wide = int(version >= 3)
        v16, v32 = (int(lib.alice_codec_test_inverse_variant(G.MIXED_KIND, (C.c_int32 * 3)(*[SR.quality_to_step(q)] * 3), wide)) for q in (q16, q32))
        assert v16 >= 2 > v32 >= 0, (version, v16, v32)


@pytest.mark.parametrize("shape", list(G.SHAPES))
@pytest.mark.parametrize("version", [2, 3])
def test_brackets_and_budget_choices_differ_and_stay_within_the_trials(version, shape):
    los = [G.brackets(version, shape, i)[0].tobytes() for i in range(G.N)]
    his = [G.brackets(version, shape, i)[1].tobytes() for i in range(G.N)]
    assert _distinct(los) and _distinct(his)
    assert _distinct(G.step_hists(version, shape, i).tobytes() for i in range(G.N))
    for i in range(G.N):       # every real container lies inside its bracket
        lo, hi = G.brackets(version, shape, i)
        q = G.QUALITIES[version][i]
        assert int(lo[q]) <= len(G.container(version, shape, i, q)) <= int(hi[q])
    plan = G.budget_plan(version, shape)
    min_q, max_q = G.BUDGET_RANGE[version]
    assert _distinct(b for b, *_ in plan) and _distinct(q for _, q, *_ in plan), [p[:4] for p in plan]
    assert _distinct(len(data) for *_, data in plan) and _distinct(data for *_, data in plan)
    assert all(trials <= SR.REFINE_TRIALS for _, _, _, trials, _ in plan)
    assert max(trials for _, _, _, trials, _ in plan) >= 1            # the refinement runs, and its trials are counted
    assert plan[G.ENCODE_BUDGETS.index("nothing")][1:3] == (min_q, False)
    assert plan[G.ENCODE_BUDGETS.index("everything")][1:4] == (max_q, True, 0)
    assert [fits for _, _, fits, _, _ in plan].count(False) == 1
    for budget, _, fits, _, data in plan:
        assert not fits or len(data) <= budget


@pytest.mark.parametrize("shape", list(G.SHAPES))
@pytest.mark.parametrize("version", [2, 3])
def test_psnr_choices_differ(version, shape):
    plan = G.psnr_plan(version, shape)
    assert _distinct(q for q, *_ in plan), [p[:4] for p in plan]
    assert _distinct(db for _, _, _, db, _ in plan) and _distinct(data for *_, data in plan)
    assert all(reached and db >= G.PSNR_TARGET[version, shape] for _, reached, _, db, _ in plan)
    assert all(1 <= trials <= 8 for _, _, trials, _, _ in plan)


@pytest.mark.parametrize("shape", list(G.SHAPES))
@pytest.mark.parametrize("version", [2, 3])
def test_transcode_plan(version, shape):
    srcs = G.sources(version, shape)
    assert _distinct(srcs) and _distinct(SR.quality_to_step(q) for q in G.SOURCES[version])
    outs = G.transcode_plan(version, shape)
    assert _distinct(outs) and _distinct(len(x) for x in outs), [len(x) for x in outs]
    assert all(len(outs[G.BIG]) > len(x) for i, x in enumerate(outs) if i != G.BIG)
    for i, (src, out) in enumerate(zip(srcs, outs)):
        s1, s2 = SR.quality_to_step(G.SOURCES[version][i]), SR.quality_to_step(G.TARGETS[version][i])
        if i % 3 == 1:
            assert s2 <= s1 and out == src, i                      # untouched
        elif i % 3 == 0:
            assert s1 < s2 <= 3 * s1 + 12 and out != src, i        # mapped
        else:
            assert s2 >= 55 and s2 >= 2 * s1 and out != src, i     # mapped far
    plan = G.transcode_budget_plan(version, shape)
    assert _distinct(b for b, *_ in plan) and _distinct(q for _, q, *_ in plan), [p[:4] for p in plan]
    assert _distinct(data for *_, data in plan)
    assert all(trials <= SR.REFINE_TRIALS for _, _, _, trials, _ in plan) and max(p[3] for p in plan) >= 1
    assert [p[2] for p in plan].count(False) == 1
    assert plan[G.TRANSCODE_BUDGETS.index("nothing")][1:3] == (G.TRANSCODE_RANGE[0], False)
    assert plan[G.TRANSCODE_BUDGETS.index("everything")][1:4] == (G.TRANSCODE_RANGE[1], True, 0)


@pytest.mark.parametrize("shape", list(G.SHAPES))
@pytest.mark.parametrize("base", G.BASES)
def test_banded_plan(base, shape):
    blobs, plain = G.bandeds(base, shape), G.containers(base, shape)
    assert _distinct(blobs) and all(b[4] == 5 and b[22] == base for b in blobs)
    assert all(len(blobs[G.BIG]) > len(b) for i, b in enumerate(blobs) if i != G.BIG)
    # the repacks are each other's inverse and meet the encoders' own bytes
    assert G.to_banded_plan(base, shape) == blobs and G.from_banded_plan(base, shape) == plain
    # a banded chunk decodes to its base chunk's pixels
    i = G.BIG
    assert np.array_equal(B5.decode(blobs[i]), G.pixels(base, shape, i, G.QUALITIES[base][i]))


def test_stride_plan_is_one_byte_short_for_one_chunk_of_the_second_group():
    assert sorted(G.STRIDE_ORDER) == list(range(G.N)) and G.STRIDE_ORDER[G.STRIDE_AT] == G.BIG
    assert G.STRIDE_AT // G.STRIDE_CAP == 1 and G.STRIDE_AT % G.STRIDE_CAP == 1       # second chunk of the second group
    assert G.STRIDE_ORDER[:G.STRIDE_CAP] == tuple(range(G.STRIDE_CAP))                # group 0 is chunks 0 and 1
    assert {G.STRIDE_VERSION[f] for f in ("banded", "to_banded", "from_banded")} == set(G.BASES)
    for family in G.STRIDE_FAMILIES:
        inputs, want = G.stride_plan(family)
        assert inputs is None or len(inputs) == G.N
        short = len(want[G.STRIDE_AT]) - 1
        assert [len(b) > short for b in want] == [i == G.STRIDE_AT for i in range(G.N)], family
        assert _distinct(want[:G.STRIDE_CAP])


def test_the_references_refuse_the_damaged_chunks():
    for version in (2, 3):
        src = (G.containers if version == 2 else G.sources)(version, "tile")[G.BIG]
        bad = G.damaged(src)
        assert len(bad) == len(src) and sum(a != b for a, b in zip(src, bad)) == 1
        (R2 if version == 2 else W3).parse_container(bad)          # the header and the directories still add up
        with pytest.raises(T.InvalidBitstream):
            (R2 if version == 2 else W3).decode_container(bad)
        with pytest.raises(T.InvalidBitstream):
            T.transcode(bad, 50)


def test_region_origins_lie_inside_the_frame_and_differ():
    w, h, _ = G.SHAPES["tile"]
    assert len(G.ORIGINS) == G.N and _distinct(G.ORIGINS)
    assert all(x + w <= G.FRAME[0] and y + h <= G.FRAME[1] for x, y in G.ORIGINS)
    assert any(x % 2 for x, _ in G.ORIGINS) and any(y % 2 for _, y in G.ORIGINS)
