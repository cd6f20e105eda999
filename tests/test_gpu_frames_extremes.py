"""Frame ranges on the MI355X where the window path can go wrong without the parity tests of
tests/test_gpu_frames.py noticing: every instance class of the window inverse at the first and last quantiser step of the
class, on volumes that hold the largest magnitudes the formats decode to; the lane decode of a block subset at lane sizes
other than 64 and with every symbol an escape; and damage in blocks that straddle a range edge or are shared by the low and
the high range.  The plan -- shapes, volumes, steps, ranges, containers and the numpy references -- is
tests/frames_extreme_cases.py's, and tests/test_frames_extremes_host.py shows without a device that it reaches what it
claims.  Every expected pixel comes from the numpy references (split_ref / wide_ref for the lanes, the numpy oracle and
reversible_ref for the inverse); equality with the library's own full decode is asserted beside that, never instead.  Every
comparison is bit-exact."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frames_extreme_cases as F  # noqa: E402
import frames_ref as FR  # noqa: E402
import reversible_ref as RR  # noqa: E402
import split_ref as R2  # noqa: E402
import transform_extremes as X  # noqa: E402
import wide_ref as R3  # noqa: E402
from test_gpu_frames import Chunk, _channel_layout, _check_stats, _lane_flip  # noqa: E402
from test_gpu_reversible_extremes import band_target  # noqa: E402

pytestmark = pytest.mark.gpu

IDS = [F.case_id(c) for c in F.CASES]
_ran = {(version, kind): {} for version in F.VERSIONS for kind in F.KINDS}      # class -> steps the window instances ran at


def _frames(ch, t0, t1):
    return ch.dev_frames(t0, t1).cpu().numpy()


# ---- 1. every planned case ----
@pytest.mark.parametrize("case", F.CASES, ids=IDS)
def test_every_planned_window_equals_the_numpy_reference(gpu_codec, case):
    shape, kind, version = case
    a = gpu_codec
    lib = a.load_library()
    w, h, f = shape
    band_kb = F.SHAPES[shape][0]
    rs = F.ranges(kind, shape)
    named = set(FR.named_ranges(kind, f))
    counts = sorted({t1 - t0 for t0, t1 in rs})
    uncut = {(n, m): lib.alice_codec_test_inverse_scratch_bytes(w, h, n, m) for n in counts for m in (0, 1)}
    told_apart, ch = set(), None
    with band_target(lib, band_kb):
        if band_kb is not None:       # the target cuts the slot of the kept frames, whatever their count and the slot's type
            for key, whole in uncut.items():
                assert 0 < lib.alice_codec_test_inverse_scratch_bytes(w, h, *key) < whole, (shape, key)
        for name, steps, v in F.cases(lib, kind, shape, version):
            assert F.variant(lib, kind, steps, version) == v, (kind, steps)
            blob = F.container(kind, shape, name, steps, version)
            if ch is None:
                ch = Chunk(a, version, shape, kind, blob=blob)
            else:
                ch.blob = blob
                ch.set_container(blob)
            for t0, t1 in rs:
                where = (F.case_id(case), name, steps, v, (t0, t1))
                want = F.reference(kind, shape, version, name, steps, t0, t1)
                plan = FR.frame_plan(kind, w, h, f, F.LANE_SYMBOLS, t0, t1)
                got = _frames(ch, t0, t1)
                bad = np.flatnonzero(got != want)
                assert bad.size == 0, (where, bad.size, bad[:4].tolist())
                _check_stats(a, plan, t1 - t0, 0)
                if (t0, t1) in named:
                    assert np.array_equal(np.asarray(a.decode_frames(blob, t0, t1 - t0)), want), where
                    _check_stats(a, plan, t1 - t0, ch.planned_bytes(plan))
                if version != 2 and F.differing_pixels(kind, shape, name, steps, t0, t1):     # this inverse ran, not its twin
                    assert not np.array_equal(got, F.reference(kind, shape, version, name, steps, t0, t1, mirrored=version != 4)), where
                    told_apart.add(v)
            if F.tile_eligible(shape):
                _ran[(version, kind)].setdefault(v, set()).add(tuple(steps))
    if version != 2 and F.tile_eligible(shape):
        assert told_apart == F.EXPECTED[version][kind], (F.case_id(case), told_apart)


# ---- 2. after the cases: every class ran through a window, at the first and the last step of the class ----
def test_every_class_ran_through_a_window_at_its_edges(gpu_codec):
    """The plan holds the first and last step of every class of every (version, wavelet); and what ran in this process
    (when the tests above ran) is the plan: per version and wavelet the expected set of classes, each at both its edges."""
    lib = gpu_codec.load_library()
    ran_any = any(_ran.values())
    for version in F.VERSIONS:
        for kind in F.KINDS:
            edges = F.class_edges(lib, kind, version)
            assert set(edges) == F.EXPECTED[version][kind], (version, kind, edges)
            planned = {}
            for steps, v in F.step_cases(lib, kind, version):
                assert F.variant(lib, kind, steps, version) == v
                planned.setdefault(v, set()).add(tuple(steps))
            ran = _ran[(version, kind)]
            for v, edge in edges.items():
                assert edge <= planned[v], (version, kind, v, edge)
                if ran_any:
                    assert set(ran) == F.EXPECTED[version][kind], (version, kind, sorted(ran))
                    assert edge <= ran[v], (version, kind, v, edge, ran[v])
            print(f"version {version} {F.NAMES[kind]}: classes {sorted(edges)} planned at their edges, ran {({v: sorted(s) for v, s in ran.items()})}")


# ---- 3. lane sizes ----
_symbols = {}


def _symbols_of(version, blob):
    """(info, [Y, Co, Cg] symbols) of split_ref / wide_ref decode_container, once per payload (versions 3 and 4 of one
    content differ in byte 4 only)"""
    key = (version == 2, hashlib.sha1(blob[5:]).digest())
    if key not in _symbols:
        _symbols[key] = R2.decode_container(blob) if version == 2 else R3.decode_container(RR.with_version(blob, 3))
    return _symbols[key]


def _reference_decode(version, blob, shape, kind):
    """the container through the reference lane decoder and the numpy inverse: interleaved RGB of the whole chunk"""
    w, h, f = shape
    info, syms = _symbols_of(version, blob)
    assert (info["width"], info["height"], info["frames"], info["wavelet"]) == (w, h, f, kind)
    qs = [F.quantised(s, version) for s in syms]
    inverse = RR.inverse_quantised if version == 4 else X.inverse_quantised_steps
    return info, syms, inverse(qs, info["step"], F.dims(shape), w, h, f, kind)


def _check_ranges(a, ch, want_full, L, ranges, where):
    w, h, f = ch.shape
    named = set(FR.named_ranges(ch.kind, f))
    n = ch.frame_bytes
    for t0, t1 in ranges:
        plan = FR.frame_plan(ch.kind, w, h, f, L, t0, t1)
        got = _frames(ch, t0, t1)
        assert np.array_equal(got, want_full[t0 * n:t1 * n]), (where, (t0, t1))
        _check_stats(a, plan, t1 - t0, 0)
        if (t0, t1) in named:
            assert np.array_equal(np.asarray(a.decode_frames(ch.blob, t0, t1 - t0)), want_full[t0 * n:t1 * n]), (where, (t0, t1))
            _check_stats(a, plan, t1 - t0, ch.planned_bytes(plan))


@pytest.mark.parametrize("version,L", [(v, L) for v in F.VERSIONS for L in F.LANE_SIZES[v]])
def test_lane_sizes(gpu_codec, version, L):
    """128x96x40 of smooth-plus-noise content encoded by the library: 60 blocks per channel at L = 128, 15 at 512, 3.75 at
    2048 (a short last block, range edges clipped inside blocks, low and high range in one block), one partly filled block
    at the format's largest L."""
    a = gpu_codec
    shape = F.LANE_SHAPE
    w, h, f = shape
    kind = F.lane_kind(version, L)
    ch = Chunk(a, version, shape, kind, q=F.LANE_QUALITY[version], seed=40 + kind, lane=L)
    info, syms, want = _reference_decode(version, ch.blob, shape, kind)
    assert info["lane_symbols"] == L and info["n_blocks"][0] == -(-syms[0].size // (64 * L))
    if version != 2:
        assert max(int(s.max()) for s in syms) >= 255       # escapes in natural content too
    assert np.array_equal(ch.full, want), "the library's full decode is not the references'"
    _check_ranges(a, ch, want, L, F.lane_ranges(kind, f), (version, L, kind))


@pytest.mark.parametrize("version,L", [(v, L) for v in (3, 4) for L in F.ESCAPE_LANES])
def test_lanes_of_escapes_only(gpu_codec, version, L):
    """The worst-sign wide volume of 104x40x16, z = 4349 / 4350 in every sample: every coded symbol is an escape, so the
    first and the last kept symbol of every lane of every clipped block is one."""
    a = gpu_codec
    shape = F.ESCAPE_SHAPE
    w, h, f = shape
    for kind in F.KINDS:
        z = F.volumes(kind, shape, version)["worst"]
        assert all(int(zz.min()) >= 255 for zz in z)
        blob = RR.with_version(R3.write_container(kind, w, h, f, L, F.ESCAPE_STEPS, z), version)
        _, syms, want = _reference_decode(version, blob, shape, kind)
        assert all(np.array_equal(s, zz) for s, zz in zip(syms, z))
        assert np.array_equal(want, F.reference(kind, shape, version, "worst", F.ESCAPE_STEPS, 0, f))
        ch = Chunk(a, version, shape, kind, blob=blob)
        full = np.asarray({3: a.decode_wide, 4: a.decode_reversible}[version](blob))
        assert np.array_equal(full, want), "the library's full decode is not the references'"
        _check_ranges(a, ch, want, L, F.lane_ranges(kind, f), (version, L, kind))


# ---- 4. damage in clipped and shared blocks ----
def _directory_flip(blob, channel, block):
    """The container with one lane length of `block` raised by one and its neighbour's lowered by one: the block's length
    still matches its directory, and every chain from the first of the two on starts or ends one byte off."""
    _, lay = _channel_layout(blob)
    pos, nb, offs, lens, plen, ns = lay[channel]
    blk = pos + int(offs[block])
    lane_len = np.frombuffer(blob, "<u2", 64, blk).astype(np.int64)
    lane = next(i for i in range(63) if lane_len[i] >= 12 and lane_len[i + 1] >= 12)
    bad = bytearray(blob)
    bad[blk + 2 * lane:blk + 2 * lane + 2] = int(lane_len[lane] + 1).to_bytes(2, "little")
    bad[blk + 2 * lane + 2:blk + 2 * lane + 4] = int(lane_len[lane + 1] - 1).to_bytes(2, "little")
    return bytes(bad)


@pytest.mark.parametrize("version", F.VERSIONS)
def test_damage_in_clipped_and_shared_blocks(gpu_codec, version):
    """50x38x13, CDF 9/7, L = 64: planes of 1900 symbols in blocks of 4096.  No single range of this shape has a clipped
    start, a clipped end and a shared block (tests/frames_extreme_cases.py says why), so [6, 7) carries the two clipped ends,
    [7, 10) the block that the low and the high range share, and [12, 13) leaves two blocks unplanned.  A planned block
    that straddles a range edge, or that both ranges share, still runs all its chains to their end checks."""
    a = gpu_codec
    shape, kind = F.DAMAGE_SHAPE, F.DAMAGE_KIND
    w, h, f = shape
    ch = Chunk(a, version, shape, kind, q=80)
    _, _, want_full = _reference_decode(version, ch.blob, shape, kind)
    assert np.array_equal(ch.full, want_full), "the library's full decode is not the references'"
    n = ch.frame_bytes
    full_decode = {2: a.decode_split, 3: a.decode_wide, 4: a.decode_reversible}[version]
    plans = {r: FR.frame_plan(kind, w, h, f, F.LANE_SYMBOLS, *r) for r in (F.DAMAGE_CLIPPED, F.DAMAGE_SHARED, F.DAMAGE_SKIPPING)}
    clipped, shared, skipping = (plans[r] for r in (F.DAMAGE_CLIPPED, F.DAMAGE_SHARED, F.DAMAGE_SKIPPING))
    assert {"start_clipped", "end_clipped"} <= clipped["classes"] and {"start_clipped", "shared_block"} <= shared["classes"]
    shared_block = shared["ranges"][1][0] // (64 * F.LANE_SYMBOLS)
    assert shared_block == shared["ranges"][0][1] // (64 * F.LANE_SYMBOLS) and shared_block in shared["planned"]

    def good(t0, t1):
        """the undamaged container right after a refusal: no flag is left behind"""
        ch.set_container(ch.blob)
        assert np.array_equal(_frames(ch, t0, t1), want_full[t0 * n:t1 * n])
        assert np.array_equal(np.asarray(a.decode_frames(ch.blob, t0, t1 - t0)), want_full[t0 * n:t1 * n])

    def refused(bad, t0, t1, message):
        ch.set_container(bad)
        with pytest.raises(a.CodecError) as e:
            ch.dev_frames(t0, t1)
        assert e.value.code == 4 and message in str(e.value), str(e.value)
        assert ch.untouched(), "a refused range wrote to its output"
        with pytest.raises(a.CodecError) as e:
            a.decode_frames(bad, t0, t1 - t0)
        assert e.value.code == 4 and message in str(e.value), str(e.value)
        good(t0, t1)

    # a byte of the first planned block (clipped start), of the last one (clipped end) and of the shared one
    for (t0, t1), channel, block in ((F.DAMAGE_CLIPPED, 0, clipped["planned"][0]), (F.DAMAGE_CLIPPED, 2, clipped["planned"][-1]),
                                     (F.DAMAGE_SHARED, 1, shared_block), (F.DAMAGE_SHARED, 0, shared["planned"][0])):
        refused(_lane_flip(version, ch.blob, channel, block), t0, t1, "end check")
    # the lane directory of a planned clipped block: the block length still matches, the chains do not
    for (t0, t1), channel, block in ((F.DAMAGE_CLIPPED, 1, clipped["planned"][0]), (F.DAMAGE_CLIPPED, 0, clipped["planned"][-1]),
                                     (F.DAMAGE_SHARED, 2, shared_block)):
        bad = _directory_flip(ch.blob, channel, block)
        assert len(bad) == len(ch.blob) and bad != ch.blob
        refused(bad, t0, t1, "")
    # a byte of an unplanned block: the range comes back as from the undamaged file, the full decode refuses it
    t0, t1 = F.DAMAGE_SKIPPING
    outside = [b for b in range(skipping["n_blocks"]) if b not in skipping["planned"]]
    assert outside == [0, 4] and {"start_clipped", "edge_inside_block"} <= skipping["classes"]
    for channel, block in ((0, outside[0]), (2, outside[-1])):
        bad = _lane_flip(version, ch.blob, channel, block)
        ch.set_container(bad)
        assert np.array_equal(_frames(ch, t0, t1), want_full[t0 * n:t1 * n])
        assert np.array_equal(np.asarray(a.decode_frames(bad, t0, t1 - t0)), want_full[t0 * n:t1 * n])
        with pytest.raises(a.CodecError) as e:
            full_decode(bad)
        assert e.value.code == 4
        good(t0, t1)
