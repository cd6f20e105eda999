"""The job table of tests/concurrent_cases.py without a device: every family is there with at least two jobs of different
shape or wavelet, every expected value has the size its call documents, the references agree where they overlap (a frame
range with the same frames of the full decode, a rectangle with the crop of that range, an item of the batched preview with
the single preview), the damaged containers are refused by the reference decoders for the reason their jobs name, and no
job reaches for a process-wide tuning hook."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import concurrent_cases as CC  # noqa: E402
import frames_ref as FR  # noqa: E402
import preview_ref as PR  # noqa: E402
import rate_ref  # noqa: E402
import reversible_ref as RR  # noqa: E402
import split_rate_ref as SR  # noqa: E402
import split_ref as R2  # noqa: E402
import wide_ref as R3  # noqa: E402
from test_frames_host import _decode_syms  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
HOOKS = ("alice_codec_test_set_tuning", "_set_grid_cap", "_set_value_table_radius", "_set_admission_budget")


def _leaves(v):
    if isinstance(v, tuple):
        for x in v:
            yield from _leaves(x)
    else:
        yield v


def test_every_family_has_two_jobs_of_different_shape_or_wavelet():
    fams = CC.by_family()
    assert set(fams) == set(CC.FAMILIES)
    for fam in CC.FAMILIES:
        names = [j.name for j in fams[fam]]
        assert len(names) >= 2 and len(set(names)) == len(names), (fam, names)
    names = [j.name for j in CC.jobs()] + [j.name for j in CC.device_jobs()]
    assert len(set(names)) == len(names)
    for j in CC.jobs() + CC.device_jobs():
        assert j.family in CC.FAMILIES and callable(j.run), j.name
        for leaf in _leaves(j.expected):
            assert isinstance(leaf, (bytes, np.ndarray, int, float, bool, str, np.integer)), (j.name, type(leaf))


def test_the_table_covers_the_shapes_the_wavelets_and_the_versions():
    cases = [CC.V2_A, CC.V2_B, CC.V3_A, CC.V3_B, CC.V4_A, CC.V4_B, CC.V4_LOSSLESS, CC.PARTIAL_A, CC.PARTIAL_B, CC.PARTIAL_C]
    assert {c[0] for c in cases} == set(CC.SHAPES) == {(64, 64, 16), (50, 38, 13), (33, 17, 5), (5, 3, 7), (40, 24, 1)}
    assert CC.LANE == 64 == FR.LANE == PR.LANE
    assert {c[1] for c in cases} == {0, 1, 2} and {c[2] for c in cases} == {2, 3, 4}
    for fam in ("frames", "preview", "rect"):
        table = {"frames": CC.FRAMES_CASES, "preview": CC.PREVIEW_CASES, "rect": CC.RECT_CASES}[fam]
        assert {c[0][2] for c in table} == {2, 3, 4} and {c[0][1] for c in table} == {0, 1, 2}, fam
    assert {c[2] for c, _, _ in CC.PREVIEWS_ITEMS} == {2, 3, 4}
    assert min(min(s[:2]) for s in CC.SHAPES) < 6, "one shape takes the generic path"


def test_expected_values_have_the_documented_sizes():
    jobs = {j.name: j for j in CC.jobs()}
    for j in CC.jobs():
        if CC.is_refusal(j.expected):
            assert j.family == "refusal" and j.expected[1] in (CC.INVALID_DIMENSIONS, CC.INVALID_BITSTREAM), j.name
    # containers: the header says what the job's name says, and the length is the header's
    for case in (CC.V2_A, CC.V2_B, CC.V3_A, CC.V3_B, CC.V4_A, CC.V4_B, CC.V4_LOSSLESS):
        shape, kind, version, q = case
        blob = CC.container(*case)
        info = {2: R2.parse_container, 3: R3.parse_container, 4: RR.parse_container}[version](blob)
        assert (info["width"], info["height"], info["frames"], info["wavelet"], info["lane_symbols"]) == (*shape, kind, 64)
        assert len(blob) == R2.HEADER + sum(info["payload_len"])
        assert CC.full_decode(*case).shape == (shape[2], shape[1], shape[0], 3)
    assert np.array_equal(CC.full_decode(*CC.V4_LOSSLESS).reshape(-1), CC.source(CC.V4_LOSSLESS[0])), "quality 100 of version 4 is exact"
    for case, t0, t1 in CC.FRAMES_CASES:
        w, h, _ = case[0]
        assert CC.frames_expected(case, t0, t1).shape == ((t1 - t0) * h * w * 3,)
    for case, t0, t1 in CC.PREVIEW_CASES:
        qw, qh = PR.preview_dims(*case[0][:2])
        assert CC.preview_expected(case, t0, t1).shape == ((t1 - t0) * qh * qw * 3,)
    for case, t0, t1, (x, y, rw, rh) in CC.RECT_CASES:
        assert CC.rect_expected(case, t0, t1, (x, y, rw, rh)).shape == ((t1 - t0) * rh * rw * 3,)
    for j in CC.by_family()["previews"]:
        assert all(isinstance(x, np.ndarray) and x.dtype == np.uint8 for x in j.expected)
    for j in CC.by_family()["rate"]:
        if "predict" in j.name:
            assert all(np.asarray(x).shape == (101,) for x in j.expected), j.name
            lo, hi = j.expected[0], j.expected[1]
            assert (np.asarray(lo) <= np.asarray(hi)).all(), j.name
        else:
            data, q, fits = j.expected
            assert isinstance(data, bytes) and 10 <= q <= 95 and isinstance(fits, bool)
    for j in CC.by_family()["quality"]:
        data, q, reached, db = j.expected
        assert isinstance(data, bytes) and 0 <= q <= 100 and reached is True and np.isfinite(db)
    for j in CC.by_family()["segment"]:
        if "segment_by" in j.name:
            w, h = map(int, re.search(r"(\d+)x(\d+)", j.name).groups())
            mask, bbox, count = j.expected
            assert mask.shape == (w * h,) and len(bbox) == 4 and count == int(mask.sum()) > 0, j.name
        elif "rle" in j.name:
            assert len(j.expected) % 3 == 0 and len(j.expected) > 3
        else:
            assert len(j.expected) % 3 == 0 and len(j.expected) > 0, j.name
    dec = jobs[f"stage/RansDecoder decode_n {CC.DECODER_CALLS} of 30000"].expected
    assert CC.DECODER_CALLS == (5000, 1, 9000, 4096, 4095) and [len(s) for s, _, _ in dec] == list(CC.DECODER_CALLS)
    assert np.array_equal(np.concatenate([s for s, _, _ in dec]), CC.decoder_stream(7, 30000)[0][:sum(CC.DECODER_CALLS)])
    assert [p for _, _, p in dec] == sorted(p for _, _, p in dec) and dec[-1][2] <= len(CC.decoder_stream(7, 30000)[2])
    assert CC.single_symbols_expected(7, 30000) == tuple(int(v) for v in CC.decoder_stream(7, 30000)[0][:5])
    for j in CC.by_family()["stage"]:
        if "RansEncoder encode_symbols" in j.name:
            assert len(j.expected) == 4 and isinstance(j.expected[3], bytes) and len(set(j.expected[:3])) == 3
    # the budget jobs make the refinement count, and the floor jobs search
    assert CC.budget_choice((33, 17, 5), CC.CDF97, False)[3] >= 1 and CC.budget_choice((40, 24, 1), CC.HAAR, True)[3] >= 1
    assert CC.psnr_choice((33, 17, 5), CC.CDF97, 2)[3] >= 3


def test_the_size_model_of_version_1_uses_the_librarys_table(codec):
    """rate_ref takes its fixed-point log table from the library; the table of split_rate_ref, computed at 60 digits, is the
    same one, so the version 1 brackets of the job table owe nothing to the library"""
    lo, hi, g = rate_ref.log_table(codec)
    rlo, rhi, rg = SR.log_table()
    assert [int(v) for v in lo[1:]] == rlo[1:] and [int(v) for v in hi[1:]] == rhi[1:] and tuple(g) == tuple(rg)


@pytest.mark.parametrize("case", [CC.PARTIAL_A, CC.PARTIAL_B, CC.PARTIAL_C, CC.V2_B, CC.V4_B], ids=str)
def test_full_decodes_agree_with_the_per_format_references(case):
    shape, kind, version, q = case
    w, h, f = shape
    _, syms, unmap, to_rgb = _decode_syms(version, CC.container(*case))
    want = to_rgb([unmap(s) for s in syms], R2.padded_dims(w, h, f), f)
    assert np.array_equal(CC.full_decode(*case).reshape(-1), np.asarray(want).reshape(-1))


def test_ranges_rectangles_and_previews_agree_where_they_overlap():
    for case, t0, t1 in CC.FRAMES_CASES:
        assert np.array_equal(CC.frames_expected(case, t0, t1), CC.full_decode(*case)[t0:t1].reshape(-1)), (case, t0, t1)
    for case, t0, t1, rect in CC.RECT_CASES:
        w, h, _ = case[0]
        x, y, rw, rh = rect
        rng = CC.frames_expected(case, t0, t1).reshape(t1 - t0, h, w, 3)
        assert np.array_equal(CC.rect_expected(case, t0, t1, rect), rng[:, y:y + rh, x:x + rw].reshape(-1)), (case, t0, t1, rect)
    # every frame and every rectangle position class of one small chunk
    case = CC.PARTIAL_C
    w, h, f = case[0]
    for t0 in range(f):
        assert np.array_equal(CC.frames_expected(case, t0, t0 + 1), CC.full_decode(*case)[t0].reshape(-1))
        assert np.array_equal(CC.rect_expected(case, t0, t0 + 1, (w - 2, 1, 2, 2)), CC.full_decode(*case)[t0, 1:3, w - 2:].reshape(-1))
    # an item of a batched list is the single preview of the same container and range
    singles = {(c, t0, t1): CC.preview_expected(c, t0, t1) for c, t0, t1 in CC.PREVIEW_CASES}
    batched = dict(zip(CC.PREVIEWS_ITEMS_B, CC.by_family()["previews"][1].expected))
    shared = set(singles) & set(batched)
    assert shared, "the lists share an item"
    for key in shared:
        assert np.array_equal(batched[key], singles[key])
    for (c, t0, t1), got in zip(CC.PREVIEWS_ITEMS, CC.by_family()["previews"][0].expected):
        assert np.array_equal(got, CC.preview_expected(c, t0, t1))
        # the preview's window is the frame range's
        assert PR.preview_plan(c[1], *c[0], 64, t0, t1)["a"] == FR.frame_plan(c[1], *c[0], 64, t0, t1)["a"]


def test_damaged_containers_fail_in_the_reference_decoders():
    for case in (CC.V2_A, CC.V3_A, CC.V4_A):
        bad = CC.lane_damaged(case, 0)
        assert len(bad) == len(CC.container(*case)) and bad != CC.container(*case)
        with pytest.raises(R2.InvalidBitstream, match="end check"):
            (R2.decode_container(bad) if case[2] == 2 else R3.decode_container(RR.with_version(bad, 3)))
    for case in (CC.PARTIAL_B, CC.REFUSAL_FRAMES_CASE, CC.PARTIAL_C):
        bad = CC.directory_damaged(case)
        with pytest.raises(R2.InvalidBitstream, match="block lengths"):
            (R2.parse_container(bad) if case[2] == 2 else R3.parse_container(RR.with_version(bad, 3)))
    t0, t1 = CC.REFUSAL_RANGE
    c = CC.REFUSAL_FRAMES_CASE
    plan = FR.frame_plan(c[1], *c[0], 64, t0, t1)
    assert len(plan["planned"]) < plan["n_blocks"] and CC.lane_damaged(c) != CC.container(*c)
    rows = CC.previews_with_damage(1)
    clean = [CC.container(*cc) for cc, _, _ in CC.PREVIEWS_ITEMS]
    assert [r[0] != b for r, b in zip(rows, clean)] == [False, True, False, False, False]
    assert CC.v1_blob()[:4] == b"ALCC" and CC.v1_blob()[4] == 1


def test_no_job_calls_a_process_wide_tuning_hook():
    text = inspect.getsource(CC) + open(os.path.join(HERE, "test_gpu_concurrent_calls.py")).read()
    for hook in HOOKS:
        assert hook not in text, hook
    assert "force_first_cap" not in text and "os.environ" not in text and "putenv" not in text
