"""tests/generic_cases.py held to the launch caps of the generic stage kernels, without a GPU: every family's table must
make its grid-stride loop take one partial trip, exactly one, exactly two, and two or more with a partial last one, at the
caps the launch code really has.  The caps are read from the sources, so a table cannot drift away from them unnoticed."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import generic_cases as G  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src(name):
    with open(os.path.join(ROOT, "alice-codec_amd", "csrc", name)) as fh:
        return fh.read()


def test_trips():
    assert [G.trips(n, 256) for n in (0, 1, 255, 256, 257, 512, 513)] == [0, 1, 1, 1, 2, 2, 3]
    assert G.trip_classes([(255, 256)]) == {"one_partial"}
    assert G.trip_classes([(256, 256)]) == {"one_full"}
    assert G.trip_classes([(512, 256)]) == {"two_full"}
    assert G.trip_classes([(257, 256)]) == G.trip_classes([(600, 256)]) == {"partial_last"}
    assert G.trip_classes([(768, 256)]) == set()
    assert G.trip_classes([(n, 256) for n in (3, 256, 512, 589)]) == G.REQUIRED


def test_the_caps_are_the_sources():
    gen, rate = _src("generic.hip"), _src("rate.hip")
    assert re.search(r"kGridCap = 65535u \* 4u;", gen) and G.DEFAULT_CAP == 65535 * 4
    # the four launches that clamp further, and nothing else
    assert len(re.findall(r"if \(g > 2048\) g = 2048;", gen)) == 4 and G.REDUCE_TRIP == 2048 * 256
    for fn in ("launch_histogram", "launch_histogram_wide", "launch_sq_diff_sum", "launch_sum_i32"):
        body = gen[gen.index("void " + fn + "("):]
        assert "if (g > 2048) g = 2048;" in body[:body.index("\n}\n")], fn
    assert "(n + 255) / 256, 1024)" in rate and G.COEF_TRIP == 1024 * 256
    assert len(re.findall(r"std::min<unsigned long long>\(rows, 65536\)", gen)) == 2 and G.REGION_ROWS == 65536
    assert len(re.findall(r"x = threadIdx\.x; x < w; x \+= 256", gen)) == 2 and G.REGION_X == 256
    assert "n / 16 : 0ull" in gen and G.HIST_VEC == 16
    # every kernel of the file that is launched through grid_for() or a clamp of it has a loop: none returns past the end
    assert not re.search(r"if \(\w+ >= \w+\) return;\s*\n\s*const unsigned long long (y|by) =", gen)


@pytest.mark.parametrize("family", sorted(G.families()))
def test_every_family_reaches_every_trip_class(family):
    pairs = G.families()[family]
    assert pairs and all(items > 0 and ipt > 0 for items, ipt in pairs)
    missing = G.REQUIRED - G.trip_classes(pairs)
    assert not missing, (family, sorted(missing))


def test_histogram_alignment_classes():
    """both alignment classes, each at every size: offset 0 takes the vector loop and a tail below 16 bytes, any other
    offset the scalar loop alone"""
    for n in G.HIST_SIZES:
        offs = G.hist_offsets(n)
        assert 0 in offs and any(o % 16 for o in offs), n
    assert set(G.HIST_OFFSETS) == {0, 1, 4, 15}
    small = set(G.HIST_SMALL)
    assert {0, 1, 15, 16, 17, 31, 32, 33} <= small                     # 16 k and 16 k +- 1
    assert {100_000, 8_388_608 + 16 * 300 + 5} <= set(G.HIST_SIZES)
    tails = {n % 16 for n in G.HIST_SIZES}
    assert {0, 1, 5, 15} <= tails                                       # no tail, the shortest, the longest


def test_the_shapes_take_the_generic_path():
    for shape in G.wavelet_shapes():
        assert not G.tile_eligible(shape), shape
    # chunks: a padded side below 6, or more than 64 frames
    for (w, h, f) in G.PIPELINE_SHAPES + G.RATE_SHAPES + [c[2:5] for c in G.REGION_CASES]:
        pw, ph, pf = G.padded_dims(w, h, f)
        assert min(pw, ph) < 6 or pf > 64, (w, h, f)
    pw, ph, pf = G.padded_dims(*G.RATE_FULL)
    assert pw * ph * pf == 281_600 > G.COEF_TRIP
    for (W, H, w, h, f, origins) in G.REGION_CASES:
        assert all(x0 + w <= W and y0 + h <= H for x0, y0 in origins), (W, H, w, h)
    assert any(h * f == 70_400 and w == 4 and W == 9 for (W, _, w, h, f, _) in G.REGION_CASES)
    assert any((w, h, f, W) == (300, 4, 3, 320) for (W, _, w, h, f, _) in G.REGION_CASES)


def test_the_issue_sizes_are_in_the_tables():
    for cap in G.HOOK_CAPS:
        t = cap * 256
        assert {t - 1, t, t + 1, 2 * t + 77, 5000} <= set(G.elementwise_sizes(cap))
    assert {(5, 3, 7), (3, 40, 4), (20, 12, 66), (1, 300, 4)} <= set(G.PIPELINE_SHAPES)
    cases = {(w, h): caps for w, h, caps in G.SSIM_CASES}
    assert set(cases[(256, 256)]) >= {1, 3, 0} and set(cases[(250, 131)]) >= {1, 3, 0} and 1 in cases[(64, 64)]
    assert {524_287, 524_288, 524_289, 600_001} <= set(G.PSNR_SIZES)
    assert {524_289, 600_001} <= set(G.RDO_SIZES)
    assert any(n > 2048 * 256 for n in G.WIDE_HIST_SIZES)
    assert {2, 3} <= set(G.WAVELET_1D) and any(n % 2 for n in G.WAVELET_1D[2:]) and any(n % 2 == 0 for n in G.WAVELET_1D[2:])
