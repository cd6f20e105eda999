"""`--format reversible` and `--lossless` of the command line: argument handling, the --lossless conflicts and the refusal of
a byte budget (host code, no device), and on a GPU the encode / info / decode round trip of a version 4 file."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_oracle as WO  # noqa: E402


def run(codec, argv, capsys):
    from alice_codec_amd import cli
    rc = cli.main(argv)
    cap = capsys.readouterr()
    return rc, cap.out, cap.err


@pytest.fixture
def tiny(tmp_path):
    src = tmp_path / "in.rgb"
    np.zeros(4 * 4 * 2 * 3, np.uint8).tofile(src)
    return src


def test_reversible_with_a_byte_budget_is_refused(codec, tiny, tmp_path, capsys):
    out = tmp_path / "o.alc"
    base = ["encode", str(tiny), "-o", str(out), "-W", "4", "-H", "4", "-f", "2"]
    for extra in (["--format", "reversible"], ["--lossless"]):
        rc, _, err = run(codec, base + extra + ["--max-bytes", "5000"], capsys)
        assert rc == 1 and "--format reversible" in err and "--max-bytes" in err and "lossless" in err and not out.exists()
        rc, _, err = run(codec, ["encode-chunks", str(tiny), "-o", str(tmp_path / "c"), "-W", "4", "-H", "4", "-c", "2", "--kbps", "100"] + extra,
                         capsys)
        assert rc == 1 and "--format reversible" in err and "--kbps" in err and not list(tmp_path.glob("c.*"))


def test_lossless_conflicts(codec, tiny, tmp_path, capsys):
    out = tmp_path / "o.alc"
    base = ["encode", str(tiny), "-o", str(out), "-W", "4", "-H", "4", "-f", "2", "--lossless"]
    rc, _, err = run(codec, base + ["-q", "90"], capsys)
    assert rc == 1 and "--lossless" in err and "--quality 90" in err and not out.exists()
    for fmt in ("wide", "split", "v1"):
        rc, _, err = run(codec, base + ["--format", fmt], capsys)
        assert rc == 1 and "--lossless" in err and f"--format {fmt}" in err and not out.exists()
    rc, _, err = run(codec, ["encode-chunks", str(tiny), "-o", str(tmp_path / "c"), "-W", "4", "-H", "4", "-c", "2", "--lossless", "-q", "0"],
                     capsys)
    assert rc == 1 and "--quality 0" in err and not list(tmp_path.glob("c.*"))


def test_lossless_is_reversible_at_quality_100(codec, capsys):
    """What --lossless turns into, read off the parsed arguments (no device): the same quality and the explicit format pass."""
    import argparse
    from alice_codec_amd import cli
    for fmt, q, lossless, want in ((None, None, True, ("reversible", 100)), ("reversible", 100, True, ("reversible", 100)),
                                   ("reversible", None, False, ("reversible", 90)), (None, None, False, (None, 90)),
                                   ("reversible", 80, False, ("reversible", 80))):
        a = argparse.Namespace(format=fmt, quality=q, lossless=lossless)
        cli._apply_lossless(a)
        assert (a.format, a.quality) == want
    assert cli.FORMAT_VERSION["reversible"] == 4
    # an unknown format is a usage error of the parser itself
    with pytest.raises(SystemExit):
        cli.main(["info", "x.alc", "--format", "lossless"])
    capsys.readouterr()


def test_info_of_an_empty_reversible_file_and_forced_formats(codec, tmp_path, capsys):
    data = codec.encode_reversible(codec.FrameEncoder.with_wavelet(100, codec.WaveletType.Haar), np.zeros(0, np.uint8), 0, 6, 2)
    p = tmp_path / "e.alc"
    p.write_bytes(data)
    rc, out, _ = run(codec, ["info", str(p)], capsys)          # auto: version 4 from the byte
    assert rc == 0 and "version 4" in out and "reversible" in out and "Haar" in out
    rc, out, _ = run(codec, ["info", str(p), "--format", "reversible"], capsys)
    assert rc == 0 and "version 4" in out
    rc, _, err = run(codec, ["info", str(p), "--format", "wide"], capsys)
    assert rc == 1 and "unsupported version: 4 (expected 3)" in err
    rc, _, err = run(codec, ["info", str(p), "--format", "split"], capsys)
    assert rc == 1 and "unsupported version: 4 (expected 2)" in err
    back = tmp_path / "x.rgb"
    rc, _, err = run(codec, ["decode", str(p), "-o", str(back)], capsys)       # an empty chunk decodes without a device
    assert rc == 0 and "decoded 0x6x2" in err and back.stat().st_size == 0
    wide = tmp_path / "w.alc"
    wide.write_bytes(data[:4] + b"\x03" + data[5:])
    rc, _, err = run(codec, ["decode", str(wide), "-o", str(back), "--format", "reversible"], capsys)
    assert rc == 1 and "unsupported version: 3 (expected 4)" in err


@pytest.mark.gpu
def test_lossless_encode_info_decode_round_trip(gpu_codec, tmp_path, capsys):
    w, h, f = 32, 24, 4
    rgb = WO.smooth_plus_noise(w, h, f)
    src, alc, back = tmp_path / "in.rgb", tmp_path / "o.alc", tmp_path / "back.rgb"
    rgb.tofile(src)
    rc, _, err = run(gpu_codec, ["encode", str(src), "-o", str(alc), "-W", str(w), "-H", str(h), "-f", str(f), "-w", "haar", "--lossless",
                                 "--lane-symbols", "64"], capsys)
    assert rc == 0 and "format=reversible" in err and "quality=100" in err
    data = alc.read_bytes()
    assert data == gpu_codec.encode_lossless(rgb, w, h, f, gpu_codec.WaveletType.Haar, 64)
    rc, out, _ = run(gpu_codec, ["info", str(alc)], capsys)
    assert rc == 0 and "version 4" in out and "Lane length: 64" in out
    rc, _, _ = run(gpu_codec, ["decode", str(alc), "-o", str(back)], capsys)
    assert rc == 0 and np.array_equal(np.fromfile(back, np.uint8), rgb)
    # chunks: two 2-frame files, each lossless
    rc, _, err = run(gpu_codec, ["encode-chunks", str(src), "-o", str(tmp_path / "c"), "-W", str(w), "-H", str(h), "-c", "2",
                                 "--format", "reversible", "-q", "100"], capsys)
    assert rc == 0
    parts = [gpu_codec.decode_alc((tmp_path / f"c.{k:05d}.alc").read_bytes()) for k in range(2)]
    assert np.array_equal(np.concatenate(parts), rgb)
