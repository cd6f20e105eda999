"""`transcode` of the command line: the refusals that are host code (no device), and on a GPU the
files written for `--quality` and `--max-bytes`, with lanes and version changed on the way."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle.alice_oracle_np as o  # noqa: E402
import transcode_cases as TC  # noqa: E402
import transcode_ref as T  # noqa: E402

W, H, F = TC.SHAPES["padding_on_every_axis"]


def run(codec, argv, capsys):
    from alice_codec_amd import cli
    rc = cli.main(argv)
    cap = capsys.readouterr()
    return rc, cap.out, cap.err


def test_refusals_without_a_device(codec, tmp_path, capsys):
    out = tmp_path / "o.alc"
    files = {}
    for v in (2, 3, 4):
        files[v] = tmp_path / f"v{v}.alc"
        files[v].write_bytes(TC.source(v, W, H, F, 0, 90))
    v1 = tmp_path / "v1.alc"
    v1.write_bytes(o.encode(TC.clip(W, H, F), W, H, F, 80, 0))
    for how in (["--quality", "50"], ["--max-bytes", "5000"]):
        rc, _, err = run(codec, ["transcode", str(v1), "-o", str(out), *how], capsys)
        assert rc == 1 and "version 1 has no random access (one serial chain per channel)" in err and not out.exists()
    for how in ([], ["--quality", "50", "--max-bytes", "5000"]):
        rc, _, err = run(codec, ["transcode", str(files[3]), "-o", str(out), *how], capsys)
        assert rc == 1 and "exactly one of --quality Q and --max-bytes N" in err and not out.exists()
    rc, _, err = run(codec, ["transcode", str(files[3]), "-o", str(out), "--max-bytes=-1"], capsys)
    assert rc == 1 and "--max-bytes wants a byte count >= 0" in err and not out.exists()
    for v, lanes in ((2, 100), (2, 32768), (3, 16384), (4, 32)):
        rc, _, err = run(codec, ["transcode", str(files[v]), "-o", str(out), "-q", "50", "--lane-symbols", str(lanes)], capsys)
        assert rc == 1 and "lane_symbols must be a power of two in [64, " in err and not out.exists(), (v, lanes)
    for v, to in ((2, 3), (2, 2), (3, 2), (4, 7)):
        rc, _, err = run(codec, ["transcode", str(files[v]), "-o", str(out), "-q", "50", "--to-version", str(to)], capsys)
        assert rc == 1 and f"out_version {to} of a version {v} chunk" in err and not out.exists(), (v, to)
    rc, _, err = run(codec, ["transcode", str(files[3]), "-o", str(out), "--max-bytes", "5000", "--min-quality", "60", "--max-quality", "50"], capsys)
    assert rc == 1 and "min_quality > max_quality" in err and not out.exists()
    for v, extra in ((4, []), (3, ["--to-version", "4"])):
        rc, _, err = run(codec, ["transcode", str(files[v]), "-o", str(out), "--max-bytes", "5000", *extra], capsys)
        assert rc == 1 and "version 4 is the lossless container" in err and "out_version = 3" in err and not out.exists()
    short = tmp_path / "short.alc"
    short.write_bytes(b"ALCC\x03")
    rc, _, err = run(codec, ["transcode", str(short), "-o", str(out), "-q", "50"], capsys)
    assert rc == 1 and "too short" in err and not out.exists()
    rc, _, err = run(codec, ["transcode", str(tmp_path / "missing.alc"), "-o", str(out), "-q", "50"], capsys)
    assert rc == 1 and not out.exists()


@pytest.mark.gpu
def test_files_written(gpu_codec, tmp_path, capsys):
    a = gpu_codec
    for version in (2, 3, 4):
        src = TC.source(version, W, H, F, 1, 95)
        alc, out = tmp_path / f"v{version}.alc", tmp_path / f"v{version}.out.alc"
        alc.write_bytes(src)
        rc, _, err = run(a, ["transcode", str(alc), "-o", str(out), "--quality", "60"], capsys)
        want = T.transcode(src, 60)
        assert rc == 0 and out.read_bytes() == want
        assert f"transcoded {len(src)} -> {len(want)} bytes" in err and "quality 60, quantiser steps [27, 27, 27], lane_symbols 64" in err
        rc, _, err = run(a, ["transcode", str(alc), "-o", str(out), "-q", "99"], capsys)
        assert rc == 0 and out.read_bytes() == src and "quantiser steps [5, 5, 5]" in err
        rc, _, err = run(a, ["transcode", str(alc), "-o", str(out), "-q", "60", "--lane-symbols", "256"], capsys)
        assert rc == 0 and out.read_bytes() == T.transcode(src, 60, 256) and "lane_symbols 256" in err
        np.testing.assert_array_equal(a.decode_alc(out.read_bytes()), a.decode_alc(want))
        if version >= 3:
            rc, _, err = run(a, ["transcode", str(alc), "-o", str(out), "-q", "60", "--to-version", str(7 - version)], capsys)
            assert rc == 0 and out.read_bytes() == T.transcode(src, 60, 0, 7 - version) and f"(version {7 - version})" in err
        budget = len(want)
        extra = ["--to-version", "3"] if version == 4 else []
        rc, _, err = run(a, ["transcode", str(alc), "-o", str(out), "--max-bytes", str(budget), "--min-quality", "20", "--max-quality", "90", *extra], capsys)
        q, fits, _, data = T.choose_transcode(src, budget, 20, 90, 0, 3 if version == 4 else 0)
        assert rc == 0 and out.read_bytes() == data and fits and len(data) <= budget
        assert f"chosen quality: {q}, budget {budget} bytes met" in err
        rc, _, err = run(a, ["transcode", str(alc), "-o", str(out), "--max-bytes", "1700", *extra], capsys)
        assert rc == 0 and "chosen quality: 10, budget 1700 bytes NOT met" in err and out.read_bytes() == T.transcode(src, 10, 0, 3 if version == 4 else 0)
