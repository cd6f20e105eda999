"""`decode --frames` of the command line: the range syntax and the refusals that are host code (no
device), and on a GPU the frames written for `A` and `A:B` from files of versions 2, 3 and 4."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle.alice_oracle_np as o  # noqa: E402
import wide_oracle as WO  # noqa: E402
from test_frames_host import _encode_ref  # noqa: E402

W, H, F = 33, 17, 5


def run(codec, argv, capsys):
    from alice_codec_amd import cli
    rc = cli.main(argv)
    cap = capsys.readouterr()
    return rc, cap.out, cap.err


def test_range_syntax():
    from alice_codec_amd import cli
    assert cli.parse_frames("3") == (3, 4) and cli.parse_frames("0:5") == (0, 5) and cli.parse_frames(" 24:40") == (24, 40)
    for bad in ("", "a", "3:", ":3", "5:5", "5:2", "-1:2", "1:2:3", "1.5", "0:4294967296"):
        with pytest.raises(ValueError, match="--frames wants A or A:B"):
            cli.parse_frames(bad)


def test_refusals_without_a_device(codec, tmp_path, capsys):
    rgb = WO.smooth_plus_noise(W, H, F)
    out = tmp_path / "o.rgb"
    v1 = tmp_path / "v1.alc"
    v1.write_bytes(o.encode(rgb, W, H, F, 80, 0))
    rc, _, err = run(codec, ["decode", str(v1), "-o", str(out), "--frames", "2"], capsys)
    assert rc == 1 and "version 1 has no random access (one serial chain per channel)" in err and not out.exists()
    v3 = tmp_path / "v3.alc"
    v3.write_bytes(_encode_ref(3, rgb, W, H, F, 80, 0, 64))
    for bad in ("2:2", "x", "4:1"):
        rc, _, err = run(codec, ["decode", str(v3), "-o", str(out), "--frames", bad], capsys)
        assert rc == 1 and "--frames wants A or A:B" in err and not out.exists()
    for outside in ("5", "3:6", "0:9"):
        rc, _, err = run(codec, ["decode", str(v3), "-o", str(out), "--frames", outside], capsys)
        assert rc == 1 and "are not a range of the chunk's 5 frames" in err and not out.exists()
    rc, _, err = run(codec, ["decode", str(v3), "-o", str(out), "--frames", "1", "--format", "split"], capsys)
    assert rc == 1 and "--format split names version 2, the file's version byte is 3" in err and not out.exists()


@pytest.mark.gpu
def test_frames_written(gpu_codec, tmp_path, capsys):
    a = gpu_codec
    rgb = WO.smooth_plus_noise(W, H, F)
    fb = W * H * 3
    for version, make, fmt in ((2, a.encode_split, "split"), (3, a.encode_wide, "wide"), (4, a.encode_reversible, "reversible")):
        blob = make(a.FrameEncoder.with_wavelet(80, a.WaveletType.Cdf97), rgb, W, H, F, 64)
        full = np.asarray(a.decode_alc(blob))
        alc, out = tmp_path / f"v{version}.alc", tmp_path / f"v{version}.rgb"
        alc.write_bytes(blob)
        for text, (t0, t1) in (("2", (2, 3)), ("1:4", (1, 4)), ("0:5", (0, 5)), ("4", (4, 5))):
            rc, _, err = run(a, ["decode", str(alc), "-o", str(out), "--frames", text], capsys)
            assert rc == 0 and f"decoded frames [{t0}, {t1}) of {W}x{H}x{F} -> {(t1 - t0) * fb} bytes" in err
            assert np.array_equal(np.fromfile(out, np.uint8), full[t0 * fb:t1 * fb]), (version, text)
        rc, _, _ = run(a, ["decode", str(alc), "-o", str(out), "--frames", "3", "--format", fmt], capsys)
        assert rc == 0 and np.array_equal(np.fromfile(out, np.uint8), full[3 * fb:4 * fb])
