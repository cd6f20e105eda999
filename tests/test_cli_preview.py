"""`decode --preview` of the command line: the refusals that are host code (no device), and on a GPU
the half-resolution frames written for `--preview` alone and with `--frames A[:B]` from files of versions 2, 3 and 4."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle.alice_oracle_np as o  # noqa: E402
import wide_oracle as WO  # noqa: E402
from test_frames_host import _encode_ref  # noqa: E402

W, H, F = 33, 17, 5
QW, QH = 17, 9


def run(codec, argv, capsys):
    from alice_codec_amd import cli
    rc = cli.main(argv)
    cap = capsys.readouterr()
    return rc, cap.out, cap.err


def test_refusals_without_a_device(codec, tmp_path, capsys):
    rgb = WO.smooth_plus_noise(W, H, F)
    out = tmp_path / "o.rgb"
    v1 = tmp_path / "v1.alc"
    v1.write_bytes(o.encode(rgb, W, H, F, 80, 0))
    for extra in ([], ["--frames", "2"]):
        rc, _, err = run(codec, ["decode", str(v1), "-o", str(out), "--preview", *extra], capsys)
        assert rc == 1 and "version 1 has no random access (one serial chain per channel)" in err and not out.exists()
    v3 = tmp_path / "v3.alc"
    v3.write_bytes(_encode_ref(3, rgb, W, H, F, 80, 0, 64))
    for bad in ("2:2", "x", "4:1"):
        rc, _, err = run(codec, ["decode", str(v3), "-o", str(out), "--preview", "--frames", bad], capsys)
        assert rc == 1 and "--frames wants A or A:B" in err and not out.exists()
    for outside in ("5", "3:6", "0:9"):
        rc, _, err = run(codec, ["decode", str(v3), "-o", str(out), "--preview", "--frames", outside], capsys)
        assert rc == 1 and "are not a range of the chunk's 5 frames" in err and not out.exists()
    rc, _, err = run(codec, ["decode", str(v3), "-o", str(out), "--preview", "--format", "split"], capsys)
    assert rc == 1 and "--format split names version 2, the file's version byte is 3" in err and not out.exists()
    short = tmp_path / "short.alc"
    short.write_bytes(b"ALCC\x03")
    rc, _, err = run(codec, ["decode", str(short), "-o", str(out), "--preview"], capsys)
    assert rc == 1 and "too short" in err and not out.exists()


@pytest.mark.gpu
def test_previews_written(gpu_codec, tmp_path, capsys):
    a = gpu_codec
    assert a.preview_dims(W, H) == (QW, QH)
    rgb = WO.smooth_plus_noise(W, H, F)
    fb = QW * QH * 3
    for version, make, fmt in ((2, a.encode_split, "split"), (3, a.encode_wide, "wide"), (4, a.encode_reversible, "reversible")):
        blob = make(a.FrameEncoder.with_wavelet(80, a.WaveletType.Cdf97), rgb, W, H, F, 64)
        alc, out = tmp_path / f"v{version}.alc", tmp_path / f"v{version}.rgb"
        alc.write_bytes(blob)
        rc, _, err = run(a, ["decode", str(alc), "-o", str(out), "--preview"], capsys)
        assert rc == 0 and f"decoded preview {QW}x{QH} of frames [0, {F}) of {W}x{H}x{F} -> {F * fb} bytes" in err
        whole = np.fromfile(out, np.uint8)
        assert np.array_equal(whole, np.asarray(a.decode_preview(blob, 0, F)))
        for text, (t0, t1) in (("2", (2, 3)), ("1:4", (1, 4)), ("0:5", (0, 5)), ("4", (4, 5))):
            rc, _, err = run(a, ["decode", str(alc), "-o", str(out), "--preview", "--frames", text], capsys)
            assert rc == 0 and f"decoded preview {QW}x{QH} of frames [{t0}, {t1}) of {W}x{H}x{F} -> {(t1 - t0) * fb} bytes" in err
            assert np.array_equal(np.fromfile(out, np.uint8), whole[t0 * fb:t1 * fb]), (version, text)
        rc, _, _ = run(a, ["decode", str(alc), "-o", str(out), "--frames", "3", "--preview", "--format", fmt], capsys)
        assert rc == 0 and np.array_equal(np.fromfile(out, np.uint8), whole[3 * fb:4 * fb])
