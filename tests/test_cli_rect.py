"""`decode --rect X,Y,W,H` of the command line: the refusals that are host code (no device), and on a
GPU the rectangles written for `--rect` alone and with `--frames A[:B]` from files of versions 2, 3 and 4."""
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


def test_refusals_without_a_device(codec, tmp_path, capsys):
    rgb = WO.smooth_plus_noise(W, H, F)
    out = tmp_path / "o.rgb"
    v1 = tmp_path / "v1.alc"
    v1.write_bytes(o.encode(rgb, W, H, F, 80, 0))
    for extra in ([], ["--frames", "2"]):
        rc, _, err = run(codec, ["decode", str(v1), "-o", str(out), "--rect", "1,2,3,4", *extra], capsys)
        assert rc == 1 and "version 1 has no random access (one serial chain per channel)" in err and not out.exists()
    v3 = tmp_path / "v3.alc"
    v3.write_bytes(_encode_ref(3, rgb, W, H, F, 80, 0, 64))
    for bad in ("1,2,3", "1,2,3,4,5", "a,2,3,4", "1,2,0,4", "1,2,3,0", "-1,2,3,4", "", "1;2;3;4", "1,2,3,4294967296"):
        rc, _, err = run(codec, ["decode", str(v3), "-o", str(out), f"--rect={bad}"], capsys)
        assert rc == 1 and "--rect wants X,Y,W,H" in err and not out.exists(), bad
    for outside in ("33,0,1,1", "0,17,1,1", "1,0,33,1", "0,1,1,17", "4294967295,0,2,1"):
        rc, _, err = run(codec, ["decode", str(v3), "-o", str(out), "--rect", outside], capsys)
        assert rc == 1 and "rectangle" in err and "33x17 frame" in err and not out.exists(), outside
    for bad in ("2:2", "x", "4:1"):
        rc, _, err = run(codec, ["decode", str(v3), "-o", str(out), "--rect", "1,2,3,4", "--frames", bad], capsys)
        assert rc == 1 and "--frames wants A or A:B" in err and not out.exists()
    for outside in ("5", "3:6", "0:9"):
        rc, _, err = run(codec, ["decode", str(v3), "-o", str(out), "--rect", "1,2,3,4", "--frames", outside], capsys)
        assert rc == 1 and "are not a range of the chunk's 5 frames" in err and not out.exists()
    for extra in ([], ["--frames", "2"]):
        rc, _, err = run(codec, ["decode", str(v3), "-o", str(out), "--rect", "1,2,3,4", "--preview", *extra], capsys)
        assert rc == 1 and "--rect and --preview cannot be combined" in err and not out.exists()
    rc, _, err = run(codec, ["decode", str(v3), "-o", str(out), "--rect", "1,2,3,4", "--format", "split"], capsys)
    assert rc == 1 and "--format split names version 2, the file's version byte is 3" in err and not out.exists()
    short = tmp_path / "short.alc"
    short.write_bytes(b"ALCC\x03")
    rc, _, err = run(codec, ["decode", str(short), "-o", str(out), "--rect", "1,2,3,4"], capsys)
    assert rc == 1 and "too short" in err and not out.exists()


@pytest.mark.gpu
def test_rectangles_written(gpu_codec, tmp_path, capsys):
    a = gpu_codec
    rgb = WO.smooth_plus_noise(W, H, F)
    for version, make, fmt in ((2, a.encode_split, "split"), (3, a.encode_wide, "wide"), (4, a.encode_reversible, "reversible")):
        blob = make(a.FrameEncoder.with_wavelet(80, a.WaveletType.Cdf97), rgb, W, H, F, 64)
        full = np.asarray({2: a.decode_split, 3: a.decode_wide, 4: a.decode_reversible}[version](blob)).reshape(F, H, W, 3)
        alc, out = tmp_path / f"v{version}.alc", tmp_path / f"v{version}.rgb"
        alc.write_bytes(blob)
        for x, y, w, h in ((0, 0, W, H), (5, 3, 7, 4), (32, 16, 1, 1), (0, 14, 33, 3)):
            text = f"{x},{y},{w},{h}"
            fb = w * h * 3
            rc, _, err = run(a, ["decode", str(alc), "-o", str(out), "--rect", text], capsys)
            assert rc == 0 and f"decoded rectangle {w}x{h} at ({x}, {y}) of frames [0, {F}) of {W}x{H}x{F} -> {F * fb} bytes" in err
            whole = np.fromfile(out, np.uint8)
            assert np.array_equal(whole, full[:, y:y + h, x:x + w].reshape(-1)), (version, text)
            for frames, (t0, t1) in (("2", (2, 3)), ("1:4", (1, 4)), ("0:5", (0, 5)), ("4", (4, 5))):
                rc, _, err = run(a, ["decode", str(alc), "-o", str(out), "--rect", text, "--frames", frames], capsys)
                assert rc == 0 and f"of frames [{t0}, {t1}) of {W}x{H}x{F} -> {(t1 - t0) * fb} bytes" in err
                assert np.array_equal(np.fromfile(out, np.uint8), whole[t0 * fb:t1 * fb]), (version, text, frames)
        rc, _, _ = run(a, ["decode", str(alc), "-o", str(out), "--frames", "3", "--rect", "5,3,7,4", "--format", fmt], capsys)
        assert rc == 0 and np.array_equal(np.fromfile(out, np.uint8), full[3:4, 3:7, 5:12].reshape(-1))
