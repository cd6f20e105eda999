"""`extract` of the command line: the refusals that are host code (no device), and on a GPU the
frames and rectangles written for `--frame K` and `--every N` over files of versions 2, 3 and 4, against decode_frames and
decode_rect per file."""
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
    v3 = tmp_path / "v3.alc"
    v3.write_bytes(_encode_ref(3, rgb, W, H, F, 80, 0, 64))
    v1 = tmp_path / "v1.alc"
    v1.write_bytes(o.encode(rgb, W, H, F, 80, 0))
    rc, _, err = run(codec, ["extract", str(v3), str(v1), "-o", str(out)], capsys)
    assert rc == 1 and "version 1 has no random access (one serial chain per channel)" in err and not out.exists()
    other = tmp_path / "other.alc"
    other.write_bytes(_encode_ref(2, WO.smooth_plus_noise(40, 24, 2), 40, 24, 2, 80, 0, 64))
    rc, _, err = run(codec, ["extract", str(v3), str(other), "-o", str(out)], capsys)
    assert rc == 1 and "output sizes differ" in err and "33x17" in err and "40x24" in err and not out.exists()
    rc, _, err = run(codec, ["extract", str(v3), str(other), "-o", str(out), "--rect", "30,0,5,4"], capsys)
    assert rc == 1 and "does not lie inside the 33x17 frame" in err and not out.exists()
    rc, _, err = run(codec, ["extract", str(v3), "-o", str(out), "--rect", "1,2,0,4"], capsys)
    assert rc == 1 and "--rect wants X,Y,W,H" in err and not out.exists()
    rc, _, err = run(codec, ["extract", str(v3), "-o", str(out), "--frame", "5"], capsys)
    assert rc == 1 and "are not a range of the chunk's 5 frames" in err and not out.exists()
    rc, _, err = run(codec, ["extract", str(v3), "-o", str(out), "--frame", "1", "--every", "2"], capsys)
    assert rc == 1 and "cannot be combined" in err and not out.exists()
    rc, _, err = run(codec, ["extract", str(v3), "-o", str(out), "--every", "0"], capsys)
    assert rc == 1 and "--every wants N >= 1" in err and not out.exists()
    short = tmp_path / "short.alc"
    short.write_bytes(b"ALCC\x03")
    rc, _, err = run(codec, ["extract", str(short), "-o", str(out)], capsys)
    assert rc == 1 and "too short" in err and not out.exists()


@pytest.mark.gpu
def test_frames_and_rectangles_written(gpu_codec, tmp_path, capsys):
    a = gpu_codec
    paths, blobs = [], []
    for i, (make, kind) in enumerate(((a.encode_split, a.WaveletType.Cdf97), (a.encode_wide, a.WaveletType.Cdf53),
                                      (a.encode_reversible, a.WaveletType.Haar), (a.encode_wide, a.WaveletType.Cdf97))):
        blob = make(a.FrameEncoder.with_wavelet(80, kind), WO.smooth_plus_noise(W, H, F, seed=i), W, H, F, 64)
        p = tmp_path / f"clip.{i:05d}.alc"
        p.write_bytes(blob)
        paths.append(str(p))
        blobs.append(blob)
    out = tmp_path / "sheet.rgb"
    for extra, frames in (([], [0]), (["--frame", "3"], [3]), (["--every", "2"], [0, 2, 4]), (["--every", "9"], [0])):
        rc, _, err = run(a, ["extract", *paths, "-o", str(out), *extra], capsys)
        n = len(paths) * len(frames)
        assert rc == 0 and f"wrote {n} frames {W}x{H} of {len(paths)} files -> {n * W * H * 3} bytes" in err, err
        want = np.concatenate([np.asarray(a.decode_frames(blob, t, 1)) for blob in blobs for t in frames])
        assert np.array_equal(np.fromfile(out, np.uint8), want), extra
        rc, _, err = run(a, ["extract", *paths, "-o", str(out), "--rect", "20,9,7,6", *extra], capsys)
        assert rc == 0 and f"wrote {n} rectangles at (20, 9) 7x6 of {len(paths)} files -> {n * 7 * 6 * 3} bytes" in err, err
        want = np.concatenate([np.asarray(a.decode_rect(blob, t, 1, 20, 9, 7, 6)) for blob in blobs for t in frames])
        assert np.array_equal(np.fromfile(out, np.uint8), want), extra
    stats = a._test_last_rects_stats()
    assert stats[0] == len(paths) and stats[1] == len(paths) and stats[2] == 1
