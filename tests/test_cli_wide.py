"""`--format wide` of the command line: refused together with a byte budget (host code, no device), and on a GPU the
encode / info / decode round trip of a version 3 file."""
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


def test_wide_with_a_byte_budget_is_refused(codec, tmp_path, capsys):
    src = tmp_path / "in.rgb"
    np.zeros(4 * 4 * 2 * 3, np.uint8).tofile(src)
    out = tmp_path / "o.alc"
    rc, _, err = run(codec, ["encode", str(src), "-o", str(out), "-W", "4", "-H", "4", "-f", "2", "--format", "wide", "--max-bytes", "5000"], capsys)
    assert rc == 1 and "--format wide" in err and "--max-bytes" in err and not out.exists()
    rc, _, err = run(codec, ["encode-chunks", str(src), "-o", str(tmp_path / "c"), "-W", "4", "-H", "4", "-c", "2", "--format", "wide",
                             "--kbps", "100"], capsys)
    assert rc == 1 and "--format wide" in err and "--kbps" in err and not list(tmp_path.glob("c.*"))


def test_info_of_an_empty_wide_file_and_forced_formats(codec, tmp_path, capsys):
    data = codec.encode_wide(codec.FrameEncoder.with_wavelet(100, codec.WaveletType.Haar), np.zeros(0, np.uint8), 0, 6, 2)
    p = tmp_path / "e.alc"
    p.write_bytes(data)
    rc, out, _ = run(codec, ["info", str(p)], capsys)
    assert rc == 0 and "version 3" in out and "Haar" in out
    rc, _, err = run(codec, ["info", str(p), "--format", "split"], capsys)
    assert rc == 1 and "unsupported version: 3 (expected 2)" in err
    rc, _, err = run(codec, ["decode", str(p), "-o", str(tmp_path / "x.rgb"), "--format", "v1"], capsys)
    assert rc == 1 and "InvalidBitstream" in err     # (the v1 parser asks for its 3138 header bytes before the version)


@pytest.mark.gpu
def test_wide_encode_info_decode_round_trip(gpu_codec, tmp_path, capsys):
    w, h, f = 32, 24, 4
    rgb = WO.smooth_plus_noise(w, h, f)
    src, alc, back = tmp_path / "in.rgb", tmp_path / "o.alc", tmp_path / "back.rgb"
    rgb.tofile(src)
    rc, _, err = run(gpu_codec, ["encode", str(src), "-o", str(alc), "-W", str(w), "-H", str(h), "-f", str(f), "-q", "100", "-w", "cdf97",
                                 "--format", "wide", "--lane-symbols", "64"], capsys)
    assert rc == 0 and "format=wide" in err
    data = alc.read_bytes()
    assert data == gpu_codec.encode_wide(gpu_codec.FrameEncoder.with_wavelet(100, gpu_codec.WaveletType.Cdf97), rgb, w, h, f, 64)
    rc, out, _ = run(gpu_codec, ["info", str(alc)], capsys)
    assert rc == 0 and "version 3" in out and "Lane length: 64" in out
    rc, _, _ = run(gpu_codec, ["decode", str(alc), "-o", str(back)], capsys)
    assert rc == 0 and np.array_equal(np.fromfile(back, np.uint8), gpu_codec.decode_wide(data))
    assert WO.psnr(rgb, np.fromfile(back, np.uint8)) > 35
