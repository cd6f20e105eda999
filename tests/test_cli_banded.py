"""`--banded` and `repack` of the command line: the refusals, each pointing at `repack`, the info of
a version 5 file and the refusals of the partial calls (host code, no device); on a GPU the encode / info / decode round
trip and the repack in both directions."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import banded_ref as B  # noqa: E402
import wide_oracle as WO  # noqa: E402


def run(argv, capsys):
    from alice_codec_amd import cli
    rc = cli.main(argv)
    cap = capsys.readouterr()
    return rc, cap.out, cap.err


@pytest.fixture
def tiny(tmp_path):
    src = tmp_path / "in.rgb"
    np.zeros(4 * 4 * 2 * 3, np.uint8).tofile(src)
    return src


def test_banded_refusals_point_at_repack(codec, tiny, tmp_path, capsys):
    out = tmp_path / "o.alc"
    base = ["encode", str(tiny), "-o", str(out), "-W", "4", "-H", "4", "-f", "2", "--banded"]
    chunks = ["encode-chunks", str(tiny), "-o", str(tmp_path / "c"), "-W", "4", "-H", "4", "-c", "2", "--banded"]
    for argv, flag in ((base, "--format split"), (base + ["--format", "v1"], "--format split"),
                       (base + ["--format", "split", "--max-bytes", "5000"], "--max-bytes"),
                       (base + ["--format", "wide", "--min-psnr", "40"], "--min-psnr"),
                       (base + ["--lossless", "--max-bytes", "5000"], "--max-bytes"),
                       (chunks, "--format split"), (chunks + ["--format", "split", "--kbps", "100"], "--kbps"),
                       (chunks + ["--format", "split", "--min-psnr", "40"], "--min-psnr")):
        rc, _, err = run(argv, capsys)
        assert rc == 1 and "--banded" in err and flag in err and "repack" in err, (argv, err)
        assert not out.exists() and not list(tmp_path.glob("c.*"))
    rc, _, err = run(["repack", str(tiny), "-o", str(out)], capsys)
    assert rc == 1 and "exactly one of --banded and --plain" in err
    rc, _, err = run(["repack", str(tiny), "-o", str(out), "--banded", "--plain"], capsys)
    assert rc == 1 and "exactly one of --banded and --plain" in err and not out.exists()


def test_info_and_refusals_of_a_version_5_file(codec, tmp_path, capsys):
    w, h, f = 6, 4, 2
    data = B.encode(WO.smooth_plus_noise(w, h, f), w, h, f, 80, 1, 3, 64)
    p = tmp_path / "b.alc"
    p.write_bytes(data)
    rc, out, _ = run(["info", str(p)], capsys)
    lines = out.splitlines()
    info = B.parse_container(data)
    assert rc == 0 and "  Format:      banded split-stream (version 5)" in lines and "  Base:        version 3" in lines
    assert "  Lane length: 64 symbols, 24 blocks" in lines and "  Wavelet:     CDF 9/7" in lines
    for c, name in enumerate(("Y:", "Co:", "Cg:")):
        want = f"  Bands {name:4s}   " + " ".join(str(v) for v in info["payload_len"][8 * c:8 * c + 8]) + " bytes"
        assert want in lines, (want, lines)
    assert f"  Payload:     {len(data) - B.HEADER} bytes" in lines
    for fmt, ver in (("split", 2), ("wide", 3), ("reversible", 4), ("v1", 1)):
        rc, _, err = run(["info", str(p), "--format", fmt], capsys)
        assert rc == 1 and f"unsupported version: 5 (expected {ver})" in err
    back = tmp_path / "x.rgb"
    for extra in (["--frames", "0"], ["--preview"], ["--rect", "0,0,2,2"]):
        rc, _, err = run(["decode", str(p), "-o", str(back)] + extra, capsys)
        assert rc == 1 and "unsupported version: 5" in err, (extra, err)
    for argv in (["thumbnails", str(p), "-o", str(back)], ["extract", str(p), "-o", str(back)],
                 ["transcode", str(p), "-o", str(back), "-q", "50"], ["repack", str(p), "-o", str(back), "--banded"]):
        rc, _, err = run(argv, capsys)
        assert rc == 1 and "unsupported version: 5" in err, (argv, err)
    p.write_bytes(data[:-1])
    rc, _, err = run(["info", str(p)], capsys)
    assert rc == 1 and "length mismatch" in err
    # an empty chunk goes through encode, repack and decode without a device
    src, e5, e2 = tmp_path / "none.rgb", tmp_path / "e5.alc", tmp_path / "e2.alc"
    src.write_bytes(b"")
    rc, _, err = run(["encode", str(src), "-o", str(e5), "-W", "0", "-H", "4", "-f", "2", "--format", "split", "--banded"], capsys)
    assert rc == 0 and "format=banded split" in err and e5.stat().st_size == 12636
    rc, _, err = run(["repack", str(e5), "-o", str(e2), "--plain", "--lane-symbols", "128"], capsys)
    assert rc == 0 and "version 2" in err and "lane_symbols 128" in err
    assert e2.read_bytes() == codec.encode_split(codec.FrameEncoder.with_wavelet(90, codec.WaveletType.Cdf53), np.zeros(0, np.uint8), 0, 4, 2, 128)
    rc, _, err = run(["decode", str(e5), "-o", str(back)], capsys)
    assert rc == 0 and "decoded 0x4x2" in err and back.stat().st_size == 0


@pytest.mark.gpu
def test_banded_encode_info_decode_and_repack(gpu_codec, tmp_path, capsys):
    a = gpu_codec
    w, h, f = 32, 24, 4
    rgb = WO.smooth_plus_noise(w, h, f)
    src, alc, back, plain, again = (tmp_path / n for n in ("in.rgb", "o.alc", "back.rgb", "p.alc", "b.alc"))
    rgb.tofile(src)
    dims = ["-W", str(w), "-H", str(h), "-f", str(f), "-w", "cdf97", "--lane-symbols", "64"]
    rc, _, err = run(["encode", str(src), "-o", str(alc), "--format", "split", "--banded", "-q", "80"] + dims, capsys)
    assert rc == 0 and "format=banded split" in err
    data = alc.read_bytes()
    assert data == B.encode(rgb, w, h, f, 80, 1, 2, 64)
    rc, out, _ = run(["info", str(alc)], capsys)
    assert rc == 0 and "version 5" in out and "Base:        version 2" in out and f"File size:   {len(data)} bytes" in out
    rc, _, _ = run(["decode", str(alc), "-o", str(back)], capsys)
    enc = a.FrameEncoder.with_wavelet(80, a.WaveletType.Cdf97)
    v2 = a.encode_split(enc, rgb, w, h, f, 64)
    assert rc == 0 and np.array_equal(np.fromfile(back, np.uint8), a.decode_split(v2))
    # repack both ways
    rc, _, err = run(["repack", str(alc), "-o", str(plain), "--plain"], capsys)
    assert rc == 0 and "version 2" in err and plain.read_bytes() == v2
    rc, _, err = run(["repack", str(plain), "-o", str(again), "--banded"], capsys)
    assert rc == 0 and "version 5" in err and again.read_bytes() == data
    rc, _, err = run(["repack", str(plain), "-o", str(again), "--banded", "--lane-symbols", "128"], capsys)
    assert rc == 0 and "lane_symbols 128" in err and again.read_bytes() == a.encode_banded(enc, rgb, w, h, f, 128, 2)
    # --lossless --banded: base 4 at quality 100 returns the input
    rc, _, err = run(["encode", str(src), "-o", str(alc), "--lossless", "--banded"] + dims, capsys)
    assert rc == 0 and "format=banded reversible" in err and "quality=100" in err
    assert alc.read_bytes() == a.encode_banded(a.FrameEncoder.with_wavelet(100, a.WaveletType.Cdf97), rgb, w, h, f, 64, 4)
    rc, _, _ = run(["decode", str(alc), "-o", str(back)], capsys)
    assert rc == 0 and np.array_equal(np.fromfile(back, np.uint8), rgb)
    # chunks: two 2-frame files
    rc, _, _ = run(["encode-chunks", str(src), "-o", str(tmp_path / "c"), "-W", str(w), "-H", str(h), "-c", "2", "--format", "wide", "--banded",
                    "-q", "80", "--lane-symbols", "64"], capsys)
    assert rc == 0
    fb = w * h * 3
    enc53 = a.FrameEncoder.with_wavelet(80, a.WaveletType.Cdf53)
    assert (tmp_path / "c.00001.alc").read_bytes() == a.encode_banded(enc53, rgb[2 * fb:], w, h, 2, 64, 3)
