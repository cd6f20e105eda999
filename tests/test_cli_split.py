"""CLI: `encode --format split` -> `info` -> `decode` on a small file, and the default encode still writes the oracle's
version 1 bytes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_ref as R  # noqa: E402


def test_info_reads_a_split_file_without_a_device(codec, tmp_path, capsys):
    from alice_codec_amd import cli
    rng = np.random.default_rng(1)
    sym = [rng.integers(0, 7, 6 * 4 * 2).astype(np.uint8) for _ in range(3)]
    p = tmp_path / "a.alc"
    p.write_bytes(R.write_container(1, 6, 4, 2, 64, [9, 9, 9], sym))
    assert cli.main(["info", str(p)]) == 0
    out = capsys.readouterr().out.splitlines()
    assert "  Format:      split-stream (version 2)" in out and "  Wavelet:     CDF 9/7" in out
    assert "  Lane length: 64 symbols, 3 blocks" in out and "  Raw size:    144 bytes (uncompressed RGB)" in out
    p.write_bytes(p.read_bytes()[:-1])
    assert cli.main(["info", str(p)]) == 1
    assert "length mismatch" in capsys.readouterr().err


@pytest.mark.gpu
def test_cli_split_round_trip_and_default_stays_v1(gpu_codec, oracle_mod, tmp_path, capsys):
    from alice_codec_amd import cli
    w, h, f = 48, 32, 10
    t, y, x = np.meshgrid(np.arange(f), np.arange(h), np.arange(w), indexing="ij")
    rgb = np.stack([(x * 5 + t) % 256, (y * 7 + 2 * t) % 256, (x + y) % 256], axis=-1).astype(np.uint8).reshape(-1)
    raw = tmp_path / "in.rgb"; rgb.tofile(raw)
    alc = tmp_path / "out.alc"
    base = ["-W", str(w), "-H", str(h), "-f", str(f), "-q", "80", "-w", "cdf97"]
    assert cli.main(["encode", str(raw), "-o", str(alc), "--format", "split", "--lane-symbols", "128"] + base) == 0
    data = alc.read_bytes()
    sym = oracle_mod.encode_symbols(rgb, w, h, f, 80, 1).reshape(3, -1)
    assert data == R.write_container(1, w, h, f, 128, [14] * 3, sym)
    capsys.readouterr()
    assert cli.main(["info", str(alc)]) == 0
    out = capsys.readouterr().out
    assert "split-stream (version 2)" in out and "Lane length: 128 symbols" in out and f"File size:   {len(data)} bytes" in out
    dec = tmp_path / "dec.rgb"
    assert cli.main(["decode", str(alc), "-o", str(dec)]) == 0
    assert np.array_equal(np.fromfile(dec, np.uint8), gpu_codec.decode_split(data))
    # chunk driver
    assert cli.main(["encode-chunks", str(raw), "-o", str(tmp_path / "c"), "-W", str(w), "-H", str(h), "-c", "4", "-q", "80",
                     "-w", "cdf97", "--format", "split"]) == 0
    fb = w * h * 3
    enc = gpu_codec.FrameEncoder.with_wavelet(80, gpu_codec.WaveletType.Cdf97)
    assert (tmp_path / "c.00002.alc").read_bytes() == gpu_codec.encode_split(enc, rgb[8 * fb:], w, h, 2)
    # the default of every subcommand stays version 1
    v1 = tmp_path / "v1.alc"
    assert cli.main(["encode", str(raw), "-o", str(v1)] + base) == 0
    assert v1.read_bytes() == oracle_mod.encode(rgb, w, h, f, 80, 1)
