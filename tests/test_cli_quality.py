"""The command line with a PSNR floor: `encode --min-psnr` and `encode-chunks --min-psnr` in the split-stream formats, and
every refusal of the flag."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quality_ref as Q  # noqa: E402
import wide_oracle as WO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = [sys.executable, "-c", "import sys, alice_codec_amd.cli as c; sys.exit(c.main())"]


def _env():
    return dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))


def _run(args):
    return subprocess.run(CLI + args, capture_output=True, text=True, env=_env(), timeout=300)


def test_cli_refuses_min_psnr_where_it_cannot_work(tmp_path):
    """Argument rules only: every one is decided before the input is read or a device is looked for."""
    raw = tmp_path / "missing.rgb"          # never opened
    base = [str(raw), "-o", str(tmp_path / "o.alc"), "-W", "8", "-H", "8", "--min-psnr", "30"]
    cases = [(["encode"] + base, "--min-psnr needs --format split or --format wide"),
             (["encode"] + base + ["--format", "v1"], "--min-psnr needs --format split or --format wide"),
             (["encode"] + base + ["--format", "reversible"], "lossless container"),
             (["encode"] + base + ["--lossless"], "lossless container"),
             (["encode"] + base + ["--format", "split", "--max-bytes", "1000"], "--min-psnr and --max-bytes are two rate controls"),
             (["encode"] + base + ["--format", "wide", "--max-bytes", "1000"], "--min-psnr and --max-bytes are two rate controls"),
             (["encode-chunks"] + base, "--min-psnr needs --format split or --format wide"),
             (["encode-chunks"] + base + ["--format", "reversible"], "no quality to search"),
             (["encode-chunks"] + base + ["--lossless"], "no quality to search"),
             (["encode-chunks"] + base + ["--format", "split", "--kbps", "500"], "--min-psnr and --kbps are two rate controls"),
             (["encode"] + base[:-1] + ["-1", "--format", "wide"], "--min-psnr must be a number of dB >= 0"),
             (["encode"] + base[:-1] + ["nan", "--format", "split"], "--min-psnr must be a number of dB >= 0")]
    for args, word in cases:
        out = _run(args)
        assert out.returncode == 1 and word in out.stderr, (args, out.stderr)
        assert not (tmp_path / "o.alc").exists()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,version", [("split", 2), ("wide", 3)])
def test_cli_min_psnr(gpu_codec, tmp_path, fmt, version):
    a = gpu_codec
    w, h, f = 32, 24, 4
    rgb = WO.smooth_plus_noise(w, h, f, seed=3)
    raw = tmp_path / "in.rgb"
    rgb.tofile(raw)
    common = ["-W", str(w), "-H", str(h), "--format", fmt, "--lane-symbols", "64", "--max-quality", "96"]
    n = rgb.size
    table = Q.step_table(version, rgb, w, h, f, 0, 96)
    t = 0.5 * (Q.psnr_from_sse(table[Q.step_of(60)], n) + Q.psnr_from_sse(table[Q.step_of(60) - 1], n))
    q, reached, _ = Q.choose(table, n, t, 10, 96)
    assert reached and 10 < q < 96
    out = _run(["encode", str(raw), "-o", str(tmp_path / "a.alc"), "-f", str(f), "--min-psnr", repr(t)] + common)
    assert out.returncode == 0, out.stderr
    data = (tmp_path / "a.alc").read_bytes()
    db = Q.psnr_from_sse(table[Q.step_of(q)], n)
    assert f"chosen quality: {q}, measured {db:.2f} dB" in out.stderr and "reached" in out.stderr and "NOT reached" not in out.stderr
    assert "warning" not in out.stderr and f"quality={q}" in out.stderr
    encode = a.encode_split if fmt == "split" else a.encode_wide
    assert a.alc_version(data) == version and data == encode(a.FrameEncoder(q, a.WaveletType.Cdf53), rgb, w, h, f, 64)
    # a floor nothing reaches: max quality, said so
    out = _run(["encode", str(raw), "-o", str(tmp_path / "b.alc"), "-f", str(f), "--min-psnr", "90"] + common)
    assert out.returncode == 0 and "chosen quality: 96" in out.stderr and "NOT reached" in out.stderr
    assert "warning: not even --max-quality 96 reaches 90 dB" in out.stderr
    assert (tmp_path / "b.alc").read_bytes() == encode(a.FrameEncoder(96, a.WaveletType.Cdf53), rgb, w, h, f, 64)
    # encode-chunks: one line per chunk with its own choice
    parts = [WO.smooth_plus_noise(w, h, 4, seed=40 + i) for i in range(3)]
    np.concatenate(parts).tofile(tmp_path / "long.rgb")
    out = _run(["encode-chunks", str(tmp_path / "long.rgb"), "-o", str(tmp_path / "c"), "-c", "4", "--min-psnr", repr(t)] + common)
    assert out.returncode == 0, out.stderr
    lines = [x for x in out.stderr.splitlines() if x.startswith("chunk ")]
    assert len(lines) == 3
    for k, part in enumerate(parts):
        tk = Q.step_table(version, part, w, h, 4, 0, 96)
        qk, rk, _ = Q.choose(tk, n, t, 10, 96)
        m = re.match(rf"chunk {k}: frames {4 * k}\.\.{4 * k + 3} -> (\d+) bytes, chosen quality: (\d+), measured ([0-9.]+|inf) dB, floor .* dB (reached|NOT reached)$",
                     lines[k])
        assert m, lines[k]
        data = (tmp_path / f"c.{k:05d}.alc").read_bytes()
        assert (int(m.group(1)), int(m.group(2)), m.group(4) == "reached") == (len(data), qk, rk)
        assert m.group(3) == f"{Q.psnr_from_sse(tk[Q.step_of(qk)], n):.2f}"
        assert data == encode(a.FrameEncoder(qk, a.WaveletType.Cdf53), part, w, h, 4, 64)
