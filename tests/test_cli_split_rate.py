"""The command line with byte budgets in the split-stream format: `encode --format split --max-bytes` and
`encode-chunks --format split --kbps`."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _source(seed, w, h, f, noise=12):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = ((x[None] * 3 + y[None] * 2 + np.arange(f)[:, None, None] * 5) % 256).astype(np.int16)
    rgb = np.stack([base, 255 - base, (base * 7) % 256], axis=3) + rng.integers(-noise, noise + 1, (f, h, w, 3))
    return np.clip(rgb, 0, 255).astype(np.uint8).reshape(-1)


def test_cli_budgets_in_v2(gpu_codec, tmp_path):
    a = gpu_codec
    w, h, f = 32, 24, 4
    rgb = _source(500, w, h, f)
    raw = tmp_path / "in.rgb"
    rgb.tofile(raw)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cli = [sys.executable, "-c", "import sys, alice_codec_amd.cli as c; sys.exit(c.main())"]
    common = ["-W", str(w), "-H", str(h), "--format", "split", "--lane-symbols", "64"]
    budget = int(a.predict_split_sizes(rgb, w, h, f, 0, 64).hi[60])
    want, q, fits = a.encode_split_to_size(rgb, w, h, f, budget, 0, 10, 95, 64)
    out = subprocess.run(cli + ["encode", str(raw), "-o", str(tmp_path / "a.alc"), "-f", str(f), "--max-bytes", str(budget)] + common,
                         capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr
    data = (tmp_path / "a.alc").read_bytes()
    assert fits and q >= 60 and f"chosen quality: {q}" in out.stderr and "warning" not in out.stderr
    assert a.alc_version(data) == 2 and len(data) <= budget and data == want
    assert a.decode_split(data).size == rgb.size
    out = subprocess.run(cli + ["encode", str(raw), "-o", str(tmp_path / "b.alc"), "-f", str(f), "--max-bytes", "10"] + common,
                         capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and "warning: not even --min-quality 10 is guaranteed to fit 10 bytes" in out.stderr
    assert a.alc_version((tmp_path / "b.alc").read_bytes()) == 2
    # encode-chunks at a bitrate: 3 chunks of 4 frames, each within floor(target_bits_per_frame * 4 / 8) bytes
    long = np.concatenate([_source(600 + i, w, h, 4) for i in range(3)])
    long.tofile(tmp_path / "long.rgb")
    kbps, fps = 2000, 30.0
    out = subprocess.run(cli + ["encode-chunks", str(tmp_path / "long.rgb"), "-o", str(tmp_path / "c"), "-c", "4", "--kbps", str(kbps),
                                "--fps", str(fps)] + common, capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr
    budget = a.budget_bytes_per_chunk(kbps, fps, 4)
    for k in range(3):
        data = (tmp_path / f"c.{k:05d}.alc").read_bytes()
        part = long[k * w * h * 4 * 3:(k + 1) * w * h * 4 * 3]
        want, qk, fk = a.encode_split_to_size(part, w, h, 4, budget, 0, 10, 95, 64)
        assert f"chunk {k}:" in out.stderr and f"chosen quality: {qk}" in out.stderr
        assert fk and data == want and len(data) <= budget
        assert a.decode_split(data).size == part.size
