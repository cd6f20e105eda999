"""Builds tests/cpp/test_cpp_quality.cpp (the C++ mirror of the quality control in include/alice_codec.hpp) with g++ against
libalice_codec.so and compares its output, line by line, with the same questions put to the Python mirror; with a GPU, its
chosen qualities with the rule of tests/quality_ref.py on the CPU oracle's numbers."""
import math
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quality_ref as Q  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x1000


def _build_and_run(*args):
    exe = os.path.join(tempfile.mkdtemp(prefix="alice_cpp_quality_"), "test_cpp_quality")
    libdir = os.path.join(ROOT, "alice-codec_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_cpp_quality.cpp"), "-L", libdir, "-lalice_codec",
                           "-Wl,-rpath," + libdir, "-o", exe])
    env = dict(os.environ, LD_LIBRARY_PATH=libdir + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    out = subprocess.run([exe, *args], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.splitlines()


def _python_lines(a):
    none, rgb, three = np.zeros(0, np.uint8), np.full(4 * 4 * 2 * 3, 7, np.uint8), np.zeros(3, np.uint8)
    k = a.WaveletType.Cdf53
    lines = [f"psnr {a.psnr_from_sse(123456789, 73728):.17g} {a.psnr_from_sse(1, 1):.17g} {int(math.isinf(a.psnr_from_sse(0, 10)))} "
             f"{int(math.isinf(a.psnr_from_sse(7, 0)))}"]
    data, q, reached, db = a.encode_wide_to_psnr(none, 5, 0, 2, math.inf, a.WaveletType.Haar, 20, 150, 128)
    same = data == a.encode_wide(a.FrameEncoder(20, a.WaveletType.Haar), none, 5, 0, 2, 128)
    lines.append(f"empty wide q={q} reached={int(reached)} inf={int(math.isinf(db))} n={len(data)} same={int(same)}")
    data, q, reached, db = a.encode_split_to_psnr(none, 0, 3, 2, 40.0)
    lines.append(f"empty split q={q} reached={int(reached)} n={len(data)}")

    def attempt(name, fn):
        try:
            fn()
            lines.append(f"{name} ok")
        except a.CodecError as e:
            lines.append(f"{name} error {e.code}")

    attempt("overflow", lambda: a.encode_wide_to_psnr(three, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 30.0, k, 10, 95, 100))
    attempt("buffer", lambda: a.encode_split_to_psnr(three, 0, 4, 4, 30.0, k, 10, 95, 100))
    attempt("lane", lambda: a.encode_wide_to_psnr(rgb, 4, 4, 2, 30.0, k, 60, 50, 16384))
    attempt("range", lambda: a.encode_split_to_psnr(rgb, 4, 4, 2, 30.0, k, 60, 50))
    attempt("negative", lambda: a.encode_wide_to_psnr(rgb, 4, 4, 2, -1.0))
    attempt("nan", lambda: a.encode_split_to_psnr(none, 0, 4, 2, float("nan")))
    attempt("range above 100", lambda: a.encode_wide_to_psnr(none, 0, 4, 2, math.inf, k, 200, 120))
    attempt("format", lambda: a.trial_sse_device(1, P, 8, 8, 2, 1, k, 80))
    attempt("trial dims", lambda: a.trial_sse_device(a.FORMAT_REVERSIBLE, P, 8, 0, 2, 1, k, 80))
    attempt("trial region", lambda: a.trial_sse_device(a.FORMAT_WIDE, P, 8, 8, 2, 1, k, 80, frame_width=10, frame_height=10, origins=[(3, 1)]))
    attempt("sse pitch", lambda: a.rgb_sse_device(P, P, 4, 4, 2, a_pitches=(11, 48), d_frame_sse_ptr=P))
    attempt("sse frame pitch", lambda: a.rgb_sse_device(P, P, 4, 4, 2, b_pitches=(16, 59), d_frame_sse_ptr=P))
    attempt("device lossless", lambda: a._encode_container_to_psnr_device("reversible", P, 8, 8, 2, 1, k, 30.0, P, 4096, 10, 95, 0, 0, 0, None, 0))
    attempt("device range", lambda: a.wide_encode_to_psnr_device(P, 8, 8, 2, 1, k, 30.0, P, 4096, 60, 50))
    return lines


def test_cpp_quality_host_checks_match_python(codec):
    got = _build_and_run()
    want = _python_lines(codec)
    assert got == want
    assert want[1] == "empty wide q=20 reached=1 inf=1 n=1630 same=1" and want[2] == "empty split q=10 reached=1 n=1630"
    assert want[3:] == ["overflow error 3", "buffer error 1", "lane error 2", "range error 2", "negative error 2", "nan error 2",
                        "range above 100 ok", "format error 4", "trial dims error 2", "trial region error 2", "sse pitch error 2",
                        "sse frame pitch error 2", "device lossless error 4", "device range error 2"]


@pytest.mark.gpu
def test_cpp_encode_to_psnr_on_gpu(gpu_codec):
    w, h, f = 32, 24, 4
    i = np.arange(w * h * f * 3, dtype=np.int64)
    rgb = ((i * 37 + i // 97) & 0xFF).astype(np.uint8)
    n = rgb.size
    wide = Q.step_table(Q.FORMAT_WIDE, rgb, w, h, f, 1, 100)
    split = Q.step_table(Q.FORMAT_SPLIT, rgb, w, h, f, 1, 96)
    s = Q.step_of(70)
    t = 0.5 * (Q.psnr_from_sse(wide[s], n) + Q.psnr_from_sse(wide[s - 1], n))
    out = _build_and_run("device", repr(t))
    for line, table, hi in ((out[-2], wide, 100), (out[-1], split, 96)):
        q, reached, _ = Q.choose(table, n, t, 10, hi)
        name = "wide" if hi == 100 else "split"
        assert line == f"device {name} q={q} reached={int(reached)} db={Q.psnr_from_sse(table[Q.step_of(q)], n):.17g}", line
