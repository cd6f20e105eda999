"""Builds tests/cpp/test_cpp_wide_rate.cpp (the C++ mirror of the version 3 rate control in include/alice_codec.hpp) with
g++ against libalice_codec.so and compares its output, line by line, with the same questions put to the Python mirror."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run(*args):
    exe = os.path.join(tempfile.mkdtemp(prefix="alice_cpp_wide_rate_"), "test_cpp_wide_rate")
    libdir = os.path.join(ROOT, "alice-codec_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_cpp_wide_rate.cpp"), "-L", libdir, "-lalice_codec",
                           "-Wl,-rpath," + libdir, "-o", exe])
    env = dict(os.environ, LD_LIBRARY_PATH=libdir + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    out = subprocess.run([exe, *args], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.splitlines()


def _python_lines(a):
    none, rgb, three = np.zeros(0, np.uint8), np.full(4 * 4 * 2 * 3, 7, np.uint8), np.zeros(3, np.uint8)
    p = a.predict_wide_sizes(none, 0, 7, 3)
    lines = [f"empty {p.lo[0]} {p.hi[0]} {p.lo[100]} {p.hi[100]} {p.status[50]}"]
    data, q, fits = a.encode_wide_to_size(none, 5, 0, 2, 10000, a.WaveletType.Haar, 20, 150, 128)
    same = data == a.encode_wide(a.FrameEncoder(100, a.WaveletType.Haar), none, 5, 0, 2, 128)
    lines.append(f"empty fits q={q} fits={int(fits)} n={len(data)} same={int(same)}")
    data, q, fits = a.encode_wide_to_size(none, 5, 0, 2, a.SPLIT_HEADER_BYTES - 1, a.WaveletType.Cdf53, 20, 30)
    lines.append(f"empty short q={q} fits={int(fits)} n={len(data)}")

    def attempt(name, fn):
        try:
            fn()
            lines.append(f"{name} ok")
        except a.CodecError as e:
            lines.append(f"{name} error {e.code}")

    attempt("overflow", lambda: a.predict_wide_sizes(three, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, a.WaveletType.Cdf53, 100))
    attempt("buffer", lambda: a.predict_wide_sizes(three, 0, 4, 4, a.WaveletType.Cdf53, 100))
    attempt("lane", lambda: a.predict_wide_sizes(rgb, 4, 4, 2, a.WaveletType.Cdf53, 100))
    attempt("lane 16384", lambda: a.predict_wide_sizes(rgb, 4, 4, 2, a.WaveletType.Cdf53, 16384))
    attempt("lane 8192", lambda: a.predict_wide_sizes(none, 0, 4, 2, a.WaveletType.Cdf53, 8192))
    attempt("lane before range", lambda: a.encode_wide_to_size(rgb, 4, 4, 2, 10000, a.WaveletType.Cdf53, 60, 50, 100))
    attempt("range", lambda: a.encode_wide_to_size(none, 0, 4, 2, 10000, a.WaveletType.Cdf53, 60, 50))
    attempt("range above 100", lambda: a.encode_wide_to_size(none, 0, 4, 2, 10000, a.WaveletType.Cdf53, 200, 120))
    return lines


def test_cpp_wide_rate_host_checks_match_python(codec):
    got = _build_and_run()
    want = _python_lines(codec)
    assert got == want
    assert want[0] == "empty 1630 1630 1630 1630 0" and want[3:] == ["overflow error 3", "buffer error 1", "lane error 2",
                                                                      "lane 16384 error 2", "lane 8192 ok", "lane before range error 2", "range error 2", "range above 100 ok"]


@pytest.mark.gpu
def test_cpp_encode_wide_to_size_on_gpu(gpu_codec):
    out = _build_and_run("device")
    assert out[-1].startswith("device q=")
