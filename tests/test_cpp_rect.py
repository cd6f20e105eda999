"""Builds tests/cpp/test_cpp_rect.cpp (the C++ mirror of the rectangle calls in include/alice_codec.hpp) with g++ against
libalice_codec.so and compares its output, line by line, with the same questions put to the Python mirror."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run(*args):
    exe = os.path.join(tempfile.mkdtemp(prefix="alice_cpp_rect_"), "test_cpp_rect")
    libdir = os.path.join(ROOT, "alice-codec_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_cpp_rect.cpp"), "-L", libdir, "-lalice_codec",
                           "-Wl,-rpath," + libdir, "-o", exe])
    env = dict(os.environ, LD_LIBRARY_PATH=libdir + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    out = subprocess.run([exe, *args], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.splitlines()


def _python_lines(a):
    lines = []
    for kind in (0, 1, 2):
        for c in ((1, 1, 0, 0, 1, 1), (33, 17, 32, 16, 1, 1), (1920, 1080, 832, 412, 256, 256), (1920, 1080, 0, 0, 1920, 1080),
                  (0xFFFFFFFE, 6, 0xFFFFFFF0, 2, 3, 1)):
            v = a.rect_window(a.WaveletType(kind), *c)
            lines.append("window %d %d %d %d %d %d %d: %d %d %d %d" % ((kind,) + c + v))

    def attempt(name, fn):
        try:
            fn()
            lines.append(f"{name} ok")
        except a.CodecError as e:
            lines.append(f"{name} error {e.code}: {str(e).split(': ', 1)[1]}")

    attempt("window empty", lambda: a.rect_window(a.WaveletType.Cdf53, 8, 8, 0, 0, 0, 1))
    attempt("window outside", lambda: a.rect_window(a.WaveletType.Cdf53, 8, 8, 4, 0, 5, 1))
    attempt("window overflow", lambda: a.rect_window(a.WaveletType.Cdf53, 0xFFFFFFFF, 8, 0, 0, 1, 1))
    none = np.zeros(0, np.uint8)
    empty = a.encode_wide(a.FrameEncoder.with_wavelet(80, a.WaveletType.Cdf97), none, 0, 4, 4, 64)
    one = (0, 0, 1, 1)
    attempt("empty chunk", lambda: a.decode_rect(empty, 0, 1, *one))
    attempt("version 1", lambda: a.decode_rect(empty[:4] + b"\x01" + empty[5:], 0, 1, *one))
    attempt("version 9", lambda: a.decode_rect(empty[:4] + b"\x09" + empty[5:], 0, 1, *one))
    attempt("magic", lambda: a.decode_rect(b"B" + empty[1:4] + b"\x09" + empty[5:], 0, 1, *one))
    attempt("no data", lambda: a.decode_rect(none, 0, 1, *one))
    attempt("device twin without pointers", lambda: a.rect_decode_device(0, 1630, 0, 1, *one, 0))
    return lines


def test_cpp_rect_host_checks_match_python(codec):
    got = _build_and_run()
    want = _python_lines(codec)
    assert got == want
    assert want[5 + 2] == "window 1 1920 1080 832 412 256 256: 828 1092 408 672"
    assert want[1] == "window 0 33 17 32 16 1 1: 30 34 14 18"
    assert [w.split(" error ")[1][0] for w in want[15:]] == ["2", "2", "3", "2", "4", "4", "4", "4", "9"]
    assert "version 1 has no random access (one serial chain per channel)" in want[19]


@pytest.mark.gpu
def test_cpp_rect_on_gpu(gpu_codec):
    out = _build_and_run("device")
    assert out[-1] == "device rectangles"
