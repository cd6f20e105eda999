"""Builds tests/cpp/test_cpp_frames.cpp (the C++ mirror of the frame-range calls in include/alice_codec.hpp) with g++
against libalice_codec.so and compares its output, line by line, with the same questions put to the Python mirror."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run(*args):
    exe = os.path.join(tempfile.mkdtemp(prefix="alice_cpp_frames_"), "test_cpp_frames")
    libdir = os.path.join(ROOT, "alice-codec_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_cpp_frames.cpp"), "-L", libdir, "-lalice_codec",
                           "-Wl,-rpath," + libdir, "-o", exe])
    env = dict(os.environ, LD_LIBRARY_PATH=libdir + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    out = subprocess.run([exe, *args], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.splitlines()


def _python_lines(a):
    lines = []
    for wt in (a.WaveletType.Cdf53, a.WaveletType.Cdf97, a.WaveletType.Haar):
        m, e, s = a.frames_window(wt, 64, 31, 1), a.frames_window(wt, 13, 12, 1), a.frames_window(wt, 1, 0, 1)
        lines.append(f"window {int(wt)}: {m[0]} {m[1]}, {e[0]} {e[1]}, {s[0]} {s[1]}")

    def attempt(name, fn):
        try:
            fn()
            lines.append(f"{name} ok")
        except a.CodecError as e:
            lines.append(f"{name} error {e.code}: {str(e).split(': ', 1)[1]}")

    attempt("window count 0", lambda: a.frames_window(a.WaveletType.Cdf53, 8, 0, 0))
    attempt("window past the end", lambda: a.frames_window(a.WaveletType.Cdf53, 8, 7, 2))
    none = np.zeros(0, np.uint8)
    empty = a.encode_wide(a.FrameEncoder.with_wavelet(80, a.WaveletType.Cdf97), none, 0, 4, 4, 64)
    attempt("empty chunk", lambda: a.decode_frames(empty, 0, 1))
    attempt("version 1", lambda: a.decode_frames(empty[:4] + b"\x01" + empty[5:], 0, 1))
    attempt("version 9", lambda: a.decode_frames(empty[:4] + b"\x09" + empty[5:], 0, 1))
    attempt("magic", lambda: a.decode_frames(b"B" + empty[1:4] + b"\x09" + empty[5:], 0, 1))
    attempt("no data", lambda: a.decode_frames(none, 0, 1))
    attempt("device twin without pointers", lambda: a.frames_decode_device(0, 1630, 0, 1, 0))
    return lines


def test_cpp_frames_host_checks_match_python(codec):
    got = _build_and_run()
    want = _python_lines(codec)
    assert got == want
    assert want[:3] == ["window 0: 28 34, 10 14, 0 2", "window 1: 26 36, 8 14, 0 2", "window 2: 28 34, 10 14, 0 2"]
    assert [w.split(" error ")[1][0] for w in want[3:]] == ["2", "2", "2", "4", "4", "4", "4", "9"]
    assert "version 1 has no random access (one serial chain per channel)" in want[6]


@pytest.mark.gpu
def test_cpp_frames_on_gpu(gpu_codec):
    out = _build_and_run("device")
    assert out[-1] == "device frames"
