"""Builds tests/cpp/test_cpp_preview.cpp (the C++ mirror of the preview calls in include/alice_codec.hpp) with g++ against
libalice_codec.so and compares its output, line by line, with the same questions put to the Python mirror."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run(*args):
    exe = os.path.join(tempfile.mkdtemp(prefix="alice_cpp_preview_"), "test_cpp_preview")
    libdir = os.path.join(ROOT, "alice-codec_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_cpp_preview.cpp"), "-L", libdir, "-lalice_codec",
                           "-Wl,-rpath," + libdir, "-o", exe])
    env = dict(os.environ, LD_LIBRARY_PATH=libdir + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    out = subprocess.run([exe, *args], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.splitlines()


def _python_lines(a):
    lines = []
    for w, h in ((1, 1), (33, 17), (1920, 1080), (0xFFFFFFFF, 2)):
        qw, qh = a.preview_dims(w, h)
        lines.append(f"dims {w} {h}: {qw} {qh}")

    def attempt(name, fn):
        try:
            fn()
            lines.append(f"{name} ok")
        except a.CodecError as e:
            lines.append(f"{name} error {e.code}: {str(e).split(': ', 1)[1]}")

    attempt("dims width 0", lambda: a.preview_dims(0, 4))
    attempt("dims height 0", lambda: a.preview_dims(4, 0))
    none = np.zeros(0, np.uint8)
    empty = a.encode_wide(a.FrameEncoder.with_wavelet(80, a.WaveletType.Cdf97), none, 0, 4, 4, 64)
    attempt("empty chunk", lambda: a.decode_preview(empty, 0, 1))
    attempt("version 1", lambda: a.decode_preview(empty[:4] + b"\x01" + empty[5:], 0, 1))
    attempt("version 9", lambda: a.decode_preview(empty[:4] + b"\x09" + empty[5:], 0, 1))
    attempt("magic", lambda: a.decode_preview(b"B" + empty[1:4] + b"\x09" + empty[5:], 0, 1))
    attempt("no data", lambda: a.decode_preview(none, 0, 1))
    attempt("device twin without pointers", lambda: a.preview_decode_device(0, 1630, 0, 1, 0))
    return lines


def test_cpp_preview_host_checks_match_python(codec):
    got = _build_and_run()
    want = _python_lines(codec)
    assert got == want
    assert want[:4] == ["dims 1 1: 1 1", "dims 33 17: 17 9", "dims 1920 1080: 960 540", "dims 4294967295 2: 2147483648 1"]
    assert [w.split(" error ")[1][0] for w in want[4:]] == ["2", "2", "2", "4", "4", "4", "4", "9"]
    assert "version 1 has no random access (one serial chain per channel)" in want[7]


@pytest.mark.gpu
def test_cpp_preview_on_gpu(gpu_codec):
    out = _build_and_run("device")
    assert out[-1] == "device previews"
