"""Builds tests/cpp/test_cpp_banded_partial.cpp (the C++ mirror of the frame-range and preview calls on version 5 chunks in
include/alice_codec.hpp) with g++ against libalice_codec.so and compares its output, line by line, with the same questions
put to the Python mirror."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run(*args):
    exe = os.path.join(tempfile.mkdtemp(prefix="alice_cpp_banded_partial_"), "test_cpp_banded_partial")
    libdir = os.path.join(ROOT, "alice-codec_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_cpp_banded_partial.cpp"), "-L", libdir, "-lalice_codec",
                           "-Wl,-rpath," + libdir, "-o", exe])
    env = dict(os.environ, LD_LIBRARY_PATH=libdir + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    out = subprocess.run([exe, *args], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.splitlines()


def _python_lines(a):
    none = np.zeros(0, np.uint8)
    enc = a.FrameEncoder.with_wavelet(50, a.WaveletType.Cdf97)
    e5, e3 = a.encode_banded(enc, none, 5, 0, 2, 128, 3), a.encode_wide(enc, none, 5, 0, 2, 128)
    magic, reserved = bytearray(e5), bytearray(e5)
    magic[0] = ord("B")
    reserved[23] = 1
    lines = []

    def attempt(name, fn):
        try:
            fn()
            lines.append(f"{name} ok")
        except a.CodecError as e:
            lines.append(f"{name} error {e.code}: {str(e).split(': ', 1)[1]}")

    attempt("frames of an empty chunk", lambda: a.decode_banded_frames(e5, 0, 1))
    attempt("preview of an empty chunk", lambda: a.decode_banded_preview(e5, 0, 1))
    attempt("frames count 0", lambda: a.decode_banded_frames(e5, 1, 0))
    attempt("preview past the end", lambda: a.decode_banded_preview(e5, 2, 1))
    attempt("frames on v3", lambda: a.decode_banded_frames(e3, 0, 1))
    attempt("preview on v3", lambda: a.decode_banded_preview(e3, 0, 0))
    attempt("frames bad magic", lambda: a.decode_banded_frames(bytes(magic), 0, 0))
    attempt("preview reserved byte", lambda: a.decode_banded_preview(bytes(reserved), 0, 1))
    attempt("frames cut short", lambda: a.decode_banded_frames(e5[:-1], 0, 1))
    attempt("preview of nothing", lambda: a.decode_banded_preview(b"", 0, 1))
    attempt("decode_frames on v5", lambda: a.decode_frames(e5, 0, 1))
    attempt("decode_preview on v5", lambda: a.decode_preview(e5, 0, 1))
    attempt("device frames null", lambda: a.banded_frames_decode_device(0, 100, 0, 1, 0))
    attempt("device preview null", lambda: a.banded_preview_decode_device(0, 100, 0, 1, 0))
    return lines


def test_cpp_banded_partial_host_checks_match_python(codec):
    got = _build_and_run()
    want = _python_lines(codec)
    assert got == want
    assert all(w.split(" error ")[1].startswith("2: ") for w in want[:4]), want[:4]       # a chunk without pixels refuses every range
    assert want[4] == "frames on v3 error 4: unsupported version: 3 (expected 5)"
    assert want[5] == "preview on v3 error 4: unsupported version: 3 (expected 5)"
    assert "bad magic" in want[6] and "reserved byte is 1" in want[7] and "too short for the header" in want[8]
    assert "too short for the fixed fields" in want[9]
    assert all("error 4: " in w and "unsupported version: 5" in w for w in want[10:12])
    assert [w.split(" error ")[1][0] for w in want[12:]] == ["9", "9"]


@pytest.mark.gpu
def test_cpp_banded_partial_on_gpu(gpu_codec):
    out = _build_and_run("device")
    assert out[-1] == "device banded partial"
