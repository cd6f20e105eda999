"""Builds tests/cpp/test_cpp_reversible.cpp (the C++ mirror of the version 4 calls in include/alice_codec.hpp) with g++
against libalice_codec.so and compares its output, line by line, with the same questions put to the Python mirror."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run(*args):
    exe = os.path.join(tempfile.mkdtemp(prefix="alice_cpp_reversible_"), "test_cpp_reversible")
    libdir = os.path.join(ROOT, "alice-codec_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_cpp_reversible.cpp"), "-L", libdir, "-lalice_codec",
                           "-Wl,-rpath," + libdir, "-o", exe])
    env = dict(os.environ, LD_LIBRARY_PATH=libdir + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    out = subprocess.run([exe, *args], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.splitlines()


def _python_lines(a):
    none, rgb = np.zeros(0, np.uint8), np.full(4 * 4 * 2 * 3, 7, np.uint8)
    enc = a.FrameEncoder.with_wavelet(100, a.WaveletType.Haar)
    e4, e3 = a.encode_reversible(enc, none, 5, 0, 2, 128), a.encode_wide(enc, none, 5, 0, 2, 128)
    i = a.reversible_info(e4)
    lines = [f"empty n={len(e4)} version={a.alc_version(e4)} L={i.lane_symbols} step={i.quant_step[0]} "
             f"lossless={int(a.encode_lossless(none, 5, 0, 2, a.WaveletType.Haar, 128) == e4)}",
             f"empty decode {a.decode_reversible(e4).size} {a.decode_alc(e4).size}",
             f"bytes equal but byte 4: {int(e3[:4] + bytes([4]) + e3[5:] == e4)}"]

    def attempt(name, fn):
        try:
            fn()
            lines.append(f"{name} ok")
        except a.CodecError as e:
            lines.append(f"{name} error {e.code}: {str(e).split(': ', 1)[1]}")

    attempt("v4 parser on v3", lambda: a.reversible_info(e3))
    attempt("v3 parser on v4", lambda: a.wide_info(e4))
    attempt("v2 parser on v4", lambda: a.split_info(e4))
    attempt("decode_reversible on v3", lambda: a.decode_reversible(e3))
    attempt("decode_wide on v4", lambda: a.decode_wide(e4))
    attempt("buffer", lambda: a.encode_reversible(enc, np.zeros(3, np.uint8), 0, 4, 4, 100))
    attempt("lane", lambda: a.encode_reversible(enc, rgb, 4, 4, 2, 100))
    attempt("lane 16384", lambda: a.encode_lossless(rgb, 4, 4, 2, a.WaveletType.Cdf53, 16384))
    attempt("lane 8192", lambda: a.encode_lossless(none, 0, 4, 2, a.WaveletType.Cdf53, 8192))
    return lines


def test_cpp_reversible_host_checks_match_python(codec):
    got = _build_and_run()
    want = _python_lines(codec)
    assert got == want
    assert want[0] == "empty n=1630 version=4 L=128 step=1 lossless=1" and want[1] == "empty decode 0 0" and want[2].endswith(": 1")
    assert want[3] == "v4 parser on v3 error 4: unsupported version: 3 (expected 4)"
    assert want[4] == "v3 parser on v4 error 4: unsupported version: 4 (expected 3)"
    assert want[5] == "v2 parser on v4 error 4: unsupported version: 4 (expected 2)"
    assert [w.split(" error ")[1][0] if " error " in w else "ok" for w in want[8:]] == ["1", "2", "2", "ok"]


@pytest.mark.gpu
def test_cpp_lossless_round_trip_and_decode_alc_on_gpu(gpu_codec):
    out = _build_and_run("device")
    assert out[-1] == "device lossless"
