"""Builds tests/cpp/test_cpp_transcode.cpp (the C++ mirror of the transcode calls in include/alice_codec.hpp) with g++ against
libalice_codec.so and compares its output, line by line, with the same questions put to the Python mirror."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run(*args):
    exe = os.path.join(tempfile.mkdtemp(prefix="alice_cpp_transcode_"), "test_cpp_transcode")
    libdir = os.path.join(ROOT, "alice-codec_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_cpp_transcode.cpp"), "-L", libdir, "-lalice_codec",
                           "-Wl,-rpath," + libdir, "-o", exe])
    env = dict(os.environ, LD_LIBRARY_PATH=libdir + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    out = subprocess.run([exe, *args], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.splitlines()


def _python_lines(a):
    lines = []

    def attempt(name, fn):
        try:
            fn()
            lines.append(f"{name} ok")
        except a.CodecError as e:
            lines.append(f"{name} error {e.code}: {str(e).split(': ', 1)[1]}")

    none = np.zeros(0, np.uint8)
    enc = a.FrameEncoder.with_wavelet(80, a.WaveletType.Cdf97)
    empty3 = a.encode_wide(enc, none, 0, 4, 4, 64)
    empty2 = a.encode_split(enc, none, 0, 4, 4, 64)
    empty4 = a.encode_reversible(enc, none, 0, 4, 4, 64)

    def empty_chunk():
        out = a.transcode(empty3, 50, 128, 4)
        i = a.reversible_info(out)
        lines.append(f"empty chunk: {len(out)} bytes, version {out[4]}, lanes {i.lane_symbols}, step {i.quant_step[0]}")

    attempt("empty chunk", empty_chunk)
    attempt("empty chunk kept", lambda: lines.append(f"kept {int(a.transcode(empty2, 90) == empty2)}"))

    def budget():
        data, q, fits = a.transcode_to_size(empty3, 1630, 10, 95)
        lines.append(f"budget: {len(data)} bytes, quality {q}, fits {int(fits)}")

    attempt("empty chunk budget", budget)

    def brackets():
        p = a.predict_transcode_sizes(empty4)
        lines.append(f"brackets: {int(p.lo[0])} {int(p.hi[100])}")

    attempt("empty chunk brackets", brackets)
    bad = bytearray(empty3); bad[4] = 1
    attempt("version 1", lambda: a.transcode(bytes(bad), 50))
    attempt("version 1 budget", lambda: a.transcode_to_size(bytes(bad), 5000))
    attempt("version 1 brackets", lambda: a.predict_transcode_sizes(bytes(bad)))
    bad[4] = 9
    attempt("version 9", lambda: a.transcode(bytes(bad), 50))
    bad[0] = ord("B")
    attempt("magic", lambda: a.transcode(bytes(bad), 50))
    attempt("no data", lambda: a.transcode(none, 50))
    bad = bytearray(empty3); bad[5] = 3
    attempt("wavelet byte", lambda: a.transcode(bytes(bad), 50))
    attempt("truncated header", lambda: a.transcode(empty3[:1629], 50))
    attempt("lanes 100", lambda: a.transcode(empty3, 50, 100))
    attempt("lanes 16384 wide", lambda: a.transcode(empty3, 50, 16384))
    attempt("lanes 16384 split", lambda: a.transcode(empty2, 50, 16384))
    attempt("version 2 to 3", lambda: a.transcode(empty2, 50, 0, 3))
    attempt("version 2 to 2", lambda: a.transcode(empty2, 50, 0, 2))
    attempt("version 3 to 2", lambda: a.transcode(empty3, 50, 0, 2))
    attempt("version 4 to 5", lambda: a.transcode(empty4, 50, 0, 5))
    attempt("quality range", lambda: a.transcode_to_size(empty3, 5000, 50, 40))
    attempt("version 4 budget", lambda: a.transcode_to_size(empty4, 5000))
    attempt("version 3 to 4 budget", lambda: a.transcode_to_size(empty3, 5000, 10, 95, 0, 4))
    attempt("version 4 to 3 budget", lambda: a.transcode_to_size(empty4, 5000, 10, 95, 0, 3))
    attempt("device twin without pointers", lambda: a.transcode_device(0, 0, [1630], 50, 0, 0))
    attempt("budget twin without pointers", lambda: a.transcode_to_budget_device(0, 0, [1630], [5000], 0, 0))
    attempt("stage call without pointers", lambda: a.requant_symbols_device(0, 0, 4, False, 1, 2))
    attempt("stage call steps", lambda: a.requant_symbols_device(4096, 4096, 4, False, 1, 65))
    return lines


def test_cpp_transcode_host_checks_match_python(codec):
    got = _build_and_run()
    want = _python_lines(codec)
    assert got == want
    assert want[0] == "empty chunk: 1630 bytes, version 4, lanes 128, step 33" and want[1] == "empty chunk ok"
    assert want[2:8] == ["kept 1", "empty chunk kept ok", "budget: 1630 bytes, quality 95, fits 1", "empty chunk budget ok",
                         "brackets: 1630 1630", "empty chunk brackets ok"]
    codes = [w.split(" error ")[1][0] if " error " in w else "-" for w in want[8:]]
    assert codes == ["4", "4", "4", "4", "4", "4", "4", "4", "2", "2", "-", "2", "2", "2", "2", "2", "4", "4", "-", "9", "9", "9", "5"]
    assert "version 1 has no random access (one serial chain per channel)" in want[8]


@pytest.mark.gpu
def test_cpp_transcode_on_gpu(gpu_codec):
    out = _build_and_run("device")
    assert out[-1] == "device transcodes"
