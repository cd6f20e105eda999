"""Builds tests/cpp/test_cpp_banded.cpp (the C++ mirror of the version 5 calls in include/alice_codec.hpp) with g++ against
libalice_codec.so and compares its output, line by line, with the same questions put to the Python mirror."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run(*args):
    exe = os.path.join(tempfile.mkdtemp(prefix="alice_cpp_banded_"), "test_cpp_banded")
    libdir = os.path.join(ROOT, "alice-codec_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_cpp_banded.cpp"), "-L", libdir, "-lalice_codec",
                           "-Wl,-rpath," + libdir, "-o", exe])
    env = dict(os.environ, LD_LIBRARY_PATH=libdir + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    out = subprocess.run([exe, *args], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.splitlines()


def _python_lines(a):
    none, rgb = np.zeros(0, np.uint8), np.full(4 * 4 * 2 * 3, 7, np.uint8)
    enc = a.FrameEncoder.with_wavelet(50, a.WaveletType.Cdf97)
    e5, e3 = a.encode_banded(enc, none, 5, 0, 2, 128, 3), a.encode_wide(enc, none, 5, 0, 2, 128)
    i = a.banded_info(e5)
    lines = [f"empty n={len(e5)} version={a.alc_version(e5)} base={i.base} L={i.lane_symbols} step={i.quant_step[0]} header={a.BANDED_HEADER_BYTES}",
             f"empty decode {a.decode_banded(e5).size} {a.decode_alc(e5).size}",
             f"empty repack {int(a.to_banded(e3) == e5)} {int(a.from_banded(e5) == e3)} {int(a.from_banded(a.to_banded(e3, 64), 128) == e3)}",
             f"bounds {a.banded_stream_bound(4096, 64, 2)} {a.banded_stream_bound(4097, 64, 3)} {a.banded_stream_bound(1, 16384, 4)}"]

    def attempt(name, fn):
        try:
            fn()
            lines.append(f"{name} ok")
        except a.CodecError as e:
            lines.append(f"{name} error {e.code}: {str(e).split(': ', 1)[1]}")

    attempt("v5 parser on v3", lambda: a.banded_info(e3))
    attempt("v3 parser on v5", lambda: a.wide_info(e5))
    attempt("v2 parser on v5", lambda: a.split_info(e5))
    attempt("decode_banded on v3", lambda: a.decode_banded(e3))
    attempt("decode_wide on v5", lambda: a.decode_wide(e5))
    attempt("to_banded on v5", lambda: a.to_banded(e5))
    attempt("transcode on v5", lambda: a.transcode(e5, 40))
    attempt("buffer", lambda: a.encode_banded(enc, np.zeros(3, np.uint8), 0, 4, 4, 100, 9))
    attempt("base", lambda: a.encode_banded(enc, rgb, 4, 4, 2, 100, 9))
    attempt("lane", lambda: a.encode_banded(enc, rgb, 4, 4, 2, 100, 2))
    attempt("lane 16384 base 3", lambda: a.encode_banded(enc, rgb, 4, 4, 2, 16384, 3))
    attempt("lane 16384 base 2", lambda: a.encode_banded(enc, none, 0, 4, 2, 16384, 2))
    return lines


def test_cpp_banded_host_checks_match_python(codec):
    got = _build_and_run()
    want = _python_lines(codec)
    assert got == want
    assert want[0] == "empty n=12636 version=5 base=3 L=128 step=33 header=12636" and want[1] == "empty decode 0 0"
    assert want[2] == "empty repack 1 1 1" and want[3] == f"bounds {388 + 2 * 4096} {2 * 388 + 4 * 4097} 0"
    assert want[4] == "v5 parser on v3 error 4: unsupported version: 3 (expected 5)"
    assert want[5] == "v3 parser on v5 error 4: unsupported version: 5 (expected 3)"
    assert want[6] == "v2 parser on v5 error 4: unsupported version: 5 (expected 2)"
    assert all("unsupported version: 5" in w for w in want[9:11])
    assert [w.split(" error ")[1][0] if " error " in w else "ok" for w in want[11:]] == ["1", "2", "2", "2", "ok"]


@pytest.mark.gpu
def test_cpp_banded_round_trip_and_repack_on_gpu(gpu_codec):
    out = _build_and_run("device")
    assert out[-1] == "device banded"
