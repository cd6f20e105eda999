"""Builds tests/cpp/test_cpp_rects.cpp (the C++ mirror of the batched frame-range / rectangle calls in
include/alice_codec.hpp) with g++ against libalice_codec.so and compares its output, line by line, with the same questions
put to the Python mirror."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run(*args):
    exe = os.path.join(tempfile.mkdtemp(prefix="alice_cpp_rects_"), "test_cpp_rects")
    libdir = os.path.join(ROOT, "alice-codec_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_cpp_rects.cpp"), "-L", libdir, "-lalice_codec",
                           "-Wl,-rpath," + libdir, "-o", exe])
    env = dict(os.environ, LD_LIBRARY_PATH=libdir + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    out = subprocess.run([exe, *args], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.splitlines()


def _python_lines(a):
    lines = []
    bad = [None]

    def attempt(name, fn):
        try:
            fn()
            lines.append(f"{name} ok")
        except a.CodecError as e:
            bad[0] = getattr(e, "bad_item", None)
            lines.append(f"{name} error {e.code}: {str(e).split(': ', 1)[1]}")

    none = np.zeros(0, np.uint8)
    empty = np.frombuffer(a.encode_wide(a.FrameEncoder.with_wavelet(80, a.WaveletType.Cdf97), none, 0, 4, 4, 64), np.uint8)
    v1 = empty.copy()
    v1[4] = 1
    lib = a.load_library()
    frame, one = (0, 0, 0, 0), (0, 0, 1, 1)

    def raw(rows):
        """rows of (array or None, len, first, count, rect) through the C ABI, as the C++ program passes them"""
        import ctypes as C
        arr = (a.RectItem * max(len(rows), 1))()
        for i, (buf, n, first, count, rect) in enumerate(rows):
            arr[i] = a.RectItem(None if buf is None else buf.ctypes.data, n, first, count, *rect, None, 0, 0)
        offsets = np.zeros(len(rows) + 1, np.uint64)
        if not lib.alice_codec_decode_rects(arr, len(rows), offsets.ctypes.data_as(C.POINTER(C.c_uint64)), None):
            a._raise_last()

    attempt("no items", lambda: a.decode_rects([]))
    attempt("too many items", lambda: a.decode_rects([(empty, 0, 1)] * 1025))
    attempt("null data in item 1", lambda: raw([(empty, empty.size, 0, 1, frame), (None, 100, 0, 1, one)]))
    attempt("empty chunk in item 0", lambda: a.decode_rects([(empty, 0, 1, *one)]))
    attempt("version 1 in item 2", lambda: raw([(v1, 10, 0, 1, one), (v1, 10, 0, 1, one), (v1, v1.size, 0, 1, one)]))
    attempt("short data in item 0", lambda: raw([(v1, 10, 0, 1, frame), (v1, v1.size, 0, 1, frame)]))
    attempt("device twin without items", lambda: a.rects_decode_device([]))
    attempt("device twin without an output in item 2",
            lambda: a.rects_decode_device([(empty.ctypes.data, empty.size, 0, 1, 0, 0, 0, 0, empty.ctypes.data, 0, 0)] * 2 +
                                          [(empty.ctypes.data, empty.size, 0, 1, 0, 0, 0, 0, None, 0, 0)]))
    lines.append(f"bad item {bad[0]}")
    return lines


def test_cpp_rects_host_checks_match_python(codec):
    got = _build_and_run()
    want = _python_lines(codec)
    assert got == want
    assert [w.split(" error ")[1][0] for w in want[:8]] == ["2", "2", "9", "2", "4", "4", "2", "9"]
    assert want[4].startswith("version 1 in item 2 error 4: item 0: ") and "too short" in want[4], "the first item that fails decides"
    assert want[3].startswith("empty chunk in item 0 error 2: item 0: ")
    assert want[8] == "bad item 2"


@pytest.mark.gpu
def test_cpp_rects_on_gpu(gpu_codec):
    out = _build_and_run("device")
    assert out[-1] == "device rects"
