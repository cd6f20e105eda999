"""Builds tests/cpp/test_cpp_segment.cpp (the C++ mirror of person segmentation in include/alice_codec.hpp) with g++
against libalice_codec.so and runs it: host-only checks on CPU, the walk-through on the device under -m gpu."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run():
    exe = os.path.join(tempfile.mkdtemp(prefix="alice_cpp_seg_"), "test_cpp_segment")
    libdir = os.path.join(ROOT, "alice-codec_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_cpp_segment.cpp"), "-L", libdir, "-lalice_codec",
                           "-Wl,-rpath," + libdir, "-o", exe])
    env = dict(os.environ, LD_LIBRARY_PATH=libdir + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def test_cpp_segment_host_checks(codec):
    assert "CPP SEGMENT OK" in _build_and_run()


@pytest.mark.gpu
def test_cpp_segment_on_gpu(gpu_codec):
    assert _build_and_run().strip() == "CPP SEGMENT OK"
