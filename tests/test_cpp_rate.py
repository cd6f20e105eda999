"""Builds tests/cpp/test_cpp_rate.cpp (the C++ mirror of the reference's rate control in include/alice_codec.hpp) with g++
against libalice_codec.so and compares its output, line by line, with the same script run through the Python mirror."""
import math
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run(*args):
    exe = os.path.join(tempfile.mkdtemp(prefix="alice_cpp_rate_"), "test_cpp_rate")
    libdir = os.path.join(ROOT, "alice-codec_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_cpp_rate.cpp"), "-L", libdir, "-lalice_codec",
                           "-Wl,-rpath," + libdir, "-o", exe])
    env = dict(os.environ, LD_LIBRARY_PATH=libdir + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    out = subprocess.run([exe, *args], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.splitlines()


def _g17(x: float) -> str:
    return "%.17g" % x


def _python_lines(codec):
    RC, Cfg = codec.RateController, codec.RateControlConfig
    sizes = [((i * 7919) % 23) * 40000 + (900000 if i % 5 == 0 else 0) for i in range(80)]
    lines = []

    def run(name, cfg, seq):
        c = RC(cfg)
        lines.append(f"{name} start q={c.recommended_quality()} target={c.target_bits_per_frame()} ratio={_g17(c.buffer_ratio())}")
        for s in seq:
            c.update(s)
            lines.append(f"{name} q={c.current_quality()} ratio={_g17(c.buffer_ratio())} avg={c.average_frame_size()} "
                         f"n={c.frame_count()} att={_g17(c.actual_to_target_ratio())}")

    run("default", Cfg(), sizes)
    run("small", Cfg(buffer_size_bits=1_000_000, min_quality=20, max_quality=80), sizes)
    run("fast", Cfg(target_bitrate_kbps=20000, framerate=59.94), sizes)
    run("zero_fps", Cfg(framerate=0.0), [1, 2, 3])
    for fps in (0.0, -1.0, 24.0, 30.0, 60.0, 1e-9, math.nan, math.inf):
        for k in (0, 1, 100, 1000, 5000, 20000, 100000):
            lines.append(f"est {k} {_g17(fps)} {codec.estimate_quality(k, 1920, 1080, fps)}")
    return lines


def _norm(line):   # printf spells NaN / infinity as nan / inf, Python's %g the same
    return line


def test_cpp_rate_controller_matches_python(codec):
    got = _build_and_run()
    want = _python_lines(codec)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert _norm(g) == _norm(w)


@pytest.mark.gpu
def test_cpp_encode_to_size_on_gpu(gpu_codec):
    out = _build_and_run("device")
    assert out[-1].startswith("device q=")
