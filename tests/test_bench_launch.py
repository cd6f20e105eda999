"""bench.py's launch logic, checked without a GPU: `--gpus N` must either BE an N-rank run (ranks started by bench.py
itself, or by a launcher whose WORLD_SIZE agrees) or exit non-zero -- never print an n_gpus=1 line under an N label."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**kw):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    e.update(kw)
    return e


def test_import_has_no_side_effects():
    """Scripts import bench for W/H/F and synth_chunk: that must not redirect stdout or import torch."""
    out = subprocess.run([sys.executable, "-c",
                          "import sys; sys.path.insert(0, %r); import bench; print('torch' in sys.modules, bench.W, bench.H, bench.F)" % ROOT],
                         capture_output=True, text=True, env=_env(), timeout=60)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["False", "1920", "1080", "64"]


def test_plan_ranks_is_one_process_per_gpu():
    sys.path.insert(0, ROOT)
    import bench
    plan = bench.plan_ranks(4, ["--gpus", "4", "--steps", "2", "--warmup", "1"], {"PATH": "x", "WORLD_SIZE": "stale"}, 12345, python="py")
    assert len(plan) == 4
    ports = set()
    for r, (cmd, env) in enumerate(plan):
        assert cmd == ["py", BENCH, "--gpus", "4", "--steps", "2", "--warmup", "1"]
        assert env["RANK"] == str(r) and env["LOCAL_RANK"] == str(r) and env["WORLD_SIZE"] == "4"
        assert env["MASTER_ADDR"] == "127.0.0.1" and env["HSA_ENABLE_IPC_MODE_LEGACY"] == "0" and env["PATH"] == "x"
        ports.add(env["MASTER_PORT"])
    assert ports == {"12345"}


def test_check_launch_cases():
    sys.path.insert(0, ROOT)
    import bench
    assert bench.check_launch(1, {}, None) == "rank"
    assert bench.check_launch(8, {"WORLD_SIZE": "8"}, None) == "rank"          # under torchrun
    assert bench.check_launch(8, {}, 8) == "spawn"                              # bare `python bench.py --gpus 8`
    assert bench.check_launch(2, {}, 1).startswith("error")                     # a 1-GPU box
    assert bench.check_launch(2, {"WORLD_SIZE": "4"}, None).startswith("error")
    assert bench.check_launch(1, {"WORLD_SIZE": "2"}, None).startswith("error")
    assert bench.check_launch(0, {}, None).startswith("error")


def test_gpus2_without_two_gpus_exits_nonzero():
    """This container has no GPU: `python bench.py --gpus 2` must fail loudly and print no result line."""
    out = subprocess.run([sys.executable, BENCH, "--gpus", "2"], capture_output=True, text=True, env=_env(), timeout=120)
    assert out.returncode != 0
    assert out.stdout.strip() == ""
    assert "--gpus 2" in out.stderr and "visible" in out.stderr


def test_world_size_mismatch_exits_nonzero():
    out = subprocess.run([sys.executable, BENCH, "--gpus", "2"], capture_output=True, text=True,
                         env=_env(WORLD_SIZE="4", RANK="0", LOCAL_RANK="0"), timeout=120)
    assert out.returncode != 0 and out.stdout.strip() == ""
    assert "WORLD_SIZE=4" in out.stderr


def test_spawn_dry_run_shows_two_children():
    out = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "3", "--warmup", "1"], capture_output=True, text=True,
                         env=_env(ALICE_BENCH_SPAWN_DRYRUN="1"), timeout=120)
    assert out.returncode == 0, out.stderr
    plan = json.loads(out.stdout)
    assert [p["env"]["RANK"] for p in plan] == ["0", "1"]
    assert all(p["env"]["WORLD_SIZE"] == "2" and p["cmd"][1:] == [BENCH, "--gpus", "2", "--steps", "3", "--warmup", "1"] for p in plan)
    assert len({p["env"]["MASTER_PORT"] for p in plan}) == 1


def test_dump_plan_is_fixed_and_within_bounds():
    """--dump-outputs: the same chunk count gives the same chunks and sample positions, inside the buffers, under 64 MB."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import bench
    px3 = bench.W * bench.H * bench.F * 3
    c1, a1, r1 = bench.dump_plan(337)
    c2, a2, r2 = bench.dump_plan(337)
    assert c1 == c2 and np.array_equal(a1, a2) and np.array_equal(r1, r2)
    assert c1 == list(bench.DUMP_CHUNKS)
    assert bench.dump_plan(3)[0] == [0, 1, 2] and bench.dump_plan(1)[0] == [0]
    assert a1.min() >= 0.0 and a1.max() < 1.0
    assert r1.dtype == np.int64 and r1.min() >= 0 and r1.max() < px3
    assert 0 < bench.dump_nbytes(337) <= 64 << 20
    assert bench.dump_nbytes(1) < bench.dump_nbytes(337)


def test_plain_run_does_only_the_headline():
    """The oracle check, the CPU baseline and the host-call measurement run after the timed steps only with --full."""
    sys.path.insert(0, ROOT)
    import bench
    assert bench.parse_args([]).full is False
    assert bench.extras(bench.parse_args(["--steps", "20", "--warmup", "5"]), 0, 1) == (False, False)
    assert bench.extras(bench.parse_args(["--dump-outputs", "d"]), 0, 1) == (False, False)
    assert bench.extras(bench.parse_args(["--full"]), 0, 1) == (True, True)
    assert bench.extras(bench.parse_args(["--full", "--no-verify"]), 0, 1) == (False, True)
    assert bench.extras(bench.parse_args(["--full", "--no-host-api"]), 0, 1) == (True, False)
    assert bench.extras(bench.parse_args(["--full"]), 1, 2) == (True, False)   # every rank checks; host calls on 1 GPU only
    assert bench.extras(bench.parse_args(["--full"]), 0, 2) == (True, False)


def test_metric_is_the_same_in_plain_and_full_runs():
    """A plain run (not checked) and a --full run that checked the batch report the same metric; a failed check does not."""
    sys.path.insert(0, ROOT)
    import bench
    name = "Mpixels/s encode+decode, 1080p x 64 CDF9/7 q=80; bit-exact vs CPU"
    assert bench.metric_name("cdf97", 80, None) == bench.metric_name("cdf97", 80, True) == name
    assert bench.metric_name("cdf97", 80, False) == "Mpixels/s encode+decode, 1080p x 64 CDF9/7 q=80; NOT bit-exact vs CPU"
    assert bench.metric_name("cdf53", 80, None) == bench.metric_name("cdf53", 80, True) == \
        "Mpixels/s encode+decode, 1080p x 64 cdf53 q=80; bit-exact vs CPU"


def test_steps_and_warmup_are_checked():
    sys.path.insert(0, ROOT)
    import bench
    a = bench.parse_args(["--steps", "7", "--warmup", "0", "--dump-outputs", "d"])
    assert (a.steps, a.warmup, a.dump_outputs) == (7, 0, "d")
    assert bench.parse_args([]).dump_outputs is None
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        out = subprocess.run([sys.executable, BENCH, "--gpus", "1"] + bad, capture_output=True, text=True, env=_env(), timeout=120)
        assert out.returncode != 0 and out.stdout.strip() == ""
