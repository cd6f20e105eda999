"""Kernel-only times of the squared-error kernel and of the byte kernel behind alice_codec_psnr, from a kernel trace: the
figures of scripts/quality_probe.py are call times (zeroing, launch and synchronisation included).

  rocprofv3 --kernel-trace --output-format csv -d TRACE_DIR -- python scripts/quality_kernel_trace.py run
  python scripts/quality_kernel_trace.py parse TRACE_DIR --out profiles/r15_quality_kernel_trace.json
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H, F = 1920, 1080, 64
LAUNCHES = 6


def run():
    import torch
    import alice_codec_amd as a
    import bench
    lib = a.load_library()
    a.set_device(0)
    dev = torch.device("cuda:0")
    rgb = bench.synth_chunk(dev, 0).reshape(-1).contiguous()
    other = (rgb ^ 3).contiguous()
    fs = torch.zeros(F, dtype=torch.int64, device=dev)
    s = C.c_uint64(0)
    for _ in range(LAUNCHES):
        a.rgb_sse_device(rgb.data_ptr(), other.data_ptr(), W, H, F, d_frame_sse_ptr=fs.data_ptr())
        a._check(lib.alice_codec_test_sq_diff_sum(rgb.data_ptr(), other.data_ptr(), rgb.numel(), C.byref(s), None))
    assert int(fs.sum()) == s.value > 0
    print("sums equal:", s.value)


def parse(trace_dir, out):
    bytes_read = 2 * W * H * F * 3
    rows = {}
    for f in sorted(glob.glob(os.path.join(trace_dir, "**", "*_kernel_trace.csv"), recursive=True)):
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"]
            key = "rgb_sse_kernel" if "rgb_sse_kernel" in name else ("sq_diff_sum_kernel" if "sq_diff_sum_kernel" in name else None)
            if key:
                rows.setdefault(key, []).append(round((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, 1))
    res = {"what": "kernel-only microseconds from a rocprofv3 kernel trace, two packed 1920x1080x64 RGB volumes (796 MB read), MI355X",
           "bytes_read": bytes_read}
    for key, us in rows.items():
        med = statistics.median(us)
        res[key] = {"us": us, "median_us": med, "gb_per_s_at_the_median": round(bytes_read / med / 1e3, 1)}
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("run", "parse"))
    ap.add_argument("trace_dir", nargs="?")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_quality_kernel_trace.json"))
    args = ap.parse_args()
    run() if args.mode == "run" else parse(args.trace_dir, args.out)
