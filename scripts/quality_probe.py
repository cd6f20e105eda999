"""Quality control on one 1920x1080x64 chunk of the benchmark's content, HIP events, in one run:

  * the squared-error kernel (alice_codec_dev_rgb_sse) on two packed 398 MB volumes, in ms and GB/s of the 796 MB it reads,
    next to the byte-at-a-time kernel behind alice_codec_psnr (launch_sq_diff_sum through its test hook) on the same buffers;
  * one trial per format (alice_codec_dev_trial_sse) next to one encode plus one decode of that format, each timed
    `--spread-runs` times: the run-to-run spread the difference is read against;
  * encode_*_to_psnr at a mid-scale target: total ms and trials.

  python scripts/quality_probe.py --out profiles/r15_quality_probe_1080p64.json
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import alice_codec_amd as a  # noqa: E402
import bench  # noqa: E402

W, H, F = 1920, 1080, 64
PX = W * H * F


def events(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def runs_of(fn, reps, n):
    v = [round(events(fn, reps), 4) for _ in range(n)]
    return {"ms": min(v), "ms_runs": v, "spread_ms": round(max(v) - min(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_quality_probe_1080p64.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spread-runs", type=int, default=5)
    ap.add_argument("--quality", type=int, default=80)
    ap.add_argument("--target-db", type=float, default=22.0, help="a floor near the middle of this content's scale")
    args = ap.parse_args()
    lib = a.load_library()
    a.set_device(0)
    dev = torch.device("cuda:0")
    wt = a.WaveletType.Cdf97
    rgb = bench.synth_chunk(dev, 0).reshape(-1).contiguous()
    back = torch.empty_like(rgb)
    cap = a.SPLIT_HEADER_BYTES + 3 * a.wide_stream_bound(PX, a.SPLIT_DEFAULT_LANE_SYMBOLS)
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    fs = torch.zeros(F, dtype=torch.int64, device=dev)
    n_bytes = int(rgb.numel())
    res = {"what": "quality control on one 1920x1080x64 chunk (bench.synth_chunk content, CDF 9/7), MI355X, HIP events",
           "reps": args.reps, "spread_runs": args.spread_runs, "raw_bytes": n_bytes, "quality": args.quality}

    # ---- the comparison pass alone: source against the version 3 decode at the probe's quality ----
    size = int(a.wide_encode_device(rgb.data_ptr(), W, H, F, 1, wt, args.quality, out.data_ptr(), cap)[0])
    a.wide_decode_device(out.data_ptr(), cap, [size], back.data_ptr())
    old_sum = C.c_uint64(0)

    def new_kernel():
        a.rgb_sse_device(rgb.data_ptr(), back.data_ptr(), W, H, F, d_frame_sse_ptr=fs.data_ptr())

    def old_kernel():
        a._check(lib.alice_codec_test_sq_diff_sum(rgb.data_ptr(), back.data_ptr(), n_bytes, C.byref(old_sum), None))

    new = runs_of(new_kernel, args.reps, args.spread_runs)
    old = runs_of(old_kernel, args.reps, args.spread_runs)
    new_sum = int(fs.cpu().numpy().view(np.uint64).sum())
    new["gb_per_s_of_bytes_read"] = round(2 * n_bytes / new["ms"] / 1e6, 1)
    old["gb_per_s_of_bytes_read"] = round(2 * n_bytes / old["ms"] / 1e6, 1)
    res["comparison_pass"] = {"rgb_sse_kernel": new, "sq_diff_sum_kernel": old, "sums_equal": new_sum == int(old_sum.value),
                              "sse": new_sum, "psnr_db": round(a.psnr_from_sse(new_sum, n_bytes), 3),
                              "new_over_old_speed": round(old["ms"] / new["ms"], 2),
                              "note": "both calls zero their result, launch, and return after the stream has drained; the old one "
                                      "also copies 8 bytes back"}
    print(json.dumps(res["comparison_pass"]))

    # ---- a trial next to an encode plus a decode, per format ----
    calls = {"split": (2, a.split_encode_device, a.split_decode_device), "wide": (3, a.wide_encode_device, a.wide_decode_device),
             "reversible": (4, a.reversible_encode_device, a.reversible_decode_device)}
    res["trial_vs_encode_plus_decode"] = {}
    for name, (version, enc, dec) in calls.items():
        q = 100 if name == "reversible" else args.quality
        got = {}

        def trial():
            got["sse"] = int(a.trial_sse_device(version, rgb.data_ptr(), W, H, F, 1, wt, q, d_frame_sse_ptr=fs.data_ptr())[0])

        def pair():
            n = int(enc(rgb.data_ptr(), W, H, F, 1, wt, q, out.data_ptr(), cap)[0])
            dec(out.data_ptr(), cap, [n], back.data_ptr())

        t = runs_of(trial, args.reps, args.spread_runs)
        p = runs_of(pair, args.reps, args.spread_runs)
        a.rgb_sse_device(rgb.data_ptr(), back.data_ptr(), W, H, F, d_frame_sse_ptr=fs.data_ptr())
        row = {"quality": q, "trial": t, "encode_plus_decode": p, "trial_minus_pair_ms": round(t["ms"] - p["ms"], 4),
               "trial_sse": got["sse"], "sse_of_the_decoded_pixels": int(fs.cpu().numpy().view(np.uint64).sum()),
               "psnr_db": round(a.psnr_from_sse(got["sse"], n_bytes), 3)}
        row["contract_holds"] = row["trial_sse"] == row["sse_of_the_decoded_pixels"]
        res["trial_vs_encode_plus_decode"][name] = row
        print(name, json.dumps(row))

    # ---- the search ----
    res["encode_to_psnr"] = {}
    trials = np.zeros(1, np.uint32)
    for name, call in (("split", a.split_encode_to_psnr_device), ("wide", a.wide_encode_to_psnr_device)):
        got = {}

        def search():
            got["r"] = call(rgb.data_ptr(), W, H, F, 1, wt, args.target_db, out.data_ptr(), cap, min_quality=10, max_quality=96)

        s = runs_of(search, 1, args.spread_runs)
        lib.alice_codec_test_last_quality_trials(trials.ctypes.data_as(C.POINTER(C.c_uint32)), 1)
        chosen, reached, db, sizes = got["r"]
        res["encode_to_psnr"][name] = {"target_db": args.target_db, "total": s, "trials": int(trials[0]), "chosen": int(chosen[0]),
                                       "reached": bool(reached[0]), "psnr_db": round(float(db[0]), 3), "bytes": int(sizes[0])}
        print(name, json.dumps(res["encode_to_psnr"][name]))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
