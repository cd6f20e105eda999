"""The reversible format (.alc v4) next to the wide format (.alc v3) on one 1920x1080x64 chunk of the benchmark's content at
q = 100, for each wavelet.

Per wavelet, in the same run: device-resident encode / decode of both formats (HIP events around the calls, which return
after their work has drained), bytes, bytes per raw byte (the compression ratio of the lossless mode), whether version 4
gives the source back exactly, and the PSNR of version 3.  The version 3 decode is timed `--spread-runs` times: the
run-to-run spread the version 4 decode is compared with (the two run the same instruction count per sample).

  python scripts/reversible_probe.py --out profiles/r14_reversible_probe_1080p64.json
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import alice_codec_amd as a  # noqa: E402
import bench  # noqa: E402

W, H, F = 1920, 1080, 64
PX = W * H * F
Q = 100


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_reversible_probe_1080p64.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spread-runs", type=int, default=5)
    ap.add_argument("--lane-symbols", type=int, default=0)
    ap.add_argument("--quick", action="store_true", help="one repetition per call and no file (for a kernel trace)")
    args = ap.parse_args()
    reps = 1 if args.quick else args.reps
    a.set_device(0)
    dev = torch.device("cuda:0")
    L = args.lane_symbols
    rgb = bench.synth_chunk(dev, 0).reshape(-1).contiguous()
    back = torch.empty_like(rgb)
    cap = a.SPLIT_HEADER_BYTES + 3 * a.wide_stream_bound(PX, L or a.SPLIT_DEFAULT_LANE_SYMBOLS)
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    res = {"what": "reversible .alc v4 against wide .alc v3 at q = 100, one 1920x1080x64 chunk (bench.synth_chunk content), MI355X",
           "reps": reps, "spread_runs": args.spread_runs, "lane_symbols": L or a.SPLIT_DEFAULT_LANE_SYMBOLS, "raw_bytes": int(rgb.numel())}

    def psnr():
        d = back.to(torch.float32) - rgb.to(torch.float32)
        mse = float((d * d).mean())
        return float("inf") if mse == 0 else 10 * torch.log10(torch.tensor(255.0 ** 2 / mse)).item()

    for wt in (a.WaveletType.Cdf53, a.WaveletType.Cdf97, a.WaveletType.Haar):
        row = {}
        for name, enc, dec in (("v3", a.wide_encode_device, a.wide_decode_device), ("v4", a.reversible_encode_device, a.reversible_decode_device)):
            size = {}

            def encode():
                size["n"] = int(enc(rgb.data_ptr(), W, H, F, 1, wt, Q, out.data_ptr(), cap, lane_symbols=L)[0])

            def decode():
                dec(out.data_ptr(), cap, [size["n"]], back.data_ptr())

            e_ms = events(encode, reps)
            runs = [events(decode, reps) for _ in range(1 if args.quick else args.spread_runs)]
            r = {"encode_ms": round(e_ms, 4), "decode_ms": round(min(runs), 4), "decode_ms_runs": [round(v, 4) for v in runs],
                 "bytes": size["n"], "bytes_per_raw_byte": round(size["n"] / rgb.numel(), 5)}
            if name == "v4":
                r["exact"] = bool(torch.equal(back, rgb))
            else:
                r["psnr_db"] = round(psnr(), 2)
            row[name] = r
        v3, v4 = row["v3"], row["v4"]
        row["v3_decode_spread_ms"] = round(max(v3["decode_ms_runs"]) - min(v3["decode_ms_runs"]), 4)
        row["v4_minus_v3_decode_ms"] = round(v4["decode_ms"] - v3["decode_ms"], 4)
        row["same_bytes"] = v4["bytes"] == v3["bytes"]
        res[wt.name] = row
        print(wt.name, json.dumps(row))
    if not args.quick:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", args.out)


if __name__ == "__main__":
    main()
