"""Transcode of one device-resident 1920x1080x64 chunk of the benchmark's content, next to the route
it replaces: decode to RGB, encode again.  CDF 9/7 and CDF 5/3; version 3 from quality 95 to 60 and version 4 from 100 to 80.

Per case, in the same run, every repetition timed on its own (HIP events around calls that return after their work has
drained), median and range reported:
  * alice_codec_dev_transcode against alice_codec_dev_decode_wide + alice_codec_dev_encode_wide (version 4: the reversible
    twins) of the same chunk -- the two calls of the pair are untouched code;
  * the two new kernels alone through their stage call and test hook, and the bytes they move per second as a share of a
    device-to-device copy of the same bytes measured here;
  * a budget transcode (the budget is the size of the fixed-quality transcode) with its trial count;
  * bytes, and PSNR against the original, of the transcode next to the direct encode at the target quality.

  python scripts/transcode_probe.py --out profiles/r27_transcode_probe_1080p64.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import alice_codec_amd as a  # noqa: E402
import bench  # noqa: E402

W, H, F = 1920, 1080, 64
PX = W * H * F


def timed(fn, reps):
    """-> {median, min, max} in ms over reps calls after one warm-up"""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1))
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_transcode_probe_1080p64.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="one repetition per call and no file (for a kernel trace)")
    args = ap.parse_args()
    reps = 1 if args.quick else args.reps
    a.set_device(0)
    lib = a.load_library()
    dev = torch.device("cuda:0")
    L = a.SPLIT_DEFAULT_LANE_SYMBOLS
    rgb = bench.synth_chunk(dev, 0).reshape(-1).contiguous()
    back = torch.empty_like(rgb)
    cap = a.SPLIT_HEADER_BYTES + 3 * a.wide_stream_bound(PX, L)
    src = torch.empty(cap, dtype=torch.uint8, device=dev)
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    sym = torch.empty(3 * PX, dtype=torch.int16, device=dev)
    sym2 = torch.empty_like(sym)
    hist = torch.zeros(256, dtype=torch.int32, device=dev)
    bins = torch.zeros(4096, dtype=torch.int32, device=dev)
    oor = torch.zeros(1, dtype=torch.int32, device=dev)
    res = {"what": "transcode of one device-resident 1920x1080x64 chunk (bench.synth_chunk content) next to decode + encode, MI355X",
           "reps": reps, "lane_symbols": L, "cases": []}

    def psnr():
        d = back.to(torch.float32) - rgb.to(torch.float32)
        mse = float((d * d).mean())
        return None if mse == 0 else round(10 * float(torch.log10(torch.tensor(255.0 ** 2 / mse))), 3)

    copy = timed(lambda: sym2.copy_(sym), reps)
    copy_gbs = 2 * sym.numel() * 2 / copy["median_ms"] / 1e6
    res["copy_of_the_symbols"] = dict(copy, bytes_moved=2 * sym.numel() * 2, gb_per_s=round(copy_gbs, 1))

    for wt in (a.WaveletType.Cdf97, a.WaveletType.Cdf53):
        for version, qs, qt in ((3, 95, 60), (4, 100, 80)):
            enc = a.wide_encode_device if version == 3 else a.reversible_encode_device
            dec = a.wide_decode_device if version == 3 else a.reversible_decode_device
            n_src = int(enc(rgb.data_ptr(), W, H, F, 1, wt, qs, src.data_ptr(), cap)[0])
            size = [0]

            def transcode():
                size[0] = int(a.transcode_device(src.data_ptr(), cap, [n_src], qt, out.data_ptr(), cap)[0])

            def pair():
                dec(src.data_ptr(), cap, [n_src], back.data_ptr())
                size[0] = int(enc(back.data_ptr(), W, H, F, 1, wt, qt, out.data_ptr(), cap)[0])

            case = {"wavelet": wt.name, "version": version, "from_quality": qs, "to_quality": qt, "source_bytes": n_src}
            case["transcode"] = timed(transcode, reps)
            case["transcode"]["bytes"] = size[0]
            dec(out.data_ptr(), cap, [size[0]], back.data_ptr())
            case["transcode"]["psnr_db"] = psnr()
            case["decode_then_encode"] = timed(pair, reps)
            case["decode_then_encode"]["bytes"] = size[0]
            dec(out.data_ptr(), cap, [size[0]], back.data_ptr())
            case["decode_then_encode"]["psnr_db"] = psnr()
            n_direct = int(enc(rgb.data_ptr(), W, H, F, 1, wt, qt, out.data_ptr(), cap)[0])
            dec(out.data_ptr(), cap, [n_direct], back.data_ptr())
            case["direct_encode"] = {"bytes": n_direct, "psnr_db": psnr()}
            t, p = case["transcode"], case["decode_then_encode"]
            case["pair_over_transcode"] = round(p["median_ms"] / t["median_ms"], 3)
            case["faster_by_more_than_the_spread"] = bool(t["max_ms"] < p["min_ms"])

            # the two kernels alone, on the chunk's own symbols (all three channels in one launch)
            s1, s2 = 64 - (qs * 63) // 100, 64 - (qt * 63) // 100
            a.forward_symbols_wide_device(rgb.data_ptr(), W, H, F, wt, qs, sym.data_ptr())
            k = timed(lambda: a.requant_symbols_device(sym.data_ptr(), sym2.data_ptr(), 3 * PX, True, s1, s2, hist.data_ptr()), reps)
            k["gb_per_s"] = round(2 * 3 * PX * 2 / k["median_ms"] / 1e6, 1)
            k["share_of_copy_rate"] = round(k["gb_per_s"] / copy_gbs, 3)
            case["requant_symbols_kernel"] = k
            b = timed(lambda: lib.alice_codec_test_symbol_bins(sym.data_ptr(), 3 * PX, 1, s1, bins.data_ptr(), oor.data_ptr(), None), reps)
            b["gb_per_s"] = round(3 * PX * 2 / b["median_ms"] / 1e6, 1)
            b["share_of_copy_rate"] = round(b["gb_per_s"] / copy_gbs, 3)
            case["symbol_bins_kernel"] = b

            # a byte budget: the size of the fixed-quality transcode (version 4 through out_version = 3)
            budget = case["transcode"]["bytes"]
            ov = 3 if version == 4 else 0
            got = [None]

            def to_budget():
                got[0] = a.transcode_to_budget_device(src.data_ptr(), cap, [n_src], [budget], out.data_ptr(), cap, 10, 95, 0, ov)

            bt = timed(to_budget, reps)
            trials = np.zeros(1, np.uint32)
            lib.alice_codec_test_last_split_trials(trials.ctypes.data_as(C.POINTER(C.c_uint32)), 1)
            chosen, fits, sizes = got[0]
            case["budget_transcode"] = dict(bt, budget=budget, chosen_quality=int(chosen[0]), fits=bool(fits[0]), bytes=int(sizes[0]),
                                            trials=int(trials[0]))
            res["cases"].append(case)
    print(json.dumps(res))
    if not args.quick:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
