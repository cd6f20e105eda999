"""The wide format (.alc v3) next to the split-stream format (.alc v2) on one 1920x1080x64 CDF 9/7 chunk of the benchmark's
content, at q = 80 (no symbol reaches 255: the two decode to the same pixels) and q = 100 (v2 wraps, v3 does not).

Per quality, in the same run: device-resident encode / decode of both formats (HIP events around the calls, which return
after their work has drained), bytes, PSNR of the round trip against the source, the share of symbols with z >= 255, and
v3 / v2 time ratios.  Where the time goes per kernel comes from a kernel trace of `--quick`.

  python scripts/wide_probe.py --out profiles/r09_wide_probe_1080p64.json
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_wide_probe_1080p64.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lane-symbols", type=int, default=0)
    ap.add_argument("--quick", action="store_true", help="one repetition per call and no file (for a kernel trace)")
    args = ap.parse_args()
    reps = 1 if args.quick else args.reps
    a.set_device(0)
    dev = torch.device("cuda:0")
    wt = a.WaveletType.Cdf97
    L = args.lane_symbols
    rgb = bench.synth_chunk(dev, 0).reshape(-1).contiguous()
    back = torch.empty_like(rgb)
    cap = a.SPLIT_HEADER_BYTES + 3 * a.wide_stream_bound(PX, L or a.SPLIT_DEFAULT_LANE_SYMBOLS)
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    sym = torch.empty(3 * PX, dtype=torch.int16, device=dev)
    res = {"what": "wide .alc v3 against split-stream .alc v2, one 1920x1080x64 CDF 9/7 chunk (bench.synth_chunk content), MI355X",
           "reps": reps, "lane_symbols": L or a.SPLIT_DEFAULT_LANE_SYMBOLS}

    def psnr():
        d = back.to(torch.float32) - rgb.to(torch.float32)
        mse = float((d * d).mean())
        return None if mse == 0 else round(10 * float(torch.log10(torch.tensor(255.0 ** 2 / mse))), 2)

    def one(q, enc_fn, dec_fn):
        size = [None]

        def enc():
            size[0] = enc_fn(rgb.data_ptr(), W, H, F, 1, wt, q, out.data_ptr(), cap, lane_symbols=L)

        e = events(enc, reps)
        d = events(lambda: dec_fn(out.data_ptr(), cap, size[0], back.data_ptr()), reps)
        return {"encode_ms": round(e, 3), "decode_ms": round(d, 3), "bytes": int(size[0][0]), "psnr_db": psnr()}

    for q in (80, 100):
        v2 = one(q, a.split_encode_device, a.split_decode_device)
        v3 = one(q, a.wide_encode_device, a.wide_decode_device)
        a.forward_symbols_wide_device(rgb.data_ptr(), W, H, F, wt, q, sym.data_ptr())
        z = sym.to(torch.int32) & 0xFFFF
        res[f"q{q}"] = {"v2": v2, "v3": v3, "share_z_ge_255": round(float((z >= 255).float().mean()), 6), "largest_z": int(z.max()),
                        "v3_over_v2_encode": round(v3["encode_ms"] / v2["encode_ms"], 3),
                        "v3_over_v2_decode": round(v3["decode_ms"] / v2["decode_ms"], 3),
                        "v3_over_v2_bytes": round(v3["bytes"] / v2["bytes"], 5)}
    print(json.dumps(res))
    if not args.quick:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
