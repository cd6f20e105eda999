"""The banded format (.alc v5) next to its base versions (.alc v2, v3) on one 1920x1080x64 chunk of the benchmark's content,
device-resident: CDF 5/3 and CDF 9/7, q in {50, 80, 95}, bases 2 and 3.

Per case, in the same run: encode and decode of the base and of the banded container, alternated round by round (HIP events
around the calls, which return after their work has drained; the figure is the minimum over the rounds and the spread is
max - min of the base's rounds), container sizes, the repack to_banded against the base's decode followed by a banded
encode, and band_hist_kernel's call against a device-to-device copy of the same symbols (the copy rate).

  python scripts/banded_probe.py --out profiles/r28_banded_probe_1080p64.json
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
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def alternate(fns, reps, rounds):
    """-> per function the list of its per-call milliseconds, one per round; the functions take turns inside a round"""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    runs = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            runs[k].append(events(fn, reps))
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_banded_probe_1080p64.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--lane-symbols", type=int, default=0)
    ap.add_argument("--quick", action="store_true", help="one case, one repetition per call and no file")
    args = ap.parse_args()
    reps, rounds = (1, 1) if args.quick else (args.reps, args.rounds)
    a.set_device(0)
    lib = a.load_library()
    dev = torch.device("cuda:0")
    L = args.lane_symbols
    Le = L or a.SPLIT_DEFAULT_LANE_SYMBOLS
    rgb = bench.synth_chunk(dev, 0).reshape(-1).contiguous()
    back = torch.empty_like(rgb)
    cap = a.BANDED_HEADER_BYTES + 3 * a.wide_stream_bound(PX, Le)
    plain = torch.empty(cap, dtype=torch.uint8, device=dev)
    banded = torch.empty(cap, dtype=torch.uint8, device=dev)
    repacked = torch.empty(cap, dtype=torch.uint8, device=dev)
    res = {"what": "banded .alc v5 against its base version, one 1920x1080x64 chunk (bench.synth_chunk content), MI355X, device-resident calls",
           "reps": reps, "rounds": rounds, "lane_symbols": Le, "raw_bytes": int(rgb.numel()), "cases": []}
    ms = lambda runs: round(min(runs), 4)                        # noqa: E731
    spread = lambda runs: round(max(runs) - min(runs), 4)        # noqa: E731
    base_calls = {2: (a.split_encode_device, a.split_decode_device), 3: (a.wide_encode_device, a.wide_decode_device)}
    cases = [(wt, q, base) for wt in (a.WaveletType.Cdf53, a.WaveletType.Cdf97) for q in (50, 80, 95) for base in (2, 3)]
    for wt, q, base in cases[:1] if args.quick else cases:
        enc, dec = base_calls[base]
        n = {}

        def encode_plain():
            n["plain"] = int(enc(rgb.data_ptr(), W, H, F, 1, wt, q, plain.data_ptr(), cap, lane_symbols=L)[0])

        def encode_banded():
            n["banded"] = int(a.banded_encode_device(rgb.data_ptr(), W, H, F, 1, wt, q, banded.data_ptr(), cap, lane_symbols=L, base=base)[0])

        def decode_plain():
            dec(plain.data_ptr(), cap, [n["plain"]], back.data_ptr())

        def decode_banded():
            a.banded_decode_device(banded.data_ptr(), cap, [n["banded"]], back.data_ptr())

        def repack():
            n["repacked"] = int(a.to_banded_device(plain.data_ptr(), cap, [n["plain"]], repacked.data_ptr(), cap)[0])

        def decode_then_encode():
            decode_plain()
            encode_banded()

        e_plain, e_banded = alternate((encode_plain, encode_banded), reps, rounds)
        d_plain, d_banded = alternate((decode_plain, decode_banded), reps, rounds)
        decode_banded()
        ref = torch.empty_like(back)
        dec(plain.data_ptr(), cap, [n["plain"]], ref.data_ptr())
        pixels_equal = bool(torch.equal(back, ref))
        r_pack, r_long = alternate((repack, decode_then_encode), reps, rounds)
        same = n["repacked"] == n["banded"] and bool(torch.equal(repacked[:n["banded"]], banded[:n["banded"]]))
        row = {"wavelet": wt.name, "quality": q, "base": base,
               "bytes": {"base": n["plain"], "banded": n["banded"], "ratio": round(n["banded"] / n["plain"], 4)},
               "encode_ms": {"base": ms(e_plain), "banded": ms(e_banded), "base_spread": spread(e_plain), "runs_base": e_plain, "runs_banded": e_banded},
               "decode_ms": {"base": ms(d_plain), "banded": ms(d_banded), "base_spread": spread(d_plain), "runs_base": d_plain, "runs_banded": d_banded},
               "repack_ms": {"to_banded": ms(r_pack), "decode_then_encode": ms(r_long), "runs_to_banded": r_pack, "runs_decode_then_encode": r_long},
               "pixels_equal_base": pixels_equal, "repack_equals_encode": same}
        res["cases"].append(row)
        print(json.dumps({k: v for k, v in row.items()}, default=lambda v: round(v, 4)))

    # band_hist_kernel's call against a device-to-device copy of the same bytes
    hist = torch.zeros(3 * 8 * 256, dtype=torch.int32, device=dev)
    padded = PX                                                   # 1920 x 1080 x 64 needs no padding
    for wide in (False, True):
        sym = torch.empty(3 * padded * (2 if wide else 1), dtype=torch.uint8, device=dev)
        if wide:
            a.forward_symbols_wide_device(rgb.data_ptr(), W, H, F, a.WaveletType.Cdf97, 80, sym.data_ptr())
        else:
            rc = lib.alice_codec_dev_forward_symbols(rgb.data_ptr(), W, H, F, int(a.WaveletType.Cdf97), 80, sym.data_ptr(), None, None)
            assert rc == 0
        dst = torch.empty_like(sym)
        h_runs, c_runs = alternate((lambda: a.band_histograms_device(sym.data_ptr(), W, H, F, wide, hist.data_ptr()), lambda: dst.copy_(sym)),
                                   1 if args.quick else 10, rounds)
        gb = sym.numel() / 1e9
        res["band_hist_u16" if wide else "band_hist_u8"] = {
            "symbol_bytes": int(sym.numel()), "call_ms": ms(h_runs), "copy_ms": ms(c_runs), "call_gb_per_s_read": round(gb / (ms(h_runs) / 1e3), 1),
            "copy_gb_per_s_read": round(gb / (ms(c_runs) / 1e3), 1), "runs_call": h_runs, "runs_copy": c_runs,
            "note": "call = memset of the 24 KiB result, the kernel and a stream synchronise; copy = torch copy_ of the same bytes (read + write)"}
        print("band_hist", "u16" if wide else "u8", json.dumps(res["band_hist_u16" if wide else "band_hist_u8"]))
    if not args.quick:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", args.out)


if __name__ == "__main__":
    main()
