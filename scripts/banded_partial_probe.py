"""Frame ranges and half-size previews of a banded chunk (.alc v5) next to the three other ways to the
same pixels, on one device-resident 1920x1080x64 chunk of the benchmark's content at L = 512.

Per configuration and range, alternated call by call inside every round of one run (HIP events around calls that return
after their work has drained; 2 warm-up rounds, 6 measured ones; each side's fastest round and its max - min spread):
  (a) banded_preview_decode_device / banded_frames_decode_device on the banded chunk
  (b) preview_decode_device / frames_decode_device on the base twin
  (c) from_banded_device followed by (b): the route before these calls existed
  (d) banded_decode_device of the whole chunk
and, from the test hooks, the blocks each side entropy-decodes and the payload bytes its host call uploads.

  python scripts/banded_partial_probe.py --out profiles/r31_banded_partial_probe_1080p64.json
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
RANGES = ((31, 32), (24, 40), (0, 64))


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


def alternate(fns, warmup, rounds):
    """-> {name: [ms per round]}; the calls take turns inside a round"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    runs = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            runs[k].append(timed(fn))
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r31_banded_partial_probe_1080p64.json"))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--quick", action="store_true", help="one configuration, one round and no file")
    args = ap.parse_args()
    warmup, rounds = (1, 1) if args.quick else (args.warmup, args.rounds)
    a.set_device(0)
    dev = torch.device("cuda:0")
    L = 512
    rgb = bench.synth_chunk(dev, 0).reshape(-1).contiguous()
    cap = a.BANDED_HEADER_BYTES + 3 * a.wide_stream_bound(PX, L)
    plain, banded, twin = (torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(3))
    out_a, out_b = torch.empty_like(rgb), torch.empty_like(rgb)
    qw, qh = a.preview_dims(W, H)
    res = {"what": "frame ranges and previews of a banded chunk (a) against the base version's calls on the base twin (b), from_banded "
                   "followed by those (c) and the full banded decode (d); one 1920x1080x64 chunk (bench.synth_chunk content), MI355X, "
                   "device-resident calls, milliseconds",
           "warmup_rounds": warmup, "rounds": rounds, "lane_symbols": L, "raw_bytes": int(rgb.numel()), "cases": []}
    fastest = lambda r: round(min(r), 4)                        # noqa: E731
    spread = lambda r: round(max(r) - min(r), 4)                # noqa: E731
    base_encode = {2: a.split_encode_device, 3: a.wide_encode_device}
    configs = [(a.WaveletType.Cdf97, 80, 2), (a.WaveletType.Cdf53, 50, 2), (a.WaveletType.Cdf97, 95, 3)]
    for wt, q, base in configs[:1] if args.quick else configs:
        n_plain = int(base_encode[base](rgb.data_ptr(), W, H, F, 1, wt, q, plain.data_ptr(), cap, lane_symbols=L)[0])
        n_banded = int(a.banded_encode_device(rgb.data_ptr(), W, H, F, 1, wt, q, banded.data_ptr(), cap, lane_symbols=L, base=base)[0])
        host_plain, host_banded = plain[:n_plain].cpu().numpy(), banded[:n_banded].cpu().numpy()
        n_twin = {}

        def repack():
            n_twin["n"] = int(a.from_banded_device(banded.data_ptr(), cap, [n_banded], twin.data_ptr(), cap)[0])

        repack()
        assert n_twin["n"] == n_plain and bool(torch.equal(twin[:n_plain], plain[:n_plain])), "from_banded is not the base chunk"
        for t0, t1 in RANGES:
            n = t1 - t0
            fns = {
                "a_preview": lambda: a.banded_preview_decode_device(banded.data_ptr(), n_banded, t0, n, out_a.data_ptr()),
                "b_preview": lambda: a.preview_decode_device(plain.data_ptr(), n_plain, t0, n, out_b.data_ptr()),
                "c_preview": lambda: (repack(), a.preview_decode_device(twin.data_ptr(), n_twin["n"], t0, n, out_b.data_ptr())),
                "a_frames": lambda: a.banded_frames_decode_device(banded.data_ptr(), n_banded, t0, n, out_a.data_ptr()),
                "b_frames": lambda: a.frames_decode_device(plain.data_ptr(), n_plain, t0, n, out_b.data_ptr()),
                "c_frames": lambda: (repack(), a.frames_decode_device(twin.data_ptr(), n_twin["n"], t0, n, out_b.data_ptr())),
                "d_full_banded_decode": lambda: a.banded_decode_device(banded.data_ptr(), cap, [n_banded], out_a.data_ptr()),
            }
            runs = alternate(fns, warmup, rounds)
            # the results, and what each side read
            equal, blocks, payload = {}, {}, {}
            for kind, nbytes in (("preview", n * qw * qh * 3), ("frames", n * W * H * 3)):
                fns["a_" + kind]()
                blocks["a_" + kind] = a._test_last_banded_partial_stats(kind)[2]
                fns["b_" + kind]()
                blocks["b_" + kind] = (a._test_last_preview_stats if kind == "preview" else a._test_last_frames_stats)()[2]
                equal[kind] = bool(torch.equal(out_a[:nbytes], out_b[:nbytes]))
                (a.decode_banded_preview if kind == "preview" else a.decode_banded_frames)(host_banded, t0, n)
                payload["a_" + kind] = a._test_last_banded_partial_stats(kind)[3]
                (a.decode_preview if kind == "preview" else a.decode_frames)(host_plain, t0, n)
                payload["b_" + kind] = (a._test_last_preview_stats if kind == "preview" else a._test_last_frames_stats)()[3]
            row = {"wavelet": wt.name, "quality": q, "base": base, "range": [t0, t1],
                   "bytes": {"base": n_plain, "banded": n_banded},
                   "ms": {k: fastest(v) for k, v in runs.items()}, "spread_ms": {k: spread(v) for k, v in runs.items()},
                   "runs_ms": {k: [round(x, 4) for x in v] for k, v in runs.items()},
                   "blocks_decoded": blocks, "payload_bytes_read": payload, "a_equals_b": equal,
                   "a_faster_than_c": {k: fastest(runs["a_" + k]) < fastest(runs["c_" + k]) for k in ("preview", "frames")}}
            res["cases"].append(row)
            print(json.dumps({k: v for k, v in row.items() if k != "runs_ms"}))
    if not args.quick:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print("wrote", args.out)


if __name__ == "__main__":
    main()
